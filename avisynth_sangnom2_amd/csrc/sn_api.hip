// sn_api.hip -- the C ABI of libsangnom_hip.so (include/sangnom_hip.h): context life cycle,
// argument validation, and per-frame dispatch of the HIP kernels.
//
// Mirrors, on the host side, the reference's constructor and GetFrame
// (/root/reference/src/SangNom2.cpp:275-330 and :332-397); all pixel work happens in the kernels
// of sn_pool_kernels.hip and the fused sweeps (sn_fused_*_v3.hip).  There is no CPU fallback in this library.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "sn_aa_plan.h"
#include "sn_copier.h"
#include "sn_pool_dispatch.h"
#include "sn_route.h"
#include "sn_sweep_args.h"
#include "sn_surface_layout.h"
#include "sn_surface_plan.h"
#include "sn_internal.h"

constexpr int kSyncChunks = 4;  // chunks of rows a pageable plane of the synchronous call is staged in

namespace sn {

// Planar chroma scratch of the surface calls (sn_process_device_surfaces, sn_aa_process_device_surfaces): U and V of `cap`
// frames in the source's chroma geometry (a semi-planar source is split into it, the planes of an MSB-aligned one are shifted
// into it) and in the destination's (merged from it); and, for an MSB-aligned source only, its luma shifted down.
struct UvScratch {
    // every part: a view of `cap` frames, its frame stride one frame of the plane (base nullptr: the part is not allocated)
    PlaneViewW in[2];   // full height; a split writes the lines the pass keeps, the rest stays 0xA5
    PlaneViewW out[2];  // full height, every line written by the pass
    PlaneViewW y;       // luma of an MSB-aligned or packed source, LSB-aligned: as `in`
    PlaneViewW yo;      // luma a packed destination is packed from: as `out`
    int cap = 0;        // frames (0: not allocated yet)
    int64_t bytes = 0;  // all of it
    int64_t split_frames = 0, merged_frames = 0, copied_frames = 0;  // sn_surface_info
};

// What the clip's geometry decides is the plan (sn_route.h: c->bh, c->process[p], c->plane_fused[p], ...); the context adds the
// device's side of it.
struct Context : ClipPlan {
    sn_policy policy{};  // zeros = defaults (sangnom_hip.h)
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool counted_live = false;  // this context is counted in g_live_contexts[device]
    int64_t uv_frames = 0;      // frames whose U and V passes ran as one sweep (sn_fused_u8_uv.hip)
    bool copies_elsewhere = false;  // a pass of sn_aa_*: planes that are not processed are copied by that call, once
    bool chroma_elsewhere = false;  // during a surface call: chroma that is not processed has gone from src to dst already
    bool luma_elsewhere = false;    // ... with an MSB-aligned side: so has luma that is not processed
    // (pool.base, plane_pool[p].base: allocated on first use when the fused kernels serve the configuration)
    int slots = 1;    // frames of a batch the pool path runs at once (1: frames in order on slot 0)
    int fslots = 1;   // frames per chunk of the fused 4:2:0 sweeps (each needs its two hand-off pools)

    // fused 8-bit path with subsampled chroma: two scratch pools per batch slot (sn_fused_u8_v3.hip, Mode)
    uint8_t* fpool[2] = {nullptr, nullptr};
    int64_t fpool_frame_bytes = 0;

    // the host ring (sn_submit_host / sn_collect_host): ring_groups x ring_per_group frame slots; a group's
    // frames are swept by one launch on the group's stream
    struct HostGroup {
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;   // D2H of the group's latest launch finished
        hipEvent_t swept = nullptr;  // its kernels finished (orders history-carrying configurations)
        int lo = 0, hi = 0;          // slots [lo, hi) of the group are staged and not yet launched
    };
    enum SlotState : uint8_t { kFree = 0, kStaged = 1, kInFlight = 2 };
    std::vector<HostGroup> ring;
    std::vector<uint8_t> slot_state;
    std::vector<int32_t> slot_parity;
    struct SlotDst {  // sn_submit_host_to: where the slot's output goes (pinned planes: straight from the device)
        void* ptr[3] = {nullptr, nullptr, nullptr};
        int32_t pitch[3] = {0, 0, 0};
        bool direct[3] = {false, false, false};
        bool given = false;
        bool kept_on_host = false;  // the output's kept lines were copied from the source at submission: only the interpolated lines travel
    };
    std::vector<SlotDst> slot_dst;
    uint8_t* ring_pin_in[3] = {nullptr, nullptr, nullptr};   // [slot][plane bytes], one allocation per plane
    uint8_t* ring_pin_out[3] = {nullptr, nullptr, nullptr};
    uint8_t* ring_dev_in[3] = {nullptr, nullptr, nullptr};
    uint8_t* ring_dev_out[3] = {nullptr, nullptr, nullptr};
    int64_t ring_bytes_in[3] = {0, 0, 0}, ring_bytes_out[3] = {0, 0, 0};  // per frame
    int ring_per_group = 0;
    Copier* copier = nullptr;
    int host_depth = 0;
    int ring_next = 0;        // slot the next submission takes
    int ring_last = -1;       // group of the latest launch (its `swept` event is what the next launch waits for)
    int ring_pitch_in[3] = {0, 0, 0}, ring_pitch_out[3] = {0, 0, 0};

    // sn_process_host pipelines its planes: copies in on one stream, out on another, the kernels of plane p between
    // the arrival of plane p and its way back (PlaneGate); run_group waits / records per plane where it can
    struct PlaneGate {
        hipStream_t in = nullptr, out = nullptr;
        hipEvent_t arrived[3] = {nullptr, nullptr, nullptr}, done[3] = {nullptr, nullptr, nullptr};
        bool waited[3] = {false, false, false}, recorded[3] = {false, false, false};
        bool on = false;
    } gate;

    // staging for sn_process_host
    uint8_t* stage_src[3] = {nullptr, nullptr, nullptr};
    uint8_t* stage_dst[3] = {nullptr, nullptr, nullptr};
    int stage_src_pitch[3] = {0, 0, 0};
    int stage_dst_pitch[3] = {0, 0, 0};
    // pinned host staging of the synchronous call for planes in PAGEABLE memory: the lines that travel, compact, at the
    // device staging's pitch (kept lines in, interpolated lines out).  The runtime never sees a pageable pointer.
    uint8_t* sync_in[3] = {nullptr, nullptr, nullptr};
    uint8_t* sync_out[3] = {nullptr, nullptr, nullptr};
    hipEvent_t sync_back[3][kSyncChunks] = {};  // chunk k of plane p's interpolated lines has arrived in sync_out[p]

    int64_t frames = 0, fused_frames = 0;
    std::string err;
    UvScratch uv;  // sn_process_device_surfaces

    // row-band sweeps of small launches (sn_sweep_args.h): per scratch slot the bands' state
    // snapshots and the frame's flag; the verification counts failed frames in band_fallbacks_dev and mirrors the count
    // into band_fallbacks, host memory the device can write (what band_pause looks at)
    // the chain of a history-carrying stream (run_chain): a ring of pool slots, one per pass in flight
    uint8_t* chain_base = nullptr;
    int chain_slots = 0, chain_origin = 0;
    uint32_t* chain_flags = nullptr;   // 8-bit chains over several workgroups per buffer: their round counters (device) ...
    uint32_t* chain_status = nullptr;  // host memory the device writes: launches of chains over several workgroups that timed out and were
                                       // redone on one workgroup per buffer (running count, mirrored after every such launch)
    bool chain_force_fault = false;    // sn_debug_raise_chain_fault: the next such launch starts with its fault word up
    int64_t chained_frames = 0;
    uint32_t* band_state = nullptr;
    int32_t* band_flags = nullptr;
    int64_t* band_fallbacks = nullptr;
    int64_t* band_fallbacks_dev = nullptr;
    int64_t band_words = 0;       // state words per slot
    int64_t banded_frames = 0;
    int band_force = 0;           // sn_debug_set_bands: bands per frame (0 = choose), < 0 = never
    int band_warm = 0;            // rows of run-up (0 = the default of the sample type)
    FallbackPause band_pause;     // as of *band_fallbacks

    // column parts (sn_options.column_parts; sn_sweep_args.h, kParts): per scratch slot the frame's seam record and its
    // flag, the count of failed frames on the device and mirrored to host memory (the pause looks at the mirror)
    int parts_force = 0, parts_ghost_force = 0;   // sn_debug_set_column_parts
    uint8_t* parts_rec = nullptr;
    int64_t parts_frame_bytes = 0;
    int parts_slots = 0;
    int32_t* parts_flags = nullptr;
    int64_t* parts_fallbacks = nullptr;
    int64_t* parts_fallbacks_dev = nullptr;
    int64_t part_frames = 0;
    FallbackPause parts_pause;  // as of *parts_fallbacks

    double threshold(int p) const
    {
        switch (cfg.bytes_per_sample) {
        case 1: return (double)(uint8_t)aaf[p];   // float -> T at the finalizePlane_c call,
        case 2: return (double)(uint16_t)aaf[p];  // SangNom2.cpp:272
        default: return (double)aaf[p];
        }
    }
};

static thread_local std::string g_last_error;

// Host memory the caller has pinned through sn_pin_host_buffer (process-wide; a handful of ranges)
struct PinnedRange {
    uintptr_t lo, hi;
};
static std::mutex g_pin_mutex;
static std::vector<PinnedRange> g_pinned;
// Devices on which this process has live contexts (index = device ordinal, value = contexts): what sn_unpin_host_buffer
// has to wait for.  It used to walk every VISIBLE device, which in a multi-rank job that sees all GPUs created a primary
// context on each of them and touched devices that belong to other ranks (round-3 advisor).
static std::mutex g_live_mutex;
static std::vector<int> g_live_contexts;
static void live_context(int device, int delta)
{
    if (device < 0) return;
    std::lock_guard<std::mutex> lk(g_live_mutex);
    if ((size_t)device >= g_live_contexts.size()) g_live_contexts.resize((size_t)device + 1, 0);
    g_live_contexts[(size_t)device] += delta;
}

// is the plane [p, p + pitch * (rows - 1) + row_bytes) inside pinned memory?
static bool plane_is_pinned(const void* p, int pitch, int row_bytes, int rows)
{
    if (rows <= 0) return false;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p), hi = lo + (uintptr_t)pitch * (rows - 1) + row_bytes;
    std::lock_guard<std::mutex> lk(g_pin_mutex);
    for (const PinnedRange& r : g_pinned)
        if (lo >= r.lo && hi <= r.hi) return true;
    return false;
}

static int fail(Context* c, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    else g_last_error = buf;
    return code;
}

#define SN_HIP(ctx, call)                                                                      \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(ctx, SN_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_));       \
    } while (0)

// Create_SangNom2, SangNom2.cpp:407-422 (RGB / non-planar clips cannot be described by sn_config;
// `opt` does not exist on this path).
static const char* validate_text(const sn_config& c)
{
    const bool is420 = c.num_planes >= 3 && c.sub_w == 1 && c.sub_h == 1;
    if (c.height % 2 != 0) return "SangNom2: height must be even.";
    if (is420 && c.height % 4) return "SangNom2: height must be mod4.";
    if (c.order < 0 || c.order > 2) return "SangNom2: order must be between 0..2.";
    if (c.aa < 0 || c.aa > 128) return "SangNom2: aa must be between 0..128.";
    if (c.aac < 0 || c.aac > 128) return "SangNom2: aac must be between 0..128.";
    return nullptr;
}

static const char* structural_text(const sn_config& c)
{
    if (c.struct_size != (int32_t)sizeof(sn_config)) return "sn_config.struct_size mismatch";
    if (c.width <= 0 || c.height <= 0) return "width and height must be positive";
    if (c.bytes_per_sample != 1 && c.bytes_per_sample != 2 && c.bytes_per_sample != 4)
        return "bytes_per_sample must be 1, 2 or 4";
    if (c.bytes_per_sample == 1 && c.bits_per_sample != 8) return "8-bit samples need bits_per_sample 8";
    if (c.bytes_per_sample == 2 && (c.bits_per_sample < 9 || c.bits_per_sample > 16))
        return "16-bit containers need bits_per_sample 9..16";
    if (c.bytes_per_sample == 4 && c.bits_per_sample != 32) return "float samples need bits_per_sample 32";
    if (c.num_planes != 1 && c.num_planes != 3) return "num_planes must be 1 or 3";
    if (c.sub_w < 0 || c.sub_w > 2 || c.sub_h < 0 || c.sub_h > 2) return "sub_w / sub_h must be 0..2";
    if (c.num_planes == 3 && ((c.width & ((1 << c.sub_w) - 1)) || (c.height & ((1 << c.sub_h) - 1))))
        return "luma size must be a multiple of the chroma subsampling";
    if (c.max_batch < 0) return "max_batch must be >= 0";
    if (c.host_depth < 0 || c.host_depth > 256) return "host_depth must be 0..256";
    if (c.isolated_planes != 0 && c.isolated_planes != 1) return "isolated_planes must be 0 or 1";
    if (c.fresh_pool != 0 && c.fresh_pool != 1) return "fresh_pool must be 0 or 1";
    if (c.mode < SN_MODE_AUTO || c.mode > SN_MODE_FUSED) return "mode must be SN_MODE_AUTO/POOL/FUSED";
    return nullptr;
}

}  // namespace sn

using sn::Context;
using sn::Copier;
using sn::KeptLines;
using sn::PartsPlan;
using sn::kMaxBands;
using sn::kMaxBandSlots;
using sn::kMaxParts;

#ifdef SN_ABORT_TRACE  // diagnostic builds only (make EXTRA=-DSN_ABORT_TRACE): where did an abort() come from?
#include <execinfo.h>
#include <fcntl.h>
#include <signal.h>
#include <unistd.h>
namespace {
void abort_trace(int sig)
{
    const int fd = open("gpurun_out/abort_trace.txt", O_WRONLY | O_CREAT | O_APPEND, 0644);
    if (fd >= 0) {
        void* frames[64];
        const int n = backtrace(frames, 64);
        dprintf(fd, "signal %d, %d frames\n", sig, n);
        backtrace_symbols_fd(frames, n, fd);
        close(fd);
    }
    signal(sig, SIG_DFL);
    raise(sig);
}
struct AbortTraceInstaller {
    AbortTraceInstaller()
    {
        signal(SIGABRT, abort_trace);
        signal(SIGSEGV, abort_trace);
        signal(SIGBUS, abort_trace);
    }
} g_abort_trace_installer;
}  // namespace
#endif

#pragma GCC visibility push(default)
extern "C" {

int sn_abi_version(void) { return SN_ABI_VERSION; }

const char* sn_last_error(const sn_context* ctx)
{
    if (ctx) return reinterpret_cast<const Context*>(ctx)->err.c_str();
    return sn::g_last_error.c_str();
}

int sn_validate(const sn_config* cfg, char* msg, size_t msg_len)
{
    if (!cfg) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "cfg is NULL");
    const char* t = sn::structural_text(*cfg);
    int rc = SN_OK;
    if (t) rc = SN_ERR_INVALID_ARG;
    else if ((t = sn::validate_text(*cfg)) != nullptr) rc = SN_ERR_CONFIG;
    if (msg && msg_len) snprintf(msg, msg_len, "%s", t ? t : "");
    if (t) sn::g_last_error = t;
    return rc;
}

void sn_destroy(sn_context* h)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->counted_live) sn::live_context(c->device, -1);
    // every stream that may still run kernels on this context's scratch drains first; only then is memory freed
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& g : c->ring)
        if (g.stream) (void)hipStreamSynchronize(g.stream);
    if (c->pool.base) (void)hipFree(c->pool.base);
    if (c->chain_base) (void)hipFree(c->chain_base);
    if (c->chain_flags) (void)hipFree(c->chain_flags);
    if (c->chain_status) (void)hipHostFree(c->chain_status);
    for (int p = 0; p < 3; ++p)
        if (c->plane_pool[p].base) (void)hipFree(c->plane_pool[p].base);
    for (int i = 0; i < 2; ++i)
        if (c->fpool[i]) (void)hipFree(c->fpool[i]);
    for (const sn::PlaneViewW& q : {c->uv.in[0], c->uv.in[1], c->uv.out[0], c->uv.out[1], c->uv.y, c->uv.yo})
        if (q.base) (void)hipFree(q.base);
    if (c->gate.in) (void)hipStreamSynchronize(c->gate.in);
    if (c->gate.out) (void)hipStreamSynchronize(c->gate.out);
    for (int p = 0; p < 3; ++p) {
        if (c->gate.arrived[p]) (void)hipEventDestroy(c->gate.arrived[p]);
        if (c->gate.done[p]) (void)hipEventDestroy(c->gate.done[p]);
    }
    if (c->gate.in) (void)hipStreamDestroy(c->gate.in);
    if (c->gate.out) (void)hipStreamDestroy(c->gate.out);
    if (c->band_state) (void)hipFree(c->band_state);
    if (c->band_flags) (void)hipFree(c->band_flags);
    if (c->band_fallbacks) (void)hipHostFree(c->band_fallbacks);
    if (c->band_fallbacks_dev) (void)hipFree(c->band_fallbacks_dev);
    if (c->parts_rec) (void)hipFree(c->parts_rec);
    if (c->parts_flags) (void)hipFree(c->parts_flags);
    if (c->parts_fallbacks) (void)hipHostFree(c->parts_fallbacks);
    if (c->parts_fallbacks_dev) (void)hipFree(c->parts_fallbacks_dev);
    delete c->copier;
    for (int p = 0; p < 3; ++p) {
        if (c->ring_pin_in[p]) (void)hipHostFree(c->ring_pin_in[p]);
        if (c->ring_pin_out[p]) (void)hipHostFree(c->ring_pin_out[p]);
        if (c->ring_dev_in[p]) (void)hipFree(c->ring_dev_in[p]);
        if (c->ring_dev_out[p]) (void)hipFree(c->ring_dev_out[p]);
    }
    for (auto& g : c->ring) {
        if (g.done) (void)hipEventDestroy(g.done);
        if (g.swept) (void)hipEventDestroy(g.swept);
        if (g.stream) (void)hipStreamDestroy(g.stream);
    }
    for (int p = 0; p < 3; ++p) {
        if (c->stage_src[p]) (void)hipFree(c->stage_src[p]);
        if (c->stage_dst[p]) (void)hipFree(c->stage_dst[p]);
        if (c->sync_in[p]) (void)hipHostFree(c->sync_in[p]);
        if (c->sync_out[p]) (void)hipHostFree(c->sync_out[p]);
        for (int k = 0; k < kSyncChunks; ++k)
            if (c->sync_back[p][k]) (void)hipEventDestroy(c->sync_back[p][k]);
    }
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// Environment overrides of the policy exist only in builds with -DSN_TEST_HOOKS (bisecting in the field); the shipped
// library reads no environment variable.
static const char* test_env(const char* name)
{
#ifdef SN_TEST_HOOKS
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

// Device scratch one context may hold per kind (pool-path slots; hand-off pools of the fused 4:2:0 sweeps):
// sn_policy.scratch_budget_mb, 24 GiB by default (the tests shrink it to exercise the chunking on small batches).
static int64_t scratch_budget(const Context* c)
{
    if (const char* e = test_env("SN_SCRATCH_BUDGET_MB"))
        if (atoll(e) > 0) return atoll(e) << 20;
    return c->policy.scratch_budget_mb > 0 ? (int64_t)c->policy.scratch_budget_mb << 20 : 24ll << 30;
}
static bool scratch_budget_is_default(const Context* c) { return c->policy.scratch_budget_mb <= 0 && !test_env("SN_SCRATCH_BUDGET_MB"); }
static bool sweeps_always(const Context* c)  // SN_SMALL_SWEEP
{
    if (const char* e = test_env("SN_PREFER_POOL")) return atoi(e) == 0;
    return c->policy.small_launches == SN_SMALL_SWEEP;
}

// The pool: zero-filled (the convention that makes the reference's output defined).
static int ensure_pool(Context* c, int plane = 0)
{
    sn::PoolArgs& pool = c->isolated ? c->plane_pool[plane] : c->pool;
    if (pool.base) return SN_OK;
    SN_HIP(c, hipMalloc(reinterpret_cast<void**>(&pool.base), (size_t)pool.slot_bytes * c->slots));
    SN_HIP(c, hipMemsetAsync(pool.base, 0, (size_t)pool.slot_bytes * c->slots, c->stream));
    SN_HIP(c, hipStreamSynchronize(c->stream));  // the first user may be a ring slot's stream
    return SN_OK;
}

// A hand-off pool of the coupled sweeps (0: luma -> U, 1: U -> V), fslots frames of it.
static int ensure_fpool(Context* c, int i)
{
    if (c->fpool[i]) return SN_OK;
    SN_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->fpool[i]), (size_t)c->fpool_frame_bytes * c->fslots));
    // cells outside the hand-off's dependency cone are never written: zero, so that the debug read-back is defined
    SN_HIP(c, hipMemsetAsync(c->fpool[i], 0, (size_t)c->fpool_frame_bytes * c->fslots, c->stream));
    if (i == 1) SN_HIP(c, hipStreamSynchronize(c->stream));  // allocated late: its first user may be a ring slot's stream
    return SN_OK;
}

// Seam records and flags for `nseams` seams per frame: allocated when the context is created (and by the test hook), never
// inside a launch; counted against the scratch budget.
static int ensure_parts(Context* c, int nseams)
{
    int nr_max = 0;
    for (int p = 0; p < c->nplanes(); ++p)
        if (c->cfg.dh || c->process[p]) nr_max = c->plane_h_out(p) / 2 - 1 > nr_max ? c->plane_h_out(p) / 2 - 1 : nr_max;
    const int64_t need = (int64_t)nseams * 2 * sn::parts_side_bytes(c->cfg.bytes_per_sample, nr_max);
    if (need <= 0) return SN_OK;
    const int64_t want = c->cfg.max_batch > c->host_depth ? c->cfg.max_batch : c->host_depth;
    if (c->parts_rec && need <= c->parts_frame_bytes) return SN_OK;
    SN_HIP(c, hipStreamSynchronize(c->stream));
    if (c->parts_rec) SN_HIP(c, hipFree(c->parts_rec));
    c->parts_rec = nullptr;
    int64_t fit = scratch_budget(c) / need;
    fit = fit < 1 ? 1 : fit > want ? want : fit;
    c->parts_frame_bytes = need;
    c->parts_slots = (int)fit;
    SN_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->parts_rec), (size_t)need * fit));
    if (!c->parts_flags) {
        SN_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->parts_flags), sizeof(int32_t) * want));
        SN_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->parts_fallbacks_dev), sizeof(int64_t)));
        SN_HIP(c, hipMemsetAsync(c->parts_fallbacks_dev, 0, sizeof(int64_t), c->stream));
        SN_HIP(c, hipStreamSynchronize(c->stream));
        SN_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&c->parts_fallbacks), sizeof(int64_t), hipHostMallocMapped));
        *c->parts_fallbacks = 0;
    }
    return SN_OK;
}

// ... and the pool slots the redo of a failed frame runs on -- or, a plane marked for parts that is never cut (no
// interpolated row: plan_parts), the pool path that serves it in every launch (run_group)
static int ensure_parts_scratch(Context* c)
{
    int nseams = 0;
    for (int p = 0; p < c->nplanes(); ++p) {
        PartsPlan pl;
        if (!sn::plan_parts(*c, p, c->parts_force, c->parts_ghost_force, pl) && !c->plane_parts[p]) continue;
        nseams = pl.n - 1 > nseams ? pl.n - 1 : nseams;
        const int rc = ensure_pool(c, c->isolated ? p : 0);
        if (rc != SN_OK) return rc;
    }
    return nseams > 0 ? ensure_parts(c, nseams) : SN_OK;
}

static int create_impl(const sn_config* cfg, Context* c)
{
    c->cfg = *cfg;
    if (c->cfg.max_batch < 1) c->cfg.max_batch = 1;
    c->host_depth = cfg->host_depth > 0 ? cfg->host_depth : 4;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return sn::fail(c, SN_ERR_NO_DEVICE, "no HIP device available (libsangnom_hip has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev)
        return sn::fail(c, SN_ERR_NO_DEVICE, "HIP device %d out of range (0..%d)", cfg->device, ndev - 1);
    c->device = cfg->device;
    SN_HIP(c, hipSetDevice(c->device));

    // what the geometry decides, and what it refuses (sn_route.h)
    {
        sn::ClipPlan plan = sn::clip_plan(c->cfg, c->arith, c->parts_on, c->policy);
        if (plan.refusal != SN_OK) return sn::fail(c, plan.refusal, "%s", plan.refusal_text.c_str());
        static_cast<sn::ClipPlan&>(*c) = plan;
    }
    if (cfg->stream) {
        c->stream = reinterpret_cast<hipStream_t>(cfg->stream);
    } else {
        SN_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }

    // Scratch is bounded: a batch larger than what scratch_budget() holds runs in chunks on the same slots
    // (only history-free configurations batch at all, and for them a slot's old content never matters).
    int rc = SN_OK;
    auto fit = [&](int64_t per_frame) {
        const int64_t n = scratch_budget(c) / per_frame;
        const int64_t want = c->cfg.max_batch > c->host_depth ? c->cfg.max_batch : c->host_depth;  // frames in flight
        return (int)(n < 1 ? 1 : n < want ? n : want);
    };
    c->slots = c->history_free ? fit(c->pool.slot_bytes) : 1;
    if (c->use_fused) {
        // the fused sweeps serve this configuration: the pool path only takes the launches that are too small to
        // be worth a sweep (sn::prefer_pool), so a few slots are enough
        const int64_t cap = (4ll << 30) / c->pool.slot_bytes;
        const int small = (int)(cap < 1 ? 1 : cap > 64 ? 64 : cap);
        if (c->slots > small) c->slots = small;
    }
    if (!c->use_fused) {
        for (int p = 0; p < (c->isolated ? c->nplanes() : 1); ++p) {
            if (c->isolated && (c->plane_fused[p] || !(cfg->dh || c->process[p]))) continue;
            rc = ensure_pool(c, p);
            if (rc != SN_OK) return rc;
        }
    }
    if (c->fused420) {
        c->fpool_frame_bytes = sn::sweep_pool_bytes(cfg->bytes_per_sample, cfg->width, c->fpool_rows);
        // a chunk is three launches of one workgroup per frame: whole rounds of resident workgroups
        // (two waves per SIMD, 256 CUs) leave no partly filled round at the end of each launch
        const int nw = sn::sweep_waves(cfg->bytes_per_sample, cfg->width);
        const int round = 256 * (8 / nw);
        // (U and V as one sweep need the luma -> U pool only: ClipPlan::uv_geometry)
        const int npools = c->uv_geometry ? 1 : 2;
        c->fslots = fit(npools * c->fpool_frame_bytes);  // fused420 implies history-free (fused_eligible)
        if (c->fslots < round && scratch_budget_is_default(c)) {
            // wide float frames: a chunk below one round leaves compute units idle in every launch, so the hand-off
            // pools may take up to a quarter of the device's memory to reach one
            size_t free_b = 0, total_b = 0;
            SN_HIP(c, hipMemGetInfo(&free_b, &total_b));
            const int64_t cap = (int64_t)(total_b / 4 < free_b / 2 ? total_b / 4 : free_b / 2) / (npools * c->fpool_frame_bytes);
            const int64_t want = c->cfg.max_batch > c->host_depth ? c->cfg.max_batch : c->host_depth;
            int64_t n = cap < round ? cap : round;
            if (n > want) n = want;
            if (n > c->fslots) c->fslots = (int)n;
        }
        if (c->fslots > round) c->fslots -= c->fslots % round;
        for (int i = 0; i < npools; ++i) {
            const int rc2 = ensure_fpool(c, i);
            if (rc2 != SN_OK) return rc2;
        }
    }
    if (c->plane_parts[0] || c->plane_parts[1] || c->plane_parts[2]) {
        rc = ensure_parts_scratch(c);
        if (rc != SN_OK) return rc;
    }
    SN_HIP(c, hipStreamSynchronize(c->stream));
    return SN_OK;
}

static const char* policy_text(const sn_policy* p)
{
    if (!p) return nullptr;
    if (p->struct_size != (int32_t)sizeof(sn_policy)) return "sn_policy.struct_size mismatch";
    if (p->small_launches != SN_SMALL_AUTO && p->small_launches != SN_SMALL_SWEEP) return "sn_policy.small_launches must be SN_SMALL_AUTO or SN_SMALL_SWEEP";
    if (p->chain != 0 && p->chain != -1 && p->chain != 1 && p->chain != 2 && p->chain != 4 && p->chain != 8)
        return "sn_policy.chain must be 0 (on), -1 (off), or 1, 2, 4, 8 (workgroups per cost buffer of a chain)";
    if (p->copy_threads < 0 || p->copy_threads > 16) return "sn_policy.copy_threads must be 0..16";
    if (p->scratch_budget_mb < 0) return "sn_policy.scratch_budget_mb must not be negative";
    if (p->chroma_sweeps != 0 && p->chroma_sweeps != 1) return "sn_policy.chroma_sweeps must be 0 (U and V as one sweep) or 1 (a sweep each)";
    if (p->sse2_sweeps != 0 && p->sse2_sweeps != 1) return "sn_policy.sse2_sweeps must be 0 (the kernels of the previous release) or 1 (sweeps wherever SN_ARITH_CXX has them)";
    return nullptr;
}

int sn_create(const sn_config* cfg, sn_context** out) { return sn_create_with_policy(cfg, nullptr, out); }

int sn_create_with_policy(const sn_config* cfg, const sn_policy* policy, sn_context** out) { return sn_create_ex(cfg, policy, nullptr, out); }

static const char* options_text(const sn_options* o)
{
    if (!o) return nullptr;
    if (o->struct_size != (int32_t)sizeof(sn_options)) return "sn_options.struct_size mismatch";
    if (o->arithmetic != SN_ARITH_CXX && o->arithmetic != SN_ARITH_SSE2) return "sn_options.arithmetic must be SN_ARITH_CXX or SN_ARITH_SSE2";
    if (o->column_parts != 0 && o->column_parts != 1) return "sn_options.column_parts must be 0 (off) or 1 (wide 16-bit and float planes in column parts)";
    for (int32_t r : o->reserved)
        if (r != 0) return "sn_options.reserved must be zero";
    return nullptr;
}

int sn_create_ex(const sn_config* cfg, const sn_policy* policy, const sn_options* options, sn_context** out)
{
    if (!cfg || !out) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "cfg / out is NULL");
    *out = nullptr;
    char msg[256];
    int rc = sn_validate(cfg, msg, sizeof msg);
    if (rc != SN_OK) return rc;  // g_last_error already holds the text
    if (const char* t = policy_text(policy)) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "%s", t);
    if (const char* t = options_text(options)) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "%s", t);
    Context* c = new (std::nothrow) Context();
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "out of host memory");
    if (options) c->arith = options->arithmetic;
    if (options) c->parts_on = options->column_parts == 1;
    if (policy) c->policy = *policy;
    c->policy.struct_size = (int32_t)sizeof(sn_policy);
    rc = create_impl(cfg, c);
    if (rc != SN_OK) {
        sn::g_last_error = c->err;
        sn_destroy(reinterpret_cast<sn_context*>(c));
        return rc;
    }
    sn::live_context(c->device, +1);
    c->counted_live = true;
    *out = reinterpret_cast<sn_context*>(c);
    return SN_OK;
}

// The host's copy threads (staging of the ring, kept lines of the synchronous call): sn_policy.copy_threads in all, the caller included.
static void ensure_copier(Context* c)
{
    if (c->copier) return;
    const char* e = test_env("SN_COPY_THREADS");
    const unsigned hw = std::thread::hardware_concurrency();
    const int asked = e ? atoi(e) : c->policy.copy_threads;  // in all, the caller included; 0 = by core count
    int workers = asked > 0 ? asked - 1 : (hw >= 8 ? 3 : hw >= 4 ? 1 : 0);
    if (workers < 0) workers = 0;
    if (workers > 15) workers = 15;
    c->copier = new Copier(workers);
}

// The other half of the same observation: the kept lines of the OUTPUT are copies of source lines (field copy, border
// line, SangNom2.cpp:361-391), and a plane that is not processed is a copy altogether.  Where the caller's source is
// still at hand (the synchronous call) the host copies those lines itself, while the device is busy, and only the
// interpolated lines come back over PCIe.
static int kept_line_jobs(const Context* c, int p, int parity, const void* src, int sp, void* dst, int dp, Copier::Job* jobs)
{
    const int row = c->plane_w(p) * c->cfg.bytes_per_sample;
    const uint8_t* s = static_cast<const uint8_t*>(src);
    uint8_t* d = static_cast<uint8_t*>(dst);
    if (!(c->cfg.dh || c->process[p])) {
        jobs[0] = {d, s, dp, sp, row, c->plane_h_in(p)};
        return 1;
    }
    const int off = sn::field_offset(c->cfg.order, parity), nk = c->plane_h_out(p) / 2, h_out = c->plane_h_out(p);
    const int first = c->cfg.dh ? 0 : off, step = c->cfg.dh ? 1 : 2;  // kept line k in the source
    jobs[0] = {d + (size_t)off * dp, s + (size_t)first * sp, 2 * dp, step * sp, row, nk};
    if (off == 0) jobs[1] = {d + (size_t)(h_out - 1) * dp, s + (size_t)(first + step * (nk - 1)) * sp, dp, sp, row, 1};  // SangNom2.cpp:380-385
    else jobs[1] = {d, s + (size_t)first * sp, dp, sp, row, 1};                                                       // :386-391
    return 2;
}

static int check_planes(Context* c, const void* const src[3], const int32_t sp[3], void* const dst[3],
                        const int32_t dp[3])
{
    if (!src || !sp || !dst || !dp) return sn::fail(c, SN_ERR_INVALID_ARG, "plane array is NULL");
    for (int p = 0; p < c->nplanes(); ++p) {
        const int rb = c->plane_w(p) * c->cfg.bytes_per_sample;
        if (!src[p] || !dst[p]) return sn::fail(c, SN_ERR_INVALID_ARG, "plane %d pointer is NULL", p);
        if (sp[p] < rb || dp[p] < rb)
            return sn::fail(c, SN_ERR_INVALID_ARG, "plane %d pitch smaller than the row size %d", p, rb);
        if (sp[p] % c->cfg.bytes_per_sample || dp[p] % c->cfg.bytes_per_sample ||
            (uintptr_t)src[p] % c->cfg.bytes_per_sample || (uintptr_t)dst[p] % c->cfg.bytes_per_sample)
            return sn::fail(c, SN_ERR_INVALID_ARG, "plane %d pointer/pitch not aligned to the sample size", p);
    }
    return SN_OK;
}

// The chroma half of a small 4:2:0 launch as chains (run_group): three ring slots per frame -- the luma plane's smoothed
// rows (left there by the bands), U's pass, V's pass -- for the frames on pool slots slot0 .. slot0 + n - 1 (launches of the
// host ring run side by side on streams of their own, each on its own slots).  The ring is this context's chain ring (a
// history-free context has no other use for it); false: no room, the pool kernels take the chroma planes one after the
// other as before.
static bool ensure_chroma_chains(Context* c, int slot0, int n, hipStream_t st)
{
    if (c->chain_slots < 0 || c->policy.chain < 0) return false;
    if (sn::pool_chain_lanes(c->cfg.bytes_per_sample, c->stride_e) < 2) return false;
    if (const char* e = test_env("SN_CHAIN"))
        if (atoi(e) == 0) return false;
    if (!c->chain_base) {
        int64_t fit = scratch_budget(c) / 8 / c->pool.slot_bytes;
        const int64_t want = 3 * (int64_t)(c->slots < kMaxBandSlots ? c->slots : kMaxBandSlots);
        if (fit > want) fit = want;
        const int64_t addressable = (int64_t)0xfffffffe / c->pool.slot_bytes;  // the chain kernels address the ring with 32-bit offsets
        if (fit > addressable) fit = addressable;
        fit -= fit % 3;
        if (fit < 3) return false;
        if (hipMalloc(reinterpret_cast<void**>(&c->chain_base), (size_t)c->pool.slot_bytes * fit) != hipSuccess) {
            (void)hipGetLastError();
            c->chain_base = nullptr;
            c->chain_slots = -1;
            return false;
        }
        c->chain_slots = (int)fit;
        // row 0 of every buffer stays zero, as in the pool; waited for once, because the next launch may come on another
        // stream (a group of the host ring)
        if (hipMemsetAsync(c->chain_base, 0, (size_t)c->pool.slot_bytes * fit, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return false;
        c->chain_origin = 0;
    }
    return 3 * (slot0 + n) <= c->chain_slots;
}

// The band fields of one sweep over pool rows 1 .. last, at most `want` bands.
static void set_bands(const Context* c, sn::FusedPool& fp, int want, int last, int slot0, bool first)
{
    const sn::BandGeometry bg = sn::band_geometry(want, last);
    fp.band_rows = bg.band_rows;
    fp.nbands = bg.nbands;
    fp.band_warm = sn::band_warm_rows(c->cfg.bytes_per_sample, c->band_warm);
    fp.band_state = c->band_state + (int64_t)slot0 * c->band_words;
    fp.band_flags = c->band_flags + slot0;
    fp.band_reset = first ? 1 : 0;
}

static int band_threads(const Context* c)
{
    return 64 * sn::sweep_waves(c->cfg.bytes_per_sample, c->cfg.width);
}

static int ensure_bands(Context* c)
{
    if (c->band_state) return SN_OK;
    c->band_words = sn::band_state_words(band_threads(c), kMaxBands);
    const int slots = c->slots < kMaxBandSlots ? c->slots : kMaxBandSlots;
    SN_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->band_state), (size_t)c->band_words * 4 * slots));
    SN_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->band_flags), sizeof(int32_t) * slots));
    SN_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->band_fallbacks_dev), sizeof(int64_t)));
    SN_HIP(c, hipMemsetAsync(c->band_fallbacks_dev, 0, sizeof(int64_t), c->stream));
    SN_HIP(c, hipStreamSynchronize(c->stream));
    SN_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&c->band_fallbacks), sizeof(int64_t), hipHostMallocMapped));
    *c->band_fallbacks = 0;
    return SN_OK;
}

// The host-facing entry points (a synchronous GetFrame, the host ring) launch a few frames at a time, i.e. they will
// want the scratch of the small-launch paths: the pool-path pool and the band state.  It is allocated here, BEFORE the
// call queues its copies from pageable host memory -- allocating in the middle of such a call (as the lazy
// ensure_pool / ensure_bands of run_group would) puts hipMalloc / hipHostMalloc between the runtime's in-flight staging
// of those copies and their completion.
constexpr int SN_CHAIN_UNAVAILABLE = -1000;  // internal: run_chain could not get its ring, run_batch falls back
static int chain_planes(const Context* c, int planes[3]);
static int ensure_chain(Context* c, int pn, hipStream_t st);

static int prepare_small_launch_scratch(Context* c)
{
    if (!c->history_free) {
        // a history-carrying clip: even ONE frame with two processed planes is a chain of passes, so the chain's ring is
        // part of what the host-facing calls need -- allocated here, before their copies are queued, not by the first
        // chained launch in the middle of a pipelined call.  A ring that cannot be had leaves the
        // context on the pass-by-pass path (chain_slots = -1), as run_chain's own fallback does.
        int planes[3];
        const int pn = chain_planes(c, planes);
        if (pn > 0) {
            const int rc = ensure_pool(c);
            if (rc != SN_OK) return rc;
            const bool had_ring = c->chain_base != nullptr;
            const int rc2 = ensure_chain(c, pn, c->stream);
            if (rc2 != SN_OK && rc2 != SN_CHAIN_UNAVAILABLE) return rc2;  // (unavailable: the pass-by-pass path, no error pending)
            // only when the ring has just been allocated and zeroed on c->stream: its first user may be a ring slot's stream
            if (!had_ring && c->chain_base) SN_HIP(c, hipStreamSynchronize(c->stream));
        }
        return SN_OK;
    }
    if (c->cfg.mode != SN_MODE_AUTO) return SN_OK;
    int rc = SN_OK;
    if (c->isolated) {
        for (int p = 0; p < c->nplanes() && rc == SN_OK; ++p)
            if (c->cfg.dh || c->process[p]) rc = ensure_pool(c, p);
    } else if (c->use_fused) {
        rc = ensure_pool(c);
    }
    if (rc == SN_OK && sn::band_rows_available(*c, c->band_force, c->parts_force) > 0) rc = ensure_bands(c);
    return rc;
}

// One plane of frames [f0, ...) of a strided batch, as the launchers take it.
static sn::PlaneArgs plane_args(const Context* c, int p, const void* const src[3], const int64_t sfs[3], const int32_t sp[3], void* const dst[3],
                                const int64_t dfs[3], const int32_t dp[3], int f0, int offset)
{
    sn::PlaneArgs a{};
    a.src = static_cast<const uint8_t*>(src[p]) + (int64_t)f0 * sfs[p];
    a.dst = static_cast<uint8_t*>(dst[p]) + (int64_t)f0 * dfs[p];
    a.src_frame_stride = sfs[p];
    a.dst_frame_stride = dfs[p];
    a.src_pitch = sp[p];
    a.dst_pitch = dp[p];
    a.w = c->plane_w(p);
    a.h_in = c->plane_h_in(p);
    a.h_out = c->plane_h_out(p);
    a.offset = offset;
    a.dh = c->cfg.dh;
    a.enabled = (c->cfg.dh || c->process[p]) ? 1 : 0;
    a.copied_elsewhere = (c->copies_elsewhere || (p > 0 ? c->chroma_elsewhere : c->luma_elsewhere)) ? 1 : 0;
    a.arith = c->saturating ? SN_ARITH_SSE2 : SN_ARITH_CXX;  // (the sweeps; the pool kernels take PoolArgs::arith)
    return a;
}

static sn::PlaneArgs frames_from(sn::PlaneArgs a, int i)
{
    a.src += (int64_t)i * a.src_frame_stride;
    a.dst += (int64_t)i * a.dst_frame_stride;
    return a;
}

// What run_group has decided about one launch, for the route that carries it out.
struct GroupLaunch {
    Context* c;
    hipStream_t st;
    int slot0, n;
    sn::PlaneArgs pa[3];
    bool fused[3] = {false, false, false};  // the plane goes through the sweeps
    PartsPlan plan[3];                       // ... in column parts where plan[p].n > 0
    int stop[3] = {0, 0, 0};                 // where stage 2 of the pool path may stop (PoolArgs::rows)
    int nbands = 0;                          // > 0: the launch is small enough for row bands
    bool parts_counted = false;

    // sn_process_host's plane pipeline: a plane's kernels wait for its copy and announce their end; the paths that are
    // not written plane by plane wait for everything first (the caller records what was not announced)
    hipError_t plane_in(int p) const
    {
        if (!c->gate.on || c->gate.waited[p]) return hipSuccess;
        c->gate.waited[p] = true;
        return hipStreamWaitEvent(st, c->gate.arrived[p], 0);
    }
    hipError_t plane_out(int p) const
    {
        if (!c->gate.on) return hipSuccess;
        c->gate.recorded[p] = true;
        return hipEventRecord(c->gate.done[p], st);
    }
    void count_parts()
    {
        if (!parts_counted) c->part_frames += n;
        parts_counted = true;
    }
};

// One plane in column parts: a sweep per window, the check of the seams, and the pool path for the frames that fail it
// (guarded launches, a chunk of pool slots at a time, that exit at once otherwise).  No k_assemble: kept lines are right
// either way.
static int parts_plane(const GroupLaunch& g, int p, const sn::PlaneArgs& a0, sn::PoolArgs pool)
{
    Context* c = g.c;
    const PartsPlan& pl = g.plan[p];
    const int B = c->cfg.bytes_per_sample;
    const int64_t side = sn::parts_side_bytes(B, a0.h_out / 2 - 1);
    const int nseams = pl.n - 1;
    if ((int64_t)nseams * 2 * side > c->parts_frame_bytes) return sn::fail(c, SN_ERR_UNSUPPORTED, "column parts: the seam record is too small for %d parts", pl.n);
    const int cap = c->parts_slots - g.slot0, pcap = c->slots - g.slot0;
    uint8_t* rec = c->parts_rec + (int64_t)g.slot0 * c->parts_frame_bytes;
    int32_t* flags = c->parts_flags + g.slot0;
    for (int i = 0; i < g.n; i += cap) {
        const int m = g.n - i < cap ? g.n - i : cap;
        const sn::PlaneArgs a = frames_from(a0, i);
        SN_HIP(c, hipMemsetAsync(flags, 0, sizeof(int32_t) * m, g.st));
        sn::FusedPool fp{};
        fp.mode = sn::v3c::kParts;  // one launch, a workgroup per part and frame
        fp.nparts = pl.n;
        fp.win_w = pl.win_w;
        for (int k = 0; k < pl.n; ++k) {
            fp.win_x[k] = pl.win_x[k];
            fp.store_lo[k] = pl.seam[k] - pl.win_x[k];
            fp.store_hi[k] = pl.seam[k + 1] - pl.win_x[k];
            fp.seam_x[k][0] = k > 0 ? pl.seam[k] - pl.win_x[k] : -1;
            fp.seam_off[k][0] = k > 0 ? (int)((2 * (k - 1) + 1) * side) : 0;  // side 1 of the seam on its left
            fp.seam_x[k][1] = k < pl.n - 1 ? pl.seam[k + 1] - pl.win_x[k] : -1;
            fp.seam_off[k][1] = k < pl.n - 1 ? (int)(2 * k * side) : 0;      // side 0 of the seam on its right
        }
        fp.seam_rec = rec;
        fp.seam_frame_stride = c->parts_frame_bytes;
        fp.seam_bytes = (int)(nseams * 2 * side);
        SN_HIP(c, sn::launch_sweep(g.st, B, a, c->threshold(p), m, &fp));
        SN_HIP(c, sn::launch_parts_verify(g.st, rec, c->parts_frame_bytes, side, nseams, m, flags, c->parts_fallbacks_dev, c->parts_fallbacks));
        for (int j = 0; j < m; j += pcap) {
            sn::PlaneArgs r = frames_from(a, j);
            r.guard = flags + j;
            pool.guard = flags + j;
            SN_HIP(c, sn::launch_pool_plane(g.st, r, pool, B, c->threshold(p), m - j < pcap ? m - j : pcap, g.slot0));
        }
    }
    return SN_OK;
}

// The latency path of one plane: bands, their check, and the pool path for the frames that fail it (its launches
// exit at once otherwise).
static int banded_plane(const GroupLaunch& g, int p, sn::PlaneArgs a, sn::PoolArgs pool)
{
    Context* c = g.c;
    const int B = c->cfg.bytes_per_sample;
    sn::FusedPool fp{};
    fp.mode = sn::v3c::kPlain;  // in bands
    set_bands(c, fp, g.nbands, a.h_out / 2 - 1, g.slot0, true);
    SN_HIP(c, sn::launch_sweep(g.st, B, a, c->threshold(p), g.n, &fp));
    SN_HIP(c, sn::launch_band_verify(g.st, fp.band_state, 64 * sn::sweep_waves(B, a.w), fp.nbands, g.n, fp.band_flags, c->band_fallbacks_dev, c->band_fallbacks));
    a.guard = fp.band_flags;
    pool.guard = fp.band_flags;
    // (no k_assemble: the kept lines the bands have copied are right whatever the check says)
    SN_HIP(c, sn::launch_pool_plane(g.st, a, pool, B, c->threshold(p), g.n, g.slot0));
    return SN_OK;
}

// Route: every plane in bands (the latency path) -- planes with pools of their own (isolated) or the shared pool.
static int run_banded_planes(GroupLaunch& g)
{
    Context* c = g.c;
    int rc = ensure_bands(c);
    if (rc == SN_OK && !c->isolated) rc = ensure_pool(c);
    if (rc != SN_OK) return rc;
    for (int p = 0; p < c->nplanes(); ++p) {
        SN_HIP(c, g.plane_in(p));
        if (!g.pa[p].enabled) {
            SN_HIP(c, sn::launch_assemble(g.st, g.pa[p], c->cfg.bytes_per_sample, g.n));
            SN_HIP(c, g.plane_out(p));
            continue;
        }
        if (c->isolated) {
            rc = ensure_pool(c, p);
            if (rc != SN_OK) return rc;
            const sn::PoolArgs& pool = c->plane_pool[p];
            if (c->fresh) SN_HIP(c, hipMemsetAsync(pool.base + (int64_t)g.slot0 * pool.slot_bytes, 0, (size_t)pool.slot_bytes * g.n, g.st));
        }
        rc = banded_plane(g, p, g.pa[p], c->isolated ? c->plane_pool[p] : c->pool);
        if (rc != SN_OK) return rc;
        SN_HIP(c, g.plane_out(p));
    }
    c->fused_frames += g.n;
    c->banded_frames += g.n;
    return SN_OK;
}

// Route: every plane on its own -- a whole-plane sweep (plain, padded or in column parts) or the pool path, over the
// plane's own pool (isolated) or the shared one.
static int run_planes(GroupLaunch& g)
{
    Context* c = g.c;
    const int B = c->cfg.bytes_per_sample;
    auto swept = [&](int p) { return g.fused[p] && (c->isolated ? c->plane_fused[p] : !c->fused420); };
    auto pool_of = [&](int p) {
        sn::PoolArgs pool = c->isolated ? c->plane_pool[p] : c->pool;
        if (!c->isolated) pool.rows = g.stop[p];
        return pool;
    };
    bool counted = false, shared_pool_path = false;
    for (int p = 0; p < c->nplanes(); ++p) {
        const sn::PlaneArgs& a = g.pa[p];
        if (swept(p)) {
            if (c->isolated && c->plane_padded[p]) {
                // the sweep covers the whole pool stride: costs are zero outside the plane, the box filter clamps
                // at the end of the stride (SangNom2.cpp:144-150)
                sn::FusedPool fp{};
                fp.mode = sn::v3c::kPadded;
                fp.sweep_w = c->plane_pool[p].stride_e;
                SN_HIP(c, sn::launch_sweep(g.st, B, a, c->threshold(p), g.n, &fp));
            } else if (g.plan[p].n > 0) {
                const int rc = parts_plane(g, p, a, pool_of(p));
                if (rc != SN_OK) return rc;
                g.count_parts();
            } else {
                SN_HIP(c, sn::launch_sweep(g.st, B, a, c->threshold(p), g.n, nullptr));
            }
            if (!counted) c->fused_frames += g.n;
            counted = true;
            continue;
        }
        SN_HIP(c, sn::launch_assemble(g.st, a, B, g.n));
        if (!a.enabled) continue;
        if (!c->isolated) {  // after the loop, chunk by chunk
            shared_pool_path = true;
            continue;
        }
        const int rc = ensure_pool(c, p);
        if (rc != SN_OK) return rc;
        const sn::PoolArgs pool = pool_of(p);
        for (int i = 0; i < g.n; i += c->slots) {
            const int m = g.n - i < c->slots ? g.n - i : c->slots;
            if (c->fresh) SN_HIP(c, hipMemsetAsync(pool.base + (int64_t)g.slot0 * pool.slot_bytes, 0, (size_t)pool.slot_bytes * m, g.st));
            SN_HIP(c, sn::launch_pool_plane(g.st, frames_from(a, i), pool, B, c->threshold(p), m, g.slot0));
        }
    }
    if (!shared_pool_path) return SN_OK;
    // Pool path, a chunk of frames at a time on the chunk's slots; within a chunk the planes run in the
    // reference's order, because with subsampled chroma a frame's chroma result depends on what its own luma
    // pass left in the slot (SangNom2.cpp:322-329).
    const int rc = ensure_pool(c);
    if (rc != SN_OK) return rc;
    for (int i = 0; i < g.n; i += c->slots) {
        const int m = g.n - i < c->slots ? g.n - i : c->slots;
        for (int p = 0; p < c->nplanes(); ++p) {
            if (!g.pa[p].enabled || swept(p)) continue;
            SN_HIP(c, sn::launch_pool_plane(g.st, frames_from(g.pa[p], i), pool_of(p), B, c->threshold(p), m, g.slot0));
        }
    }
    return SN_OK;
}

// Route: a small launch of a 4:2:0 clip.  The luma plane in bands, leaving its smoothed rows where the pool path's luma
// pass would (the chroma sweeps of the coupling cannot be cut: sn_sweep_args.h); the luma plane of a frame that
// fails the check is redone by the pool kernels; then the chroma planes by the pool kernels.
static int run_coupled_banded(GroupLaunch& g)
{
    Context* c = g.c;
    hipStream_t st = g.st;
    const int n = g.n, slot0 = g.slot0;
    const sn::PlaneArgs* pa = g.pa;
    int rc = ensure_bands(c);
    if (rc == SN_OK) rc = ensure_pool(c);
    if (rc != SN_OK) return rc;
    const int B = c->cfg.bytes_per_sample;
    // Round 3: U and V as ONE chain of two passes per frame (k_smooth_*_chain; 8-bit: both in the same waves, V fifteen rows
    // behind U) on ring slots 3 f (luma's smoothed rows), 3 f + 1 (U), 3 f + 2 (V), instead of two stage-2 launches one after
    // the other: a 2160p YUV420P8 frame 0.617 -> 0.486 ms on the device, YUV420P16 0.73 -> 0.65.  Not for float samples: two
    // float passes on one CU take longer than one after the other (0.94 -> 1.11 ms).
    const bool chroma_chain = B != 4 && pa[1].enabled && pa[2].enabled && pa[1].w == pa[2].w && pa[1].h_out == pa[2].h_out && pa[1].w % 8 == 0 &&
                              ensure_chroma_chains(c, slot0, n, st);
    sn::PoolArgs ring = c->pool;
    if (chroma_chain) {
        ring.base = c->chain_base;
        ring.guard = nullptr;
        ring.rows = 0;
        ring.slot_step = 3;
        ring.slot_mod = c->chain_slots;
    }
    sn::FusedPool fp{};
    fp.mode = sn::v3c::kLumaSpill;
    fp.sweep_w = c->cfg.width;
    fp.pool_out = chroma_chain ? c->chain_base + (int64_t)3 * slot0 * c->pool.slot_bytes : c->pool.base + (int64_t)slot0 * c->pool.slot_bytes;
    fp.frame_stride = chroma_chain ? 3 * c->pool.slot_bytes : c->pool.slot_bytes;
    fp.pool_rows = c->bh + 1;
    fp.pool_row_bytes = c->stride_e * B;
    fp.rows_out = g.stop[1] < c->bh - 1 ? g.stop[1] : c->bh - 1;  // what U's stage 2 reads: rows up to the one it stops at
    fp.cone_nr = 1 << 20;  // every column is kept
    set_bands(c, fp, g.nbands, pa[0].h_out / 2 - 1, slot0, true);
    SN_HIP(c, g.plane_in(0));
    SN_HIP(c, sn::launch_sweep(st, B, pa[0], c->threshold(0), n, &fp));
    SN_HIP(c, sn::launch_band_verify(st, fp.band_state, band_threads(c), fp.nbands, n, fp.band_flags, c->band_fallbacks_dev, c->band_fallbacks));
    sn::PlaneArgs a = pa[0];
    a.guard = fp.band_flags;
    sn::PoolArgs pool = chroma_chain ? ring : c->pool;
    pool.guard = fp.band_flags;
    pool.rows = g.stop[0];
    SN_HIP(c, sn::launch_pool_plane(st, a, pool, B, c->threshold(0), n, chroma_chain ? 3 * slot0 : slot0));  // (kept lines: already copied by the bands)
    SN_HIP(c, g.plane_out(0));
    if (chroma_chain) {
        sn::ChainArgs ch{};
        ch.npass = 2;
        ch.pn = 2;
        ch.origin = 3 * slot0;
        ch.rows = g.stop[1] > g.stop[2] ? g.stop[1] : g.stop[2];
        ch.nchains = n;
        ch.chain_step = 3;
        for (int p = 1; p < 3; ++p) {
            ch.w[p - 1] = pa[p].w;
            ch.nr[p - 1] = pa[p].h_out / 2 - 1;
            SN_HIP(c, g.plane_in(p));
            SN_HIP(c, sn::launch_assemble(st, pa[p], B, n));
            SN_HIP(c, sn::launch_pool_prepare(st, pa[p], ring, B, n, 3 * slot0 + p));
        }
        SN_HIP(c, sn::launch_pool_chain(st, ring, ch, B));
        for (int p = 1; p < 3; ++p) {
            SN_HIP(c, sn::launch_pool_finalize(st, pa[p], ring, B, c->threshold(p), n, 3 * slot0 + p));
            SN_HIP(c, g.plane_out(p));
        }
    } else {
        for (int p = 1; p < 3; ++p) {
            pool = c->pool;
            pool.rows = g.stop[p];
            SN_HIP(c, g.plane_in(p));
            SN_HIP(c, sn::launch_assemble(st, pa[p], B, n));
            SN_HIP(c, sn::launch_pool_plane(st, pa[p], pool, B, c->threshold(p), n, slot0));
            SN_HIP(c, g.plane_out(p));
        }
    }
    c->fused_frames += n;  // (luma through the sweeps; banded_frames counts a subset of fused_frames, sangnom_hip.h)
    c->banded_frames += n;
    return SN_OK;
}

// Route: fused 4:2:0.  The luma sweep leaves its smoothed rows in hand-off pool 0, U reads pool 0 and leaves pool 1,
// V reads pool 1 -- so the three sweeps of a chunk of frames run back to back on that chunk's pools.
static int run_coupled(GroupLaunch& g)
{
    Context* c = g.c;
    const int n = g.n, slot0 = g.slot0;
    const sn::PlaneArgs* pa = g.pa;
    const int nr_c = c->plane_h_out(1) / 2 - 1;
    const int reach = c->fpool_rows - 1;
    const int sweep_u = sn::coupled_sweep_u(nr_c, c->bh);
    // 8-bit: U and V as ONE sweep (sn_fused_u8_uv.hip) -- only the luma -> U hand-off goes through a pool
    const bool one_chroma_sweep = c->uv_geometry && c->policy.chroma_sweeps == 0 && pa[1].enabled && pa[2].enabled && pa[1].h_in == pa[2].h_in;
    if (!one_chroma_sweep) {
        const int rc2 = ensure_fpool(c, 1);
        if (rc2 != SN_OK) return rc2;
    }
    for (int i = 0; i < n; i += c->fslots) {
        const int m = n - i < c->fslots ? n - i : c->fslots;
        for (int p = 0; p < 3; ++p) {
            sn::FusedPool fp{};
            fp.sweep_w = c->cfg.width;
            fp.frame_stride = c->fpool_frame_bytes;
            fp.pool_rows = c->fpool_rows;
            fp.cone_w = c->plane_w(1);  // the hand-off's dependency cone (sn_sweep_args.h, Args)
            fp.cone_nr = nr_c;
            fp.cone_in = p == 1 ? 6 : 0;
            fp.cone_out = p == 0 ? 6 : 0;
            if (p == 0) {
                fp.mode = sn::v3c::kLumaSpill;
                fp.pool_out = c->fpool[0] + (int64_t)slot0 * c->fpool_frame_bytes;
                fp.rows_out = reach;
            } else {
                fp.mode = sn::v3c::kChroma;
                fp.pool_in = c->fpool[p - 1] + (int64_t)slot0 * c->fpool_frame_bytes;
                fp.pool_out = p == 1 ? c->fpool[1] + (int64_t)slot0 * c->fpool_frame_bytes : nullptr;
                fp.rows_in = p == 1 ? reach : sweep_u;
                fp.sweep_rows = p == 1 ? sweep_u : nr_c;
                fp.rows_out = p == 1 ? sweep_u : 0;
            }
            const sn::PlaneArgs a = frames_from(pa[p], i);
            if (p == 1 && one_chroma_sweep) {
                SN_HIP(c, sn::launch_fused_u8_uv(g.st, a, frames_from(pa[2], i), c->threshold(1), c->threshold(2), m, fp));
                break;
            }
            SN_HIP(c, sn::launch_sweep(g.st, c->cfg.bytes_per_sample, a, c->threshold(p), m, &fp));
        }
    }
    if (one_chroma_sweep) c->uv_frames += n;
    c->fused_frames += n;
    return SN_OK;
}

// Runs frames [f0, f0 + n) of a strided batch with one common field offset.
// `st` is the stream to launch on and `slot0` the first scratch slot the frames may use (the batch entry points
// pass the context's stream and slot 0, the host ring one frame on its slot's stream and scratch).
// Builds the planes' arguments, decides what each plane goes through, and hands the launch to ONE route (run_* above).
static int run_group(Context* c, hipStream_t st, int slot0, int n, const void* const src[3], const int64_t sfs[3],
                     const int32_t sp[3], void* const dst[3], const int64_t dfs[3], const int32_t dp[3], int f0, int offset)
{
    GroupLaunch g;
    g.c = c;
    g.st = st;
    g.slot0 = slot0;
    g.n = n;
    sn::LaunchInput in;
    in.n = n;
    in.slot0 = slot0;
    for (int p = 0; p < c->nplanes(); ++p) {
        g.pa[p] = plane_args(c, p, src, sfs, sp, dst, dfs, dp, f0, offset);
        in.layout_ok[p] = sn::fused_layout_ok(g.pa[p]);
    }
    in.sweeps_always = sweeps_always(c);
    in.band_force = c->band_force;
    in.band_warm = c->band_warm;
    in.parts_force = c->parts_force;
    in.parts_ghost_force = c->parts_ghost_force;
    in.slots = c->slots;
    in.parts_slots = c->parts_slots;
    in.seam_record = c->parts_rec != nullptr;
    in.chroma_sweeps = c->policy.chroma_sweeps;
    // a launch that would be cut asks the pause of its kind first (and no other launch does: the pauses count launches)
    const bool bands_paused = c->band_force == 0 && c->band_fallbacks && sn::launch_bands(*c, in) > 0 && c->band_pause.paused(*c->band_fallbacks);
    sn::LaunchDecision d = sn::decide_launch(*c, in, bands_paused, false);
    if (d.parts_cut && c->parts_fallbacks && c->parts_pause.paused(*c->parts_fallbacks)) d = sn::decide_launch(*c, in, bands_paused, true);
    for (int p = 0; p < 3; ++p) {
        g.fused[p] = d.fused[p];
        g.plan[p] = d.plan[p];
        g.stop[p] = d.stop[p];
    }
    g.nbands = d.nbands;
    if (g.nbands == 0)
        for (int p = 0; p < c->nplanes(); ++p) SN_HIP(c, g.plane_in(p));
    switch (d.route) {
    case sn::Route::kBandedPlanes: return run_banded_planes(g);
    case sn::Route::kCoupled: return run_coupled(g);
    case sn::Route::kCoupledBanded: return run_coupled_banded(g);
    default: return run_planes(g);
    }
}

// History-carrying clips, two passes or more of one field offset (several frames, or one frame with two or three processed
// planes): the reference's passes -- every processed plane of every
// frame, in order, each starting from the pool the pass before it left -- as ONE chain (sn_pool_kernels.hip,
// k_smooth_u8_chain): stage 1 of all passes into a slot each, one stage-2 launch that keeps several passes in
// flight, stage 3 of all passes.  The pool of slot 0 is where the chain starts and where its last pass's pool ends
// up, so frames that come one at a time (and the pool's readers) carry on from there.
constexpr size_t kChainFlagBytes = (size_t)sn::kBuffers * sn::kChainMaxGroups * 32 * sizeof(uint32_t);
// behind the round counters: [0] the fault word of the launch in flight (zeroed with the counters), [32] launches redone so far
constexpr size_t kChainFaultWord = kChainFlagBytes / sizeof(uint32_t), kChainRedoneWord = kChainFaultWord + 32;
constexpr size_t kChainFlagAlloc = kChainFlagBytes + 64 * sizeof(uint32_t);
#ifndef SN_CHAIN_DEFAULT_GROUPS
#define SN_CHAIN_DEFAULT_GROUPS 8
#endif
constexpr int kChainDefaultGroups = SN_CHAIN_DEFAULT_GROUPS;  // sn_policy.chain = 0
constexpr int kChainSlack = 2;  // rounds a workgroup's slots start later than lockstep with the workgroup before it would need

static int chain_planes(const Context* c, int planes[3])
{
    if (c->chain_slots < 0 || c->policy.chain < 0) return 0;
    if (const char* e = test_env("SN_CHAIN"))
        if (atoi(e) == 0) return 0;
    return sn::chain_planes(*c, sn::pool_chain_lanes(c->cfg.bytes_per_sample, c->stride_e), planes);
}

// The chain's ring of pool slots: one per pass in flight, sized for the launches this context can see (max_batch or the
// host ring's depth, at most an eighth of the scratch budget; a synchronous single-frame user gets 2 * pn + 1 slots).
static int ensure_chain(Context* c, int pn, hipStream_t st)
{
    if (c->chain_slots < 0) return SN_CHAIN_UNAVAILABLE;
    if (c->chain_base) return SN_OK;
    int64_t fit = scratch_budget(c) / 8 / c->pool.slot_bytes;  // passes per launch
    const int64_t want = (int64_t)(c->cfg.max_batch > c->host_depth ? c->cfg.max_batch : c->host_depth) * pn;
    fit = fit > want ? want : fit;
    fit = fit > 1536 ? 1536 : fit;
    const int64_t addressable = (int64_t)0xfffffffe / c->pool.slot_bytes - 1;  // the chain kernels address the ring with 32-bit offsets
    fit = fit > addressable ? addressable : fit;
    if (addressable < 2 * pn) {  // (a pool slot of more than 600 MB: no chain, the frame-by-frame path)
        c->chain_slots = -1;
        return SN_CHAIN_UNAVAILABLE;
    }
    if (fit < 2 * pn) fit = 2 * pn;
    c->chain_slots = (int)fit + 1;
    if (hipMalloc(reinterpret_cast<void**>(&c->chain_base), (size_t)c->pool.slot_bytes * c->chain_slots) != hipSuccess) {
        (void)hipGetLastError();  // no room for the ring: this context keeps the frame-by-frame path
        c->chain_base = nullptr;
        c->chain_slots = -1;
        return SN_CHAIN_UNAVAILABLE;
    }
    // the round counters and the status word of chains over several workgroups: without them the ring is no use (all or nothing)
    if (hipMalloc(reinterpret_cast<void**>(&c->chain_flags), kChainFlagAlloc) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&c->chain_status), sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        if (c->chain_flags) (void)hipFree(c->chain_flags);
        (void)hipFree(c->chain_base);
        c->chain_flags = nullptr;
        c->chain_status = nullptr;
        c->chain_base = nullptr;
        c->chain_slots = -1;
        return SN_CHAIN_UNAVAILABLE;
    }
    *c->chain_status = 0;
    SN_HIP(c, hipMemsetAsync(c->chain_flags, 0, kChainFlagAlloc, st));
    SN_HIP(c, hipMemsetAsync(c->chain_base, 0, (size_t)c->pool.slot_bytes * c->chain_slots, st));
    c->chain_origin = 0;
    return SN_OK;
}

// A workgroup of a chain over several workgroups that gives up waiting for the one before it (sn_pool_kernels.hip, ChainSync:
// it was never scheduled next to its neighbour -- e.g. another context's sweep holds every CU slot, the reference's
// MT_MULTI_INSTANCE model, src/SangNom2.h:63-66) raises the launch's fault word.  Round 3 turned that into a sticky error
// after wrong frames had been delivered.  Now every such launch is followed by its own guarded redo (run_chain): stage 1 of
// all passes again and the chain on ONE workgroup per buffer, which waits for nobody; they exit at once unless the word is
// up.  The count of redone launches travels to sn_info.chain_redone.

// Workgroups per buffer for a chain of npass passes.  A short chain -- a single frame's two or three passes, two frames --
// stays on one workgroup, where a pass follows its predecessor without a trip through memory: 720x480 YUV420P8, one frame
// 0.168 ms against 0.193 with eight workgroups per buffer, two frames 0.188 either way, three 0.267 against 0.251, sixteen
// 0.761 against 0.577 (16-bit and float alike: tools/chain_small_groups.sh).  An explicit sn_policy.chain is taken as it is.
static int chain_groups(const Context* c, int npass)
{
    int want = c->policy.chain > 0 ? c->policy.chain : kChainDefaultGroups;
    if (const char* e = test_env("SN_CHAIN_GROUPS")) want = atoi(e);
    else if (c->policy.chain == 0 && npass < 9) want = 1;
    return c->chain_flags ? sn::pool_chain_groups(c->cfg.bytes_per_sample, c->stride_e, want) : 1;
}

static int run_chain(Context* c, hipStream_t st, int n, const void* const src[3], const int64_t sfs[3], const int32_t sp[3],
                     void* const dst[3], const int64_t dfs[3], const int32_t dp[3], int f0, int offset, const int planes[3], int pn)
{
    if (c->chain_slots < 0) return SN_CHAIN_UNAVAILABLE;
    int rc = ensure_pool(c);
    if (rc != SN_OK) return rc;
    const int B = c->cfg.bytes_per_sample;
    rc = ensure_chain(c, pn, st);  // (the host-facing entry points have done this before queueing their copies)
    if (rc != SN_OK) return rc;
    sn::PlaneArgs pa[3];
    for (int p = 0; p < c->nplanes(); ++p) {
        if (c->gate.on && !c->gate.waited[p]) {  // sn_process_host's plane pipeline: the chain needs every plane's copy
            c->gate.waited[p] = true;
            SN_HIP(c, hipStreamWaitEvent(st, c->gate.arrived[p], 0));
        }
        pa[p] = plane_args(c, p, src, sfs, sp, dst, dfs, dp, f0, offset);
        SN_HIP(c, sn::launch_assemble(st, pa[p], B, n));
    }
    sn::PoolArgs ring = c->pool;
    ring.base = c->chain_base;
    ring.rows = 0;
    ring.guard = nullptr;
    ring.slot_step = pn;
    ring.slot_mod = c->chain_slots;
    const int per_launch = (c->chain_slots - 1) / pn;  // frames
    for (int i = 0; i < n; i += per_launch) {
        const int m = n - i < per_launch ? n - i : per_launch;
        uint8_t* first = c->chain_base + (int64_t)c->chain_origin * c->pool.slot_bytes;
        SN_HIP(c, hipMemcpyAsync(first, c->pool.base, (size_t)c->pool.slot_bytes, hipMemcpyDeviceToDevice, st));
        sn::ChainArgs ch{};
        ch.npass = m * pn;
        ch.pn = pn;
        ch.origin = c->chain_origin;
        ch.groups = chain_groups(c, ch.npass);
        uint32_t* const fault = c->chain_flags ? c->chain_flags + kChainFaultWord : nullptr;
        if (ch.groups > 1) {
            ch.slack = kChainSlack;
            ch.flags = c->chain_flags;
            ch.status = fault;
            SN_HIP(c, hipMemsetAsync(c->chain_flags, 0, kChainFlagBytes + sizeof(uint32_t), st));  // round counters and the fault word
            if (c->chain_force_fault) {  // test hook: as if the launch timed out at once
                SN_HIP(c, hipMemsetAsync(fault, 1, 1, st));
                c->chain_force_fault = false;
            }
        }
        for (int k = 0; k < pn; ++k) {
            sn::PlaneArgs a = frames_from(pa[planes[k]], i);
            ch.w[k] = a.w;
            ch.nr[k] = a.h_out / 2 - 1;
            SN_HIP(c, sn::launch_pool_prepare(st, a, ring, B, m, (c->chain_origin + 1 + k) % c->chain_slots));
        }
        SN_HIP(c, sn::launch_pool_chain(st, ring, ch, B));
        if (ch.groups > 1) {
            // the guarded redo (see the comment above chain_groups): the costs again -- stage 2 has smoothed them in place -- and the chain on one
            // workgroup per buffer; every cell a pass's slot holds is rewritten by one of the two, the slot the chain starts
            // from (the copy of the pool before this launch) is only ever read
            sn::PoolArgs guarded = ring;
            guarded.guard = reinterpret_cast<const int32_t*>(fault);
            guarded.guard_single = 1;
            for (int k = 0; k < pn; ++k) {
                sn::PlaneArgs a = frames_from(pa[planes[k]], i);
                a.guard = reinterpret_cast<const int32_t*>(fault);
                a.guard_single = 1;
                SN_HIP(c, sn::launch_pool_prepare(st, a, guarded, B, m, (c->chain_origin + 1 + k) % c->chain_slots));
            }
            sn::ChainArgs again = ch;
            again.groups = 1;
            again.slack = 0;
            again.flags = nullptr;
            again.status = nullptr;
            again.only_if = fault;
            SN_HIP(c, sn::launch_pool_chain(st, ring, again, B));
            SN_HIP(c, sn::launch_chain_redo_count(st, fault, c->chain_flags + kChainRedoneWord, c->chain_status));
        }
        for (int k = 0; k < pn; ++k) {
            sn::PlaneArgs a = frames_from(pa[planes[k]], i);
            SN_HIP(c, sn::launch_pool_finalize(st, a, ring, B, c->threshold(planes[k]), m, (c->chain_origin + 1 + k) % c->chain_slots));
        }
        c->chain_origin = (c->chain_origin + ch.npass) % c->chain_slots;
        const uint8_t* last = c->chain_base + (int64_t)c->chain_origin * c->pool.slot_bytes;
        SN_HIP(c, hipMemcpyAsync(c->pool.base, last, (size_t)c->pool.slot_bytes, hipMemcpyDeviceToDevice, st));
    }
    c->chained_frames += n;
    return SN_OK;
}

// Splits a batch into runs of equal field offset; history-carrying configurations run one frame at a time on
// pool slot 0, exactly like one reference instance -- or, several frames of one offset, as a chain (run_chain).
static int run_batch(Context* c, hipStream_t st, int slot0, int nframes, const void* const src[3], const int64_t sfs[3],
                     const int32_t sp[3], void* const dst[3], const int64_t dfs[3], const int32_t dp[3], const int32_t* parity)
{
    int f = 0;
    int planes[3] = {0, 0, 0};
    const int pn = slot0 == 0 ? chain_planes(c, planes) : 0;
    while (f < nframes) {
        const sn::FieldRun run = sn::field_run(parity, f, nframes, [c](int par) { return sn::field_offset(c->cfg.order, par); }, c->history_free || pn);
        const int off = run.offset;
        int g = run.end;
        // (a single frame with two or three processed planes is a chain too: its passes follow each other rows apart)
        int rc = !c->history_free && (g - f) * pn > 1 ? run_chain(c, st, g - f, src, sfs, sp, dst, dfs, dp, f, off, planes, pn)
                                               : run_group(c, st, slot0, g - f, src, sfs, sp, dst, dfs, dp, f, off);
        if (rc == SN_CHAIN_UNAVAILABLE) {  // nothing was queued yet: this frame and the rest one at a time
            g = f + 1;
            rc = run_group(c, st, slot0, 1, src, sfs, sp, dst, dfs, dp, f, off);
        }
        if (rc != SN_OK) return rc;
        f = g;
    }
    c->frames += nframes;
    return SN_OK;
}

int sn_process_device_strided(sn_context* h, int32_t nframes, const void* const src[3],
                              const int64_t sfs[3], const int32_t sp[3], void* const dst[3],
                              const int64_t dfs[3], const int32_t dp[3], const int32_t* parity)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    if (nframes < 0 || nframes > c->cfg.max_batch)
        return sn::fail(c, SN_ERR_INVALID_ARG, "nframes %d outside 0..max_batch (%d)", nframes, c->cfg.max_batch);
    if (!sfs || !dfs) return sn::fail(c, SN_ERR_INVALID_ARG, "frame stride array is NULL");
    int rc = check_planes(c, src, sp, dst, dp);
    if (rc != SN_OK) return rc;
    if (nframes == 0) return SN_OK;
    SN_HIP(c, hipSetDevice(c->device));

    return run_batch(c, c->stream, 0, nframes, src, sfs, sp, dst, dfs, dp, parity);
}

int sn_process_device(sn_context* h, const void* const src[3], const int32_t sp[3], void* const dst[3],
                      const int32_t dp[3], int32_t parity)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    const int64_t zero[3] = {0, 0, 0};
    return sn_process_device_strided(h, 1, src, zero, sp, dst, zero, dp, &parity);
}

// -- decoder and encoder surfaces (sn_surfaces) -------------------------------------------------------------------------
// What both surface calls share: the checks of a surface description, the scratch, and the walk over a batch in chunks of what
// the scratch holds -- split (and shift down), the call's passes on planar LSB-aligned planes, merge (and shift up).

struct SurfaceGeometry {  // of the call that walks: the batch call's clip, or the anti-aliasing call's (dh: output twice as wide and high)
    int B = 1, bits = 8, planes = 1, max_batch = 1, sub_w = 0, sub_h = 0;
    int w_in[3] = {0, 0, 0}, h_in[3] = {0, 0, 0}, w_out[3] = {0, 0, 0}, h_out[3] = {0, 0, 0};
    bool luma_processed = true, chroma_processed = true;
    bool all_lines = true;  // the passes read every line of the source's planes (dh; the anti-aliasing call's turns)
};

struct SurfaceSide {  // a checked sn_surfaces
    bool semi = false;
    int packing = 0;  // sn::Packing: plane[0] holds Y, U and V (SN_LAYOUT_PACKED_*)
    int shift = 0;  // SN_LAYOUT_*_MSB: 16 - bits_per_sample, the zero bits below every sample (0: the layout without _MSB)
    uint8_t* p[3] = {nullptr, nullptr, nullptr};
    int32_t pitch[3] = {0, 0, 0};
    int64_t fs[3] = {0, 0, 0};
    sn::PlaneViewW view(int q) const { return sn::PlaneViewW{p[q], fs[q], pitch[q]}; }
    sn::PlanSide plan_side() const { return sn::PlanSide{semi, packing, shift}; }
};

// the description on its own: SN_OK, or the code and the text that names the field
static int surface_header(const char* name, const sn_surfaces* s, std::string& msg)
{
    if (!s) return msg = std::string(name) + " is NULL", SN_ERR_INVALID_ARG;
    if (s->struct_size != (int32_t)sizeof(sn_surfaces)) return msg = std::string(name) + ": sn_surfaces.struct_size mismatch", SN_ERR_INVALID_ARG;
    if (!sn::surface_layout(s->layout).valid)
        return msg = std::string(name) + ": sn_surfaces.layout must be SN_LAYOUT_PLANAR, SN_LAYOUT_SEMIPLANAR, one of their _MSB forms or SN_LAYOUT_PACKED_*",
               SN_ERR_INVALID_ARG;
    if (s->reserved != 0) return msg = std::string(name) + ": sn_surfaces.reserved must be zero", SN_ERR_INVALID_ARG;
    return SN_OK;
}

static bool surface_plain(const sn_surfaces* s) { return s->layout == SN_LAYOUT_PLANAR; }

// ... against the planes it has to hold: w[p] samples per row of plane p (the UV plane: 2 w[1]; a packed plane: sn_surface_layout.h)
static int surface_side(const char* name, const sn_surfaces* s, const int w[3], const SurfaceGeometry& g, SurfaceSide& out, std::string& msg)
{
    const std::string n(name);
    const sn::SurfaceLayout L = sn::surface_layout(s->layout);
    const int B = g.B;
    if (const char* why = sn::surface_refusal(L, g.planes, g.sub_w, g.sub_h, B, g.bits)) return msg = n + ": " + why, SN_ERR_UNSUPPORTED;
    out.semi = L.semi;
    out.packing = L.packing;
    out.shift = sn::surface_shift(L, g.bits);
    for (int p = sn::surface_null_from(L); p < 3; ++p)
        if (s->plane[p])
            return msg = n + ": sn_surfaces.plane[" + std::to_string(p) + "] must be NULL with " +
                         (L.packing ? "SN_LAYOUT_PACKED_* (plane[0] is the whole surface)" : "SN_LAYOUT_SEMIPLANAR (plane[1] is the UV plane)"),
                   SN_ERR_INVALID_ARG;
    const int np = sn::surface_planes(L, g.planes), unit = sn::surface_align(L, B);
    for (int p = 0; p < np; ++p) {
        const int64_t row = sn::surface_row_bytes(L, p, w[0], w[1], B);
        const std::string ps = std::to_string(p);
        if (!s->plane[p]) return msg = n + ": sn_surfaces.plane[" + ps + "] is NULL", SN_ERR_INVALID_ARG;
        if (s->pitch[p] < row)
            return msg = n + ": sn_surfaces.pitch[" + ps + "] " + std::to_string(s->pitch[p]) + " smaller than the row size " + std::to_string(row), SN_ERR_INVALID_ARG;
        if (s->pitch[p] % unit || s->frame_stride[p] % unit || (uintptr_t)s->plane[p] % unit)
            return msg = n + ": sn_surfaces plane[" + ps + "] / pitch[" + ps + "] / frame_stride not aligned to " +
                         (unit == B ? std::string("the sample size") : std::to_string(unit) + " bytes"),
                   SN_ERR_INVALID_ARG;
        out.p[p] = static_cast<uint8_t*>(s->plane[p]);
        out.pitch[p] = s->pitch[p];
        out.fs[p] = s->frame_stride[p];
    }
    return SN_OK;
}

static sn::SurfacePlan surface_plan_of(const SurfaceGeometry& g, const SurfaceSide& src, const SurfaceSide& dst)
{
    return sn::surface_plan(src.plan_side(), dst.plan_side(), g.planes, g.luma_processed, g.chroma_processed, g.all_lines);
}

static void surface_scratch_free(sn::UvScratch& S)
{
    for (sn::PlaneViewW* q : {&S.in[0], &S.in[1], &S.out[0], &S.out[1], &S.y, &S.yo}) {
        if (q->base) (void)hipFree(q->base);
        *q = sn::PlaneViewW{};
    }
    S.cap = 0;
    S.bytes = 0;
}

// The scratch, once per part: for min(max_batch, what a sixteenth of the budget holds, at least 1) frames (sangnom_hip.h).
// `need` is the plan's (sn_surface_plan.h; sangnom_hip.h has the table).  Allocated before anything of the call is queued; the
// stream is drained so that whichever stream comes first finds it filled.  A context that holds some parts and now needs another
// gives back what it holds and takes the union, so that the sum obeys the rule; calls without an MSB-aligned source or a packed
// side never ask for luma and allocate what they always did.
static hipError_t surface_scratch(sn::UvScratch& S, hipStream_t st, const SurfaceGeometry& g, int64_t budget, sn::SurfaceNeeds need)
{
    if ((!need.in || S.in[0].base) && (!need.out || S.out[0].base) && (!need.y || S.y.base) && (!need.yo || S.yo.base)) return hipSuccess;
    need.in = need.in || S.in[0].base;
    need.out = need.out || S.out[0].base;
    need.y = need.y || S.y.base;
    need.yo = need.yo || S.yo.base;
    hipError_t e = hipStreamSynchronize(st);  // (what an earlier call queued may still read the part that goes)
    if (e != hipSuccess) return e;
    surface_scratch_free(S);
    // one frame of a part: w samples a row, the pitch rounded up to 256 bytes
    auto part = [&](int w, int h) {
        const int32_t pitch = (w * g.B + 255) & ~255;
        return sn::PlaneViewW{nullptr, (int64_t)pitch * h, pitch};
    };
    const sn::PlaneViewW in = part(g.w_in[1], g.h_in[1]), out = part(g.w_out[1], g.h_out[1]), y = part(g.w_in[0], g.h_in[0]), yo = part(g.w_out[0], g.h_out[0]);
    const int64_t per_frame = (need.in ? 2 * in.fs : 0) + (need.out ? 2 * out.fs : 0) + (need.y ? y.fs : 0) + (need.yo ? yo.fs : 0);
    const int64_t fit = budget / 16 / per_frame;
    const int cap = (int)(fit < 1 ? 1 : fit < g.max_batch ? fit : g.max_batch);
    // a split writes only the lines its pass keeps: a pass that read another line of a source part would read the 0xA5 pattern
    auto take = [&](sn::PlaneViewW& q, const sn::PlaneViewW& shape, bool fill) {
        q = shape;
        e = hipMalloc(reinterpret_cast<void**>(&q.base), (size_t)q.fs * cap);
        if (e == hipSuccess && fill) e = hipMemsetAsync(q.base, 0xA5, (size_t)q.fs * cap, st);
    };
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        if (need.in) take(S.in[k], in, true);
        if (need.out && e == hipSuccess) take(S.out[k], out, false);
    }
    if (need.y && e == hipSuccess) take(S.y, y, true);
    if (need.yo && e == hipSuccess) take(S.yo, yo, false);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        surface_scratch_free(S);
        return e;
    }
    S.cap = cap;
    S.bytes = per_frame * cap;
    return hipSuccess;
}

struct SurfacePasses {  // the call's passes on planar planes: `m` frames, the views at the first of them
    void* self;
    int (*run)(void* self, int m, const sn::PlaneView s[3], const sn::PlaneViewW d[3], const int32_t* parity);
    int (*offset)(void* self, int parity);  // the field offset of a frame (unless all_lines)
};

// Executes a plan (sn_surface_plan.h, which decides every launch): the planes that go from source to destination once, then
// per chunk of what the scratch holds the source as planar LSB-aligned planes, the call's passes on them, and the destination
// finished from where the passes -- or, for a plane that is not processed, the source's planar form -- left each plane.
// MSB-aligned sides (shift ss of the source, ds of the destination): the passes see LSB-aligned planes; samples are shifted down
// on their way in and up on their way out, or where the passes wrote them.
// A HIP error of the walk itself comes back as SN_ERR_HIP with its text in msg; an error of the passes leaves msg empty (the
// context holds the text).
static int surface_walk(sn::UvScratch& S, hipStream_t st, const SurfaceGeometry& g, const sn::SurfacePlan& P, int n, const SurfaceSide& src,
                        const SurfaceSide& dst, const int32_t* parity, const SurfacePasses& passes, std::string& msg)
{
#define SN_UV_HIP(call)                                                      \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if (e_ != hipSuccess) {                                              \
            msg = std::string(#call " failed: ") + hipGetErrorString(e_);    \
            return SN_ERR_HIP;                                               \
        }                                                                    \
    } while (0)
    using View = sn::PlaneViewW;
    const int B = g.B;
    // one step of the plan: m frames from `from` to `to` (the step's stage says which planes those are), planes of w x h
    auto step = [&](const sn::PlanStep& s, const View from[3], const View to[3], int m, const int w[3], const int h[3], int lines, int ss, int ds) -> int {
        const int p = s.plane, pw = s.uv_row ? 2 * w[p] : w[p];
        switch (s.op) {
        case sn::kOpShift16: SN_UV_HIP(sn::launch_shift16(st, m, from[p], pw, h[p], to[p], lines, ss, ds)); break;
        case sn::kOpUvSplit: SN_UV_HIP(sn::launch_uv_split(st, B, m, from[1], w[1], h[1], to[1], to[2], lines, ss, ds)); break;
        case sn::kOpUvMerge: SN_UV_HIP(sn::launch_uv_merge(st, B, m, from[1], from[2], w[1], h[1], to[1], ss, ds)); break;
        case sn::kOpUnpack: SN_UV_HIP(sn::launch_unpack(st, src.packing, B, m, from[0], w[0], h[0], to[0], to[1], to[2], lines, ss)); break;
        case sn::kOpPack: SN_UV_HIP(sn::launch_pack(st, dst.packing, B, m, from[0], from[1], from[2], w[0], h[0], to[0], ds)); break;
        default:
            if (s.op == sn::kOpCopyOrShift16 && B == 2) {
                SN_UV_HIP(sn::launch_shift16(st, m, from[p], pw, h[p], to[p], lines, ss, ds));
                break;
            }
            for (int f = 0; f < m; ++f)
                SN_UV_HIP(hipMemcpy2DAsync(to[p].at(f).base, (size_t)to[p].pitch, from[p].at(f).base, (size_t)from[p].pitch, (size_t)pw * B, (size_t)h[p],
                                           hipMemcpyDeviceToDevice, st));
        }
        return SN_OK;
    };
    // a plane of the plan at frame f0 of the call: scratch holds the chunk, so its frame 0 is frame f0
    auto at = [&](const sn::PlaneRef& r, int64_t f0) -> View {
        switch (r.buf) {
        case sn::kBufIn: return S.in[r.idx];
        case sn::kBufOut: return S.out[r.idx];
        case sn::kBufY: return S.y;
        case sn::kBufYo: return S.yo;
        case sn::kBufDst: return dst.view(r.idx).at(f0);
        default: return src.view(r.idx).at(f0);
        }
    };
    const int ss = src.shift, ds = dst.shift;
    const View sv[3] = {src.view(0), src.view(1), src.view(2)}, dv[3] = {dst.view(0), dst.view(1), dst.view(2)};
    for (int i = 0; i < P.nonce; ++i)
        if (int rc = step(P.once[i], sv, dv, n, g.w_in, g.h_in, -1, ss, ds)) return rc;
    if (P.count_copied == sn::kCountPerCall) S.copied_frames += n;
    const int cap = P.chunked ? S.cap : n;
    for (int f0 = 0; f0 < n; f0 += cap) {
        const int m = n - f0 < cap ? n - f0 : cap;
        const int32_t* par = parity ? parity + f0 : nullptr;
        View rd[3], wr[3], res[3], sf[3], df[3], to[3];
        for (int p = 0; p < 3; ++p) rd[p] = at(P.read[p], f0), wr[p] = at(P.write[p], f0), res[p] = at(P.result[p], f0), df[p] = dv[p].at(f0);
        // the source: the lines the passes keep, one launch per run of frames with the same field offset (field_run, as run_batch
        // cuts them), or every line and the chunk in one run
        for (int g0 = 0; g0 < m && P.nsource;) {
            sn::FieldRun run{m, -1};
            if (!P.source_all_lines) run = sn::field_run(par, g0, m, [&](int parity_of_frame) { return passes.offset(passes.self, parity_of_frame); });
            for (int p = 0; p < 3; ++p) sf[p] = sv[p].at(f0 + g0), to[p] = rd[p].at(g0);
            for (int i = 0; i < P.nsource; ++i)
                if (int rc = step(P.source[i], sf, to, run.end - g0, g.w_in, g.h_in, run.offset, ss, 0)) return rc;
            g0 = run.end;
        }
        if (P.count_split == sn::kCountPerChunk) S.split_frames += m;
        const sn::PlaneView rdc[3] = {rd[0], rd[1], rd[2]};
        if (int rc = passes.run(passes.self, m, rdc, wr, par)) return rc;
        for (int i = 0; i < P.nafter; ++i)
            if (int rc = step(P.after[i], res, df, m, g.w_out, g.h_out, -1, 0, ds)) return rc;
        if (P.count_merged == sn::kCountPerChunk) S.merged_frames += m;
        if (P.count_copied == sn::kCountPerChunk) S.copied_frames += m;
    }
    return SN_OK;
#undef SN_UV_HIP
}


static int surface_info(const sn::UvScratch& S, sn_surface_info* info)
{
    if (!info || info->struct_size != (int32_t)sizeof(sn_surface_info)) return SN_ERR_INVALID_ARG;
    info->reserved = 0;
    info->scratch_bytes = S.bytes;
    info->split_frames = S.split_frames;
    info->merged_frames = S.merged_frames;
    info->copied_frames = S.copied_frames;
    return SN_OK;
}

static int sn_surface_offset(void* self, int parity) { return sn::field_offset(static_cast<Context*>(self)->cfg.order, parity); }

// plane views as the arrays run_batch and the ABI take
struct PlaneArrays {
    const void* s[3];
    void* d[3];
    int64_t sfs[3], dfs[3];
    int32_t sp[3], dp[3];
    PlaneArrays(const sn::PlaneView sv[3], const sn::PlaneViewW dv[3])
    {
        for (int p = 0; p < 3; ++p) {
            s[p] = sv[p].base, sfs[p] = sv[p].fs, sp[p] = sv[p].pitch;
            d[p] = dv[p].base, dfs[p] = dv[p].fs, dp[p] = dv[p].pitch;
        }
    }
};

static int sn_surface_run(void* self, int m, const sn::PlaneView sv[3], const sn::PlaneViewW dv[3], const int32_t* parity)
{
    Context* c = static_cast<Context*>(self);
    const PlaneArrays a(sv, dv);
    // chroma that is not processed has gone from src to dst already: launch_assemble leaves those planes alone
    // (PlaneArgs::copied_elsewhere) and copies a luma plane that is not processed either, as in the planar call
    c->chroma_elsewhere = !(c->cfg.dh || c->process[1]);
    const int rc = run_batch(c, c->stream, 0, m, a.s, a.sfs, a.sp, a.d, a.dfs, a.dp, parity);
    c->chroma_elsewhere = false;
    return rc;
}

int sn_process_device_surfaces(sn_context* h, int32_t nframes, const sn_surfaces* src, const sn_surfaces* dst, const int32_t* parity)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    std::string msg;
    int rc = surface_header("src", src, msg);
    if (rc == SN_OK) rc = surface_header("dst", dst, msg);
    if (rc != SN_OK) return sn::fail(c, rc, "%s", msg.c_str());
    if (surface_plain(src) && surface_plain(dst))  // the planar call itself
        return sn_process_device_strided(h, nframes, src->plane, src->frame_stride, src->pitch, dst->plane, dst->frame_stride, dst->pitch, parity);
    if (nframes < 0 || nframes > c->cfg.max_batch)
        return sn::fail(c, SN_ERR_INVALID_ARG, "nframes %d outside 0..max_batch (%d)", nframes, c->cfg.max_batch);
    SurfaceGeometry g;
    g.B = c->cfg.bytes_per_sample;
    g.bits = c->cfg.bits_per_sample;
    g.planes = c->nplanes();
    g.sub_w = c->cfg.sub_w, g.sub_h = c->cfg.sub_h;
    g.max_batch = c->cfg.max_batch;
    for (int p = 0; p < g.planes; ++p) g.w_in[p] = g.w_out[p] = c->plane_w(p), g.h_in[p] = c->plane_h_in(p), g.h_out[p] = c->plane_h_out(p);
    g.luma_processed = c->cfg.dh || c->process[0];
    g.chroma_processed = c->cfg.dh || c->process[1];
    g.all_lines = c->cfg.dh != 0;
    SurfaceSide ss, ds;
    rc = surface_side("src", src, g.w_in, g, ss, msg);
    if (rc == SN_OK) rc = surface_side("dst", dst, g.w_out, g, ds, msg);
    if (rc != SN_OK) return sn::fail(c, rc, "%s", msg.c_str());
    if (nframes == 0) return SN_OK;
    SN_HIP(c, hipSetDevice(c->device));
    const sn::SurfacePlan plan = surface_plan_of(g, ss, ds);
    SN_HIP(c, surface_scratch(c->uv, c->stream, g, scratch_budget(c), plan.need));
    const SurfacePasses passes{c, sn_surface_run, sn_surface_offset};
    c->luma_elsewhere = (ss.shift != 0 || ds.shift != 0 || ss.packing || ds.packing) && !g.luma_processed;
    rc = surface_walk(c->uv, c->stream, g, plan, nframes, ss, ds, parity, passes, msg);
    c->luma_elsewhere = false;
    if (rc != SN_OK && !msg.empty()) return sn::fail(c, rc, "%s", msg.c_str());
    return rc;
}

int sn_get_surface_info(sn_context* h, sn_surface_info* info)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    if (surface_info(c->uv, info) != SN_OK) return sn::fail(c, SN_ERR_INVALID_ARG, "info is NULL or sn_surface_info.struct_size mismatch");
    return SN_OK;
}

int sn_process_host(sn_context* h, const void* const src[3], const int32_t sp[3], void* const dst[3],
                    const int32_t dp[3], int32_t parity)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    int rc = check_planes(c, src, sp, dst, dp);
    if (rc != SN_OK) return rc;
    SN_HIP(c, hipSetDevice(c->device));
    rc = prepare_small_launch_scratch(c);
    if (rc != SN_OK) return rc;
    const int B = c->cfg.bytes_per_sample;
    for (int p = 0; p < c->nplanes(); ++p) {
        // every resource is checked on its own: a call that failed half-way (SN_HIP returns) leaves the rest to the next call
        c->stage_src_pitch[p] = (c->plane_w(p) * B + 255) & ~255;
        c->stage_dst_pitch[p] = c->stage_src_pitch[p];
        if (!c->stage_src[p])
            SN_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->stage_src[p]), (size_t)c->stage_src_pitch[p] * c->plane_h_in(p)));
        if (!c->stage_dst[p])
            SN_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->stage_dst[p]), (size_t)c->stage_dst_pitch[p] * c->plane_h_out(p)));
        if (!c->sync_in[p])
            SN_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&c->sync_in[p]), (size_t)c->stage_src_pitch[p] * c->plane_h_in(p), hipHostMallocDefault));
        if (!c->sync_out[p])
            SN_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&c->sync_out[p]), (size_t)c->stage_dst_pitch[p] * (c->plane_h_out(p) / 2 + 1), hipHostMallocDefault));
        for (int k = 0; k < kSyncChunks; ++k)
            if (!c->sync_back[p][k]) SN_HIP(c, hipEventCreateWithFlags(&c->sync_back[p][k], hipEventDisableTiming));
    }
    ensure_copier(c);
    // Several planes: the copies go on streams of their own, so that plane p + 1 arrives and plane p - 1 leaves while plane
    // p is in the kernels (a 2160p YUV420P8 call: 1.16 -> 0.9 ms).  One plane: everything in order on the context's stream.
    Context::PlaneGate& g = c->gate;
    const bool piped = c->nplanes() > 1;
    if (piped && !g.in) {
        SN_HIP(c, hipStreamCreateWithFlags(&g.in, hipStreamNonBlocking));
        SN_HIP(c, hipStreamCreateWithFlags(&g.out, hipStreamNonBlocking));
        for (int p = 0; p < 3; ++p) {
            SN_HIP(c, hipEventCreateWithFlags(&g.arrived[p], hipEventDisableTiming));
            SN_HIP(c, hipEventCreateWithFlags(&g.done[p], hipEventDisableTiming));
        }
    }
    for (int p = 0; p < c->nplanes(); ++p) {
        if (!(c->cfg.dh || c->process[p])) {  // a copied plane never visits the device: the host copies it (kept_line_jobs below)
            if (piped) SN_HIP(c, hipEventRecord(g.arrived[p], g.in));
            continue;
        }
        const KeptLines kl = sn::kept_lines(*c, p, parity);
        const uint8_t* from = static_cast<const uint8_t*>(src[p]) + (int64_t)kl.first * sp[p];
        size_t from_pitch = (size_t)kl.step * sp[p];
        if (!sn::plane_is_pinned(src[p], sp[p], c->plane_w(p) * B, c->plane_h_in(p))) {
            // A plane in pageable memory: the host's copy threads bring the lines that travel into the context's pinned
            // staging first (while the previous plane is on the link).  Rounds 1-2 handed the caller's pointer to
            // hipMemcpy2DAsync and left pinning or staging to the runtime; that path produced "DMA buffer failed"
            // fall-backs and, once in a few hundred calls in a long-lived process, a GPU access fault at an address of the
            // caller's heap (profiles/r3_page_fault.md).  A plane inside memory the caller pinned is DMA'd as it lies.
            // in a few chunks of rows, so that a chunk crosses PCIe while the threads copy the next one
            const int chunks = kl.rows >= 4 * kSyncChunks ? kSyncChunks : 1;
            for (int k = 0; k < chunks; ++k) {
                const int y0 = (int)((int64_t)kl.rows * k / chunks), y1 = (int)((int64_t)kl.rows * (k + 1) / chunks);
                const Copier::Job job = {c->sync_in[p] + (size_t)y0 * c->stage_src_pitch[p], from + (size_t)y0 * from_pitch, c->stage_src_pitch[p],
                                         (int)from_pitch, c->plane_w(p) * B, y1 - y0};
                c->copier->run(&job, 1);
                SN_HIP(c, hipMemcpy2DAsync(c->stage_src[p] + ((int64_t)kl.first + (int64_t)y0 * kl.step) * c->stage_src_pitch[p],
                                           (size_t)kl.step * c->stage_src_pitch[p], c->sync_in[p] + (size_t)y0 * c->stage_src_pitch[p],
                                           (size_t)c->stage_src_pitch[p], (size_t)c->plane_w(p) * B, y1 - y0, hipMemcpyHostToDevice,
                                           piped ? g.in : c->stream));
            }
        } else {
            SN_HIP(c, hipMemcpy2DAsync(c->stage_src[p] + (int64_t)kl.first * c->stage_src_pitch[p], (size_t)kl.step * c->stage_src_pitch[p],
                                       from, from_pitch, (size_t)c->plane_w(p) * B, kl.rows, hipMemcpyHostToDevice, piped ? g.in : c->stream));
        }
        if (piped) SN_HIP(c, hipEventRecord(g.arrived[p], g.in));
    }
    const void* dsrc[3] = {c->stage_src[0], c->stage_src[1], c->stage_src[2]};
    void* ddst[3] = {c->stage_dst[0], c->stage_dst[1], c->stage_dst[2]};
    if (piped) {
        g.on = true;
        for (int p = 0; p < 3; ++p) g.waited[p] = g.recorded[p] = false;
    }
    rc = sn_process_device(h, dsrc, c->stage_src_pitch, ddst, c->stage_dst_pitch, parity);
    g.on = false;
    if (rc != SN_OK) {
        if (piped) (void)hipStreamSynchronize(g.in);  // nothing of this call may still be reading the caller's planes
        return rc;
    }
    {   // while the device works: the output's kept lines, from the caller's source to the caller's destination
        Copier::Job jobs[6];
        int nj = 0;
        for (int p = 0; p < c->nplanes(); ++p) nj += kept_line_jobs(c, p, parity, src[p], sp[p], dst[p], dp[p], jobs + nj);
        ensure_copier(c);
        c->copier->run(jobs, nj);
    }
    bool staged_back[3] = {false, false, false};
    for (int p = 0; p < c->nplanes(); ++p) {
        if (piped) {
            if (!g.recorded[p]) SN_HIP(c, hipEventRecord(g.done[p], c->stream));  // a path that is not written plane by plane: all done here
            SN_HIP(c, hipStreamWaitEvent(g.out, g.done[p], 0));
        }
        // only the interpolated lines come back: offset + 1, offset + 3, ... (nr of them)
        const int off = sn::field_offset(c->cfg.order, parity), nr = c->plane_h_out(p) / 2 - 1;
        staged_back[p] = false;
        if ((c->cfg.dh || c->process[p]) && nr > 0) {
            hipStream_t so = piped ? g.out : c->stream;
            const uint8_t* from = c->stage_dst[p] + (int64_t)(off + 1) * c->stage_dst_pitch[p];
            if (!sn::plane_is_pinned(dst[p], dp[p], c->plane_w(p) * B, c->plane_h_out(p))) {  // pageable: through the pinned staging, in chunks
                staged_back[p] = true;
                const int chunks = nr >= 4 * kSyncChunks ? kSyncChunks : 1;
                for (int k = 0; k < chunks; ++k) {
                    const int y0 = (int)((int64_t)nr * k / chunks), y1 = (int)((int64_t)nr * (k + 1) / chunks);
                    SN_HIP(c, hipMemcpy2DAsync(c->sync_out[p] + (size_t)y0 * c->stage_dst_pitch[p], (size_t)c->stage_dst_pitch[p],
                                               from + (size_t)y0 * 2 * c->stage_dst_pitch[p], (size_t)2 * c->stage_dst_pitch[p],
                                               (size_t)c->plane_w(p) * B, y1 - y0, hipMemcpyDeviceToHost, so));
                    SN_HIP(c, hipEventRecord(c->sync_back[p][k], so));
                }
            } else {
                SN_HIP(c, hipMemcpy2DAsync(static_cast<uint8_t*>(dst[p]) + (int64_t)(off + 1) * dp[p], (size_t)2 * dp[p], from,
                                           (size_t)2 * c->stage_dst_pitch[p], (size_t)c->plane_w(p) * B, nr, hipMemcpyDeviceToHost, so));
            }
        }
    }
    for (int p = 0; p < c->nplanes(); ++p) {  // the staged planes: from the pinned staging into the caller's lines, chunk by chunk as they arrive
        if (!staged_back[p]) continue;
        const int off = sn::field_offset(c->cfg.order, parity), nr = c->plane_h_out(p) / 2 - 1;
        const int chunks = nr >= 4 * kSyncChunks ? kSyncChunks : 1;
        for (int k = 0; k < chunks; ++k) {
            const int y0 = (int)((int64_t)nr * k / chunks), y1 = (int)((int64_t)nr * (k + 1) / chunks);
            SN_HIP(c, hipEventSynchronize(c->sync_back[p][k]));
            const Copier::Job job = {static_cast<uint8_t*>(dst[p]) + (size_t)(off + 1 + 2 * y0) * dp[p], c->sync_out[p] + (size_t)y0 * c->stage_dst_pitch[p],
                                     2 * dp[p], c->stage_dst_pitch[p], c->plane_w(p) * B, y1 - y0};
            c->copier->run(&job, 1);
        }
    }
    if (piped) SN_HIP(c, hipStreamSynchronize(g.out));
    SN_HIP(c, hipStreamSynchronize(c->stream));
    // The copies on g.in are complete by now (the kernels waited for them), but the RUNTIME has to hear of it as well: a
    // stream that is never synchronised keeps its commands -- and with them the runtime's transient registration of the
    // caller's pageable planes -- alive after the call has returned and the caller has freed or recycled that memory.
    if (piped) SN_HIP(c, hipStreamSynchronize(g.in));
    return SN_OK;
}

// ---- the host ring: SURVEY 8(f)-1, pipelining behind GetFrame --------------------------------------------
// Frame slots with pinned staging and device copies of one source and one output frame each.  The slots form
// up to four groups; a group has a stream of its own, and when its slots are all staged (or one of them is
// collected early) ONE launch sweeps the group's frames: the runtime maps streams onto a handful of hardware
// queues (four by default), so one stream per frame would keep only four 5 ms sweeps in flight (870 frames/s
// at 2160p).  H2D of a frame is queued when it is submitted, D2H behind the group's sweeps; groups overlap.
// History-carrying configurations keep the reference's frame order: a group's sweeps wait for the previous
// launch's sweeps, and all frames use scratch slot 0.
static int ensure_ring(Context* c)
{
    if (!c->ring.empty()) return SN_OK;
    const int B = c->cfg.bytes_per_sample;
    int depth = c->host_depth;
    if (c->history_free) {  // every frame in flight needs scratch of its own
        if (!c->use_fused && depth > c->slots) depth = c->slots;
        if (c->fused420 && depth > c->fslots) depth = c->fslots;
    }
    const int groups = depth < 4 ? depth : 4;
    c->ring_per_group = depth / groups;
    depth = groups * c->ring_per_group;
    for (int p = 0; p < c->nplanes(); ++p) {
        c->ring_pitch_in[p] = (c->plane_w(p) * B + 255) & ~255;
        c->ring_pitch_out[p] = c->ring_pitch_in[p];
        c->ring_bytes_in[p] = (int64_t)c->ring_pitch_in[p] * c->plane_h_in(p);
        c->ring_bytes_out[p] = (int64_t)c->ring_pitch_out[p] * c->plane_h_out(p);
        SN_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&c->ring_pin_in[p]), (size_t)c->ring_bytes_in[p] * depth, hipHostMallocDefault));
        SN_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&c->ring_pin_out[p]), (size_t)c->ring_bytes_out[p] * depth, hipHostMallocDefault));
        SN_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->ring_dev_in[p]), (size_t)c->ring_bytes_in[p] * depth));
        SN_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->ring_dev_out[p]), (size_t)c->ring_bytes_out[p] * depth));
    }
    c->slot_state.assign(depth, Context::kFree);
    c->slot_parity.assign(depth, 1);
    c->slot_dst.assign(depth, Context::SlotDst{});
    c->ring.resize(groups);
    for (auto& g : c->ring) {
        SN_HIP(c, hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
        SN_HIP(c, hipEventCreateWithFlags(&g.done, hipEventDisableTiming));
        SN_HIP(c, hipEventCreateWithFlags(&g.swept, hipEventDisableTiming));
    }
    ensure_copier(c);
    return SN_OK;
}

// Sweeps the staged slots [lo, hi) of group gi and queues their D2H.
static int launch_ring_group(Context* c, int gi)
{
    Context::HostGroup& g = c->ring[gi];
    const int n = g.hi - g.lo;
    if (n <= 0) return SN_OK;
    const int first = gi * c->ring_per_group + g.lo;
    if (!c->history_free && c->ring_last >= 0 && c->ring_last != gi) SN_HIP(c, hipStreamWaitEvent(g.stream, c->ring[c->ring_last].swept, 0));
    const void* dsrc[3] = {nullptr, nullptr, nullptr};
    void* ddst[3] = {nullptr, nullptr, nullptr};
    for (int p = 0; p < c->nplanes(); ++p) {
        dsrc[p] = c->ring_dev_in[p] + (int64_t)first * c->ring_bytes_in[p];
        ddst[p] = c->ring_dev_out[p] + (int64_t)first * c->ring_bytes_out[p];
    }
    const int rc = run_batch(c, g.stream, c->history_free ? first : 0, n, dsrc, c->ring_bytes_in, c->ring_pitch_in, ddst, c->ring_bytes_out,
                             c->ring_pitch_out, &c->slot_parity[first]);
    if (rc != SN_OK) return rc;
    SN_HIP(c, hipEventRecord(g.swept, g.stream));
    const int B = c->cfg.bytes_per_sample;
    for (int p = 0; p < c->nplanes(); ++p) {
        bool one_transfer = true;  // the whole group's plane p in one transfer into the pinned staging?
        for (int k = 0; k < n; ++k) one_transfer = one_transfer && !c->slot_dst[first + k].direct[p] && !c->slot_dst[first + k].kept_on_host;
        if (one_transfer) {
            SN_HIP(c, hipMemcpyAsync(c->ring_pin_out[p] + (int64_t)first * c->ring_bytes_out[p], ddst[p], (size_t)c->ring_bytes_out[p] * n,
                                     hipMemcpyDeviceToHost, g.stream));
            continue;
        }
        for (int k = 0; k < n; ++k) {
            const Context::SlotDst& sd = c->slot_dst[first + k];
            const uint8_t* from = static_cast<const uint8_t*>(ddst[p]) + (int64_t)k * c->ring_bytes_out[p];
            uint8_t* to = sd.direct[p] ? static_cast<uint8_t*>(sd.ptr[p]) : c->ring_pin_out[p] + (int64_t)(first + k) * c->ring_bytes_out[p];
            const int to_pitch = sd.direct[p] ? sd.pitch[p] : c->ring_pitch_out[p];
            if (sd.kept_on_host) {  // only the interpolated lines: offset + 1, offset + 3, ...
                const int off = sn::field_offset(c->cfg.order, c->slot_parity[first + k]), nr = c->plane_h_out(p) / 2 - 1;
                if ((c->cfg.dh || c->process[p]) && nr > 0)
                    SN_HIP(c, hipMemcpy2DAsync(to + (int64_t)(off + 1) * to_pitch, (size_t)2 * to_pitch, from + (int64_t)(off + 1) * c->ring_pitch_out[p],
                                               (size_t)2 * c->ring_pitch_out[p], (size_t)c->plane_w(p) * B, nr, hipMemcpyDeviceToHost, g.stream));
            } else if (!sd.direct[p]) {  // the context's own staging (same pitch on both sides, padding its own): one linear transfer
                SN_HIP(c, hipMemcpyAsync(to, from, (size_t)c->ring_bytes_out[p] - (c->ring_pitch_out[p] - c->plane_w(p) * B), hipMemcpyDeviceToHost, g.stream));
            } else {  // the caller's pinned plane, row by row: the bytes between its rows are not ours to write
                SN_HIP(c, hipMemcpy2DAsync(to, to_pitch, from, c->ring_pitch_out[p], (size_t)c->plane_w(p) * B, c->plane_h_out(p), hipMemcpyDeviceToHost, g.stream));
            }
        }
    }
    SN_HIP(c, hipEventRecord(g.done, g.stream));
    for (int k = 0; k < n; ++k) c->slot_state[first + k] = Context::kInFlight;
    g.lo = g.hi;
    c->ring_last = gi;
    return SN_OK;
}

int sn_host_slots(sn_context* h)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return 0;
    if (hipSetDevice(c->device) != hipSuccess || ensure_ring(c) != SN_OK) return 0;
    return (int)c->slot_state.size();
}

static int submit_impl(sn_context* h, const void* const src[3], const int32_t sp[3], void* const dst[3], const int32_t dp[3], int32_t parity,
                       int32_t* slot_out)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    if (!src || !sp || !slot_out) return sn::fail(c, SN_ERR_INVALID_ARG, "plane array / slot pointer is NULL");
    const int B = c->cfg.bytes_per_sample;
    for (int p = 0; p < c->nplanes(); ++p) {
        if (!src[p]) return sn::fail(c, SN_ERR_INVALID_ARG, "plane %d pointer is NULL", p);
        if (sp[p] < c->plane_w(p) * B) return sn::fail(c, SN_ERR_INVALID_ARG, "plane %d pitch smaller than the row size %d", p, c->plane_w(p) * B);
    }
    SN_HIP(c, hipSetDevice(c->device));
    int rc = ensure_ring(c);
    if (rc == SN_OK) rc = prepare_small_launch_scratch(c);
    if (rc != SN_OK) return rc;
    const int slot = c->ring_next;
    if (c->slot_state[slot] != Context::kFree)
        return sn::fail(c, SN_ERR_BUSY, "all %d host slots are in flight: collect slot %d first", (int)c->slot_state.size(), slot);
    const int gi = slot / c->ring_per_group, k = slot % c->ring_per_group;
    Context::HostGroup& g = c->ring[gi];
    if (k == 0) g.lo = g.hi = 0;  // the ring came round to this group again

    Context::SlotDst sd{};
    if (dst) {
        if (!dp) return sn::fail(c, SN_ERR_INVALID_ARG, "plane array is NULL");
        sd.given = true;
        for (int p = 0; p < c->nplanes(); ++p) {
            if (!dst[p]) return sn::fail(c, SN_ERR_INVALID_ARG, "plane %d pointer is NULL", p);
            if (dp[p] < c->plane_w(p) * B) return sn::fail(c, SN_ERR_INVALID_ARG, "plane %d pitch smaller than the row size %d", p, c->plane_w(p) * B);
            sd.ptr[p] = dst[p];
            sd.pitch[p] = dp[p];
            sd.direct[p] = sn::plane_is_pinned(dst[p], dp[p], c->plane_w(p) * B, c->plane_h_out(p));
        }
    }
    // (worth it where the interpolated lines then go straight into the caller's pinned planes; with a pageable destination
    // the extra host copy at submission costs the submitting thread more than the PCIe crossing it saves)
    sd.kept_on_host = sd.given;
    for (int p = 0; p < c->nplanes(); ++p) sd.kept_on_host = sd.kept_on_host && sd.direct[p];
    c->slot_dst[slot] = sd;
    // source planes: pinned ones are DMA'd as they lie, the others are staged (copy threads) first; with the destination
    // announced, the output's kept lines (copies of source lines) go there now, on the host
    Copier::Job jobs[9];
    bool direct_in[3] = {false, false, false};
    int njobs = 0;
    if (sd.kept_on_host)
        for (int p = 0; p < c->nplanes(); ++p) njobs += kept_line_jobs(c, p, parity, src[p], sp[p], sd.ptr[p], sd.pitch[p], jobs + njobs);
    bool on_device[3] = {true, true, true};  // a copied plane whose copy the host has just made never visits the device
    for (int p = 0; p < c->nplanes(); ++p) {
        on_device[p] = !(sd.kept_on_host && !(c->cfg.dh || c->process[p]));
        if (!on_device[p]) continue;
        direct_in[p] = sn::plane_is_pinned(src[p], sp[p], c->plane_w(p) * B, c->plane_h_in(p));
        if (!direct_in[p]) {
            const KeptLines kl = sn::kept_lines(*c, p, parity);  // only the lines that are read are staged ...
            jobs[njobs++] = {c->ring_pin_in[p] + (int64_t)slot * c->ring_bytes_in[p] + (int64_t)kl.first * c->ring_pitch_in[p],
                             static_cast<const uint8_t*>(src[p]) + (int64_t)kl.first * sp[p], kl.step * c->ring_pitch_in[p], kl.step * sp[p],
                             c->plane_w(p) * B, kl.rows};
        }
    }
    if (njobs) c->copier->run(jobs, njobs);
    for (int p = 0; p < c->nplanes(); ++p) {
        if (!on_device[p]) continue;
        uint8_t* dev = c->ring_dev_in[p] + (int64_t)slot * c->ring_bytes_in[p];
        const KeptLines kl = sn::kept_lines(*c, p, parity);  // ... and cross PCIe
        const uint8_t* from = direct_in[p] ? static_cast<const uint8_t*>(src[p]) : c->ring_pin_in[p] + (int64_t)slot * c->ring_bytes_in[p];
        const int from_pitch = direct_in[p] ? sp[p] : c->ring_pitch_in[p];
        if (kl.step == 1 && from_pitch == c->ring_pitch_in[p])  // every line, same pitch on both sides: one linear transfer
            SN_HIP(c, hipMemcpyAsync(dev, from, (size_t)c->ring_bytes_in[p] - (c->ring_pitch_in[p] - c->plane_w(p) * B), hipMemcpyHostToDevice, g.stream));
        else
            SN_HIP(c, hipMemcpy2DAsync(dev + (int64_t)kl.first * c->ring_pitch_in[p], (size_t)kl.step * c->ring_pitch_in[p],
                                       from + (int64_t)kl.first * from_pitch, (size_t)kl.step * from_pitch, (size_t)c->plane_w(p) * B, kl.rows,
                                       hipMemcpyHostToDevice, g.stream));
    }
    c->slot_state[slot] = Context::kStaged;
    c->slot_parity[slot] = parity;
    g.hi = k + 1;
    c->ring_next = (slot + 1) % (int)c->slot_state.size();
    *slot_out = slot;
    if (g.hi == c->ring_per_group) return launch_ring_group(c, gi);
    return SN_OK;
}

int sn_submit_host(sn_context* h, const void* const src[3], const int32_t sp[3], int32_t parity, int32_t* slot_out)
{
    return submit_impl(h, src, sp, nullptr, nullptr, parity, slot_out);
}

int sn_submit_host_to(sn_context* h, const void* const src[3], const int32_t sp[3], void* const dst[3], const int32_t dp[3], int32_t parity,
                      int32_t* slot_out)
{
    if (!dst || !dp) return sn::fail(reinterpret_cast<Context*>(h), SN_ERR_INVALID_ARG, "plane array is NULL");
    return submit_impl(h, src, sp, dst, dp, parity, slot_out);
}

int sn_collect_host(sn_context* h, int32_t slot, void* const dst_arg[3], const int32_t dp_arg[3])
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    if (slot < 0 || slot >= (int)c->slot_state.size() || c->slot_state[slot] == Context::kFree)
        return sn::fail(c, SN_ERR_INVALID_ARG, "slot %d holds no frame", slot);
    // the destination: named now, or at submission (sn_submit_host_to)
    const Context::SlotDst sd = c->slot_dst[slot];
    void* const* dst = dst_arg ? dst_arg : (sd.given ? sd.ptr : nullptr);
    const int32_t* dp = dst_arg ? dp_arg : (sd.given ? sd.pitch : nullptr);
    if (!dst || !dp) return sn::fail(c, SN_ERR_INVALID_ARG, "plane array is NULL");
    const int B = c->cfg.bytes_per_sample;
    for (int p = 0; p < c->nplanes(); ++p) {
        if (!dst[p]) return sn::fail(c, SN_ERR_INVALID_ARG, "plane %d pointer is NULL", p);
        if (dp[p] < c->plane_w(p) * B) return sn::fail(c, SN_ERR_INVALID_ARG, "plane %d pitch smaller than the row size %d", p, c->plane_w(p) * B);
    }
    SN_HIP(c, hipSetDevice(c->device));
    const int gi = slot / c->ring_per_group;
    if (c->slot_state[slot] == Context::kStaged) {  // its group is not full yet: sweep what is staged
        const int rc = launch_ring_group(c, gi);
        if (rc != SN_OK) return rc;
    }
    SN_HIP(c, hipEventSynchronize(c->ring[gi].done));
    Copier::Job jobs[3];
    int njobs = 0;
    for (int p = 0; p < c->nplanes(); ++p) {
        if (sd.direct[p] && dst[p] == sd.ptr[p]) continue;  // already written there by the device
        const uint8_t* from = c->ring_pin_out[p] + (int64_t)slot * c->ring_bytes_out[p];
        if (sd.direct[p]) {  // collected into another place than announced: that plane never reached the staging
            for (int y = 0; y < c->plane_h_out(p); ++y)  // host to host: no business of the runtime's
                memcpy(static_cast<uint8_t*>(dst[p]) + (size_t)y * dp[p], static_cast<const uint8_t*>(sd.ptr[p]) + (size_t)y * sd.pitch[p], (size_t)c->plane_w(p) * B);
            continue;
        }
        // (sd.kept_on_host implies direct[p] for every plane: handled above)
        jobs[njobs++] = {static_cast<uint8_t*>(dst[p]), from, dp[p], c->ring_pitch_out[p], c->plane_w(p) * B, c->plane_h_out(p)};
    }
    if (njobs) c->copier->run(jobs, njobs);
    c->slot_state[slot] = Context::kFree;
    c->slot_dst[slot] = Context::SlotDst{};
    return SN_OK;
}

int sn_pin_host_buffer(void* ptr, size_t bytes)
{
    if (!ptr || !bytes) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "sn_pin_host_buffer: NULL or empty");
    const hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterPortable);
    if (e != hipSuccess) return sn::fail(nullptr, SN_ERR_HIP, "hipHostRegister failed: %s", hipGetErrorString(e));
    std::lock_guard<std::mutex> lk(sn::g_pin_mutex);
    sn::g_pinned.push_back({reinterpret_cast<uintptr_t>(ptr), reinterpret_cast<uintptr_t>(ptr) + bytes});
    return SN_OK;
}

int sn_unpin_host_buffer(void* ptr)
{
    {
        std::lock_guard<std::mutex> lk(sn::g_pin_mutex);
        bool found = false;
        for (size_t i = 0; i < sn::g_pinned.size() && !found; ++i) found = sn::g_pinned[i].lo == reinterpret_cast<uintptr_t>(ptr);
        if (!found) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "sn_unpin_host_buffer: not pinned through sn_pin_host_buffer");
    }
    // Nothing of this process may still be moving data through the mapping: the registry is process-wide and the
    // buffers are registered portable, so a context on any device may have a transfer in flight on a stream of its own.
    // Only devices that HAVE a context of this library are waited for (no primary context is created elsewhere).
    std::vector<int> live;
    {
        std::lock_guard<std::mutex> lk(sn::g_live_mutex);
        for (size_t d = 0; d < sn::g_live_contexts.size(); ++d)
            if (sn::g_live_contexts[d] > 0) live.push_back((int)d);
    }
    int cur = 0;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    if (!have_cur) (void)hipGetLastError();
    for (int d : live)
        if (hipSetDevice(d) == hipSuccess) (void)hipDeviceSynchronize();
    if (have_cur && !live.empty()) (void)hipSetDevice(cur);
    const hipError_t e = hipHostUnregister(ptr);
    if (e != hipSuccess) {  // still registered, and still known to the library: the caller may try again
        (void)hipGetLastError();
        return sn::fail(nullptr, SN_ERR_HIP, "hipHostUnregister failed: %s", hipGetErrorString(e));
    }
    std::lock_guard<std::mutex> lk(sn::g_pin_mutex);
    for (size_t i = 0; i < sn::g_pinned.size(); ++i)
        if (sn::g_pinned[i].lo == reinterpret_cast<uintptr_t>(ptr)) {
            sn::g_pinned.erase(sn::g_pinned.begin() + (long)i);
            break;
        }
    return SN_OK;
}

int sn_turn_device(sn_context* h, int32_t direction, int32_t nframes, const void* src, int64_t sfs, int32_t sp, int32_t width,
                   int32_t height, void* dst, int64_t dfs, int32_t dp)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    const int B = c->cfg.bytes_per_sample;
    if (!src || !dst || direction == 0 || nframes < 0 || width <= 0 || height <= 0)
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_turn_device: bad pointer, direction or size");
    if (sp < width * B || dp < height * B || sp % B || dp % B || (uintptr_t)src % B || (uintptr_t)dst % B)
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_turn_device: pitch smaller than the row or misaligned");
    SN_HIP(c, hipSetDevice(c->device));
    SN_HIP(c, sn::launch_turn(c->stream, B, direction > 0 ? 1 : 0, nframes, sn::PlaneView{static_cast<const uint8_t*>(src), sfs, sp}, width, height,
                              sn::PlaneViewW{static_cast<uint8_t*>(dst), dfs, dp}));
    return SN_OK;
}

int sn_reduce_device(sn_context* h, int32_t kernel, int32_t nframes, const void* src, int64_t sfs, int32_t sp, int32_t width, int32_t height,
                     int32_t ox, int32_t oy, void* dst, int64_t dfs, int32_t dp)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    const int B = c->cfg.bytes_per_sample;
    if (!src || !dst || nframes < 0 || width <= 0 || height <= 0 || width > INT32_MAX / 8 || height > INT32_MAX / 2)
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_reduce_device: bad pointer or size");
    if (kernel != SN_AA_REDUCE_TENT && kernel != SN_AA_REDUCE_HALFBAND)
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_reduce_device: kernel must be 1 (tent) or 2 (half-band)");
    if (ox < 0 || ox > 1 || oy < 0 || oy > 1) return sn::fail(c, SN_ERR_INVALID_ARG, "sn_reduce_device: ox and oy must be 0 or 1");
    if (sp < 2 * width * B || dp < width * B || sp % B || dp % B || sfs % B || dfs % B || (uintptr_t)src % B || (uintptr_t)dst % B)
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_reduce_device: pitch smaller than the row or misaligned");
    SN_HIP(c, hipSetDevice(c->device));
    SN_HIP(c, sn::launch_reduce(c->stream, B, c->cfg.bits_per_sample, kernel, nframes, sn::PlaneView{static_cast<const uint8_t*>(src), sfs, sp}, width,
                                height, ox, oy, sn::PlaneViewW{static_cast<uint8_t*>(dst), dfs, dp}));
    return SN_OK;
}

int sn_mask_merge_device(sn_context* h, const sn_aa_mask* mask, int32_t nframes, const void* src, int64_t sfs, int32_t sp, const void* aa, int64_t afs,
                         int32_t ap, int32_t width, int32_t height, void* dst, int64_t dfs, int32_t dp)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    const int B = c->cfg.bytes_per_sample;
    if (!mask) return sn::fail(c, SN_ERR_INVALID_ARG, "sn_mask_merge_device: mask is NULL");
    const std::string problem = sn::mask_problem(mask);
    if (!problem.empty()) return sn::fail(c, SN_ERR_INVALID_ARG, ("sn_mask_merge_device: " + problem).c_str());
    if (mask->kind != SN_AA_MASK_SOBEL) return sn::fail(c, SN_ERR_INVALID_ARG, "sn_mask_merge_device: sn_aa_mask.kind must be 1 (Sobel)");
    if (!src || !dst || nframes < 0 || width <= 0 || height <= 0 || width > INT32_MAX / 8 || height > INT32_MAX / 2)
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_mask_merge_device: bad pointer or size");
    if (sp < width * B || dp < width * B || sp % B || dp % B || sfs % B || dfs % B || (uintptr_t)src % B || (uintptr_t)dst % B ||
        (aa && (ap < width * B || ap % B || afs % B || (uintptr_t)aa % B)))
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_mask_merge_device: pitch smaller than the row or misaligned");
    SN_HIP(c, hipSetDevice(c->device));
    SN_HIP(c, sn::launch_mask_merge(c->stream, B, c->cfg.bits_per_sample, mask->lo, mask->hi, mask->expand, nframes,
                                    sn::PlaneView{static_cast<const uint8_t*>(src), sfs, sp}, sn::PlaneView{static_cast<const uint8_t*>(aa), afs, ap}, width,
                                    height, sn::PlaneViewW{static_cast<uint8_t*>(dst), dfs, dp}));
    return SN_OK;
}

int sn_contra_sharpen_device(sn_context* h, int32_t amount, int32_t nframes, const void* src, int64_t sfs, int32_t sp, const void* aa, int64_t afs, int32_t ap,
                             int32_t width, int32_t height, void* dst, int64_t dfs, int32_t dp)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    const int B = c->cfg.bytes_per_sample;
    if (amount < 1 || amount > 255) return sn::fail(c, SN_ERR_INVALID_ARG, "sn_contra_sharpen_device: amount must be 1..255");
    if (!src || !aa || !dst || nframes < 0 || width <= 0 || height <= 0 || width > INT32_MAX / 8 || height > INT32_MAX / 2)
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_contra_sharpen_device: bad pointer or size");
    if (sp < width * B || ap < width * B || dp < width * B || sp % B || ap % B || dp % B || sfs % B || afs % B || dfs % B || (uintptr_t)src % B ||
        (uintptr_t)aa % B || (uintptr_t)dst % B)
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_contra_sharpen_device: pitch smaller than the row or misaligned");
    if (dst == aa || dst == src)  // the stencil reads neighbours of both planes: no workgroup may overwrite what another still reads
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_contra_sharpen_device: dst must overlap neither src nor aa");
    SN_HIP(c, hipSetDevice(c->device));
    SN_HIP(c, sn::launch_contra_sharpen(c->stream, B, c->cfg.bits_per_sample, amount, nframes, sn::PlaneView{static_cast<const uint8_t*>(src), sfs, sp},
                                        sn::PlaneView{static_cast<const uint8_t*>(aa), afs, ap}, width, height,
                                        sn::PlaneViewW{static_cast<uint8_t*>(dst), dfs, dp}));
    return SN_OK;
}

// [first byte, one past the last byte) of `n` frames of `rows` rows of `row_bytes` each
static void plane_span(const void* base, int64_t fs, int32_t pitch, int32_t n, int32_t rows, int64_t row_bytes, uintptr_t& lo, uintptr_t& hi)
{
    const int64_t last_frame = (int64_t)(n - 1) * fs, last_row = (int64_t)(rows - 1) * pitch;
    lo = (uintptr_t)((intptr_t)base + (last_frame < 0 ? last_frame : 0));
    hi = (uintptr_t)((intptr_t)base + (last_frame > 0 ? last_frame : 0) + last_row + row_bytes);
}

int sn_merge_device(sn_context* h, int32_t nframes, const void* a, int64_t afs, int32_t ap, const void* b, int64_t bfs, int32_t bp, int32_t width,
                    int32_t height, void* dst, int64_t dfs, int32_t dp)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    const int B = c->cfg.bytes_per_sample;
    if (!a || !b || !dst || nframes < 0 || width <= 0 || height <= 0 || width > INT32_MAX / 8 || height > INT32_MAX / 2)
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_merge_device: bad pointer or size");
    if (ap < width * B || bp < width * B || dp < width * B || ap % B || bp % B || dp % B || afs % B || bfs % B || dfs % B || (uintptr_t)a % B ||
        (uintptr_t)b % B || (uintptr_t)dst % B)
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_merge_device: pitch smaller than the row or misaligned");
    if (nframes > 0) {  // in place on a or b exactly: each sample is read by the thread that overwrites it; nothing else may overlap
        uintptr_t dlo, dhi;
        plane_span(dst, dfs, dp, nframes, height, (int64_t)width * B, dlo, dhi);
        const struct { const void* base; int64_t fs; int32_t pitch; } in[2] = {{a, afs, ap}, {b, bfs, bp}};
        for (const auto& q : in) {
            if (q.base == dst && q.fs == dfs && q.pitch == dp) continue;
            uintptr_t lo, hi;
            plane_span(q.base, q.fs, q.pitch, nframes, height, (int64_t)width * B, lo, hi);
            if (lo < dhi && dlo < hi) return sn::fail(c, SN_ERR_INVALID_ARG, "sn_merge_device: dst overlaps a or b without being that very plane");
        }
    }
    SN_HIP(c, hipSetDevice(c->device));
    SN_HIP(c, sn::launch_merge(c->stream, B, nframes, sn::PlaneView{static_cast<const uint8_t*>(a), afs, ap},
                               sn::PlaneView{static_cast<const uint8_t*>(b), bfs, bp}, width, height, sn::PlaneViewW{static_cast<uint8_t*>(dst), dfs, dp}));
    return SN_OK;
}

int sn_turn_merge_device(sn_context* h, int32_t direction, int32_t nframes, const void* a, int64_t afs, int32_t ap, const void* b, int64_t bfs, int32_t bp,
                         int32_t width, int32_t height, void* dst, int64_t dfs, int32_t dp)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    const int B = c->cfg.bytes_per_sample;
    if (!a || !b || !dst || direction == 0 || nframes < 0 || width <= 0 || height <= 0 || width > INT32_MAX / 8 || height > INT32_MAX / 8)
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_turn_merge_device: bad pointer, direction or size");
    if (ap < width * B || bp < width * B || dp < height * B || ap % B || bp % B || dp % B || afs % B || bfs % B || dfs % B || (uintptr_t)a % B ||
        (uintptr_t)b % B || (uintptr_t)dst % B)
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_turn_merge_device: pitch smaller than the row or misaligned");
    if (nframes > 0) {  // a tile's writes land where another tile still reads
        uintptr_t dlo, dhi, lo, hi;
        plane_span(dst, dfs, dp, nframes, width, (int64_t)height * B, dlo, dhi);
        plane_span(a, afs, ap, nframes, height, (int64_t)width * B, lo, hi);
        bool overlap = lo < dhi && dlo < hi;
        plane_span(b, bfs, bp, nframes, height, (int64_t)width * B, lo, hi);
        overlap = overlap || (lo < dhi && dlo < hi);
        if (overlap) return sn::fail(c, SN_ERR_INVALID_ARG, "sn_turn_merge_device: dst must overlap neither a nor b");
    }
    SN_HIP(c, hipSetDevice(c->device));
    SN_HIP(c, sn::launch_turn_merge(c->stream, B, direction > 0 ? 1 : 0, nframes, sn::PlaneView{static_cast<const uint8_t*>(a), afs, ap},
                                    sn::PlaneView{static_cast<const uint8_t*>(b), bfs, bp}, width, height,
                                    sn::PlaneViewW{static_cast<uint8_t*>(dst), dfs, dp}));
    return SN_OK;
}

int sn_repair_device(sn_context* h, int32_t rank, int32_t nframes, const void* src, int64_t sfs, int32_t sp, const void* aa, int64_t afs, int32_t ap,
                     int32_t width, int32_t height, void* dst, int64_t dfs, int32_t dp)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    const int B = c->cfg.bytes_per_sample;
    if (rank < 1 || rank > 4) return sn::fail(c, SN_ERR_INVALID_ARG, "sn_repair_device: rank must be 1..4");
    if (!src || !aa || !dst || nframes < 0 || width <= 0 || height <= 0 || width > INT32_MAX / 8 || height > INT32_MAX / 2)
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_repair_device: bad pointer or size");
    if (sp < width * B || ap < width * B || dp < width * B || sp % B || ap % B || dp % B || sfs % B || afs % B || dfs % B || (uintptr_t)src % B ||
        (uintptr_t)aa % B || (uintptr_t)dst % B)
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_repair_device: pitch smaller than the row or misaligned");
    if (nframes > 0) {  // other workgroups read the neighbours of src; R is read by the thread that overwrites it, in place exactly
        uintptr_t dlo, dhi, lo, hi;
        plane_span(dst, dfs, dp, nframes, height, (int64_t)width * B, dlo, dhi);
        plane_span(src, sfs, sp, nframes, height, (int64_t)width * B, lo, hi);
        if (lo < dhi && dlo < hi) return sn::fail(c, SN_ERR_INVALID_ARG, "sn_repair_device: dst must not overlap src");
        if (!(aa == dst && afs == dfs && ap == dp)) {
            plane_span(aa, afs, ap, nframes, height, (int64_t)width * B, lo, hi);
            if (lo < dhi && dlo < hi) return sn::fail(c, SN_ERR_INVALID_ARG, "sn_repair_device: dst and aa overlap without being the same plane");
        }
    }
    SN_HIP(c, hipSetDevice(c->device));
    SN_HIP(c, sn::launch_repair(c->stream, B, rank, nframes, sn::PlaneView{static_cast<const uint8_t*>(src), sfs, sp},
                                sn::PlaneView{static_cast<const uint8_t*>(aa), afs, ap}, width, height, sn::PlaneViewW{static_cast<uint8_t*>(dst), dfs, dp}));
    return SN_OK;
}

int sn_mask_merge_luma_device(sn_context* h, const sn_aa_mask* mask, int32_t nframes, const void* luma, int64_t lfs, int32_t lp, int32_t sub_w, int32_t sub_h,
                              const void* const src[2], const int64_t sfs[2], const int32_t sp[2], const void* const aa[2], const int64_t afs[2],
                              const int32_t ap[2], int32_t width, int32_t height, void* const dst[2], const int64_t dfs[2], const int32_t dp[2])
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    const int B = c->cfg.bytes_per_sample;
    if (!mask) return sn::fail(c, SN_ERR_INVALID_ARG, "sn_mask_merge_luma_device: mask is NULL");
    const std::string problem = sn::mask_problem(mask);
    if (!problem.empty()) return sn::fail(c, SN_ERR_INVALID_ARG, ("sn_mask_merge_luma_device: " + problem).c_str());
    if (mask->kind != SN_AA_MASK_SOBEL) return sn::fail(c, SN_ERR_INVALID_ARG, "sn_mask_merge_luma_device: sn_aa_mask.kind must be 1 (Sobel)");
    if (sub_w < 0 || sub_w > 2 || sub_h < 0 || sub_h > 2) return sn::fail(c, SN_ERR_INVALID_ARG, "sn_mask_merge_luma_device: sub_w and sub_h must be 0..2");
    if (!luma || !src || !sfs || !sp || !dst || !dfs || !dp || !src[0] || !dst[0] || nframes < 0 || width <= 0 || height <= 0 ||
        width > INT32_MAX / 32 || height > INT32_MAX / 8)
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_mask_merge_luma_device: bad pointer or size");
    const int planes = src[1] ? 2 : 1;
    const bool merge = aa && aa[0];
    if (merge && (!afs || !ap)) return sn::fail(c, SN_ERR_INVALID_ARG, "sn_mask_merge_luma_device: bad pointer or size");
    if (planes == 1 ? dst[1] || (aa && aa[1]) : !dst[1] || (aa && !aa[0] != !aa[1]))
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_mask_merge_luma_device: src[1], aa[1] and dst[1] must be given together (aa: all planes or none)");
    bool bad = lp < (width << sub_w) * B || lp % B || lfs % B || (uintptr_t)luma % B;
    for (int p = 0; p < planes; ++p) {
        bad = bad || sp[p] < width * B || dp[p] < width * B || sp[p] % B || dp[p] % B || sfs[p] % B || dfs[p] % B || (uintptr_t)src[p] % B ||
              (uintptr_t)dst[p] % B || (merge && (ap[p] < width * B || ap[p] % B || afs[p] % B || (uintptr_t)aa[p] % B));
    }
    if (bad) return sn::fail(c, SN_ERR_INVALID_ARG, "sn_mask_merge_luma_device: pitch smaller than the row or misaligned");
    sn::PlaneView s[2], a[2];
    sn::PlaneViewW d[2];
    for (int p = 0; p < planes; ++p) {
        s[p] = sn::PlaneView{static_cast<const uint8_t*>(src[p]), sfs[p], sp[p]};
        if (merge) a[p] = sn::PlaneView{static_cast<const uint8_t*>(aa[p]), afs[p], ap[p]};
        d[p] = sn::PlaneViewW{static_cast<uint8_t*>(dst[p]), dfs[p], dp[p]};
    }
    SN_HIP(c, hipSetDevice(c->device));
    SN_HIP(c, sn::launch_mask_merge_luma(c->stream, B, c->cfg.bits_per_sample, mask->lo, mask->hi, mask->expand, nframes,
                                         sn::PlaneView{static_cast<const uint8_t*>(luma), lfs, lp}, sub_w, sub_h, planes, s, a, width, height, d));
    return SN_OK;
}

int sn_synchronize(sn_context* h)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    SN_HIP(c, hipSetDevice(c->device));
    SN_HIP(c, hipStreamSynchronize(c->stream));
    for (auto& g : c->ring)
        if (g.stream) SN_HIP(c, hipStreamSynchronize(g.stream));
    return SN_OK;
}

void* sn_get_stream(sn_context* h)
{
    Context* c = reinterpret_cast<Context*>(h);
    return c ? reinterpret_cast<void*>(c->stream) : nullptr;
}

int sn_get_arithmetic(sn_context* h)
{
    Context* c = reinterpret_cast<Context*>(h);
    return c ? c->arith : -1;
}

int sn_get_info(sn_context* h, sn_info* info)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    if (!info || info->struct_size != (int32_t)sizeof(sn_info))
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_info.struct_size mismatch");
    info->out_height = c->out_height;
    info->pool_stride = c->stride_e;
    info->pool_rows = c->bh + 1;
    info->fused_eligible = sn::fused_eligible(c->cfg) ? 1 : 0;
    if (c->saturating && !c->saturating_sweeps) {
        info->fused_eligible = 0;  // SN_ARITH_SSE2 without sn_policy.sse2_sweeps: the pool path serves every plane
    } else if (c->isolated) {
        info->fused_eligible = 1;
        for (int p = 0; p < c->nplanes(); ++p)
            if ((c->cfg.dh || c->process[p]) && !sn::fused_plane_eligible(c->cfg.bytes_per_sample, c->plane_w(p)) &&
                !(c->fresh && sn::fused_padded_plane_eligible(c->cfg.bytes_per_sample, c->plane_w(p))))
                info->fused_eligible = 0;
    }
    if (c->plane_parts[0] || c->plane_parts[1] || c->plane_parts[2]) info->fused_eligible = c->parts_eligible ? 1 : 0;
    info->history_free = c->history_free ? 1 : 0;
    info->frames = c->frames;
    info->fused_frames = c->fused_frames;
    info->coupled_rows = c->fused420 ? c->fpool_rows : 0;
    info->uv_sweeps = c->uv_frames > 0 ? 1 : 0;
    info->chain_redone = c->chain_status ? (int64_t)__atomic_load_n(c->chain_status, __ATOMIC_RELAXED) : 0;
    info->banded_frames = c->banded_frames;
    info->chained_frames = c->chained_frames;
    info->band_fallbacks = 0;
    if (c->band_fallbacks_dev) {  // the device's own count (the host mirror may lag behind a launch with several failing frames)
        SN_HIP(c, hipSetDevice(c->device));
        SN_HIP(c, hipMemcpy(&info->band_fallbacks, c->band_fallbacks_dev, sizeof(int64_t), hipMemcpyDeviceToHost));
    }
    for (int p = 0; p < 3; ++p) info->threshold[p] = p < c->nplanes() ? c->threshold(p) : 0.0;
    return SN_OK;
}

int sn_get_parts_info(sn_context* h, sn_parts_info* info)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    if (!info || info->struct_size != (int32_t)sizeof(sn_parts_info))
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_parts_info.struct_size mismatch");
    bool any = false;
    for (int p = 0; p < 3; ++p) {
        PartsPlan pl;
        const bool cut = p < c->nplanes() && (c->isolated ? c->plane_fused[p] : c->use_fused) && sn::plan_parts(*c, p, c->parts_force, c->parts_ghost_force, pl);
        info->parts[p] = cut ? pl.n : 0;
        any = any || cut;
    }
    info->ghost_columns = any ? (c->parts_ghost_force > 0 ? c->parts_ghost_force : sn::parts_ghost(c->cfg.bytes_per_sample)) : 0;
    info->part_frames = c->part_frames;
    info->part_fallbacks = 0;
    if (c->parts_fallbacks_dev) {  // the device's own count (the host mirror may lag behind a launch with several failing frames)
        SN_HIP(c, hipSetDevice(c->device));
        SN_HIP(c, hipStreamSynchronize(c->stream));
        SN_HIP(c, hipMemcpy(&info->part_fallbacks, c->parts_fallbacks_dev, sizeof(int64_t), hipMemcpyDeviceToHost));
    }
    return SN_OK;
}

int sn_debug_set_column_parts(sn_context* h, int32_t parts, int32_t ghost_columns)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    if (!c->parts_on || c->cfg.bytes_per_sample < 2) return sn::fail(c, SN_ERR_UNSUPPORTED, "sn_debug_set_column_parts: the context was created without sn_options.column_parts, or for 8-bit samples");
    if (parts < 0 || parts == 1 || parts > kMaxParts) return sn::fail(c, SN_ERR_INVALID_ARG, "sn_debug_set_column_parts: parts must be 0 or 2..%d", kMaxParts);
    if (ghost_columns < 0 || ghost_columns % 8 != 0) return sn::fail(c, SN_ERR_INVALID_ARG, "sn_debug_set_column_parts: ghost_columns must be 0 or a multiple of 8");
    SN_HIP(c, hipSetDevice(c->device));
    c->parts_force = parts;
    c->parts_ghost_force = ghost_columns;
    c->parts_pause.forget();
    return ensure_parts_scratch(c);  // (allocates here, outside any launch)
}

int sn_debug_read_pool(sn_context* h, int32_t slot, void* host_dst, size_t bytes)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    const size_t need = (size_t)sn::kBuffers * (c->bh + 1) * c->stride_e * c->cfg.bytes_per_sample;
    if (!c->pool.base) return sn::fail(c, SN_ERR_INVALID_ARG, "sn_debug_read_pool: the pool path has not run on this context");
    if (!host_dst || bytes < need || slot < 0 || slot >= c->slots)
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_debug_read_pool: bad slot or buffer too small (%zu needed)", need);
    SN_HIP(c, hipSetDevice(c->device));
    SN_HIP(c, hipStreamSynchronize(c->stream));
    SN_HIP(c, hipMemcpy(host_dst, c->pool.base + (int64_t)slot * c->pool.slot_bytes, need, hipMemcpyDeviceToHost));
    return SN_OK;
}

int sn_get_policy(sn_context* h, sn_policy* policy)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    if (!policy || policy->struct_size != (int32_t)sizeof(sn_policy)) return sn::fail(c, SN_ERR_INVALID_ARG, "sn_policy.struct_size mismatch");
    *policy = c->policy;
    return SN_OK;
}

int sn_set_policy(sn_context* h, const sn_policy* policy)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    if (!policy) return sn::fail(c, SN_ERR_INVALID_ARG, "policy is NULL");
    if (const char* t = policy_text(policy)) return sn::fail(c, SN_ERR_INVALID_ARG, "%s", t);
    c->policy.small_launches = policy->small_launches;
    c->policy.chain = policy->chain;
    c->policy.copy_threads = policy->copy_threads;  // (a copier that already runs keeps its threads)
    c->policy.chroma_sweeps = policy->chroma_sweeps;
    // (scratch_budget_mb and sse2_sweeps are read at creation only)
    return SN_OK;
}

int sn_debug_raise_chain_fault(sn_context* h)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    if (!c->chain_status) return sn::fail(c, SN_ERR_UNSUPPORTED, "sn_debug_raise_chain_fault: this context has not run a chain");
    c->chain_force_fault = true;
    return SN_OK;
}

int sn_debug_set_bands(sn_context* h, int32_t bands, int32_t warm_rows)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    if (bands > kMaxBands || warm_rows < 0) return sn::fail(c, SN_ERR_INVALID_ARG, "sn_debug_set_bands: at most %d bands, warm_rows >= 0", kMaxBands);
    c->band_force = bands;
    c->band_warm = warm_rows;
    return SN_OK;
}

int sn_debug_read_coupled_rows(sn_context* h, int32_t which, void* host_dst, size_t bytes)
{
    Context* c = reinterpret_cast<Context*>(h);
    if (!c) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    const size_t need = (size_t)sn::kBuffers * c->fpool_rows * c->cfg.width * c->cfg.bytes_per_sample;
    if (!c->fused420 || which < 0 || which > 1 || !c->fpool[which] || !host_dst || bytes < need)
        return sn::fail(c, SN_ERR_INVALID_ARG, "sn_debug_read_coupled_rows: no such hand-off or buffer too small (%zu needed)", need);
    SN_HIP(c, hipSetDevice(c->device));
    SN_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<uint32_t> raw((size_t)c->fpool_frame_bytes / 4);
    SN_HIP(c, hipMemcpy(raw.data(), c->fpool[which], (size_t)c->fpool_frame_bytes, hipMemcpyDeviceToHost));
    sn::sweep_pool_unpack(c->cfg.bytes_per_sample, raw.data(), c->cfg.width, c->fpool_rows, host_dst);
    return SN_OK;
}

// ---- the anti-aliasing idiom as one call -------------------------------------------------------
// Two filter instances (the turned clip, the clip) on ONE stream and the turn kernel between them.  A batch runs in
// chunks of as many frames as the intermediates hold: turn the chunk, first pass over it, turn back, second pass, so
// that each instance sees its frames in order.  Host frames go through groups of frame slots: upload on one stream, the
// device work of every group on the call's stream (in submission order, which is what a history-carrying pass needs),
// download on a third; events order the three, nothing waits inside a kernel.
// With cfg.dh both passes double the height: the idiom enlarges by two in both directions.  The first pass's output is
// then twice as high as the turned clip, the second pass's input twice as wide as the clip and its output (the
// destination) twice as wide and twice as high; without dh every one of these geometries is the clip's or the turned one.
// With a reduction (sn_aa_options.reduce, dh only) the second pass writes a fourth intermediate E in its own geometry
// (ow x oh) and sn_reduce.hip brings it to the destination, which has the clip's geometry again (dstw x dsth): nine plane
// sizes of intermediates per processed plane and frame instead of five.
// With a contra-sharpening (sn_aa_sharpen.amount) the last step -- the second pass, or the reduction -- writes a sharpened
// plane into one more intermediate of the destination's geometry and sn_sharpen.hip writes the destination from it and the
// source: one plane size more per sharpened plane and frame.  The edge mask follows, unchanged.
// With both fields (sn_aa_fields.mode; never with dh) each pass has an order-2 twin, a filter instance of its own on the same
// stream: the turn writes every line, both instances of a pass read the same input, the turn back takes the average of the
// first pass's two outputs (sn_turn.hip with a second source), and the second pass's two outputs are averaged in place where the
// order-1 instance wrote (sn_merge.hip): five plane sizes of intermediates per processed plane and frame instead of three.
// With a rank repair (sn_aa_repair.rank) sn_repair.hip clamps the result so far into the source's 3 x 3 rank range, in place on
// the destination, behind the sharpening and before the edge mask: no intermediate.
struct sn_aa_context {
    sn_config cfg{};
    sn_context* first = nullptr;   // the turned clip
    sn_context* second = nullptr;  // the clip itself, on first's stream
    sn_context* twin[2] = {nullptr, nullptr};  // both fields: the order-2 instances next to first and second, on first's stream
    hipStream_t stream = nullptr;
    hipStream_t up = nullptr, down = nullptr;  // host frames: H2D / D2H (created with the first group of slots)
    sn::AaPlan plan;                                   // every size, option and step of the call (sn_aa_plan.h)
    int cap = 0;                                       // frames the intermediates hold (a chunk)
    uint8_t* d[sn::kAaBuffers][3] = {};                // the intermediates (sn::AaBuf; the caller's planes have none)
    // host frames: `per_group` slots form a group whose frames one batch works on; the ring's groups, then one group of
    // one slot for the synchronous call
    struct Slot {
        uint8_t state = Context::kFree;
        int32_t parity = 1;
        void* out[3] = {nullptr, nullptr, nullptr};  // pinned destination planes named before the launch: written from the device
        int32_t out_pitch[3] = {0, 0, 0};
        bool copied[3] = {false, false, false};      // a plane that is not processed and already lies in its destination
    };
    struct Group {
        int n = 0;
        uint8_t* d_src[3] = {nullptr, nullptr, nullptr};
        uint8_t* d_out[3] = {nullptr, nullptr, nullptr};
        uint8_t* h_src[3] = {nullptr, nullptr, nullptr};  // pinned staging for planes the caller holds in pageable memory
        uint8_t* h_dst[3] = {nullptr, nullptr, nullptr};
        hipEvent_t arrived = nullptr, swept = nullptr, done = nullptr;
        int lo = 0, hi = 0;  // slots [lo, hi) are staged and not yet launched
        std::vector<Slot> slot;
    };
    std::vector<Group> groups;  // [0, ring_groups): the ring; [ring_groups]: the synchronous call's
    sn::UvScratch uv;           // sn_aa_process_device_surfaces
    bool luma_elsewhere = false;  // ... with an MSB-aligned side: luma that is not processed has gone from src to dst already
    int ring_next = 0;
    bool ring_ready = false;
    Copier* copier = nullptr;  // the first context's
    std::string err;
};

static thread_local std::string g_aa_error;

const char* sn_aa_last_error(const sn_aa_context* a) { return a ? a->err.c_str() : g_aa_error.c_str(); }

static int aa_fail(sn_aa_context* a, int code, const std::string& m)
{
    if (a) a->err = m;
    else g_aa_error = m;
    return code;
}

#define SN_AA_HIP(call)                                                                                          \
    do {                                                                                                         \
        hipError_t e_ = (call);                                                                                  \
        if (e_ != hipSuccess) return aa_fail(a, SN_ERR_HIP, std::string(#call " failed: ") + hipGetErrorString(e_)); \
    } while (0)
#define SN_AA_SN(ctx, call)                                            \
    do {                                                               \
        const int rc_ = (call);                                        \
        if (rc_ != SN_OK) return aa_fail(a, rc_, sn_last_error(ctx));  \
    } while (0)

static void aa_free_group(sn_aa_context::Group& g)
{
    for (int p = 0; p < 3; ++p) {
        for (uint8_t* q : {g.d_src[p], g.d_out[p]})
            if (q) (void)hipFree(q);
        for (uint8_t* q : {g.h_src[p], g.h_dst[p]})
            if (q) (void)hipHostFree(q);
    }
    for (hipEvent_t e : {g.arrived, g.swept, g.done})
        if (e) (void)hipEventDestroy(e);
}

// The intermediates for chunks of `frames` frames, or of what the scratch budget holds (a batch beyond that is walked in
// more chunks).  At creation for cfg.max_batch; the ring asks again for a group's frames when it is first used.
static int aa_ensure_intermediates(sn_aa_context* a, int frames)
{
    if (frames <= a->cap) return SN_OK;
    const int cap = sn::aa_chunk_frames(a->plan, scratch_budget(reinterpret_cast<Context*>(a->first)), frames);
    if (cap <= a->cap) return SN_OK;
    SN_AA_HIP(hipStreamSynchronize(a->stream));
    for (int p = 0; p < a->plan.planes; ++p) {
        for (int buf = 0; buf < sn::kAaBuffers; ++buf) {
            if (!sn::aa_buf_needed(a->plan, p, buf)) continue;
            const size_t nb = (size_t)sn::aa_buf_frame_bytes(a->plan, p, buf) * cap;
            uint8_t*& q = a->d[buf][p];
            if (q) SN_AA_HIP(hipFree(q));
            q = nullptr;
            SN_AA_HIP(hipMalloc(reinterpret_cast<void**>(&q), nb));
            // the turns write only the lines the next pass keeps: a pass that read another line would read this pattern
            SN_AA_HIP(hipMemsetAsync(q, 0xA5, nb, a->stream));
        }
    }
    SN_AA_HIP(hipStreamSynchronize(a->stream));
    a->cap = cap;
    return SN_OK;
}

void sn_aa_destroy(sn_aa_context* a)
{
    if (!a) return;
    (void)hipSetDevice(a->cfg.device);
    for (hipStream_t st : {a->up, a->stream, a->down})  // frames in flight: in the order their work was queued
        if (st) (void)hipStreamSynchronize(st);
    for (sn_context* t : {a->twin[1], a->twin[0], a->second})
        if (t) sn_destroy(t);
    if (a->first) sn_destroy(a->first);  // owns the stream unless the caller gave one
    for (auto& planes : a->d)
        for (uint8_t* q : planes)
            if (q) (void)hipFree(q);
    for (const sn::PlaneViewW& q : {a->uv.in[0], a->uv.in[1], a->uv.out[0], a->uv.out[1], a->uv.y, a->uv.yo})
        if (q.base) (void)hipFree(q.base);
    for (auto& g : a->groups) aa_free_group(g);
    for (hipStream_t st : {a->up, a->down})
        if (st) (void)hipStreamDestroy(st);
    delete a;
}

int sn_aa_create(const sn_config* cfg, sn_aa_context** out) { return sn_aa_create_with_policy(cfg, nullptr, out); }

int sn_aa_create_with_policy(const sn_config* cfg, const sn_policy* policy, sn_aa_context** out) { return sn_aa_create_ex(cfg, policy, nullptr, out); }

int sn_aa_create_ex(const sn_config* cfg, const sn_policy* policy, const sn_options* options, sn_aa_context** out)
{
    return sn_aa_create_ex2(cfg, policy, options, nullptr, out);
}

int sn_aa_create_ex2(const sn_config* cfg, const sn_policy* policy, const sn_options* options, const sn_aa_options* aa_options, sn_aa_context** out)
{
    return sn_aa_create_ex3(cfg, policy, options, aa_options, nullptr, out);
}

int sn_aa_create_ex3(const sn_config* cfg, const sn_policy* policy, const sn_options* options, const sn_aa_options* aa_options, const sn_aa_mask* mask,
                     sn_aa_context** out)
{
    return sn_aa_create_ex4(cfg, policy, options, aa_options, mask, nullptr, out);
}

int sn_aa_create_ex4(const sn_config* cfg, const sn_policy* policy, const sn_options* options, const sn_aa_options* aa_options, const sn_aa_mask* mask,
                     const sn_aa_mask_ex* mask_ex, sn_aa_context** out)
{
    return sn_aa_create_ex5(cfg, policy, options, aa_options, mask, mask_ex, nullptr, out);
}

int sn_aa_create_ex5(const sn_config* cfg, const sn_policy* policy, const sn_options* options, const sn_aa_options* aa_options, const sn_aa_mask* mask,
                     const sn_aa_mask_ex* mask_ex, const sn_aa_sharpen* sharpen, sn_aa_context** out)
{
    return sn_aa_create_ex6(cfg, policy, options, aa_options, mask, mask_ex, sharpen, nullptr, out);
}

int sn_aa_create_ex6(const sn_config* cfg, const sn_policy* policy, const sn_options* options, const sn_aa_options* aa_options, const sn_aa_mask* mask,
                     const sn_aa_mask_ex* mask_ex, const sn_aa_sharpen* sharpen, const sn_aa_fields* fields, sn_aa_context** out)
{
    return sn_aa_create_ex7(cfg, policy, options, aa_options, mask, mask_ex, sharpen, fields, nullptr, out);
}

int sn_aa_create_ex7(const sn_config* cfg, const sn_policy* policy, const sn_options* options, const sn_aa_options* aa_options, const sn_aa_mask* mask,
                     const sn_aa_mask_ex* mask_ex, const sn_aa_sharpen* sharpen, const sn_aa_fields* fields, const sn_aa_repair* repair, sn_aa_context** out)
{
    auto fail_aa = [](sn_aa_context* a, int code, const std::string& msg) {
        g_aa_error = msg;
        if (a) sn_aa_destroy(a);
        return code;
    };
    if (!cfg || !out) return fail_aa(nullptr, SN_ERR_INVALID_ARG, "cfg / out is NULL");
    *out = nullptr;
    // check, build the geometry, create the passes, allocate (sn_aa_plan.h decides; nothing below does)
    sn::AaOptions opt;
    std::string msg;
    if (int rc = sn::aa_check(*cfg, aa_options, mask, mask_ex, sharpen, fields, repair, opt, msg)) return fail_aa(nullptr, rc, msg);
    sn_aa_context* a = new (std::nothrow) sn_aa_context();
    if (!a) return fail_aa(nullptr, SN_ERR_INVALID_ARG, "out of host memory");
    a->cfg = *cfg;
    a->plan = sn::aa_geometry(*cfg, opt);
    sn::aa_steps(a->plan);
    sn_config c1 = a->plan.c1, c2 = a->plan.c2;
    c1.stream = cfg->stream;
    int rc = sn_create_ex(&c1, policy, options, &a->first);
    if (rc != SN_OK) return fail_aa(a, rc, sn_last_error(nullptr));
    if (cfg->dh && cfg->width > INT32_MAX / 2)  // what the second pass's own check would say, had 2W fitted its field
        return fail_aa(a, SN_ERR_UNSUPPORTED, "width " + std::to_string(2 * (int64_t)cfg->width) + " exceeds the supported maximum of 8192");
    c2.stream = sn_get_stream(a->first);
    rc = sn_create_ex(&c2, policy, options, &a->second);
    if (rc != SN_OK) return fail_aa(a, rc, sn_last_error(nullptr));
    Context* f1 = reinterpret_cast<Context*>(a->first);
    f1->copies_elsewhere = reinterpret_cast<Context*>(a->second)->copies_elsewhere = true;
    a->stream = f1->stream;
    if (opt.fields == SN_AA_FIELDS_BOTH) {  // the order-2 twins: the same configuration, policy and options, on the same stream
        sn_config cb[2] = {a->plan.c1b, a->plan.c2b};
        for (int k = 0; k < 2; ++k) {
            cb[k].stream = c2.stream;
            rc = sn_create_ex(&cb[k], policy, options, &a->twin[k]);
            if (rc != SN_OK) return fail_aa(a, rc, sn_last_error(nullptr));
            reinterpret_cast<Context*>(a->twin[k])->copies_elsewhere = true;
        }
    }
    if (int rc2 = aa_ensure_intermediates(a, a->plan.max_batch)) return fail_aa(a, rc2, a->err);
    *out = a;
    return SN_OK;
}

// One step of the plan on frames [f0, f0 + m) of the batch, the chunk the intermediates hold from their frame 0.
static int aa_step(sn_aa_context* a, const sn::AaStep& s, int f0, int m, const sn::PlaneView src[3], const sn::PlaneViewW dst[3], const int32_t* par)
{
    const sn::AaPlan& P = a->plan;
    const int B = P.B;
    hipStream_t st = a->stream;
    auto wr = [&](int buf, int p) {
        return buf == sn::kAaDst ? dst[p].at(f0) : sn::PlaneViewW{a->d[buf][p], sn::aa_buf_frame_bytes(P, p, buf), sn::aa_buf_pitch(P, p, buf)};
    };
    auto rd = [&](int buf, int p) { return buf == sn::kAaSrc ? src[p].at(f0) : sn::PlaneView(wr(buf, p)); };
    if (sn::aa_is_pass(s.kind)) {
        // planes that are not processed are never touched by the passes (copies_elsewhere): their pointers only have to be there
        sn::PlaneView r[3];
        sn::PlaneViewW w[3];
        for (int p = 0; p < P.planes; ++p) {
            r[p] = rd(s.read[0], p), w[p] = wr(s.write[p], p);
            if (!s.on(p)) r[p].base = src[p].base, w[p].base = dst[p].at(f0).base;
        }
        const PlaneArrays v(r, w);
        sn_context* h = s.kind == sn::kAaPass1 ? a->first : s.kind == sn::kAaPass2 ? a->second : a->twin[s.kind == sn::kAaPass2B];
        SN_AA_SN(h, run_batch(reinterpret_cast<Context*>(h), st, 0, m, v.s, v.sfs, v.sp, v.d, v.dfs, v.dp, par));
        return SN_OK;
    }
    const sn_aa_mask& mask = P.opt.mask;
    for (int g0 = 0; g0 < m;) {
        const sn::FieldRun run = sn::aa_step_run(P, s, par, g0, m);
        const int n = run.end - g0;
        if (s.kind == sn::kAaMaskLuma) {
            const sn::PlaneView cs[2] = {rd(s.read[0], 1), rd(s.read[0], 2)}, ca[2] = {rd(s.read[1], 1), rd(s.read[1], 2)};
            const sn::PlaneViewW cd[2] = {wr(s.write[1], 1), wr(s.write[2], 2)};
            SN_AA_HIP(sn::launch_mask_merge_luma(st, B, P.bits, mask.lo, mask.hi, mask.expand, n, rd(s.read[0], 0), P.c2.sub_w, P.c2.sub_h, 2, cs, ca,
                                                 P.plane[1].w, P.plane[1].h, cd));
        }
        for (int p = 0; p < P.planes && s.kind != sn::kAaMaskLuma; ++p) {
            if (!s.on(p)) continue;
            const sn::AaPlane& g = P.plane[p];
            const sn::PlaneView from = rd(s.read[0], p).at(g0);
            const sn::PlaneViewW to = wr(s.write[p], p).at(g0);
            switch (s.kind) {
            case sn::kAaTurnLeft:  // the clip's plane -> h wide, w high
                SN_AA_HIP(sn::launch_turn(st, B, 0, n, from, g.w, g.h, to, run.offset));
                break;
            case sn::kAaTurnRight:  // of the first pass's output
                SN_AA_HIP(sn::launch_turn(st, B, 1, n, from, g.h, g.ow, to, run.offset));
                break;
            case sn::kAaTurnRightMerge:  // of the average of the first pass's two outputs
                SN_AA_HIP(sn::launch_turn_merge(st, B, 1, n, from, rd(s.read[1], p).at(g0), g.h, g.ow, to));
                break;
            case sn::kAaMerge:  // in place: the order-1 output lies where the average goes
                SN_AA_HIP(sn::launch_merge(st, B, n, sn::PlaneView(to), from, g.dstw, g.dsth, to));
                break;
            case sn::kAaReduce:  // the run's field offset is where the source samples lie in E
                SN_AA_HIP(sn::launch_reduce(st, B, P.bits, s.arg, n, from, g.w, g.h, 1 - run.offset, run.offset, to));
                break;
            case sn::kAaSharpen:
                SN_AA_HIP(sn::launch_contra_sharpen(st, B, P.bits, s.arg, n, from, rd(s.read[1], p).at(g0), g.w, g.h, to));
                break;
            case sn::kAaRepair:  // in place: R is read by the thread that overwrites it
                SN_AA_HIP(sn::launch_repair(st, B, s.arg, n, from, rd(s.read[1], p).at(g0), g.w, g.h, to));
                break;
            case sn::kAaMask:
                SN_AA_HIP(sn::launch_mask_merge(st, B, P.bits, mask.lo, mask.hi, mask.expand, n, from, rd(s.read[1], p).at(g0), g.w, g.h, to));
                break;
            default: return aa_fail(a, SN_ERR_INVALID_ARG, "SangNomAA: a step of the plan that is none of its kinds");
            }
        }
        g0 = run.end;
    }
    return SN_OK;
}

// Frames [0, n) of a strided device batch through the plan's steps, on the call's stream: in chunks of what the intermediates hold.
static int aa_run(sn_aa_context* a, int n, const sn::PlaneView src[3], const sn::PlaneViewW dst[3], const int32_t* parity)
{
    for (int f0 = 0; f0 < n; f0 += a->cap) {
        const int m = n - f0 < a->cap ? n - f0 : a->cap;
        for (int i = 0; i < a->plan.nsteps; ++i)
            if (int rc = aa_step(a, a->plan.step[i], f0, m, src, dst, parity ? parity + f0 : nullptr)) return rc;
    }
    return SN_OK;
}

// the plane arrays of the ABI as views (planes the clip does not have: empty)
static void plane_views(int planes, const void* const src[3], const int64_t sfs[3], const int32_t sp[3], void* const dst[3], const int64_t dfs[3],
                        const int32_t dp[3], sn::PlaneView sv[3], sn::PlaneViewW dv[3])
{
    for (int p = 0; p < planes; ++p) {
        sv[p] = sn::PlaneView{static_cast<const uint8_t*>(src[p]), sfs[p], sp[p]};
        dv[p] = sn::PlaneViewW{static_cast<uint8_t*>(dst[p]), dfs[p], dp[p]};
    }
}

// a plane that is not processed: source to destination, once; no turn and no pass
static int aa_copy_plane(sn_aa_context* a, int p, int n, const sn::PlaneView& s, const sn::PlaneViewW& d)
{
    const sn::AaPlane& g = a->plan.plane[p];
    for (int f = 0; f < n; ++f)
        SN_AA_HIP(hipMemcpy2DAsync(d.at(f).base, (size_t)d.pitch, s.at(f).base, (size_t)s.pitch, (size_t)g.w * a->cfg.bytes_per_sample, g.h,
                                   hipMemcpyDeviceToDevice, a->stream));
    return SN_OK;
}

int sn_aa_process_device_strided(sn_aa_context* a, int32_t nframes, const void* const src[3], const int64_t sfs[3], const int32_t sp[3],
                                 void* const dst[3], const int64_t dfs[3], const int32_t dp[3], const int32_t* parity)
{
    if (!a) return aa_fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    if (nframes < 0 || nframes > a->plan.max_batch)
        return aa_fail(a, SN_ERR_INVALID_ARG, "nframes " + std::to_string(nframes) + " outside 0..max_batch (" + std::to_string(a->plan.max_batch) + ")");
    if (!src || !sfs || !sp || !dst || !dfs || !dp) return aa_fail(a, SN_ERR_INVALID_ARG, "plane / stride array is NULL");
    const int B = a->cfg.bytes_per_sample;
    for (int p = 0; p < a->plan.planes; ++p) {
        if (!src[p] || !dst[p] || sp[p] < a->plan.plane[p].w * B || dp[p] < a->plan.plane[p].dstw * B)
            return aa_fail(a, SN_ERR_INVALID_ARG, "plane pointer is NULL or pitch smaller than the row");
        if (sp[p] % B || dp[p] % B || sfs[p] % B || dfs[p] % B || (uintptr_t)src[p] % B || (uintptr_t)dst[p] % B)
            return aa_fail(a, SN_ERR_INVALID_ARG, "plane pointer / pitch / frame stride not aligned to the sample size");
    }
    if (nframes == 0) return SN_OK;
    SN_AA_HIP(hipSetDevice(a->cfg.device));
    sn::PlaneView sv[3];
    sn::PlaneViewW dv[3];
    plane_views(a->plan.planes, src, sfs, sp, dst, dfs, dp, sv, dv);
    for (int p = 0; p < a->plan.planes; ++p)
        if (!a->plan.plane[p].process)
            if (int rc = aa_copy_plane(a, p, nframes, sv[p], dv[p])) return rc;
    return aa_run(a, nframes, sv, dv, parity);
}

static int aa_surface_run(void* self, int m, const sn::PlaneView s[3], const sn::PlaneViewW d[3], const int32_t* parity)
{
    sn_aa_context* a = static_cast<sn_aa_context*>(self);
    if (!a->plan.plane[0].process && !a->luma_elsewhere)  // luma that is not processed: source to destination, once (chroma: surface_walk)
        if (int rc = aa_copy_plane(a, 0, m, s[0], d[0])) return rc;
    return aa_run(a, m, s, d, parity);
}


int sn_aa_process_device_surfaces(sn_aa_context* a, int32_t nframes, const sn_surfaces* src, const sn_surfaces* dst, const int32_t* parity)
{
    if (!a) return aa_fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    std::string msg;
    int rc = surface_header("src", src, msg);
    if (rc == SN_OK) rc = surface_header("dst", dst, msg);
    if (rc != SN_OK) return aa_fail(a, rc, msg);
    if (surface_plain(src) && surface_plain(dst))  // the planar call itself
        return sn_aa_process_device_strided(a, nframes, src->plane, src->frame_stride, src->pitch, dst->plane, dst->frame_stride, dst->pitch, parity);
    if (nframes < 0 || nframes > a->plan.max_batch)
        return aa_fail(a, SN_ERR_INVALID_ARG, "nframes " + std::to_string(nframes) + " outside 0..max_batch (" + std::to_string(a->plan.max_batch) + ")");
    SurfaceGeometry g;
    g.B = a->cfg.bytes_per_sample;
    g.bits = a->cfg.bits_per_sample;
    g.planes = a->plan.planes;
    g.sub_w = a->cfg.sub_w, g.sub_h = a->cfg.sub_h;
    g.max_batch = a->plan.max_batch;
    const sn::AaPlane* pl = a->plan.plane;
    for (int p = 0; p < g.planes; ++p) g.w_in[p] = pl[p].w, g.h_in[p] = pl[p].h, g.w_out[p] = pl[p].dstw, g.h_out[p] = pl[p].dsth;
    g.luma_processed = pl[0].process;
    g.chroma_processed = g.planes < 3 || pl[1].process;
    g.all_lines = true;  // a turn reads whole source rows, whichever destination lines it writes
    SurfaceSide ss, ds;
    rc = surface_side("src", src, g.w_in, g, ss, msg);
    if (rc == SN_OK) rc = surface_side("dst", dst, g.w_out, g, ds, msg);
    if (rc != SN_OK) return aa_fail(a, rc, msg);
    if (nframes == 0) return SN_OK;
    SN_AA_HIP(hipSetDevice(a->cfg.device));
    const sn::SurfacePlan plan = surface_plan_of(g, ss, ds);
    SN_AA_HIP(surface_scratch(a->uv, a->stream, g, scratch_budget(reinterpret_cast<Context*>(a->first)), plan.need));
    const SurfacePasses passes{a, aa_surface_run, nullptr};
    a->luma_elsewhere = (ss.shift != 0 || ds.shift != 0 || ss.packing || ds.packing) && !g.luma_processed;
    rc = surface_walk(a->uv, a->stream, g, plan, nframes, ss, ds, parity, passes, msg);
    a->luma_elsewhere = false;
    if (rc != SN_OK && !msg.empty()) return aa_fail(a, rc, msg);
    return rc;
}

int sn_aa_get_surface_info(sn_aa_context* a, sn_surface_info* info)
{
    if (!a) return aa_fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    if (surface_info(a->uv, info) != SN_OK) return aa_fail(a, SN_ERR_INVALID_ARG, "info is NULL or sn_surface_info.struct_size mismatch");
    return SN_OK;
}

int sn_aa_synchronize(sn_aa_context* a)
{
    if (!a) return aa_fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    SN_AA_HIP(hipSetDevice(a->cfg.device));
    SN_AA_SN(a->first, sn_synchronize(a->first));  // the call's stream, and what a chain may have to report
    SN_AA_SN(a->second, sn_synchronize(a->second));
    for (sn_context* t : a->twin)
        if (t) SN_AA_SN(t, sn_synchronize(t));
    if (a->down) SN_AA_HIP(hipStreamSynchronize(a->down));
    return SN_OK;
}

void* sn_aa_get_stream(sn_aa_context* a) { return a ? reinterpret_cast<void*>(a->stream) : nullptr; }

int sn_aa_get_reduce(sn_aa_context* a) { return a ? a->plan.opt.reduce : -1; }

int sn_aa_get_mask(sn_aa_context* a, sn_aa_mask* out)
{
    if (!a) return aa_fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    if (!out || out->struct_size != (int32_t)sizeof(sn_aa_mask)) return aa_fail(a, SN_ERR_INVALID_ARG, "out is NULL or sn_aa_mask.struct_size mismatch");
    *out = a->plan.opt.mask;
    return SN_OK;
}

int sn_aa_get_mask_ex(sn_aa_context* a, sn_aa_mask_ex* out)
{
    if (!a) return aa_fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    if (!out || out->struct_size != (int32_t)sizeof(sn_aa_mask_ex))
        return aa_fail(a, SN_ERR_INVALID_ARG, "out is NULL or sn_aa_mask_ex.struct_size mismatch");
    *out = sn_aa_mask_ex{};
    out->struct_size = (int32_t)sizeof(sn_aa_mask_ex);
    out->chroma = a->plan.opt.mask_chroma;
    return SN_OK;
}

int sn_aa_get_sharpen(sn_aa_context* a, sn_aa_sharpen* out)
{
    if (!a) return aa_fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    if (!out || out->struct_size != (int32_t)sizeof(sn_aa_sharpen))
        return aa_fail(a, SN_ERR_INVALID_ARG, "out is NULL or sn_aa_sharpen.struct_size mismatch");
    *out = a->plan.opt.sharpen;
    return SN_OK;
}

int sn_aa_get_repair(sn_aa_context* a, sn_aa_repair* out)
{
    if (!a) return aa_fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    if (!out || out->struct_size != (int32_t)sizeof(sn_aa_repair)) return aa_fail(a, SN_ERR_INVALID_ARG, "out is NULL or sn_aa_repair.struct_size mismatch");
    *out = a->plan.opt.repair;
    return SN_OK;
}

int sn_aa_get_fields(sn_aa_context* a, sn_aa_fields* out)
{
    if (!a) return aa_fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    if (!out || out->struct_size != (int32_t)sizeof(sn_aa_fields)) return aa_fail(a, SN_ERR_INVALID_ARG, "out is NULL or sn_aa_fields.struct_size mismatch");
    *out = sn_aa_fields{};
    out->struct_size = (int32_t)sizeof(sn_aa_fields);
    out->mode = a->plan.opt.fields;
    return SN_OK;
}

// the filter instance `pass` names: 0 / 1, and with both fields 2 / 3 for their order-2 twins
static sn_context* aa_instance(sn_aa_context* a, int32_t pass)
{
    if (pass == 0 || pass == 1) return pass ? a->second : a->first;
    if ((pass == 2 || pass == 3) && a->twin[0]) return a->twin[pass - 2];
    aa_fail(a, SN_ERR_INVALID_ARG, a->twin[0] ? "pass must be 0 (the turned clip), 1 (the clip), or 2 / 3 (their order-2 twins)"
                                             : "pass must be 0 (the turned clip) or 1 (the clip)");
    return nullptr;
}

int sn_aa_get_info(sn_aa_context* a, int32_t pass, sn_info* info)
{
    if (!a) return aa_fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    sn_context* c = aa_instance(a, pass);
    if (!c) return SN_ERR_INVALID_ARG;
    SN_AA_SN(c, sn_get_info(c, info));
    return SN_OK;
}

int sn_aa_get_parts_info(sn_aa_context* a, int32_t pass, sn_parts_info* info)
{
    if (!a) return aa_fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    sn_context* c = aa_instance(a, pass);
    if (!c) return SN_ERR_INVALID_ARG;
    SN_AA_SN(c, sn_get_parts_info(c, info));
    return SN_OK;
}

// -- host frames ------------------------------------------------------------------------------------------------
static int aa_ensure_group(sn_aa_context* a, int gi, int n)
{
    const sn::AaPlane* pl = a->plan.plane;
    if (!a->up) {
        SN_AA_HIP(hipStreamCreateWithFlags(&a->up, hipStreamNonBlocking));
        SN_AA_HIP(hipStreamCreateWithFlags(&a->down, hipStreamNonBlocking));
        a->groups.resize((size_t)a->plan.ring_groups + 1);
        ensure_copier(reinterpret_cast<Context*>(a->first));
        a->copier = reinterpret_cast<Context*>(a->first)->copier;  // the first pass's copy threads (it never uses them itself here)
    }
    sn_aa_context::Group& g = a->groups[(size_t)gi];
    if (g.n) return SN_OK;
    for (int p = 0; p < a->plan.planes; ++p) {
        const size_t nb = (size_t)pl[p].cbytes * n, onb = (size_t)pl[p].dstbytes * n;
        // a plane that is not processed never visits the device: its staging carries it from submission to collection
        SN_AA_HIP(hipHostMalloc(reinterpret_cast<void**>(&g.h_src[p]), nb, hipHostMallocDefault));
        if (!pl[p].process) continue;
        SN_AA_HIP(hipHostMalloc(reinterpret_cast<void**>(&g.h_dst[p]), onb, hipHostMallocDefault));
        SN_AA_HIP(hipMalloc(reinterpret_cast<void**>(&g.d_src[p]), nb));
        SN_AA_HIP(hipMalloc(reinterpret_cast<void**>(&g.d_out[p]), onb));
    }
    for (hipEvent_t* e : {&g.arrived, &g.swept, &g.done}) SN_AA_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    g.slot.assign((size_t)n, sn_aa_context::Slot{});
    g.n = n;
    return SN_OK;
}

static int aa_ensure_ring(sn_aa_context* a)
{
    if (a->ring_ready) return SN_OK;
    for (int gi = 0; gi < a->plan.ring_groups; ++gi)
        if (int rc = aa_ensure_group(a, gi, a->plan.per_group)) return rc;
    if (int rc = aa_ensure_intermediates(a, a->plan.per_group)) return rc;
    SN_AA_SN(a->first, prepare_small_launch_scratch(reinterpret_cast<Context*>(a->first)));
    SN_AA_SN(a->second, prepare_small_launch_scratch(reinterpret_cast<Context*>(a->second)));
    for (sn_context* t : a->twin)
        if (t) SN_AA_SN(t, prepare_small_launch_scratch(reinterpret_cast<Context*>(t)));
    a->ring_ready = true;
    return SN_OK;
}

static int aa_check_host_planes(sn_aa_context* a, const void* const ptr[3], const int32_t pitch[3], bool out = false)
{
    if (!ptr || !pitch) return aa_fail(a, SN_ERR_INVALID_ARG, "plane array is NULL");
    for (int p = 0; p < a->plan.planes; ++p)
        if (!ptr[p] || pitch[p] < (out ? a->plan.plane[p].dstw : a->plan.plane[p].w) * a->cfg.bytes_per_sample)
            return aa_fail(a, SN_ERR_INVALID_ARG, "plane pointer is NULL or pitch smaller than the row");
    return SN_OK;
}

// Slot k of group g takes a frame: pageable planes into the pinned staging (the copy threads), then H2D; pinned ones are
// DMA'd as they lie.  With the destination at hand (the synchronous call) a plane that is not processed goes there at once.
static int aa_stage(sn_aa_context* a, sn_aa_context::Group& g, int k, const void* const src[3], const int32_t sp[3], void* const dst[3],
                    const int32_t dp[3], int32_t parity)
{
    const sn::AaPlane* pl = a->plan.plane;
    const int B = a->cfg.bytes_per_sample;
    sn_aa_context::Slot sl{};
    sl.parity = parity;
    Copier::Job jobs[3];
    int nj = 0;
    bool direct[3] = {false, false, false};
    for (int p = 0; p < a->plan.planes; ++p) {
        if (!pl[p].process) {  // host to host, once where the destination is known
            sl.copied[p] = dst != nullptr;
            jobs[nj++] = {dst ? static_cast<uint8_t*>(dst[p]) : g.h_src[p] + k * pl[p].cbytes, static_cast<const uint8_t*>(src[p]),
                          dst ? dp[p] : pl[p].pitch, sp[p], pl[p].w * B, pl[p].h};
            continue;
        }
        direct[p] = sn::plane_is_pinned(src[p], sp[p], pl[p].w * B, pl[p].h);
        if (!direct[p]) jobs[nj++] = {g.h_src[p] + k * pl[p].cbytes, static_cast<const uint8_t*>(src[p]), pl[p].pitch, sp[p], pl[p].w * B, pl[p].h};
        if (dst && sn::plane_is_pinned(dst[p], dp[p], pl[p].dstw * B, pl[p].dsth)) sl.out[p] = dst[p], sl.out_pitch[p] = dp[p];
    }
    if (nj) a->copier->run(jobs, nj);
    for (int p = 0; p < a->plan.planes; ++p) {
        if (!pl[p].process) continue;
        SN_AA_HIP(hipMemcpy2DAsync(g.d_src[p] + k * pl[p].cbytes, pl[p].pitch, direct[p] ? src[p] : g.h_src[p] + k * pl[p].cbytes,
                                   direct[p] ? (size_t)sp[p] : (size_t)pl[p].pitch, (size_t)pl[p].w * B, pl[p].h, hipMemcpyHostToDevice, a->up));
    }
    sl.state = Context::kStaged;
    g.slot[(size_t)k] = sl;
    g.hi = k + 1;
    return SN_OK;
}

// The staged slots [lo, hi) of a group: one batch on the call's stream behind their uploads, their downloads behind it.
static int aa_launch(sn_aa_context* a, sn_aa_context::Group& g)
{
    const sn::AaPlane* pl = a->plan.plane;
    const int n = g.hi - g.lo;
    if (n <= 0) return SN_OK;
    const int B = a->cfg.bytes_per_sample;
    SN_AA_HIP(hipEventRecord(g.arrived, a->up));
    SN_AA_HIP(hipStreamWaitEvent(a->stream, g.arrived, 0));
    std::vector<int32_t> par((size_t)n);
    for (int k = 0; k < n; ++k) par[(size_t)k] = g.slot[(size_t)(g.lo + k)].parity;
    sn::PlaneView sv[3];
    sn::PlaneViewW dv[3];
    bool any = false;
    for (int p = 0; p < a->plan.planes; ++p) {
        any = any || pl[p].process;
        sv[p] = sn::PlaneView{pl[p].process ? g.d_src[p] + g.lo * pl[p].cbytes : g.h_src[p], pl[p].cbytes, pl[p].pitch};  // (not processed: never read on the device)
        dv[p] = sn::PlaneViewW{pl[p].process ? g.d_out[p] + g.lo * pl[p].dstbytes : g.h_src[p], pl[p].dstbytes, pl[p].dstpitch};
    }
    if (any)
        if (int rc = aa_run(a, n, sv, dv, par.data())) return rc;
    SN_AA_HIP(hipEventRecord(g.swept, a->stream));
    SN_AA_HIP(hipStreamWaitEvent(a->down, g.swept, 0));
    for (int k = g.lo; k < g.hi; ++k) {
        sn_aa_context::Slot& sl = g.slot[(size_t)k];
        for (int p = 0; p < a->plan.planes; ++p) {
            if (!pl[p].process) continue;
            SN_AA_HIP(hipMemcpy2DAsync(sl.out[p] ? sl.out[p] : g.h_dst[p] + k * pl[p].dstbytes, sl.out[p] ? (size_t)sl.out_pitch[p] : (size_t)pl[p].dstpitch,
                                       g.d_out[p] + k * pl[p].dstbytes, pl[p].dstpitch, (size_t)pl[p].dstw * B, pl[p].dsth, hipMemcpyDeviceToHost, a->down));
        }
        sl.state = Context::kInFlight;
    }
    SN_AA_HIP(hipEventRecord(g.done, a->down));
    g.lo = g.hi;
    return SN_OK;
}

int sn_aa_host_slots(sn_aa_context* a)
{
    if (!a) return 0;
    if (hipSetDevice(a->cfg.device) != hipSuccess || aa_ensure_ring(a) != SN_OK) return 0;
    return a->plan.depth;
}

int sn_aa_submit_host(sn_aa_context* a, const void* const src[3], const int32_t sp[3], int32_t parity, int32_t* slot_out)
{
    if (!a) return aa_fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    if (!slot_out) return aa_fail(a, SN_ERR_INVALID_ARG, "slot pointer is NULL");
    if (int rc = aa_check_host_planes(a, src, sp)) return rc;
    SN_AA_HIP(hipSetDevice(a->cfg.device));
    if (int rc = aa_ensure_ring(a)) return rc;
    const int slot = a->ring_next, gi = slot / a->plan.per_group, k = slot % a->plan.per_group;
    sn_aa_context::Group& g = a->groups[(size_t)gi];
    if (g.slot[(size_t)k].state != Context::kFree)
        return aa_fail(a, SN_ERR_BUSY, "all " + std::to_string(a->plan.depth) + " host slots are in flight: collect slot " + std::to_string(slot) + " first");
    if (k == 0) g.lo = g.hi = 0;  // the ring came round to this group again
    if (int rc = aa_stage(a, g, k, src, sp, nullptr, nullptr, parity)) return rc;
    a->ring_next = (slot + 1) % a->plan.depth;
    *slot_out = slot;
    return g.hi == g.n ? aa_launch(a, g) : SN_OK;
}

// Waits for slot k of group g and brings its planes into the caller's.
static int aa_finish(sn_aa_context* a, sn_aa_context::Group& g, int k, void* const dst[3], const int32_t dp[3])
{
    const sn::AaPlane* pl = a->plan.plane;
    const int B = a->cfg.bytes_per_sample;
    sn_aa_context::Slot& sl = g.slot[(size_t)k];
    if (sl.state == Context::kStaged)  // its group is not full yet: run what is staged
        if (int rc = aa_launch(a, g)) return rc;
    SN_AA_HIP(hipEventSynchronize(g.done));
    Copier::Job jobs[3];
    int nj = 0;
    for (int p = 0; p < a->plan.planes; ++p) {
        if (pl[p].process ? sl.out[p] == dst[p] : sl.copied[p]) continue;  // already there
        // (a plane that is not processed has the clip's geometry on both sides: there is none with dh)
        if (pl[p].process)
            jobs[nj++] = {static_cast<uint8_t*>(dst[p]), g.h_dst[p] + k * pl[p].dstbytes, dp[p], pl[p].dstpitch, pl[p].dstw * B, pl[p].dsth};
        else
            jobs[nj++] = {static_cast<uint8_t*>(dst[p]), g.h_src[p] + k * pl[p].cbytes, dp[p], pl[p].pitch, pl[p].w * B, pl[p].h};
    }
    if (nj) a->copier->run(jobs, nj);
    sl = sn_aa_context::Slot{};
    return SN_OK;
}

int sn_aa_collect_host(sn_aa_context* a, int32_t slot, void* const dst[3], const int32_t dp[3])
{
    if (!a) return aa_fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    const int per_group = a->plan.per_group;
    if (!a->ring_ready || slot < 0 || slot >= a->plan.depth || a->groups[(size_t)(slot / per_group)].slot[(size_t)(slot % per_group)].state == Context::kFree)
        return aa_fail(a, SN_ERR_INVALID_ARG, "slot " + std::to_string(slot) + " holds no frame");
    if (int rc = aa_check_host_planes(a, dst, dp, true)) return rc;
    SN_AA_HIP(hipSetDevice(a->cfg.device));
    return aa_finish(a, a->groups[(size_t)(slot / per_group)], slot % per_group, dst, dp);
}

// The one-frame case: a slot of its own (so that frames in the ring stay where they are), staged, run and collected at once.
int sn_aa_process_host(sn_aa_context* a, const void* const src[3], const int32_t sp[3], void* const dst[3], const int32_t dp[3],
                       int32_t parity)
{
    if (!a) return sn::fail(nullptr, SN_ERR_INVALID_ARG, "ctx is NULL");
    if (!src || !sp || !dst || !dp) return aa_fail(a, SN_ERR_INVALID_ARG, "plane array is NULL");
    if (int rc = aa_check_host_planes(a, src, sp)) return rc;
    if (int rc = aa_check_host_planes(a, dst, dp, true)) return rc;
    SN_AA_HIP(hipSetDevice(a->cfg.device));
    SN_AA_SN(a->first, prepare_small_launch_scratch(reinterpret_cast<Context*>(a->first)));
    SN_AA_SN(a->second, prepare_small_launch_scratch(reinterpret_cast<Context*>(a->second)));
    for (sn_context* t : a->twin)
        if (t) SN_AA_SN(t, prepare_small_launch_scratch(reinterpret_cast<Context*>(t)));
    if (int rc = aa_ensure_group(a, a->plan.ring_groups, 1)) return rc;
    sn_aa_context::Group& g = a->groups[(size_t)a->plan.ring_groups];
    g.lo = g.hi = 0;
    if (int rc = aa_stage(a, g, 0, src, sp, dst, dp, parity)) return rc;
    return aa_finish(a, g, 0, dst, dp);
}
#undef SN_AA_HIP
#undef SN_AA_SN

}  // extern "C"
#pragma GCC visibility pop

