// sn_internal.h -- shared declarations of libsangnom_hip.so (not part of the public ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "sangnom_hip.h"

namespace sn {

constexpr int kBuffers = 9;  // TOTAL_BUFFERS, /root/reference/src/SangNom2.h:22
constexpr int kMaxColumnParts = 8;  // column parts of one plane (sn_options.column_parts)

// One plane of one launch (all frames of a batch share it; frame f adds f * *_frame_stride).
struct PlaneArgs {
    const uint8_t* src;
    uint8_t* dst;
    int64_t src_frame_stride;  // bytes
    int64_t dst_frame_stride;  // bytes
    int32_t src_pitch;         // bytes
    int32_t dst_pitch;         // bytes
    int32_t w;                 // pixels
    int32_t h_in;              // source rows
    int32_t h_out;             // destination rows
    int32_t offset;            // first kept line (0 or 1)
    int32_t dh;
    int32_t enabled;           // processPlane[i] || dh
    const int32_t* guard;      // pool-path kernels: when set, frame f is worked on only if guard[f] != 0 (sn_band.hip)
    int32_t guard_single;      // ... 1: ONE word decides for every frame of the launch (guard[0]; the redo of a chain that timed out)
    int32_t arith = 0;         // SN_ARITH_*: which instances of the fused sweeps run (the pool kernels take PoolArgs::arith)
    int32_t copied_elsewhere = 0;  // a plane that is not enabled is copied by the caller (sn_aa_*): launch_assemble leaves it alone
};

// Scratch pool geometry (src/SangNom2.cpp:287-288,305-310), in elements of T.
struct PoolArgs {
    uint8_t* base;             // slot 0
    int64_t slot_bytes;        // 9 * rows * stride_e * sizeof(T)
    int32_t stride_e;          // roundup(luma width, 32)
    int32_t bh;                // bufferHeight; a buffer has bh + 1 rows
    const int32_t* guard;      // as PlaneArgs::guard
    int32_t guard_single;      // as PlaneArgs::guard_single
    int32_t rows;              // stage 2 stops before this pool row (0 = bh: the whole pool, as the reference does)
    int32_t slot_step = 0;     // k_prepare / k_finalize: frame f uses slot (slot0 + f * slot_step) % slot_mod
    int32_t slot_mod = 0;      // (0 / 0: slot0 + f)
    int32_t arith = 0;         // SN_ARITH_*: which instances of the integer kernels run (sn_pixel.h, PxA); float ignores it
};

// Stage 2 of a history-carrying clip as a chain of passes (one per processed plane and frame, in the reference's
// order): pass j smooths slot (origin + 1 + j) % slot_mod and takes every cell its own k_prepare did not write --
// columns from w[j % pn] on, rows above nr[j % pn], row 0 -- from the slot of the pass before it.
constexpr int kChainMaxGroups = 8;  // workgroups per buffer of an 8-bit chain (k_smooth_u8_chain<true>)
struct ChainArgs {
    int32_t npass, pn;
    int32_t w[3], nr[3];
    int32_t origin;
    int32_t groups, slack;  // 8-bit: workgroups per buffer (<= 1: one) and the rounds of slack between two of them
    uint32_t* flags;        // groups > 1: kBuffers * kChainMaxGroups * 32 words, zero at launch (rounds completed per workgroup)
    uint32_t* status;       // groups > 1: device word, set when a workgroup stopped waiting for the one before it (zero at launch
                            // unless a test forces the fault: then every wait is skipped, as after a real time-out)
    const uint32_t* only_if;  // != nullptr: the launch runs only if this word is not zero (the guarded redo on one workgroup per buffer)
    int32_t rows;           // > 0: stage 2 stops there (rows 1 .. rows - 1 are smoothed), as PoolArgs::rows
    int32_t nchains, chain_step;  // nchains > 1: that many independent chains of npass passes (blockIdx.y), chain y starting at
                                  // slot origin + y * chain_step (> npass; no wrap around the ring; one workgroup per buffer)
};

struct Context;

// A plane of a strided batch: frame f starts at base + f * fs, its rows are `pitch` bytes apart.  PlaneView is read-only,
// PlaneViewW writable (and readable: it converts).
struct PlaneView {
    const uint8_t* base = nullptr;
    int64_t fs = 0;     // bytes
    int32_t pitch = 0;  // bytes
    PlaneView at(int64_t frame) const { return PlaneView{base + frame * fs, fs, pitch}; }
};
struct PlaneViewW {
    uint8_t* base = nullptr;
    int64_t fs = 0;
    int32_t pitch = 0;
    PlaneViewW at(int64_t frame) const { return PlaneViewW{base + frame * fs, fs, pitch}; }
    operator PlaneView() const { return PlaneView{base, fs, pitch}; }
};

// sn_turn.hip: quarter turn of a plane (right = clockwise), for device-resident anti-aliasing pipelines;
// line_parity 0 / 1: only the destination lines of that parity are written, < 0: all of them
hipError_t launch_turn(hipStream_t s, int bytes, int right, int nframes, PlaneView src, int w, int h, PlaneViewW dst, int line_parity = -1);

// ... and the turn of avg(a, b) (sn_avg.h; the both-fields call): every line is written
hipError_t launch_turn_merge(hipStream_t s, int bytes, int right, int nframes, PlaneView a, PlaneView b, int w, int h, PlaneViewW dst);

// sn_merge.hip: dst = avg(a, b) of the both-fields anti-aliasing call, sample by sample (sangnom_hip.h, "Both fields": integers
// (a + b + 1) >> 1, float (a + b) * 0.5f with every NaN as 0x7FC00000).  dst may be the plane a or b lies in (same base, pitch
// and frame stride); any other overlap is the caller's to refuse.
hipError_t launch_merge(hipStream_t s, int bytes, int nframes, PlaneView a, PlaneView b, int w, int h, PlaneViewW dst);

// sn_reduce.hip: the 2w x 2h plane of the anti-aliasing call with dh back to w x h (of dst): kernel 1 = tent [1 2 1],
// 2 = half-band [-1 0 9 16 9 0 -1], centred on src[2y + oy][2x + ox], edges clamped; integer results clamped to `bits`
hipError_t launch_reduce(hipStream_t s, int bytes, int bits, int kernel, int nframes, PlaneView src, int w, int h, int ox, int oy, PlaneViewW dst);

// sn_mask.hip: the edge mask of the anti-aliasing call.  A Sobel mask of src (w x h; lo, hi in 8-bit scale, expand 0 / 1:
// sangnom_hip.h has the arithmetic) merges aa into src: dst = src where the mask is 0, aa where it is 256.  aa.base == nullptr:
// dst is the mask itself.  dst may be the plane aa lies in (same base, pitch and frame stride); src must not overlap dst.
hipError_t launch_mask_merge(hipStream_t s, int bytes, int bits, int lo, int hi, int expand, int nframes, PlaneView src, PlaneView aa, int w, int h,
                             PlaneViewW dst);
// ... and `planes` (1 or 2) chroma planes of w x h merged through the mask of the luma plane above them, (w << sub_w) x
// (h << sub_h), reduced to chroma's geometry by the block mean (sangnom_hip.h, "Edge mask": mc).  aa[p].base == nullptr (all
// planes or none): dst is the reduced mask.  dst[p] may be the plane aa[p] lies in; luma and src must not overlap dst.
hipError_t launch_mask_merge_luma(hipStream_t s, int bytes, int bits, int lo, int hi, int expand, int nframes, PlaneView luma, int sub_w, int sub_h,
                                  int planes, const PlaneView src[2], const PlaneView aa[2], int w, int h, const PlaneViewW dst[2]);

// sn_sharpen.hip: the contra-sharpening of the anti-aliasing call (sangnom_hip.h, "Contra-sharpening", has the arithmetic).
// aa (w x h, the call's result) is sharpened by amount / 64 (1..255) of an unsharp mask, limited by what src - aa allows
// over 3 x 3, and written to dst.  dst must overlap neither src nor aa.
hipError_t launch_contra_sharpen(hipStream_t s, int bytes, int bits, int amount, int nframes, PlaneView src, PlaneView aa, int w, int h, PlaneViewW dst);

// sn_repair.hip: the rank repair of the anti-aliasing call (sangnom_hip.h, "Rank repair", has the arithmetic).  Each sample of
// aa (w x h, the call's result) is clamped into [a[rank], a[10 - rank]] of the nine src samples around it (rank 1..4) and
// written to dst.  dst may be the plane aa lies in (same base, pitch and frame stride); src must not overlap dst.
hipError_t launch_repair(hipStream_t s, int bytes, int rank, int nframes, PlaneView src, PlaneView aa, int w, int h, PlaneViewW dst);

// sn_uv.hip: semi-planar chroma (a UV plane of U,V sample pairs: NV12 / P016 / NV16 / NV24) <-> a U and a V plane of cw x h
// samples each.  line_parity 0 / 1: only the lines of that parity are read and written (the lines the pass that follows
// keeps), < 0: all of them.  One side is never written: split reads uv, merge reads u and v.
// ss / ds (16-bit samples only): every sample goes through (x >> ss) << ds on its way (MSB-aligned sides: P010 / P012).
hipError_t launch_uv_split(hipStream_t s, int bytes, int nframes, PlaneView uv, int cw, int h, PlaneViewW u, PlaneViewW v, int line_parity = -1, int ss = 0,
                           int ds = 0);
hipError_t launch_uv_merge(hipStream_t s, int bytes, int nframes, PlaneView u, PlaneView v, int cw, int h, PlaneViewW uv, int ss = 0, int ds = 0);
// ... and one plane of w x h 16-bit words on its own: dst = (src >> ss) << ds, the same line_parity; src == dst is allowed
hipError_t launch_shift16(hipStream_t s, int nframes, PlaneView src, int w, int h, PlaneViewW dst, int line_parity, int ss, int ds);

// sn_packed.hip: packed 4:2:2 (one plane of Y, U and V; packing = sn::Packing of sn_surface_layout.h: 1 YUYV, 2 UYVY, 3 v210)
// <-> a Y plane of w x h samples and a U and a V plane of w / 2 x h.  line_parity as above (the pack writes every line).
// ss: the unpack shifts every 16-bit word it reads down; ds: the pack shifts every sample up (MSB-aligned words: Y210 / Y212).
// v210 packs sample & 0x3FF and zero fields for pixels at or beyond w.  One side is never written.
hipError_t launch_unpack(hipStream_t s, int packing, int bytes, int nframes, PlaneView pk, int w, int h, PlaneViewW y, PlaneViewW u, PlaneViewW v,
                         int line_parity, int ss);
hipError_t launch_pack(hipStream_t s, int packing, int bytes, int nframes, PlaneView y, PlaneView u, PlaneView v, int w, int h, PlaneViewW pk, int ds);

// sn_pool_kernels.hip: the three-kernel path over the HBM-resident pool (every format).
hipError_t launch_assemble(hipStream_t s, const PlaneArgs& p, int bytes, int nframes);
hipError_t launch_pool_plane(hipStream_t s, const PlaneArgs& p, const PoolArgs& pool, int bytes,
                             double threshold, int nframes, int slot0);
// (pool_chain_lanes and pool_chain_groups, which pools a chain takes and over how many workgroups: sn_pool_dispatch.h)
hipError_t launch_pool_prepare(hipStream_t s, const PlaneArgs& p, const PoolArgs& pool, int bytes, int nframes, int slot0);
hipError_t launch_pool_finalize(hipStream_t s, const PlaneArgs& p, const PoolArgs& pool, int bytes, double threshold, int nframes,
                                int slot0);
hipError_t launch_pool_chain(hipStream_t s, const PoolArgs& pool, const ChainArgs& chain, int bytes);
// after the guarded redo of a chain launch: *redone += (*fault != 0), and the running count into *host_mirror (host memory the device writes)
hipError_t launch_chain_redo_count(hipStream_t s, const uint32_t* fault, uint32_t* redone, uint32_t* host_mirror);

// Which configurations the fused sweeps serve: sn_route.h (fused_eligible, fused_*plane_eligible, fused_needs_pools,
// sweep_plane_ok, sweep_waves, fused_uv_ok).  A fused launch also does the plane's frame assembly, so launch_assemble must
// not be called for a plane it serves.
// sn_fused_select.hip:
// 8-byte alignment of bases, pitches and frame strides, and pitch * (rows + kFusedRowSlack) <= INT32_MAX on both sides
constexpr int kFusedRowSlack = 16;
bool fused_layout_ok(const PlaneArgs& p);
// The fused sweeps (sn_fused_u8_v3.hip: 8-bit, two virtual wavefronts packed into every register, up to 7680 wide;
// sn_fused_u16_v3.hip: 9..16-bit and sn_fused_f32_v3.hip: float, one pixel per register, up to 3840 wide) behind one entry,
// launch_sweep below.  FusedPool says which sweep a launch is (`mode`: a v3c::Mode of sn_sweep_args.h, which also holds
// the one function that turns a PlaneArgs and a FusedPool into the kernels' arguments) and carries what that mode needs:
// the scratch-pool coupling between the luma sweep and the subsampled-chroma sweeps, the row bands, the column parts.
struct FusedPool {
    int mode;                // v3c::kPlain = plane on its own, kLumaSpill = luma sweep that leaves its smoothed rows, kChroma = chroma sweep,
                             // kPadded = padded plane (no pools), kParts = a plane in column parts (the win_* / store_* / seam_* fields below)
    int sweep_w;             // luma width (the pool's width)
    const uint8_t* pool_in;  // chroma: what the previous pass left
    uint8_t* pool_out;       // luma / first chroma pass: where this pass leaves its rows (may be null)
    int64_t frame_stride;    // bytes between the pools of consecutive frames
    int pool_rows;           // rows per pool buffer
    int pool_row_bytes;      // > 0 (kLumaSpill): pool_out is a pool of the pool path with this row pitch (Args::pool_row_bytes)
    int rows_in, rows_out;   // valid rows in pool_in / rows to write to pool_out
    int sweep_rows;          // chroma: pool rows to sweep
    int cone_w, cone_nr;     // the chroma plane's width and interpolated lines (dependency cone of the hand-off, Args)
    int cone_in, cone_out;   // extra columns: what this pass loads / stores beyond the final pass's cone
    // nbands > 1: the sweep is cut into bands of rows (sn_sweep_args.h); to be verified by launch_band_verify
    int band_rows, band_warm, nbands, band_reset;
    uint32_t* band_state;    // nframes * band_state_words(threads, nbands) words
    int32_t* band_flags;     // one per frame
    // kParts (column parts, sn_sweep_args.h): nparts windows [win_x[k], win_x[k] + win_w) of the plane, each swept as a
    // plane of its own by one launch; columns [store_lo[k], store_hi[k]) of the WINDOW are stored; seam_x[k][side] (window
    // columns, < 0: none) are the seams next to the window's inner edges and seam_off[k][side] where its half of each seam's
    // record starts in the frame's record
    int nparts, win_w;
    int win_x[kMaxColumnParts], store_lo[kMaxColumnParts], store_hi[kMaxColumnParts];
    int seam_x[kMaxColumnParts][2], seam_off[kMaxColumnParts][2];
    uint8_t* seam_rec;
    int64_t seam_frame_stride;
    int seam_bytes;
};
// sn_band.hip: the check of a launch in column parts.  A frame's record is [seam][side][rows][kBuffers][16] samples; side 0
// (the window left of the seam) must equal side 1 bit for bit, else flags[f] is raised and the frame counted, as above.
inline int64_t parts_side_bytes(int bytes, int rows) { return (int64_t)rows * kBuffers * 16 * bytes; }
hipError_t launch_parts_verify(hipStream_t s, const uint8_t* rec, int64_t frame_stride, int64_t side_bytes, int nseams, int nframes,
                               int32_t* flags, int64_t* fallbacks, int64_t* host_mirror);
// sn_band.hip: words of band state per frame for a sweep of `threads` threads; the check of a band launch -- flags[f] != 0
// afterwards means frame f has to be redone by the pool path (its guarded launches look at the same flags);
// *fallbacks (device memory, may be null) counts such frames, *host_mirror (host memory the device can write, may be
// null) receives the count as well.
inline int64_t band_state_words(int threads, int nbands) { return (int64_t)nbands * 2 * kBuffers * 8 * threads; }
hipError_t launch_band_verify(hipStream_t s, const uint32_t* state, int threads, int nbands, int nframes, int32_t* flags, int64_t* fallbacks,
                              int64_t* host_mirror);
// sn_fused_select.hip: one sweep of `nframes` frames of plane p.  pool == nullptr: a plane on its own (kPlain); a launch the
// kernels have no instance for is hipErrorInvalidValue (v3c::build_sweep)
hipError_t launch_sweep(hipStream_t s, int bytes_per_sample, const PlaneArgs& p, double threshold, int nframes, const FusedPool* pool);
int64_t sweep_pool_bytes(int bytes_per_sample, int sweep_w, int rows);  // one hand-off pool of one frame: [9][rows][threads] slots
// host: scatter one hand-off pool (thread-slot layout) into [9][rows][sweep_w] samples (test hook)
void sweep_pool_unpack(int bytes_per_sample, const uint32_t* raw, int sweep_w, int rows, void* out);
// sn_fused_u8_uv.hip: the U and V passes of an 8-bit 4:2:0 frame as one sweep (U in the low halves of the registers, V in the
// high halves two rows behind); `pool`: sweep_w, pool_in / frame_stride / pool_rows / rows_in = the luma sweep's hand-off
// pool, sweep_rows = the U pass's last row.
hipError_t launch_fused_u8_uv(hipStream_t s, const PlaneArgs& pu, const PlaneArgs& pv, double thr_u, double thr_v, int nframes, const FusedPool& pool);
#ifdef SN_EXPERIMENT_V4  // tools/experiments/sn_fused_u8_v4.hip (four waves per SIMD; slower: profiles/r2_v4_experiment.md)
bool fused_v4_plane_ok(int w);
int fused_v4_waves(int w);
hipError_t launch_fused_u8_v4(hipStream_t s, const PlaneArgs& p, double threshold, int nframes);
#endif

}  // namespace sn
