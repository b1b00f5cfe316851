// sn_route.h -- which kernels serve a clip and a launch: every decision the host takes over the clip's geometry, with no
// device call in it.  A host compiler takes this header as it is (tests/c/route_check.cpp checks the answers against
// values written out by hand and answers queries for tests/test_small_planes_cpu.py).  sn_api.hip asks it: clip_plan()
// when a context is created, decide_launch() once per launch (run_group).
#pragma once

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <string>

#include "sangnom_hip.h"
#include "sn_surface_plan.h"
#include "sn_sweep_args.h"

namespace sn {

// ---- widths: which planes the fused sweeps serve ----------------------------------------------------------------------
// A configuration is eligible when every plane fits one workgroup (width a multiple of 32; up to 7680 columns for
// 8-bit, 3840 for 16-bit and float samples) and either every processed plane is as large as the pool (no pass can
// see another pass's leftovers: SURVEY.md 0.7) or the chroma planes are subsampled AND luma is processed first --
// then the sweeps couple the passes through hand-off pools; without a luma pass the chroma passes
// would see the previous FRAME's leftovers, which only the pool path reproduces.
inline bool fused_needs_pools(const sn_config& c)  // subsampled chroma: luma / chroma sweeps coupled through scratch pools
{
    const int np = c.num_planes < 3 ? c.num_planes : 3;
    return np == 3 && (c.dh || c.chroma) && (c.sub_w != 0 || c.sub_h != 0);
}

inline int sweep_waves(int bytes_per_sample, int sweep_w)  // waves of a workgroup that sweeps sweep_w columns
{
    const int nvw = v3c::strips_for(sweep_w / v3c::PXL);
    return v3c::sweep_traits(bytes_per_sample).packed ? (nvw + 1) / 2 : nvw;
}

// w within what one workgroup of the type's sweep takes (a multiple of 32)
inline bool sweep_plane_ok(int bytes_per_sample, int w) { return w % 32 == 0 && sweep_waves(bytes_per_sample, w) <= v3c::sweep_traits(bytes_per_sample).max_waves; }

// one plane of width w on its own (plain sweep): sample size and width within what the fused kernels take
inline bool fused_plane_eligible(int bytes_per_sample, int w) { return sweep_plane_ok(bytes_per_sample, w); }

// ... swept over its pool stride roundup(w, 32) with zero costs in the padding (fresh_pool)
inline bool fused_padded_plane_eligible(int bytes_per_sample, int w)
{
    if (w % 8 != 0) return false;  // the plane must end on a lane boundary (8 columns per lane)
    return fused_plane_eligible(bytes_per_sample, (w + 31) & ~31);
}

// ... too wide for one workgroup but served in column parts (sn_options.column_parts): 16-bit / float, w % 32 == 0, w <= 8192
inline bool fused_parts_plane_eligible(int bytes_per_sample, int w)
{
    if (bytes_per_sample != 2 && bytes_per_sample != 4) return false;
    if (w % 32 != 0 || w > 8192) return false;
    return !fused_plane_eligible(bytes_per_sample, w);
}

inline bool fused_eligible(const sn_config& c)
{
    if (!fused_plane_eligible(c.bytes_per_sample, c.width)) return false;
    if (fused_needs_pools(c)) {
        if (!(c.dh || c.luma)) return false;
        if ((c.width >> c.sub_w) % 8 != 0) return false;
    }
    return true;
}

namespace uv {                // sn_fused_u8_uv.hip: U and V of an 8-bit frame as one sweep
constexpr int kSkew = 2;      // steps the V pass runs behind the U pass
constexpr int kMaxWaves = 8;  // strips of the luma-wide pool: 3840 columns
}  // namespace uv

// Which subsampled geometries the one-sweep chroma passes take; everything else keeps the two chroma sweeps of
// sn_fused_u8_v3.hip.  Both chroma planes processed and alike, the region a whole number of lanes, enough rows for the skew.
// 4:2:0: the U pass has an extra row (nr_c + 1) and the V pass's last row finds it; 4:2:2: the pool ends with the chroma
// planes' last row, the U pass has no extra row and V's last row takes nothing from it.
inline bool fused_uv_ok(int sweep_w, int region_w, int nk_c, int bh)
{
    if (sweep_w % 32 != 0 || region_w % 8 != 0 || region_w <= 0 || region_w >= sweep_w) return false;
    if (v3c::strips_for(sweep_w / v3c::PXL) > uv::kMaxWaves) return false;
    const int nr = nk_c - 1;
    return nr >= 2 * uv::kSkew + 2 && nr <= bh - 1;
}

// ---- the clip's plan ----------------------------------------------------------------------------------------------------
// Rows of the hand-off pools a coupled chroma sweep can reach: 1 .. min(nr_c + 2, bh - 1) (plus row 0), and the last
// row of the U sweep
inline int coupled_reach(int nr_c, int bh) { return nr_c + 2 < bh - 1 ? nr_c + 2 : bh - 1; }
inline int coupled_sweep_u(int nr_c, int bh) { return nr_c + 1 < bh - 1 ? nr_c + 1 : bh - 1; }

// Everything creation derives from sn_config, the arithmetic, column_parts and the policy, before it touches the device.
struct ClipPlan {
    sn_config cfg{};
    int arith = SN_ARITH_CXX;  // sn_options.arithmetic, fixed for the context's life
    bool parts_on = false;     // sn_options.column_parts
    // a refusal on geometry alone (SN_OK: none): what sn_create_* returns, and its text
    int refusal = SN_OK;
    std::string refusal_text;

    int out_height = 0;  // vi.height after dh, SangNom2.cpp:284-285
    int stride_e = 0;    // SangNom2.cpp:287
    int bh = 0;          // SangNom2.cpp:288
    float aaf[3] = {0, 0, 0};
    bool process[3] = {true, true, true};
    bool history_free = false;
    // cfg.isolated_planes: every plane is its own filter instance (own pool geometry, own pool)
    bool isolated = false;
    // cfg.fresh_pool: on top of that every frame starts from a zero-filled pool (planes narrower than their pool
    // stride are swept over the whole stride with zero costs in the padding columns)
    bool fresh = false;
    // SN_ARITH_SSE2 on integer samples: the saturating instances of the pool kernels (float has one arithmetic)
    bool saturating = false;
    // ... and which sweeps it uses there.  Every sweep has such instances, but by default (sn_policy.sse2_sweeps = 0) a
    // context keeps the kernels of the release that introduced the arithmetic: sweeps for 8-bit planes on their own
    // (plain, padded and row-band sweeps of sn_fused_u8_v3.hip), the pool kernels for the pool-coupled sweeps of subsampled
    // chroma and for 9..16-bit clips.  sse2_sweeps = 1: whatever has sweeps in the default arithmetic
    bool saturating_sweeps = false;

    // pool geometry (stride_e, bh, slot_bytes, arith) of the shared pool and of the planes' own; base stays null here:
    // the context allocates on first use
    PoolArgs pool{};
    PoolArgs plane_pool[3] = {};
    bool plane_fused[3] = {false, false, false};
    bool plane_padded[3] = {false, false, false};
    bool plane_parts[3] = {false, false, false};  // the plane is too wide for one workgroup and is cut (column parts)
    bool parts_eligible = false;                  // ... and what sn_info.fused_eligible says of such a context
    bool use_fused = false;
    // fused path with subsampled chroma: hand-off pools between the sweeps (sn_fused_u8_v3.hip, Mode), fpool_rows rows each
    bool fused420 = false;
    int fpool_rows = 0;
    bool uv_geometry = false;  // the clip's geometry allows U and V as one sweep (then only the luma -> U pool exists from the start)

    int plane_w(int p) const { return p == 0 ? cfg.width : cfg.width >> cfg.sub_w; }
    int plane_h_in(int p) const { return p == 0 ? cfg.height : cfg.height >> cfg.sub_h; }
    int plane_h_out(int p) const { return p == 0 ? out_height : out_height >> cfg.sub_h; }
    int nplanes() const { return cfg.num_planes < 3 ? cfg.num_planes : 3; }
    bool enabled(int p) const { return cfg.dh || process[p]; }  // processPlane[p] || dh
};

// A frame's result cannot depend on earlier frames iff every pool cell that a pass reads was
// written earlier in the same frame or is never written at all (rows 0 and bh).  See SURVEY.md
// section 0.7 / 7-H2: needs stride_e == width, and for subsampled chroma a luma pass before it.
inline bool compute_history_free(const ClipPlan& c)
{
    if (c.stride_e != c.cfg.width) return false;
    if (c.nplanes() == 1) return true;
    const bool luma_pass = c.cfg.dh || c.cfg.luma;
    const bool chroma_pass = c.cfg.dh || c.cfg.chroma;
    if (!chroma_pass) return true;
    if (c.cfg.sub_w == 0 && c.cfg.sub_h == 0) return true;  // chroma rewrites the whole pool
    return luma_pass;
}

__attribute__((format(printf, 3, 4))) inline const ClipPlan& refuse(ClipPlan& c, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    c.refusal = code;
    c.refusal_text = buf;
    return c;
}

inline ClipPlan clip_plan(const sn_config& cfg, int arith, bool column_parts, const sn_policy& policy)
{
    ClipPlan c;
    c.cfg = cfg;
    c.arith = arith;
    c.parts_on = column_parts;
    // constructor arithmetic, SangNom2.cpp:276-288
    const int aa[3] = {cfg.aa, cfg.aac, cfg.aac};
    for (int i = 0; i < c.nplanes(); ++i)
        c.aaf[i] = cfg.bytes_per_sample < 4
                       ? (aa[i] * 21.0f / 16.0f) * (float)(1 << (cfg.bits_per_sample - 8))
                       : (aa[i] * 21.0f / 16.0f) / 256.0f;
    for (int p = 0; p < 3; ++p) c.process[p] = plane_selected(cfg, p);
    c.out_height = cfg.dh ? cfg.height * 2 : cfg.height;
    c.stride_e = (cfg.width + 31) & ~31;
    c.bh = (c.out_height + 1) >> 1;
    if (c.stride_e > 8192) return refuse(c, SN_ERR_UNSUPPORTED, "width %d exceeds the supported maximum of 8192", cfg.width);
    if (c.out_height / 2 > 65535) return refuse(c, SN_ERR_UNSUPPORTED, "height %d exceeds the supported maximum", cfg.height);
    c.history_free = compute_history_free(c);
    c.fresh = cfg.fresh_pool != 0;
    c.isolated = c.fresh || (cfg.isolated_planes != 0 && c.nplanes() > 1);
    c.saturating = arith == SN_ARITH_SSE2 && cfg.bytes_per_sample < 4;
    c.saturating_sweeps = policy.sse2_sweeps == 1 || (cfg.bytes_per_sample == 1 && (c.isolated || !fused_needs_pools(cfg)));

    bool eligible = fused_eligible(cfg);
    if (c.isolated) {
        // Every plane as its own Y clip: pool stride and height from the plane itself, nothing shared -- what a
        // script gets from ExtractY/U/V -> SangNom2 -> CombinePlanes with the reference.  A plane is history-free
        // iff its own width is a multiple of 32, and then the plain fused sweep serves it.
        c.history_free = true;
        eligible = true;
        for (int p = 0; p < c.nplanes(); ++p) {
            PoolArgs& pool = c.plane_pool[p];
            pool.stride_e = (c.plane_w(p) + 31) & ~31;
            pool.bh = (c.plane_h_out(p) + 1) >> 1;
            pool.slot_bytes = ((int64_t)kBuffers * (pool.bh + 1) * pool.stride_e * cfg.bytes_per_sample + 255) & ~(int64_t)255;
            if (!c.enabled(p)) continue;  // copied planes need nothing
            if (pool.stride_e != c.plane_w(p) && !c.fresh) c.history_free = false;
            c.plane_fused[p] = fused_plane_eligible(cfg.bytes_per_sample, c.plane_w(p));
            if (!c.plane_fused[p] && c.parts_on && !c.fresh && fused_parts_plane_eligible(cfg.bytes_per_sample, c.plane_w(p)))
                c.plane_fused[p] = c.plane_parts[p] = true;  // in column parts
            if (c.fresh && !c.plane_fused[p] && fused_padded_plane_eligible(cfg.bytes_per_sample, c.plane_w(p)))
                c.plane_fused[p] = c.plane_padded[p] = true;
            eligible = eligible && c.plane_fused[p];
        }
    }
    if (!c.isolated && !eligible && c.parts_on && !fused_needs_pools(cfg) && fused_parts_plane_eligible(cfg.bytes_per_sample, cfg.width)) {
        // Y and 4:4:4 (and clips whose subsampled chroma is only copied): every processed plane is as wide as the pool
        eligible = true;
        for (int p = 0; p < c.nplanes(); ++p) c.plane_parts[p] = c.enabled(p) && c.plane_w(p) == cfg.width;
    }
    if (arith == SN_ARITH_SSE2) {
        // The reference's SSE2 stage drivers read one vector to the left of the last full one, so its output is defined
        // for planes of at least two vectors (src/SangNom2_SSE2.cpp:705-715): 32 / 16 / 8 samples.  Every processed plane.
        const int least = 32 / cfg.bytes_per_sample;
        for (int p = 0; p < c.nplanes(); ++p)
            if (c.enabled(p) && c.plane_w(p) < least)
                return refuse(c, SN_ERR_UNSUPPORTED,
                              "SN_ARITH_SSE2: plane %d is %d samples wide; the reference's SSE2 path is defined from %d samples (two vectors) on", p,
                              c.plane_w(p), least);
    }
    if (c.saturating) {
        // Without sn_policy.sse2_sweeps only the 8-bit sweeps of planes on their own run in this arithmetic; every other
        // integer plane runs on the pool kernels, and the context says so (sn_info.fused_eligible = 0).  DESIGN.md 4.5.
        if (!c.saturating_sweeps) {
            if (cfg.mode == SN_MODE_FUSED)
                return refuse(c, SN_ERR_UNSUPPORTED,
                              "SN_MODE_FUSED requested but in SN_ARITH_SSE2 only 8-bit planes on their own have fused sweeps; "
                              "this clip (%s) runs on the pool path in that mode",
                              cfg.bytes_per_sample == 2 ? "9..16-bit samples" : "subsampled chroma sharing the luma pool");
            eligible = false;
            for (int p = 0; p < 3; ++p) c.plane_fused[p] = c.plane_padded[p] = c.plane_parts[p] = false;
        }
        c.pool.arith = SN_ARITH_SSE2;
        for (int p = 0; p < 3; ++p) c.plane_pool[p].arith = SN_ARITH_SSE2;
    }
    if (cfg.mode == SN_MODE_FUSED && !eligible) return refuse(c, SN_ERR_UNSUPPORTED, "SN_MODE_FUSED requested but this configuration is not eligible");
    c.use_fused = eligible && cfg.mode != SN_MODE_POOL;
    c.parts_eligible = eligible;
    c.fused420 = c.use_fused && !c.isolated && fused_needs_pools(cfg);
    if (cfg.mode == SN_MODE_POOL)  // the pool path serves every plane
        for (int p = 0; p < 3; ++p) {
            if (c.isolated) c.plane_fused[p] = false;
            c.plane_parts[p] = false;
        }
    c.pool.stride_e = c.stride_e;
    c.pool.bh = c.bh;
    c.pool.slot_bytes = ((int64_t)kBuffers * (c.bh + 1) * c.stride_e * cfg.bytes_per_sample + 255) & ~(int64_t)255;
    if (c.fused420) {
        c.fpool_rows = coupled_reach(c.plane_h_out(1) / 2 - 1, c.bh) + 1;
        // 8-bit clips whose U and V passes run as one sweep (sn_fused_u8_uv.hip) need the luma -> U pool only; the U -> V pool of
        // the two-sweep form is allocated when that form first runs (sn_policy.chroma_sweeps = 1, or a launch of planes the one
        // sweep does not take)
        c.uv_geometry = cfg.bytes_per_sample == 1 && c.plane_w(1) == c.plane_w(2) && c.plane_h_out(1) == c.plane_h_out(2) &&
                        fused_uv_ok(cfg.width, c.plane_w(1), c.plane_h_out(1) / 2, c.bh);
    }
    return c;
}

// ---- fields and kept lines --------------------------------------------------------------------------------------------
// (field_offset, GetFrame's field choice: sn_surface_plan.h, with the cutter of runs of frames)
// Of a processed plane only the kept field is ever read (the other lines are the ones being interpolated,
// SangNom2.cpp:361-366), so only those lines need to cross PCIe: line `first`, then every `step`-th, `rows` of them.  A
// copied plane and a double-height clip (whose every line is kept) go as a whole.
struct KeptLines {
    int first, step, rows;
};

inline KeptLines kept_lines(const ClipPlan& c, int p, int parity)
{
    if (c.cfg.dh || !c.process[p]) return {0, 1, c.plane_h_in(p)};
    return {field_offset(c.cfg.order, parity), 2, c.plane_h_out(p) / 2};
}

// ---- column parts -----------------------------------------------------------------------------------------------------
// Column parts (sn_options.column_parts): a 16-bit or float plane on its own that is too wide for one workgroup is cut into
// 2 .. kMaxParts windows of at most kPartsWindow columns -- four waves, so that two workgroups share a compute unit as the
// sweeps of narrower planes do.  Seams lie on multiples of 32; a window reaches at least kPartsGhost columns (rounded up to
// 32) beyond each of its seams; all windows of a plane are equally wide, so that one launch sweeps them all (the narrower
// ones are widened, away from the image edge or to both sides).  DESIGN.md 4.6 has the numbers behind the ghosts.
constexpr int kMaxParts = kMaxColumnParts;
constexpr int kPartsWindow = (v3c::kFirst + 3 * v3c::kInner) * v3c::PXL;  // 1936
constexpr int kPartsGhost16 = 64, kPartsGhost32 = 96;
struct PartsPlan {
    int n = 0;
    int win_w = 0;
    int win_x[kMaxParts] = {};
    int seam[kMaxParts + 1] = {};  // seam[k], k = 1 .. n - 1: the first own column of part k
};
inline int parts_ghost(int bytes_per_sample) { return bytes_per_sample == 2 ? kPartsGhost16 : kPartsGhost32; }

// parts_force / ghost_force: sn_debug_set_column_parts (0: choose)
inline bool plan_parts(const ClipPlan& c, int p, int parts_force, int ghost_force, PartsPlan& pl)
{
    pl.n = 0;
    const int B = c.cfg.bytes_per_sample;
    if (!c.parts_on || B < 2 || c.fresh || p >= c.nplanes()) return false;
    if (!c.enabled(p)) return false;
    if (c.isolated ? c.plane_padded[p] : fused_needs_pools(c.cfg)) return false;  // planes on their own only
    const int w = c.plane_w(p);
    if (w % 32 != 0 || c.plane_h_out(p) / 2 - 1 < 1) return false;
    const int G = (parts_ghost(B) + 31) & ~31;
    int P = parts_force;
    if (P == 0) {
        if (!fused_parts_plane_eligible(B, w)) return false;
        for (P = 2; P <= kMaxParts; ++P)
            if ((((w + P - 1) / P + 31) & ~31) + 2 * G <= kPartsWindow) break;
    }
    if (P < 2 || P > kMaxParts) return false;
    pl.seam[0] = 0;
    pl.seam[P] = w;
    for (int k = 1; k < P; ++k) pl.seam[k] = (int)(((int64_t)k * w / P + 16) & ~31);
    int lo[kMaxParts], ww = 0;
    for (int k = 0; k < P; ++k) {
        if (pl.seam[k + 1] - pl.seam[k] < 32) return false;  // not wide enough to hold that many parts
        lo[k] = k == 0 ? 0 : pl.seam[k] - G;
        const int hi = k == P - 1 ? w : pl.seam[k + 1] + G;
        if (lo[k] < 0 || hi > w) return false;
        ww = hi - lo[k] > ww ? hi - lo[k] : ww;
    }
    if (v3c::strips_for(ww / v3c::PXL) > 8) return false;
    pl.win_w = ww;
    for (int k = 0; k < P; ++k) {  // every window as wide as the widest
        const int hi = k == P - 1 ? w : pl.seam[k + 1] + G;
        int x = lo[k] - (((ww - (hi - lo[k])) / 2) & ~31);
        x = x < 0 ? 0 : x > w - ww ? w - ww : x;
        pl.win_x[k] = x;
    }
    if (ghost_force > 0) {  // the test hook: every seam that far from the end of the window left of it
        for (int k = 1; k < P; ++k) {
            pl.seam[k] = pl.win_x[k - 1] + pl.win_w - ghost_force;
            if (pl.seam[k] < pl.win_x[k] + 8 || pl.seam[k] <= pl.seam[k - 1]) return false;
        }
    }
    pl.n = P;
    return true;
}

// ---- what a launch brings ---------------------------------------------------------------------------------------------
// The launch itself, and the context's state and test hooks the decision reads.
struct LaunchInput {
    int n = 1, slot0 = 0;                           // frames, first scratch slot
    bool layout_ok[3] = {true, true, true};         // fused_layout_ok of the plane's pointers and pitches
    bool sweeps_always = false;                     // SN_SMALL_SWEEP
    int band_force = 0, band_warm = 0;              // sn_debug_set_bands
    int parts_force = 0, parts_ghost_force = 0;     // sn_debug_set_column_parts
    int slots = 1, parts_slots = 0;                 // pool slots, slots of the seam record
    bool seam_record = false;                       // the seam record exists
    int chroma_sweeps = 0;                          // sn_policy.chroma_sweeps
};

// After a launch with a frame that failed its check (row bands, column parts) the next launches go straight to the pool
// path: content on which the check keeps failing (flat or periodic material) would pay for both.  8 launches, twice as
// many after every further failure up to 1024; 64 good launches in a row forget it.  `fallbacks`: the running count of
// failed frames as of the last such launch that has finished.  True: this launch is paused.
struct FallbackPause {
    int64_t seen = 0;
    int pause = 0, next = 0, good = 0;
    bool paused(int64_t fallbacks)
    {
        if (fallbacks != seen) {
            seen = fallbacks;
            next = next < 8 ? 8 : next < 1024 ? 2 * next : 1024;
            pause = next;
            good = 0;
        } else if (pause == 0 && ++good >= 64) {
            next = 0;
        }
        if (pause == 0) return false;
        --pause;
        return true;
    }
    void forget() { pause = next = good = 0; }
};

// ---- small launches: the pool path or the sweeps ------------------------------------------------------------------------
// A fused sweep walks a plane row by row: its time hardly depends on how many frames the launch carries (up to a round of
// resident workgroups) but it never takes less than rows x 2.6 - 4.7 us.  The pool path spreads ONE frame over the whole chip
// and costs 13 - 33 ps per pool element and frame beyond that.  Both are exact, so in SN_MODE_AUTO a launch that is neither cut
// into row bands (band_count) nor large goes to whichever this estimate says is faster.  Constants: fitted in round 4 to
// tools/prefer_pool_calib.py (profiles/r4_prefer_pool.md: launches of 1 .. 128 device-resident frames through both paths, 1080p /
// 2160p / 4320p, the three sample types, 4:2:0) -- round 1's had the pool path's fixed cost three times too high (stage 2 has
// since moved to the strip kernels) and a row of a sweep that has its CU to itself 30 % too slow, which cancelled except at
// 4320p, where launches of 16 .. 32 frames took the sweeps at up to twice the pool path's time.
//   sweep: rows x t_row; t_row = 2.6 us (8-bit; 3.8 us for planes of more than eight strips: eight waves), 2.8 us (16-bit),
//          4.3 us (float); the chroma planes of a coupled 4:2:0 clip sweep the luma-wide pool: 8-bit U and V as one sweep
//          3.8 us per chroma row for both (1.9 us booked to each plane), otherwise 3.0 us (8-bit) / 3.15 us (16-bit) / 4.7 us
//          (float) per row and plane
//   pool : bh x (a + 0.036 us x ceil(stride / 1024)) + 60 us + n x stride x bh x per_elem per processed plane;
//          a = 0.25 / 0.22 / 0.33 us, per_elem = 12.9 / 19.4 / 32.6 ps for 8-bit / 16-bit / float
inline bool prefer_pool(const ClipPlan& c, const LaunchInput& in)
{
    const int n = in.n;
    if (c.cfg.mode != SN_MODE_AUTO || !c.history_free || in.slot0 + n > in.slots) return false;
    if (in.sweeps_always) return false;  // SN_SMALL_SWEEP (the tests use it to reach the sweeps with small clips)
    const int B = c.cfg.bytes_per_sample;
    const double per_elem = B == 1 ? 12.9e-12 : B == 2 ? 19.4e-12 : 32.6e-12;
    const double a_fix = B == 1 ? 0.25e-6 : B == 2 ? 0.22e-6 : 0.33e-6;
    double fused = 0, pool = 0;
    for (int p = 0; p < c.nplanes(); ++p) {
        if (!c.enabled(p)) continue;
        const bool own = c.isolated;  // own pool geometry per plane, else the luma-sized shared pool
        const int stride = own ? c.plane_pool[p].stride_e : c.stride_e;
        const int bh = own ? c.plane_pool[p].bh : c.bh;
        const int rows = c.plane_h_out(p) / 2;
        const bool coupled_chroma = c.fused420 && p > 0;
        double t_row = B == 1 ? (stride > 3840 ? 3.8e-6 : 2.6e-6) : B == 2 ? 2.8e-6 : 4.3e-6;
        if (coupled_chroma) t_row = B == 1 ? (c.uv_geometry && in.chroma_sweeps == 0 ? 1.9e-6 : 3.0e-6) : B == 2 ? 3.15e-6 : 4.7e-6;
        fused += rows * t_row;
        const int cols_per_thread = (stride + 1023) / 1024;
        // (a pass of the shared pool stops at the last row a later pass of this frame can still read: pool_stops)
        const int bh_run = !own && rows + 2 < bh ? rows + 2 : bh;
        pool += bh_run * (a_fix + 0.036e-6 * cols_per_thread) + 60e-6 + (double)n * stride * bh_run * per_elem;
    }
    return pool < fused;
}

// ---- row bands ----------------------------------------------------------------------------------------------------------
// Row bands: a launch of a few frames -- a synchronous GetFrame, a short look-ahead -- cannot fill the
// device with one workgroup per frame, so each frame is cut into bands of rows that start from a guessed state and are
// verified afterwards (sn_sweep_args.h, sn_band.hip).  The run-up is what the guess needs to be forgotten on
// ordinary content: 8-bit sums settle within 17-23 rows of noise, 16-bit within 30, float within 37.
constexpr int kMaxBands = 128;
constexpr int kMinBandRows = 8;
constexpr int kMaxBandSlots = 192;  // launches of more frames than that fill the device without bands

inline int band_warm_rows(int bytes_per_sample, int band_warm)  // band_warm: sn_debug_set_bands (0 = the default of the sample type)
{
    if (band_warm > 0) return band_warm;
    return bytes_per_sample == 1 ? 32 : bytes_per_sample == 2 ? 40 : 48;
}

// Rows of the shortest processed plane if this context can cut small launches into bands at all, else 0.
inline int band_rows_available(const ClipPlan& c, int band_force, int parts_force)
{
    if (c.plane_parts[0] || c.plane_parts[1] || c.plane_parts[2] || parts_force > 0) return 0;  // never combined with column parts
    if (band_force < 0 || c.cfg.mode != SN_MODE_AUTO || !c.history_free) return 0;
    if (c.isolated) {  // every processed plane must have the sweep for planes on their own (not the padded one)
        for (int p = 0; p < c.nplanes(); ++p)
            if (c.enabled(p) && (!c.plane_fused[p] || c.plane_padded[p])) return 0;
    } else if (!c.use_fused) {
        return 0;
    }
    int nr_min = 1 << 30;
    for (int p = 0; p < c.nplanes(); ++p)
        if (c.enabled(p)) nr_min = c.plane_h_out(p) / 2 - 1 < nr_min ? c.plane_h_out(p) / 2 - 1 : nr_min;
    return nr_min == (1 << 30) || nr_min < 2 * kMinBandRows ? 0 : nr_min;
}

// Bands per frame for the launch, 0 = do not cut -- before the pause (FallbackPause) has its say.
inline int band_count(const ClipPlan& c, const LaunchInput& in)
{
    const int nr_min = band_rows_available(c, in.band_force, in.parts_force);
    if (nr_min == 0) return 0;
    if (in.slot0 + in.n > in.slots || in.slot0 + in.n > kMaxBandSlots) return 0;  // the fallback needs the frames' pool slots
    if (in.band_force == 0 && in.sweeps_always) return 0;  // whole-plane sweeps always (see prefer_pool)
    int nb = in.band_force > 0 ? in.band_force : 512 / in.n;  // about two workgroups per CU in all
    if (nb > nr_min / kMinBandRows) nb = nr_min / kMinBandRows;
    if (nb > kMaxBands) nb = kMaxBands;
    if (nb < (in.band_force > 0 ? 2 : 3)) return 0;  // a launch of hundreds of frames fills the device with whole-plane sweeps
    const int warm = band_warm_rows(c.cfg.bytes_per_sample, in.band_warm);
    if (in.band_force == 0 && nr_min / nb < warm / 4) nb = nr_min / (warm / 4);  // run-up <= 4 x own rows
    return nb < 2 ? 0 : nb;
}

// The plane goes through the sweeps unless a later step of decide_launch takes it off them
inline bool plane_swept(const ClipPlan& c, const LaunchInput& in, int p) { return c.enabled(p) && (c.isolated ? c.plane_fused[p] : c.use_fused) && in.layout_ok[p]; }

// ... for the launch as a whole: bands only if every processed plane goes through the sweeps
inline int launch_bands(const ClipPlan& c, const LaunchInput& in)
{
    for (int p = 0; p < c.nplanes(); ++p)
        if (c.enabled(p) && !plane_swept(c, in, p)) return 0;
    return band_count(c, in);
}

// The bands of one sweep over pool rows 1 .. last, at most `want` of them.
struct BandGeometry {
    int band_rows, nbands;
};
inline BandGeometry band_geometry(int want, int last)
{
    int nb = want < last / kMinBandRows ? want : last / kMinBandRows;
    if (nb < 1) nb = 1;
    BandGeometry g;
    g.band_rows = (last + nb - 1) / nb;
    g.nbands = (last + g.band_rows - 1) / g.band_rows;
    if (g.nbands < 2) {  // a launcher takes one band as "not cut"; two bands of which the second is empty cannot happen
        g.band_rows = (last + 1) / 2;
        g.nbands = 2;
    }
    return g;
}

// ---- chains -------------------------------------------------------------------------------------------------------------
// The geometry half of "the batch of a history-carrying clip runs as a chain of passes": the processed planes in order,
// 0 = no chain.  lanes: pool_chain_lanes() of the pool (passes one workgroup keeps in flight).
inline int chain_planes(const ClipPlan& c, int lanes, int planes[3])
{
    if (c.history_free || c.isolated || c.cfg.mode == SN_MODE_FUSED) return 0;
    if (lanes < 2 || c.bh < 2) return 0;
    int pn = 0;
    for (int p = 0; p < c.nplanes(); ++p) {
        if (!c.enabled(p)) continue;
        if (c.plane_w(p) % 8 != 0 || c.plane_h_out(p) / 2 - 1 >= c.bh || c.plane_h_out(p) / 2 - 1 < 1) return 0;
        planes[pn++] = p;
    }
    return pn;
}

// ---- the launch ---------------------------------------------------------------------------------------------------------
enum class Route {
    kPlanes,         // every plane on its own: a whole-plane sweep (plain, padded, in column parts) or the pool path
    kBandedPlanes,   // every plane in row bands
    kCoupled,        // fused 4:2:0: luma, U and V sweeps coupled through the hand-off pools
    kCoupledBanded,  // a small 4:2:0 launch: luma in bands, chroma by the pool kernels
};

struct LaunchDecision {
    bool fused[3] = {false, false, false};  // the plane goes through the sweeps
    PartsPlan plan[3];                       // ... in column parts where plan[p].n > 0
    int stop[3] = {0, 0, 0};                 // where stage 2 of the pool path may stop (PoolArgs::rows)
    int nbands = 0;                          // > 0: the launch is small enough for row bands
    Route route = Route::kPlanes;
    bool parts_cut = false;  // planes of this launch are cut and nothing but the pause (parts_paused) sends them to the pool path
};

// What a launch goes through.  bands_paused / parts_paused: FallbackPause's answer where it was asked -- for the bands when
// launch_bands() > 0 without sn_debug_set_bands, for the parts when parts_cut -- else false.
inline LaunchDecision decide_launch(const ClipPlan& c, const LaunchInput& in, bool bands_paused, bool parts_paused)
{
    LaunchDecision d;
    for (int p = 0; p < c.nplanes(); ++p) d.fused[p] = plane_swept(c, in, p);
    d.nbands = bands_paused ? 0 : launch_bands(c, in);
    if (d.nbands == 0 && prefer_pool(c, in))
        for (int p = 0; p < 3; ++p) d.fused[p] = false;
    // Column parts: which planes of this launch are cut
    bool any_parts = false;
    for (int p = 0; p < c.nplanes(); ++p) any_parts = (d.fused[p] && plan_parts(c, p, in.parts_force, in.parts_ghost_force, d.plan[p])) || any_parts;
    if (any_parts) {
        // under SN_SMALL_AUTO a launch small enough for row bands goes where it went before the option existed
        bool to_pool = in.slot0 >= in.parts_slots || in.slot0 >= in.slots || !in.seam_record;
        if (c.cfg.mode == SN_MODE_AUTO && !in.sweeps_always && 512 / in.n >= 3) to_pool = true;
        d.parts_cut = !to_pool;
        if (to_pool || parts_paused) {
            // the planes that only the parts can sweep go to the pool path; forced parts of a narrower plane to its whole-plane sweep
            for (int p = 0; p < c.nplanes(); ++p) {
                if (d.plan[p].n > 0 && c.plane_parts[p]) d.fused[p] = false;
                d.plan[p].n = 0;
            }
        }
    }
    // Creation marks a plane for column parts by its width alone (plane_parts), and plan_parts cuts only planes with a row to
    // interpolate.  A marked plane without a plan has no whole-plane sweep to fall back on -- it is wider than any instance --
    // and nothing to interpolate either: the pool path's assemble is all it needs, and part_frames does not count it.
    for (int p = 0; p < c.nplanes(); ++p)
        if (d.fused[p] && c.plane_parts[p] && d.plan[p].n == 0) d.fused[p] = false;
    // The reference smooths the whole luma-sized pool in every pass (SangNom2.cpp:126-159).  A plane of fewer lines reads
    // back only rows 1 .. nr of it, and a later pass of this frame reads one row further than it smooths -- when nothing
    // is carried into the next frame, rows beyond that are never looked at again and stage 2 of the pool path stops
    // there (4:2:0: the two chroma passes take half the time).  SN_MODE_POOL keeps the full emulation, pool contents included.
    if (c.history_free && c.cfg.mode != SN_MODE_POOL) {
        int later = 0;
        for (int p = c.nplanes() - 1; p >= 0; --p) {
            if (!c.enabled(p)) continue;
            const int own = c.plane_h_out(p) / 2;  // rows 1 .. nr = own - 1
            d.stop[p] = own > later + 1 ? own : later + 1;
            later = d.stop[p];
        }
    }
    if (c.isolated) d.route = d.nbands ? Route::kBandedPlanes : Route::kPlanes;
    else if (c.fused420 && d.fused[0] && d.fused[1] && d.fused[2]) d.route = d.nbands ? Route::kCoupledBanded : Route::kCoupled;
    else if (d.nbands && !c.fused420) d.route = Route::kBandedPlanes;
    else d.route = Route::kPlanes;
    return d;
}

}  // namespace sn
