// sn_sweep_args.h -- the host side of the fused sweeps (8-bit, 16-bit and float alike): the kernels' argument block, the
// modes, the geometry of a sweep, and the ONE function that turns a plane and its pool coupling into a launch.  No device
// code: a host compiler takes this header as it is (tests/c/sweep_args_check.cpp); sn_fused_v3_common.h adds the device side.
#pragma once

#include <stdint.h>

#include "sn_internal.h"

namespace sn {
namespace v3c {

constexpr int PXL = 8;           // pixels per lane and per strip
constexpr int GH = 2;            // ghost lanes on each inner side of a strip
constexpr int K = GH * PXL / 3;  // rows between two seam refreshes (5)
constexpr int kFirst = 64 - GH;      // real lanes of strip 0
constexpr int kInner = 64 - 2 * GH;  // real lanes of every later strip

constexpr int kMaxColumnParts = sn::kMaxColumnParts;

struct Args {
    const uint8_t* src;
    uint8_t* dst;
    int64_t src_frame_stride;
    int64_t dst_frame_stride;
    int32_t src_pitch;
    int32_t dst_pitch;
    int32_t w;
    int32_t nk;      // kept lines
    int32_t offset;  // first kept line in dst
    int32_t dh;
    int32_t thr;
    int32_t nl;      // real lanes = w / 8
    int32_t nvw;     // virtual wavefronts
    int32_t nw;      // physical waves
    int32_t src_bytes;  // bytes of one source plane (buffer descriptor range)
    int32_t dst_bytes;  // bytes of one destination plane
    // Dependency cone of the pool coupling.  A hand-off cell (pool row q, column x) can reach a chroma output only if
    // x < cone_w + 3 * (cone_nr - q + 2) (+6 for the luma -> U hand-off, whose cells act through U's sweep): stage 2
    // spreads 3 columns per row and the chroma region ends at column cone_w, row cone_nr.  Inside the region
    // (x < cone_w) a cell matters only below it (q > cone_nr).  Lanes whose columns lie outside neither store nor
    // load their slot (out-of-range voffset: no branch, no HBM traffic).
    int32_t cone_w, cone_nr;   // chroma width, chroma nr = interpolated lines
    int32_t cone_in, cone_out; // extra columns of the loads (U: 6, V: 0) / of the stores (luma: 6, U: 0)
    // pool coupling for subsampled chroma (modes kLumaSpill / kChroma, see below)
    const uint8_t* pool_in;   // smoothed buffers left by the previous pass (kChroma)
    uint8_t* pool_out;        // where this pass leaves its smoothed buffers (kLumaSpill, first kChroma pass)
    int64_t pool_frame_stride;
    int32_t pool_rows;        // rows a pool buffer holds (row index 1 .. pool_rows - 1 used)
    int32_t pool_row_bytes;   // 0: pool_out has the sweeps' own layout (a slot per thread); > 0 (kLumaSpill): it is a pool
                              // of the pool path, [buffer][row][column] samples with this row pitch (sn_pool_kernels.hip)
    int32_t rows_in;          // rows 1 .. rows_in of pool_in are valid, later rows read as zero
    int32_t rows_out;         // rows 1 .. rows_out are written to pool_out (0 = none)
    int32_t region_w;         // the plane's own width; has_region modes: columns < region_w belong to the plane
    int32_t sweep_rows;       // kChroma: pool rows to sweep (>= nk - 1)
    int32_t turn_shift;       // log2 of the priority time slice in 100 MHz ticks (TurnTaking)
    int32_t nframes;          // frames of this launch (the last workgroup may hold fewer than group_of(nw))
    // row bands (kernel template parameter BAND): blockIdx.y = band; see below
    int32_t band_rows;        // pool rows per band
    int32_t band_warm;        // rows a band sweeps before its first own row, starting from a zero guess of the state
    int32_t nbands;
    uint32_t* band_state;     // [frame][band][warm, end][kBuffers * PXL][threads of the plane] state words, ghosts zeroed
    int32_t* band_flags;      // [frame]: set by the verification that follows (sn_band.hip)
    int32_t band_reset;       // this sweep clears band_flags first (the first plane of a frame)
    int32_t arith;            // SN_ARITH_*: which instances the launcher picks (every integer sweep has both)
    // column parts (mode kParts): blockIdx.y = part; every part sweeps a window of the same width w that starts at column
    // part_x of the plane (the kernel advances src / dst and shortens src_bytes / dst_bytes by that much)
    int32_t nparts;
    int32_t part_x[kMaxColumnParts];
    int32_t part_store_lo[kMaxColumnParts], part_store_hi[kMaxColumnParts];  // window columns [lo, hi) are the part's own: only those are stored to dst
    int32_t part_seam_x[kMaxColumnParts][2];    // window column of the seam on the left / right inner side (multiple of 8), < 0: an image edge
    int32_t part_seam_off[kMaxColumnParts][2];  // byte offset of this window's side of that seam's record in the frame's record
    uint8_t* seam_rec;           // [frame][seam][side][row 1 .. nr][kBuffers][16 samples]: smoothed values of columns seam - 8 .. seam + 7
    int64_t seam_frame_stride;
    int32_t seam_bytes;          // bytes of one frame's record
};

// The reference's nine buffers are sized for the luma plane and shared by all planes, so a
// subsampled chroma pass smooths a pool that still holds the previous pass's results outside the
// chroma region.  Exact emulation in the fused kernel:
//   kLumaSpill  the luma sweep also leaves its smoothed values O of the rows the chroma passes can
//               reach in a scratch pool;
//   kChroma     the sweep runs over the whole luma-wide pool: inside the chroma region the cost of
//               the next row comes from the chroma lines (stage 1), elsewhere it is the previous
//               pass's O read back from the pool; stage 3 and the output exist only inside the region.
// Pool layout: [buffer][row][thread][4 dwords], dword k = O[2k] | O[2k+1] << 8 (packed pairs), i.e. every
// thread re-reads what the thread with the same columns wrote; ghost lanes read their owner's slot.
//   kPadded     a plane narrower than its pool stride on a zero-filled pool (sn_config.fresh_pool): the sweep covers
//               the whole stride, costs are zero in the padding columns, nothing is read back or left behind.
//   kChromaLast the last chroma sweep of a frame: kChroma that hands nothing on (8-bit sweep only: no packing of stores
//               that would all be dropped)
// Row bands (BAND, every mode): the plane is cut into bands of rows, one workgroup per band, so that ONE frame fills the
// device (the latency path: a synchronous GetFrame, a short look-ahead).  Stage 2 is a recurrence from the top of the
// plane, so a band cannot know its starting state; but the recurrence forgets (each row keeps 7/16 of the previous
// one), so the band starts `band_warm` rows early from a zero state and has, on ordinary content, the exact state when
// it reaches its own rows.  "Ordinary" is not "always" (a rounding difference of one can live on for ever on flat or
// periodic content), so every band leaves the state it reached its first row with and the state it ends with;
// sn_band.hip compares each band's end with the next band's start -- equal everywhere means, by induction from band 0,
// that every band computed what the top-to-bottom sweep computes -- and a frame that fails is redone by the pool path
// (guarded launches that otherwise exit at once).
// Column parts (kParts; 16-bit and float sweeps): the same trust-nothing pattern turned by ninety degrees, for planes wider
// than one workgroup holds.  The plane is cut into windows that overlap by a ghost margin on each inner side; a window is
// swept by a workgroup of its own (all parts of all frames in one grid) like a plane of its own (kPlain on advanced pointers: it clamps at the window's edges, which is wrong at an inner
// edge, but the error dies out within the margin on ordinary content) and stores only its own columns.  For every smoothed
// row both windows around a seam leave their values of the 16 columns around it; sn_band.hip compares them bit for bit.
// Equal means exact: by induction over the rows, a window's own columns of row y depend on row y - 1 only up to three
// columns beyond the seam, where agreement says the window holds what the other one -- exact there -- holds.
// Planes on their own are cut (kPlain), and the luma sweep that leaves its rows in a pool of the POOL PATH
// (kLumaSpill with pool_row_bytes): a single 4:2:0 frame takes its luma plane through the bands and its chroma planes
// through the pool kernels, which find in the pool what the reference's luma pass would have left there.  The pool-coupled sweeps were tried and work mechanically -- a band
// starts from the hand-off row of its first row and hands on its own rows only -- but the last chroma sweep never passes
// the check: outside the chroma region it re-smooths what two passes have smoothed already, data so even that the
// rounding difference between the run-up and the true history does not die out (256 x 400 noise needs a run-up of 128
// rows, 3840 x 2160 is still wrong after 128), so every such frame would be done twice.
enum Mode { kPlain = 0, kLumaSpill = 1, kChroma = 2, kPadded = 3, kChromaLast = 4, kParts = 5 };
constexpr int kModes = 6;
__host__ __device__ constexpr bool plain_mode(int mode) { return mode == kPlain || mode == kParts; }  // a plane (or window) on its own
__host__ __device__ constexpr bool chroma_mode(int mode) { return mode == kChroma || mode == kChromaLast; }
__host__ __device__ constexpr bool has_region(int mode) { return chroma_mode(mode) || mode == kPadded; }  // lines narrower than the sweep
__host__ __device__ constexpr bool has_pools(int mode) { return mode == kLumaSpill || chroma_mode(mode); }

// Frames per workgroup.  A plane that needs only one or two waves shares its workgroup with other frames' planes so
// that every workgroup has four waves, one per SIMD (TurnTaking relies on that shape).  The frames of a
// workgroup are independent: each has its own slice of the dynamic LDS and they only meet at the barriers.
__host__ __device__ constexpr int group_of(int nw) { return nw == 1 ? 4 : nw == 2 ? 2 : 1; }

// Args::turn_shift of workgroups of eight waves in the 8-bit sweep: no time slices, a priority that falls with the rows
// done since the last seam barrier (TurnTaking::kLadder, sn_fused_v3_common.h)
constexpr int kTurnLadder = -1;

// slice = about a quarter of the time a sweep of nk kept lines takes (a row costs roughly 4.5 us) for workgroups of four
// waves: those put one wave on each SIMD, two workgroups fill a CU, and the partners on all four SIMDs are the same two
// workgroups in opposite slots.  (2-wave workgroups lost 8 % with turns: the waves of a workgroup -- tied to each other by
// the seam refresh -- would hold different priorities at the same time.)
// Workgroups of EIGHT waves (4320p 8-bit planes, 16-bit and float planes from 2160p on) hold both waves of every SIMD
// themselves, waves k and k + 4.  Round 3 left them without turns ("they cannot drift apart"); they do, inside every block
// of five rows: tools/row_timing.py (s_memtime around the phases of a row) finds a 4320p wave waiting at the seam barrier
// for 22 % of its cycles (2160p, two workgroups per CU: 4 %) -- equal priorities are served oldest first, so wave k issues
// whenever it can, reaches the barrier early and waits, and wave k + 4 then finishes the block alone at a single wave's
// issue rate.  Removing the barrier gains nothing (the kernel is as slow as its slowest wave); keeping the pair in step
// does.  Measured at 4320p Y8 (profiles/r4_ab_experiments.md 3., 7., 8.): time slices of 10 us +3.3 % (5 us +2 %, 20 us +1 %,
// 40 us and more -1 %); row numbers exchanged through LDS, the wave behind takes the priority: +2.9 %; the same by buffer
// steps: -19 % (nine LDS round trips per row); and what ships -- kTurnLadder, a priority that falls with the rows done
// since the last barrier, which needs no exchange at all because the barrier is the pair's common clock: **+8.3 %** (8-bit
// only: 2160p Y16 +0.8 % over the slices, YUV420P16 -1 %, Y32 and YUV444PS -7 %: those keep the slices of 10 us).
inline int turn_shift_for(int nk, int waves, int bytes_per_sample)
{
    // (the ladder is for the 8-bit sweep, whose rows are all but pure vector arithmetic; the float sweep, which moves three
    // buffers' state through LDS in every row, loses 7 % with it and the 16-bit sweep gains nothing over the slices)
    if (waves == 8) return bytes_per_sample == 1 ? kTurnLadder : 10;
    if (waves != 4) return 0;
    int s = 10;
    while ((128ll * nk) >> (s + 1)) ++s;
    return s;
}

inline int strips_for(int nl) { return nl <= 64 ? 1 : 1 + (nl - kFirst + kInner - 1) / kInner; }

// What the three sample types differ in, as far as a launch's arguments go.
struct SweepTraits {
    int bytes;       // bytes per sample
    bool packed;     // 8-bit: two virtual wavefronts (strips) share every register, so a wave holds two strips
    int max_waves;   // physical waves of a workgroup
    bool parts;      // the type has kParts instances
};
constexpr SweepTraits kSweepU8{1, true, 8, false}, kSweepU16{2, false, 8, true}, kSweepF32{4, false, 8, true};
inline const SweepTraits& sweep_traits(int bytes_per_sample) { return bytes_per_sample == 4 ? kSweepF32 : bytes_per_sample == 2 ? kSweepU16 : kSweepU8; }

// One launch: the kernel's arguments and which instance takes them.
struct Sweep {
    Args args;
    Mode mode;
    bool band;  // the BAND instance: the sweep is cut into args.nbands bands of rows
};

// pool == nullptr: a plane on its own (kPlain).  Otherwise pool->mode names the sweep (a chroma sweep without pool_out
// is kChromaLast) and, unless that is kPlain, pool->sweep_w is the width the sweep covers -- p always describes the plane
// being interpolated.  Every refusal of a launch the kernels have no instance or no room for is here, and nowhere else.
// Fields a mode's kernel does not read stay zero, except region_w (always the plane's width).
inline hipError_t build_sweep(const SweepTraits& t, const PlaneArgs& p, double threshold, int nframes, const FusedPool* pool, Sweep& s)
{
    s = Sweep{};
    Args& a = s.args;
    const int m = pool ? pool->mode : (int)kPlain;
    if (m < 0 || m >= kModes) return hipErrorInvalidValue;
    s.mode = chroma_mode(m) ? (pool->pool_out ? kChroma : kChromaLast) : (Mode)m;
    // no instance: an error, never wrapping pixels in SN_ARITH_SSE2 (the float sweep has one instance for both)
    if (p.arith != SN_ARITH_CXX && p.arith != SN_ARITH_SSE2) return hipErrorInvalidValue;
    if (s.mode == kParts && (!t.parts || pool->nparts < 2 || pool->nparts > kMaxColumnParts || pool->win_w % 32 != 0 || !pool->seam_rec)) return hipErrorInvalidValue;
    a.src = p.src;
    a.dst = p.dst;
    a.src_frame_stride = p.src_frame_stride;
    a.dst_frame_stride = p.dst_frame_stride;
    a.src_pitch = p.src_pitch;
    a.dst_pitch = p.dst_pitch;
    a.w = s.mode == kPlain ? p.w : s.mode == kParts ? pool->win_w : pool->sweep_w;  // sweep_w: the pool stride a narrower plane is swept over
    a.region_w = p.w;
    a.nk = p.h_out / 2;
    a.offset = p.offset;
    a.dh = p.dh;
    a.thr = (int)threshold;
    a.nl = a.w / PXL;
    a.nvw = strips_for(a.nl);
    a.nw = t.packed ? (a.nvw + 1) / 2 : a.nvw;
    if (a.nw > t.max_waves) return hipErrorInvalidValue;
    a.turn_shift = turn_shift_for(a.nk, a.nw * group_of(a.nw), t.bytes);
    a.nframes = nframes;
    a.src_bytes = (int)((int64_t)p.src_pitch * p.h_in);
    a.dst_bytes = (int)((int64_t)p.dst_pitch * p.h_out);
    a.arith = p.arith;
    if (pool && pool->nbands > 1) {
        // planes on their own are cut, and of the pool-coupled sweeps only the luma one (see above); column parts never
        if (s.mode != kPlain && s.mode != kLumaSpill) return hipErrorInvalidValue;
        s.band = true;
        a.band_rows = pool->band_rows;
        a.band_warm = pool->band_warm;
        a.nbands = pool->nbands;
        a.band_state = pool->band_state;
        a.band_flags = pool->band_flags;
        a.band_reset = pool->band_reset;
    }
    if (has_pools(s.mode)) {
        a.pool_in = pool->pool_in;
        a.pool_out = pool->pool_out;
        a.pool_frame_stride = pool->frame_stride;
        a.pool_rows = pool->pool_rows;
        a.pool_row_bytes = s.mode == kLumaSpill ? pool->pool_row_bytes : 0;
        a.rows_in = pool->rows_in;
        a.rows_out = pool->pool_out ? pool->rows_out : 0;
        a.sweep_rows = pool->sweep_rows;
        a.cone_w = pool->cone_w;
        a.cone_nr = pool->cone_nr;
        a.cone_in = pool->cone_in;
        a.cone_out = pool->cone_out;
    }
    if (s.mode == kParts) {  // a plane in column parts, all windows in one grid
        a.nparts = pool->nparts;
        for (int k = 0; k < pool->nparts; ++k) {
            // the window lies inside the plane, its own columns inside the window
            if (pool->win_x[k] % PXL != 0 || pool->win_x[k] < 0 || pool->win_x[k] + pool->win_w > p.w || pool->store_lo[k] % PXL != 0 ||
                pool->store_hi[k] % PXL != 0 || pool->store_lo[k] < 0 || pool->store_hi[k] > pool->win_w)
                return hipErrorInvalidValue;
            a.part_x[k] = pool->win_x[k];
            a.part_store_lo[k] = pool->store_lo[k];
            a.part_store_hi[k] = pool->store_hi[k];
            for (int e = 0; e < 2; ++e) {
                const int sx = pool->seam_x[k][e], off = pool->seam_off[k][e];
                // both lanes next to a seam lie inside the window, and their rows inside the frame's record
                if (sx >= 0 && (sx % PXL != 0 || sx < PXL || sx + PXL > a.w || off < 0 || off + parts_side_bytes(t.bytes, a.nk - 1) > pool->seam_bytes))
                    return hipErrorInvalidValue;
                a.part_seam_x[k][e] = sx;
                a.part_seam_off[k][e] = off;
            }
        }
        a.seam_rec = pool->seam_rec;
        a.seam_frame_stride = pool->seam_frame_stride;
        a.seam_bytes = pool->seam_bytes;
    }
    return hipSuccess;
}

}  // namespace v3c

// The per-type halves of launch_sweep (sn_fused_select.hip): from mode, band and arithmetic to the kernel instance.
hipError_t launch_sweep_u8(hipStream_t st, const v3c::Sweep& s);   // sn_fused_u8_v3.hip (both of its objects, see there)
hipError_t launch_sweep_u16(hipStream_t st, const v3c::Sweep& s);  // sn_fused_u16_v3.hip
hipError_t launch_sweep_f32(hipStream_t st, const v3c::Sweep& s, float aaf);  // sn_fused_f32_v3.hip; aaf: the threshold as the float kernels take it

}  // namespace sn
