// sn_fused_select.hip -- the sweeps' one entry point, the layout their addressing takes, and the hand-off pools' size and
// layout (host code only).  Which configurations the sweeps serve is sn_route.h's.
#include <stdint.h>
#include <string.h>

#include "sn_route.h"

namespace sn {

// a slot per thread and pool row: the eight columns of each strip the thread holds (two for 8-bit samples)
static int slot_bytes(const v3c::SweepTraits& t) { return (t.packed ? 2 : 1) * v3c::PXL * t.bytes; }

int64_t sweep_pool_bytes(int bytes_per_sample, int sweep_w, int rows)
{
    return (int64_t)kBuffers * rows * sweep_waves(bytes_per_sample, sweep_w) * 64 * slot_bytes(v3c::sweep_traits(bytes_per_sample));
}

// A pool row is [strip kinds][threads][8 samples]: the eight columns the lane owns in its strip `wave` and, 8-bit only (kind 1,
// the high halves of the registers), in its strip `wave + nw`, as the kernels' PoolIO::store leaves them.  Ghost lanes and lanes
// past the sweep width own nothing; cells outside the dependency cone are never written: `out` keeps what the caller put there.
void sweep_pool_unpack(int bytes_per_sample, const uint32_t* raw, int sweep_w, int rows, void* out)
{
    using namespace v3c;
    const SweepTraits& t = sweep_traits(bytes_per_sample);
    const int nl = sweep_w / PXL, nvw = strips_for(nl), nw = sweep_waves(bytes_per_sample, sweep_w), nt = nw * 64, cell = PXL * t.bytes;
    const uint8_t* from = reinterpret_cast<const uint8_t*>(raw);
    uint8_t* to = static_cast<uint8_t*>(out);
    for (int64_t br = 0; br < (int64_t)kBuffers * rows; ++br)
        for (int tid = 0; tid < nt; ++tid)
            for (int h = 0; h < (t.packed ? 2 : 1); ++h) {
                const int wave = tid / 64, lane = tid % 64, vw = wave + h * nw;
                const int gl = vw == 0 ? lane : kFirst + kInner * (vw - 1) + (lane - GH);
                const bool ghost = vw == 0 ? (nvw > 1 && lane >= 64 - GH) : (lane < GH || (lane >= 64 - GH && vw < nvw - 1));
                if (vw >= nvw || ghost || gl >= nl) continue;
                memcpy(to + (br * sweep_w + gl * PXL) * t.bytes, from + (br * nt * slot_bytes(t) + ((int64_t)h * nt + tid) * cell), cell);
            }
}

hipError_t launch_sweep(hipStream_t st, int bytes_per_sample, const PlaneArgs& p, double threshold, int nframes, const FusedPool* pool)
{
#ifdef SN_EXPERIMENT_V4  // A/B builds of tools/experiments only
    if (bytes_per_sample == 1 && !pool && fused_v4_plane_ok(p.w)) return launch_fused_u8_v4(st, p, threshold, nframes);
#endif
    v3c::Sweep s;
    const hipError_t e = v3c::build_sweep(v3c::sweep_traits(bytes_per_sample), p, threshold, nframes, pool, s);
    if (e != hipSuccess) return e;
    if (bytes_per_sample == 4) return launch_sweep_f32(st, s, (float)threshold);
    if (bytes_per_sample == 2) return launch_sweep_u16(st, s);
    return launch_sweep_u8(st, s);
}

// Pointer / pitch alignment the 8-byte vector accesses need, and the size the sweeps' addressing holds: they reach a plane
// through a buffer descriptor of pitch * rows bytes and form row offsets as 32-bit integers (a few rows past the last one
// included, which the descriptor's range check drops), so pitch * (rows + kFusedRowSlack) has to fit in 31 bits on both
// sides.  A larger plane -- a column window of a very wide surface -- is served by the pool path, whose kernels address
// rows with 64-bit pointers.
bool fused_layout_ok(const PlaneArgs& p)
{
    auto a8 = [](uintptr_t v) { return (v & 7) == 0; };
    auto fits = [](int32_t pitch, int32_t rows) { return (int64_t)pitch * ((int64_t)rows + kFusedRowSlack) <= (int64_t)INT32_MAX; };
    return a8((uintptr_t)p.src) && a8((uintptr_t)p.dst) && a8((uintptr_t)p.src_pitch) && a8((uintptr_t)p.dst_pitch) &&
           a8((uintptr_t)p.src_frame_stride) && a8((uintptr_t)p.dst_frame_stride) && fits(p.src_pitch, p.h_in) && fits(p.dst_pitch, p.h_out);
}

}  // namespace sn
