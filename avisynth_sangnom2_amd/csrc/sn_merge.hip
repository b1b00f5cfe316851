// sn_merge.hip -- the average of the both-fields anti-aliasing call (sangnom_hip.h, "Both fields"): dst = avg(a, b), sample by
// sample.  Elementwise and HBM-bound: 3 x W x H x B bytes per plane (2 reads, 1 write), a handful of VALU instructions per 16
// bytes.  A row is cut into pieces of 16 bytes and every lane takes one piece of one row: consecutive lanes take consecutive
// pieces, so a wave instruction moves 1 KB of a row (or of several short rows).  Where every row of all three planes starts on a
// multiple of 16 bytes (`vec`: bases, pitches and frame strides), a whole piece moves as one 16-byte access each way; the
// piece a row ends in, and every piece of planes that are not aligned so, goes sample by sample.  Nothing beyond the row's
// samples is read or written.  dst may be a or b exactly: each piece is read by the lane that overwrites it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sn_avg.h"
#include "sn_internal.h"

namespace sn {

template <class T>
__global__ void __launch_bounds__(256) k_merge(const uint8_t* a, int64_t afs, int apitch, const uint8_t* b, int64_t bfs, int bpitch, uint8_t* dst,
                                               int64_t dfs, int dpitch, int w, int h, int pieces, int vec)
{
    constexpr int B = (int)sizeof(T);
    constexpr int V = 16 / B;  // samples of a piece
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)pieces * h) return;
    const int y = (int)(i / pieces), q = (int)(i - (int64_t)y * pieces);
    const int x0 = q * V;  // < w: pieces = ceil(w / V)
    const int f = blockIdx.z;
    const uint8_t* ar = a + (int64_t)f * afs + (int64_t)y * apitch + (int64_t)x0 * B;
    const uint8_t* br = b + (int64_t)f * bfs + (int64_t)y * bpitch + (int64_t)x0 * B;
    uint8_t* dr = dst + (int64_t)f * dfs + (int64_t)y * dpitch + (int64_t)x0 * B;
    if (vec && x0 + V <= w) {
        const uint4 va = *reinterpret_cast<const uint4*>(ar), vb = *reinterpret_cast<const uint4*>(br);
        uint4 o;
        o.x = avg_dword<B>(va.x, vb.x);
        o.y = avg_dword<B>(va.y, vb.y);
        o.z = avg_dword<B>(va.z, vb.z);
        o.w = avg_dword<B>(va.w, vb.w);
        *reinterpret_cast<uint4*>(dr) = o;
        return;
    }
    const int n = w - x0 < V ? w - x0 : V;
    const T* as = reinterpret_cast<const T*>(ar);
    const T* bs = reinterpret_cast<const T*>(br);
    T* ds = reinterpret_cast<T*>(dr);
    for (int k = 0; k < n; ++k) ds[k] = (T)avg_sample<B>(as[k], bs[k]);
}

hipError_t launch_merge(hipStream_t st, int bytes, int nframes, PlaneView a, PlaneView b, int w, int h, PlaneViewW d)
{
    if (nframes <= 0 || w <= 0 || h <= 0) return hipSuccess;
    auto rows16 = [](const uint8_t* base, int pitch, int64_t fs) { return (uintptr_t)base % 16 == 0 && pitch % 16 == 0 && fs % 16 == 0; };
    const int vec = rows16(a.base, a.pitch, a.fs) && rows16(b.base, b.pitch, b.fs) && rows16(d.base, d.pitch, d.fs) ? 1 : 0;
    const int V = 16 / bytes;
    const int pieces = (w + V - 1) / V;
    const int64_t blocks = ((int64_t)pieces * h + 255) / 256;
    if (blocks > INT32_MAX || nframes > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks, 1, (unsigned)nframes), block(256);
    switch (bytes) {
    case 1: hipLaunchKernelGGL(k_merge<uint8_t>, grid, block, 0, st, a.base, a.fs, a.pitch, b.base, b.fs, b.pitch, d.base, d.fs, d.pitch, w, h, pieces, vec); break;
    case 2: hipLaunchKernelGGL(k_merge<uint16_t>, grid, block, 0, st, a.base, a.fs, a.pitch, b.base, b.fs, b.pitch, d.base, d.fs, d.pitch, w, h, pieces, vec); break;
    default: hipLaunchKernelGGL(k_merge<uint32_t>, grid, block, 0, st, a.base, a.fs, a.pitch, b.base, b.fs, b.pitch, d.base, d.fs, d.pitch, w, h, pieces, vec); break;
    }
    return hipGetLastError();
}

}  // namespace sn
