// sn_reduce.hip -- the 2W x 2H plane E of the anti-aliasing call with dh, brought back to W x H on the device.
//
// out(x, y) is a symmetric odd filter over E centred on E[2y + oy][2x + ox], the position at which the source sample
// (x, y) reappears in E (oy = the kept-field offset, ox = 1 - oy): no sub-pixel shift.  Coordinates outside E are
// clamped to its edge.  Two tap sets, separable, horizontal sums first (include/sangnom_hip.h has the contract):
//   kernel 1 (tent):      [1 2 1],            shift 2 per direction
//   kernel 2 (half-band): [-1 0 9 16 9 0 -1], shift 5 per direction
// Integer samples: 32-bit sums, out = clamp((v + (1 << (2s - 1))) >> 2s, 0, 2^bits - 1).  Float samples: one rounding per
// written operation in the order of tap_sum() below, no contraction, no clamp.
//
// Tile constants: a workgroup of 256 threads owns kReduceTileBytes / B x kReduceTileH output samples of one frame: 256 x 16
// for 8-bit samples, 128 x 16 for 16-bit ones, 64 x 16 for float -- 256 bytes of an output row and 512 contiguous bytes of
// an E row whatever the sample type (with 64 columns for every type the 8-bit kernel read runs of 160 bytes and stayed
// 20 % behind the turn kernel on the same planes).
// It stages the 2 * 16 + 2r rows of E it needs (r = 1 / 3: the halo) through LDS, each row from one 16-byte unit left of
// E column 2 * x0 to one unit right of the tile's last column, so that an E sample leaves memory once per tile and not
// once per tap; the clamp is applied while staging.  A thread sums one output column of 16 / 8 / 4 rows (the horizontal
// sums of 2 rows - 1 + 2r rows of E in registers), the results go back through LDS and leave as whole rows.  HBM-bound:
// 4 W H B bytes read, W H B written.
// Source base, pitch and frame stride multiples of 16: 16 bytes per lane and access while staging (a unit that crosses
// E's edge goes sample by sample); the same on the destination side for the stores (a unit that crosses the plane's right
// edge goes sample by sample).  Anything else takes sample-wide accesses, as k_turn does without dword_ok.  Nothing outside
// width * B bytes of a destination row is written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "sn_internal.h"

#pragma clang fp contract(off)

namespace sn {

constexpr int kReduceTileBytes = 256, kReduceTileH = 16;  // the tile is kReduceTileBytes / sizeof(sample) columns wide

template <int K>
__device__ __forceinline__ int32_t tap_sum(const int32_t* a)
{
    if (K == 1) return a[0] + 2 * a[1] + a[2];
    return 9 * (a[2] + a[4]) + 16 * a[3] - (a[0] + a[6]);
}

template <int K>
__device__ __forceinline__ float tap_sum(const float* a)
{
    if (K == 1) return (a[0] + a[2]) + (a[1] + a[1]);
    return ((a[2] + a[4]) * 9.0f + a[3] * 16.0f) - (a[0] + a[6]);
}

template <int K>
__device__ __forceinline__ int32_t tap_finish(int32_t v, int maxv)
{
    constexpr int S2 = K == 1 ? 4 : 10;
    const int32_t q = (v + (1 << (S2 - 1))) >> S2;
    return q < 0 ? 0 : q > maxv ? maxv : q;
}

template <int K>
__device__ __forceinline__ float tap_finish(float v, int)
{
    return v * (K == 1 ? 0.0625f : 0.0009765625f);
}

template <class T, int K>
__global__ void __launch_bounds__(256) k_reduce(const uint8_t* src, int64_t sfs, int spitch, int w, int h, int ox, int oy, uint8_t* dst, int64_t dfs,
                                                int dpitch, int maxv, int src16, int dst16)
{
    using A = typename std::conditional<std::is_same<T, float>::value, float, int32_t>::type;
    constexpr int R = K == 1 ? 1 : 3;
    constexpr int V = 16 / (int)sizeof(T);           // samples per 16 bytes
    constexpr int kReduceTileW = kReduceTileBytes / (int)sizeof(T);
    constexpr int kReduceRowsPerThread = kReduceTileH * kReduceTileW / 256;  // 256 threads = the tile's columns x 1 / 2 / 4 groups of rows
    constexpr int LW = 2 * kReduceTileW + 2 * V;     // samples per staged row: LDS column c is E column 2 x0 - V + c
    constexpr int LR = 2 * kReduceTileH + 2 * R;     // staged rows: LDS row j is E row 2 y0 - R + j
    constexpr int NH = 2 * kReduceRowsPerThread - 1 + 2 * R;  // horizontal sums a thread holds
    __shared__ uint4 lds4[LR * LW / V];
    T* lds = reinterpret_cast<T*>(lds4);

    const int x0 = blockIdx.x * kReduceTileW, y0 = blockIdx.y * kReduceTileH;
    const int tw = w - x0 < kReduceTileW ? w - x0 : kReduceTileW, th = h - y0 < kReduceTileH ? h - y0 : kReduceTileH;
    const int W2 = 2 * w, H2 = 2 * h;
    const uint8_t* s = src + (int64_t)blockIdx.z * sfs;
    uint8_t* d = dst + (int64_t)blockIdx.z * dfs;

    // the rows and 16-byte units this tile reads: LDS columns V - R .. V + 2 tw + R, rows 0 .. 2 th + 2 R - 1
    const int nrows = 2 * th + 2 * R, nvec = (V + 2 * tw + R) / V + 1;
    for (int i = threadIdx.x; i < nrows * nvec; i += 256) {
        const int j = i / nvec, q = i % nvec;
        int ey = 2 * y0 - R + j;
        ey = ey < 0 ? 0 : ey > H2 - 1 ? H2 - 1 : ey;
        const int ec = 2 * x0 - V + q * V;
        const T* row = reinterpret_cast<const T*>(s + (int64_t)ey * spitch);
        if (src16 && ec >= 0 && ec + V <= W2) {
            lds4[j * (LW / V) + q] = *reinterpret_cast<const uint4*>(row + ec);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                int c = ec + k;
                c = c < 0 ? 0 : c > W2 - 1 ? W2 - 1 : c;
                lds[j * LW + q * V + k] = row[c];
            }
        }
    }
    __syncthreads();

    // (threads beyond the tile's ragged edges sum rows and columns that were not staged: in bounds of the array, never stored)
    const int tx = threadIdx.x % kReduceTileW, ty = threadIdx.x / kReduceTileW;
    const T* p = lds + (2 * kReduceRowsPerThread * ty + oy) * LW + V + 2 * tx + ox - R;
    A hs[NH];
#pragma unroll
    for (int n = 0; n < NH; ++n) {
        A a[2 * R + 1];
#pragma unroll
        for (int i = 0; i < 2 * R + 1; ++i) a[i] = (A)p[n * LW + i];
        hs[n] = tap_sum<K>(a);
    }
    T out[kReduceRowsPerThread];
#pragma unroll
    for (int k = 0; k < kReduceRowsPerThread; ++k) out[k] = (T)tap_finish<K>(tap_sum<K>(hs + 2 * k), maxv);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kReduceRowsPerThread; ++k) lds[(kReduceRowsPerThread * ty + k) * kReduceTileW + tx] = out[k];
    __syncthreads();

    constexpr int VO = kReduceTileW / V;  // 16-byte units of an output row of the tile
    for (int i = threadIdx.x; i < th * VO; i += 256) {
        const int r = i / VO, q = i % VO;
        const int xs = x0 + q * V;
        if (xs >= w) continue;
        T* drow = reinterpret_cast<T*>(d + (int64_t)(y0 + r) * dpitch);
        if (dst16 && xs + V <= w) {
            *reinterpret_cast<uint4*>(drow + xs) = lds4[r * VO + q];
        } else {
            for (int k = 0; k < V && xs + k < w; ++k) drow[xs + k] = lds[r * kReduceTileW + q * V + k];
        }
    }
}

template <class T>
static void reduce_launch(hipStream_t st, int kernel, int nframes, const uint8_t* src, int64_t sfs, int spitch, int w, int h, int ox, int oy, uint8_t* dst,
                          int64_t dfs, int dpitch, int maxv, int src16, int dst16)
{
    constexpr int kReduceTileW = kReduceTileBytes / (int)sizeof(T);
    const dim3 grid((w + kReduceTileW - 1) / kReduceTileW, (h + kReduceTileH - 1) / kReduceTileH, nframes);
    if (kernel == 1)
        hipLaunchKernelGGL((k_reduce<T, 1>), grid, dim3(256), 0, st, src, sfs, spitch, w, h, ox, oy, dst, dfs, dpitch, maxv, src16, dst16);
    else
        hipLaunchKernelGGL((k_reduce<T, 2>), grid, dim3(256), 0, st, src, sfs, spitch, w, h, ox, oy, dst, dfs, dpitch, maxv, src16, dst16);
}

hipError_t launch_reduce(hipStream_t st, int bytes, int bits, int kernel, int nframes, PlaneView s, int w, int h, int ox, int oy, PlaneViewW d)
{
    const uint8_t* const src = s.base;
    uint8_t* const dst = d.base;
    const int64_t sfs = s.fs, dfs = d.fs;
    const int spitch = s.pitch, dpitch = d.pitch;
    if (nframes <= 0 || w <= 0 || h <= 0) return hipSuccess;
    if (kernel != 1 && kernel != 2) return hipErrorInvalidValue;
    const int src16 = (uintptr_t)src % 16 == 0 && spitch % 16 == 0 && sfs % 16 == 0;
    const int dst16 = (uintptr_t)dst % 16 == 0 && dpitch % 16 == 0 && dfs % 16 == 0;
    const int maxv = bytes == 4 ? 0 : (1 << bits) - 1;
    switch (bytes) {
    case 1: reduce_launch<uint8_t>(st, kernel, nframes, src, sfs, spitch, w, h, ox, oy, dst, dfs, dpitch, maxv, src16, dst16); break;
    case 2: reduce_launch<uint16_t>(st, kernel, nframes, src, sfs, spitch, w, h, ox, oy, dst, dfs, dpitch, maxv, src16, dst16); break;
    default: reduce_launch<float>(st, kernel, nframes, src, sfs, spitch, w, h, ox, oy, dst, dfs, dpitch, maxv, src16, dst16); break;
    }
    return hipGetLastError();
}

}  // namespace sn
