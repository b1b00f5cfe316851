// sn_turn.hip -- TurnRight / TurnLeft of a plane on the device.
//
// Anti-aliasing scripts run SangNom2 twice around a quarter turn (TurnLeft().SangNom2().TurnRight().SangNom2(),
// README.md:3 of the reference: "mainly used in anti-aliasing scripts").  With the turn on the device the
// frame stays in HBM between the two passes instead of crossing PCIe four times.
//   right (clockwise):      dst[y'][x'] = src[H-1-x'][y'],  dst is H wide and W high
//   left (anti-clockwise):  dst[y'][x'] = src[x'][W-1-y']
// 64 x 64 sample tiles go through LDS so that both the reads and the writes are row-contiguous; HBM-bound:
// 2 x W x H x B bytes per plane.
// Field form (line_parity 0 / 1): only the destination lines of that parity are written -- the lines the SangNom2 pass
// that follows keeps, the only ones it reads.  A destination line is a source column, so a tile still reads whole source
// rows but writes 32 of its 64 lines: 1.5 x W x H x B bytes.  The other lines of the destination are left as they were.
// With a second source (kMerge; the both-fields call, sangnom_hip.h "Both fields") the tile is filled with avg(src, src2)
// instead of src, on both paths; everything behind the fill is the same code.  3 x W x H x B bytes, where the average as a
// kernel of its own and a turn behind it would move five.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sn_avg.h"
#include "sn_internal.h"

namespace sn {

constexpr int kTile = 64;

template <class T, bool kMerge>
__global__ void __launch_bounds__(256) k_turn(const uint8_t* src, int64_t sfs, int spitch, const uint8_t* src2, int64_t sfs2, int spitch2, int w, int h,
                                             uint8_t* dst, int64_t dfs, int dpitch, int right, int dword_ok, int line_parity)
{
    constexpr int P = 4 / (int)sizeof(T);  // samples per dword
    constexpr int RD = kTile / P;          // dwords per tile row
    __shared__ uint32_t tile32[kTile][RD + 1];
    T(*tile)[(RD + 1) * P] = reinterpret_cast<T(*)[(RD + 1) * P]>(tile32);
    const int f = blockIdx.z;
    const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;  // tile origin in the source
    const uint8_t* s = src + (int64_t)f * sfs;
    const uint8_t* s2 = kMerge ? src2 + (int64_t)f * sfs2 : nullptr;
    uint8_t* d = dst + (int64_t)f * dfs;

    // Whole tiles with dword-aligned rows move as dwords on both sides (a byte-wide global access wastes most of
    // the 64 bytes a wave instruction moves); ragged edges and odd alignments take the sample-wide path.
    if (dword_ok && x0 + kTile <= w && y0 + kTile <= h) {
        for (int i = threadIdx.x; i < kTile * RD; i += 256) {
            const int r = i / RD, q = i % RD;
            uint32_t v = reinterpret_cast<const uint32_t*>(s + (int64_t)(y0 + r) * spitch)[x0 / P + q];
            if constexpr (kMerge) v = avg_dword<(int)sizeof(T)>(v, reinterpret_cast<const uint32_t*>(s2 + (int64_t)(y0 + r) * spitch2)[x0 / P + q]);
            tile32[r][q] = v;
        }
        __syncthreads();
        // destination line of tile column r: x0 + r (right) or w - 1 - x0 - r (left); the field form takes every other column
        const int rstep = line_parity < 0 ? 1 : 2;
        const int r0 = line_parity < 0 ? 0 : ((right ? x0 : w - 1 - x0) ^ line_parity) & 1;
        for (int i = threadIdx.x; i < kTile / rstep * RD; i += 256) {
            const int r = r0 + rstep * (i / RD), q = i % RD;  // r: source column inside the tile = destination row; q: dword of that row
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j < P; ++j) {
                const int dxj = P * q + j;  // position along the destination row, inside the tile
                const int sy = right ? kTile - 1 - dxj : dxj;
                v |= (uint32_t)tile[sy][r] << (8 * (int)sizeof(T) * j);
            }
            const int dy = right ? x0 + r : w - 1 - (x0 + r);
            const int dx0 = right ? h - y0 - kTile : y0;  // first destination column of the tile
            reinterpret_cast<uint32_t*>(d + (int64_t)dy * dpitch)[dx0 / P + q] = v;
        }
        return;
    }

    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 64 x 4 threads
    for (int r = ty; r < kTile; r += 4) {
        const int x = x0 + tx, y = y0 + r;
        if (x < w && y < h) {
            T v = reinterpret_cast<const T*>(s + (int64_t)y * spitch)[x];
            if constexpr (kMerge) v = (T)avg_sample<(int)sizeof(T)>(v, reinterpret_cast<const T*>(s2 + (int64_t)y * spitch2)[x]);
            tile[r][tx] = v;
        }
    }
    __syncthreads();
    // destination rows correspond to source columns; a destination row segment is a source column segment
    for (int r = ty; r < kTile; r += 4) {
        const int sx = x0 + r;
        if (sx >= w) continue;
        // right: dst[sx][h-1-y] = src[y][sx] (x' runs backwards in y);  left: dst[w-1-sx][y] = src[y][sx]
        const int sy = right ? y0 + (kTile - 1 - tx) : y0 + tx;
        if (sy >= h) continue;
        const int dx = right ? h - 1 - sy : sy;
        const int dy = right ? sx : w - 1 - sx;
        if (line_parity >= 0 && ((dy ^ line_parity) & 1)) continue;
        reinterpret_cast<T*>(d + (int64_t)dy * dpitch)[dx] = tile[sy - y0][r];
    }
}

// s2.base == nullptr: the turn of s; otherwise of avg(s, s2)
static hipError_t turn(hipStream_t st, int bytes, int right, int nframes, PlaneView s, PlaneView s2, int w, int h, PlaneViewW d, int line_parity)
{
    const uint8_t* const src = s.base;
    const uint8_t* const src2 = s2.base;
    uint8_t* const dst = d.base;
    const int64_t sfs = s.fs, sfs2 = s2.fs, dfs = d.fs;
    const int spitch = s.pitch, spitch2 = s2.pitch, dpitch = d.pitch;
    if (nframes <= 0 || w <= 0 || h <= 0) return hipSuccess;
    dim3 grid((w + kTile - 1) / kTile, (h + kTile - 1) / kTile, nframes), block(256);
    const int per = 4 / bytes;  // samples per dword: the turned tile must start on a dword of the destination row
    const int dword_ok = ((uintptr_t)src % 4 == 0 && (uintptr_t)dst % 4 == 0 && spitch % 4 == 0 && dpitch % 4 == 0 && sfs % 4 == 0 && dfs % 4 == 0 &&
                          (!src2 || ((uintptr_t)src2 % 4 == 0 && spitch2 % 4 == 0 && sfs2 % 4 == 0)) && (!right || h % per == 0))
                             ? 1
                             : 0;
#define SN_TURN(T)                                                                                                                                  \
    do {                                                                                                                                            \
        if (src2)                                                                                                                                   \
            hipLaunchKernelGGL((k_turn<T, true>), grid, block, 0, st, src, sfs, spitch, src2, sfs2, spitch2, w, h, dst, dfs, dpitch, right, dword_ok, \
                               line_parity);                                                                                                        \
        else                                                                                                                                        \
            hipLaunchKernelGGL((k_turn<T, false>), grid, block, 0, st, src, sfs, spitch, src2, sfs2, spitch2, w, h, dst, dfs, dpitch, right, dword_ok, \
                               line_parity);                                                                                                        \
    } while (0)
    switch (bytes) {
    case 1: SN_TURN(uint8_t); break;
    case 2: SN_TURN(uint16_t); break;
    default: SN_TURN(uint32_t); break;
    }
#undef SN_TURN
    return hipGetLastError();
}

hipError_t launch_turn(hipStream_t st, int bytes, int right, int nframes, PlaneView s, int w, int h, PlaneViewW d, int line_parity)
{
    return turn(st, bytes, right, nframes, s, PlaneView{}, w, h, d, line_parity);
}

hipError_t launch_turn_merge(hipStream_t st, int bytes, int right, int nframes, PlaneView a, PlaneView b, int w, int h, PlaneViewW d)
{
    if (!b.base) return hipErrorInvalidValue;
    return turn(st, bytes, right, nframes, a, b, w, h, d, -1);
}

}  // namespace sn
