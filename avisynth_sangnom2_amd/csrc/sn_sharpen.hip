// sn_sharpen.hip -- the contra-sharpening of the anti-aliasing call: the call's result R is sharpened by an unsharp mask of
// [1 2 1] x [1 2 1], but only as far as the filter changed the picture and only towards the source S
// (include/sangnom_hip.h, "Contra-sharpening", has the contract).
//
//   h  = R(y,x-1) + 2 R(y,x) + R(y,x+1);  B = (h(y-1) + 2 h(y) + h(y+1) + 8) >> 4 (float: * 0.0625f);  d = R - B
//   d1 = sgn(d) ((|d| amount) >> 6)       (float: d * (amount / 64))
//   mn = min(0, min of S - R over 3 x 3),  mx = max(0, max of S - R over 3 x 3),  coordinates clamped to the plane's edge
//   out = clamp(R + min(max(d1, mn), mx), 0, 2^bits - 1)       float: R where d1 is NaN or the correction is 0, else R + it
//
// Tile constants: a workgroup of 256 threads owns kSharpenTileBytes / B x kSharpenTileH output samples of one frame -- 256
// bytes of a row x 16 rows whatever the sample type, as k_mask_merge and k_reduce do.  Two steps, LDS between them:
//   1. S and R rows y0 - 1 .. y0 + 16, each from one 16-byte unit left of the tile to one unit right of it, go to LDS with
//      the edge clamp applied: a sample leaves memory once per tile, not once per tap, and step 2 needs no clamp of its own.
//   2. A thread owns 16 bytes of one output row, in blocks of at most eight samples.  For each of its three rows it reads a
//      block and the two samples beside it of S and of R from LDS (one 8- or 16-byte read and two sample reads per plane) and
//      takes the horizontal half of the
//      separable stencil -- h, and the minimum and maximum of S - R over three columns --; the vertical half joins the three
//      rows in registers: the [1 2 1] sum of h in the written order, the running minimum and maximum.  Then the limit, the
//      clamp, one store.  (Horizontal first is the contract's order for float samples; integers do not care.)
// HBM-bound by design: 2 W H B read, W H B written.  A side (src, aa, dst) whose base, pitch and frame stride are multiples of
// 16 moves 16 bytes per lane and access (a unit that crosses the plane's edge goes sample by sample); any other side takes
// sample-wide accesses.  Nothing outside width * B bytes of a destination row is written.  dst must overlap neither src nor
// aa: other workgroups read the neighbours of both.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "sn_internal.h"

// No contraction: one rounding per written operation.  (R - v * 0.0625f itself could only differ fused where the product
// underflows -- the factor is a power of two, so the product is exact everywhere else -- but d * k and R + c have no such
// excuse, and the file does not leave it to luck: this pragma, and -ffp-contract=off in the Makefile.)
#pragma clang fp contract(off)

namespace sn {

constexpr int kSharpenTileBytes = 256, kSharpenTileH = 16;  // the tile is kSharpenTileBytes / sizeof(sample) columns wide

template <class T>
struct SharpenTile {
    static constexpr int V = 16 / (int)sizeof(T);  // samples per 16 bytes
    static constexpr int TW = kSharpenTileBytes / (int)sizeof(T), TH = kSharpenTileH;
    static constexpr int LW = TW + 2 * V;  // samples per staged row: LDS column c is plane column x0 - V + c
    static constexpr int LR = TH + 2;      // staged rows: LDS row j is plane row y0 - 1 + j
    static constexpr int NV = LW / V;      // 16-byte units per staged row
};

// Step 1 for one plane: rows y0 - 1 .. y0 + th, units 0 .. nvec - 1 of each, coordinates clamped to the plane
template <class T>
__device__ __forceinline__ void sharpen_stage(const uint8_t* p, int pitch, int fast, int w, int h, int x0, int y0, int tw, int th, uint4* lds4)
{
    using M = SharpenTile<T>;
    constexpr int V = M::V, LW = M::LW, NV = M::NV;
    T* lds = reinterpret_cast<T*>(lds4);
    const int nrows = th + 2, nvec = (V + tw) / V + 1;  // LDS columns V - 1 .. V + tw are read
    for (int i = threadIdx.x; i < nrows * NV; i += 256) {
        const int j = i / NV, q = i % NV;
        if (q >= nvec) continue;
        int sy = y0 - 1 + j;
        sy = sy < 0 ? 0 : sy > h - 1 ? h - 1 : sy;
        const int sc = x0 - V + q * V;
        const T* row = reinterpret_cast<const T*>(p + (int64_t)sy * pitch);
        if (fast && sc >= 0 && sc + V <= w) {
            lds4[j * NV + q] = *reinterpret_cast<const uint4*>(row + sc);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                int c = sc + k;
                c = c < 0 ? 0 : c > w - 1 ? w - 1 : c;
                lds[j * LW + q * V + k] = row[c];
            }
        }
    }
}

// Step 1 for both planes.  A tile whose staged units all lie inside the plane, on two aligned sides -- every tile but those on the
// plane's left and right edge --, has at most two units of each plane per thread: all four loads are issued before the first
// LDS store, so a thread waits for memory once, not four times.
template <class T>
__device__ __forceinline__ void sharpen_stage_both(const uint8_t* s, int spitch, int src16, const uint8_t* a, int apitch, int aa16, int w, int h, int x0,
                                                   int y0, int tw, int th, uint4* s4, uint4* r4)
{
    using M = SharpenTile<T>;
    constexpr int V = M::V, NV = M::NV;
    static_assert(M::LR * NV <= 512, "two units of a plane per thread");
    const int nrows = th + 2, nvec = (V + tw) / V + 1;
    if (!(src16 && aa16 && x0 >= V && x0 - V + nvec * V <= w)) {
        sharpen_stage<T>(s, spitch, src16, w, h, x0, y0, tw, th, s4);
        sharpen_stage<T>(a, apitch, aa16, w, h, x0, y0, tw, th, r4);
        return;
    }
    const int i0 = (int)threadIdx.x, i1 = i0 + 256;
    const int j0 = i0 / NV, q0 = i0 % NV, j1 = i1 / NV, q1 = i1 % NV;
    const bool ok0 = i0 < nrows * NV && q0 < nvec, ok1 = i1 < nrows * NV && q1 < nvec;
    auto row_of = [&](int j) {
        const int sy = y0 - 1 + j;
        return sy < 0 ? 0 : sy > h - 1 ? h - 1 : sy;
    };
    const int64_t c0 = (int64_t)(x0 - V + q0 * V) * (int)sizeof(T), c1 = (int64_t)(x0 - V + q1 * V) * (int)sizeof(T);
    uint4 sv0 = {}, rv0 = {}, sv1 = {}, rv1 = {};
    if (ok0) {
        sv0 = *reinterpret_cast<const uint4*>(s + (int64_t)row_of(j0) * spitch + c0);
        rv0 = *reinterpret_cast<const uint4*>(a + (int64_t)row_of(j0) * apitch + c0);
    }
    if (ok1) {
        sv1 = *reinterpret_cast<const uint4*>(s + (int64_t)row_of(j1) * spitch + c1);
        rv1 = *reinterpret_cast<const uint4*>(a + (int64_t)row_of(j1) * apitch + c1);
    }
    if (ok0) s4[j0 * NV + q0] = sv0, r4[j0 * NV + q0] = rv0;
    if (ok1) s4[j1 * NV + q1] = sv1, r4[j1 * NV + q1] = rv1;
}

template <class T>
__global__ void __launch_bounds__(256) k_contra_sharpen(const uint8_t* src, int64_t sfs, int spitch, const uint8_t* aa, int64_t afs, int apitch,
                                                        uint8_t* dst, int64_t dfs, int dpitch, int w, int h, int amount, float kf, int maxv, int src16,
                                                        int aa16, int dst16)
{
    constexpr bool kFloat = std::is_same<T, float>::value;
    using A = typename std::conditional<kFloat, float, int32_t>::type;
    using M = SharpenTile<T>;
    constexpr int V = M::V, TW = M::TW, TH = M::TH, LW = M::LW, LR = M::LR, NV = M::NV;
    __shared__ uint4 s4[LR * NV];
    __shared__ uint4 r4[LR * NV];

    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int tw = w - x0 < TW ? w - x0 : TW, th = h - y0 < TH ? h - y0 : TH;
    sharpen_stage_both<T>(src + (int64_t)blockIdx.z * sfs, spitch, src16, aa + (int64_t)blockIdx.z * afs, apitch, aa16, w, h, x0, y0, tw, th, s4, r4);
    __syncthreads();

    // 2. 16 bytes of one row per thread
    const int r = threadIdx.x / (TW / V), q = threadIdx.x % (TW / V);
    const int xs = x0 + q * V, y = y0 + r;
    if (r >= th || xs >= w) return;
    const int n = w - xs < V ? w - xs : V;
    union Unit {
        uint4 v;
        T t[V];
    };
    // The unit in blocks of U samples, one after the other (8-bit: two blocks of eight): with all sixteen samples of an 8-bit
    // unit in flight the kernel held 113 VGPRs and four waves per SIMD, and ran 14.7 us per 2160p plane against the mask kernel's 8.9
    constexpr int U = V > 8 ? 8 : V;
    struct alignas(U * sizeof(T)) Block {
        T t[U];
    };
    const T* sl = reinterpret_cast<const T*>(s4);
    const T* rl = reinterpret_cast<const T*>(r4);
    Unit out;
#pragma unroll
    for (int o = 0; o < V; o += U) {
        if (o) __builtin_amdgcn_sched_barrier(0);  // (keeps the blocks apart: nothing of the next one is started early)
        A hs[kFloat ? 3 : 1][U];  // float: h of the three rows (the contract orders their sum); integers: the weighted sum so far
        A mn[U], mx[U], rc[U];
#pragma unroll
        for (int k = 0; k < U; ++k) mn[k] = mx[k] = (A)0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {  // LDS row r + j is plane row y - 1 + j
            const int at = (r + j) * LW + V + q * V + o;  // column xs + o
            const Block su = *reinterpret_cast<const Block*>(sl + at), ru = *reinterpret_cast<const Block*>(rl + at);
            A rr[U + 2], dd[U + 2];  // columns xs + o - 1 .. xs + o + U
            rr[0] = (A)rl[at - 1];
            rr[U + 1] = (A)rl[at + U];
            dd[0] = (A)sl[at - 1] - rr[0];
            dd[U + 1] = (A)sl[at + U] - rr[U + 1];
#pragma unroll
            for (int k = 0; k < U; ++k) {
                rr[k + 1] = (A)ru.t[k];
                dd[k + 1] = (A)su.t[k] - rr[k + 1];
            }
#pragma unroll
            for (int k = 0; k < U; ++k) {
                const A hh = (rr[k] + rr[k + 2]) + (rr[k + 1] + rr[k + 1]);
                if constexpr (kFloat) {
                    hs[j][k] = hh;
#pragma unroll
                    for (int i = 0; i < 3; ++i) {  // a NaN is ignored: both comparisons are false
                        if (dd[k + i] < mn[k]) mn[k] = dd[k + i];
                        if (dd[k + i] > mx[k]) mx[k] = dd[k + i];
                    }
                } else {
                    hs[0][k] = j == 0 ? hh : hs[0][k] + (j == 1 ? hh + hh : hh);
                    const A lo = dd[k] < dd[k + 1] ? dd[k] : dd[k + 1], hi = dd[k] > dd[k + 1] ? dd[k] : dd[k + 1];
                    const A lo3 = lo < dd[k + 2] ? lo : dd[k + 2], hi3 = hi > dd[k + 2] ? hi : dd[k + 2];
                    mn[k] = mn[k] < lo3 ? mn[k] : lo3;
                    mx[k] = mx[k] > hi3 ? mx[k] : hi3;
                }
                if (j == 1) rc[k] = rr[k + 1];
            }
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            if constexpr (kFloat) {
                const float v = (hs[0][k] + hs[2][k]) + (hs[1][k] + hs[1][k]);
                const float b = v * 0.0625f;
                const float d = rc[k] - b;
                const float d1 = d * kf;
                float c = d1;
                if (c < mn[k]) c = mn[k];
                if (c > mx[k]) c = mx[k];
                out.t[o + k] = (d1 != d1 || c == 0.0f) ? rc[k] : rc[k] + c;  // never a NaN of our making: R is finite here and c is no NaN
            } else {
                const int32_t b = (hs[0][k] + 8) >> 4;
                const int32_t d = rc[k] - b;
                const int32_t m = ((d < 0 ? -d : d) * amount) >> 6;  // |d| * 255 < 2^24
                int32_t c = d < 0 ? -m : m;
                c = c < mn[k] ? mn[k] : c;
                c = c > mx[k] ? mx[k] : c;
                int32_t ov = rc[k] + c;
                ov = ov < 0 ? 0 : ov > maxv ? maxv : ov;
                out.t[o + k] = (T)ov;
            }
        }
    }
    T* drow = reinterpret_cast<T*>(dst + (int64_t)blockIdx.z * dfs + (int64_t)y * dpitch) + xs;
    if (dst16 && n == V) {
        *reinterpret_cast<uint4*>(drow) = out.v;
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (k < n) drow[k] = out.t[k];
    }
}

template <class T>
static void sharpen_launch(hipStream_t st, int nframes, const uint8_t* src, int64_t sfs, int spitch, const uint8_t* aa, int64_t afs, int apitch, uint8_t* dst,
                           int64_t dfs, int dpitch, int w, int h, int amount, float kf, int maxv, int src16, int aa16, int dst16)
{
    constexpr int TW = kSharpenTileBytes / (int)sizeof(T);
    const dim3 grid((w + TW - 1) / TW, (h + kSharpenTileH - 1) / kSharpenTileH, nframes);
    hipLaunchKernelGGL((k_contra_sharpen<T>), grid, dim3(256), 0, st, src, sfs, spitch, aa, afs, apitch, dst, dfs, dpitch, w, h, amount, kf, maxv, src16, aa16,
                       dst16);
}

hipError_t launch_contra_sharpen(hipStream_t st, int bytes, int bits, int amount, int nframes, PlaneView s, PlaneView a, int w, int h, PlaneViewW d)
{
    if (nframes <= 0 || w <= 0 || h <= 0) return hipSuccess;
    if (amount < 1 || amount > 255) return hipErrorInvalidValue;
    auto fast = [](const uint8_t* base, int pitch, int64_t fs) { return (int)((uintptr_t)base % 16 == 0 && pitch % 16 == 0 && fs % 16 == 0); };
    const int src16 = fast(s.base, s.pitch, s.fs), aa16 = fast(a.base, a.pitch, a.fs), dst16 = fast(d.base, d.pitch, d.fs);
    const float kf = (float)amount * 0.015625f;  // exact
    const int maxv = bytes == 4 ? 0 : (1 << bits) - 1;
    switch (bytes) {
    case 1: sharpen_launch<uint8_t>(st, nframes, s.base, s.fs, s.pitch, a.base, a.fs, a.pitch, d.base, d.fs, d.pitch, w, h, amount, kf, maxv, src16, aa16, dst16); break;
    case 2: sharpen_launch<uint16_t>(st, nframes, s.base, s.fs, s.pitch, a.base, a.fs, a.pitch, d.base, d.fs, d.pitch, w, h, amount, kf, maxv, src16, aa16, dst16); break;
    default: sharpen_launch<float>(st, nframes, s.base, s.fs, s.pitch, a.base, a.fs, a.pitch, d.base, d.fs, d.pitch, w, h, amount, kf, maxv, src16, aa16, dst16); break;
    }
    return hipGetLastError();
}

}  // namespace sn
