// sn_mask.hip -- the edge mask of the anti-aliasing call: a Sobel mask of the SOURCE plane S, two thresholds, one optional
// 3 x 3 expansion, and the merge of the call's result R into S through it (include/sangnom_hip.h, "Edge mask", has the contract).
//
//   e  = (|gx| + |gy|) >> 2 (float: * 0.25f) of the 3 x 3 Sobel pair over S, coordinates clamped to S's edge
//   m0 = 0 up to Tlo, 256 from Thi on, a floor ramp between;  m = m0, or with expand its maximum over 3 x 3 (clamped)
//   out = (S (256 - m) + R m + 128) >> 8      float: S, R, or S + (R - S) * (m / 256), one rounding per operation
// With aa == nullptr the mask itself is written: (m maxv + 128) >> 8, float m / 256.
//
// Tile constants: a workgroup of 256 threads owns kMaskTileBytes / B x kMaskTileH output samples of one frame -- 256 bytes of a
// row x 16 rows whatever the sample type, as k_reduce does.  Three steps, LDS between them:
//   1. S rows y0 - (1 + expand) .. y0 + 16 + expand, each from one 16-byte unit left of the tile to one unit right of it, go
//      to LDS with the edge clamp applied: an S sample leaves memory once per tile, not once per tap.
//   2. A thread walks down one column of the tile plus its halo of `expand` with a window of three S rows in registers
//      (three LDS reads per row), computes m0 per row and, with expand, its running maximum over three rows: the vertical half
//      of the separable 3 x 3 maximum.  m0 at positions outside the plane is 0, which is what the clamped maximum amounts
//      to (the clamp only repeats positions the window already holds).  The result goes to LDS as 16-bit values.  The two
//      halo columns right of the tile are walked row by row by 32 threads.  8-bit samples: |gx| + |gy| is one packed 16-bit
//      SAD and m0 a table of 257 entries in LDS, filled by the workgroup with the contract's own division (the 8-bit kernel
//      is bound by its instructions, not by memory; with the ramp computed per sample it was slower than k_reduce).
//   3. A thread owns 16 bytes of one output row: the horizontal half of the maximum over its V + 2 values, S from LDS, R
//      from memory (not read where all of its m are 0), the merge, one store.  Each thread reads exactly the R samples
//      it overwrites, so dst may be the plane R lies in.
// HBM-bound by design: 2 W H B read, W H B written.  A side (src, aa, dst) whose base, pitch and frame stride are multiples of
// 16 moves 16 bytes per lane and access (a unit that crosses the plane's edge goes sample by sample); any other side takes
// sample-wide accesses.  Nothing outside width * B bytes of a destination row is written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "sn_internal.h"

#pragma clang fp contract(off)

namespace sn {

constexpr int kMaskTileBytes = 256, kMaskTileH = 16;  // the tile is kMaskTileBytes / sizeof(sample) columns wide

// Thresholds as the kernel takes them.  Integer samples: tlo, thi in the clip's scale, span = thi - tlo (1 when they are
// equal: no sample reaches the ramp) and rspan = 1.0f / span.  Float samples: flo, fhi and k = 256.0f / (fhi - flo),
// computed on the host in single precision (k only when hi > lo).
struct MaskThresholds {
    int32_t tlo, thi, span;
    float rspan, flo, fhi, k;
};

// floor(n / d) for 0 <= n < 2^24, 0 < d < 2^16 and n < 256 d: the single-precision product is within one of it, the remainder says which
__device__ __forceinline__ int32_t ramp_div(int32_t n, int32_t d, float rd)
{
    int32_t q = (int32_t)((float)n * rd);
    int32_t r = n - q * d;
    if (r < 0) --q, r += d;
    if (r >= d) ++q;
    return q;
}

// e = (|gx| + |gy|) >> 2 from the operands of the two differences (all of them sums of samples, not negative)
__device__ __forceinline__ int32_t edge_of(int32_t xp, int32_t xm, int32_t yp, int32_t ym) { return (int32_t)(__usad(xp, xm, __usad(yp, ym, 0u)) >> 2); }

__device__ __forceinline__ int32_t mask_of(int32_t e, const MaskThresholds& t)
{
    if (e <= t.tlo) return 0;  // (branches: a wave with no sample on the ramp, most waves of a real frame, skips the division; measured
    if (e >= t.thi) return 256;  // on 2160p Y16, expand 1: 12.4 us against 15.8 without branches on a constant plane, 16.3 against 16.5 on noise)
    return ramp_div((e - t.tlo) << 8, t.span, t.rspan);
}

__device__ __forceinline__ int32_t mask_of(float gx, float gy, const MaskThresholds& t)
{
    const float e = (__builtin_fabsf(gx) + __builtin_fabsf(gy)) * 0.25f;
    if (!(e > t.flo)) return 0;  // a NaN keeps the source
    if (e >= t.fhi) return 256;
    const int32_t m = (int32_t)((e - t.flo) * t.k);
    return m > 256 ? 256 : m;
}

// [1 2 1] over three samples in the written order: (a + c) + (b + b)
template <class A>
__device__ __forceinline__ A smooth3(A a, A b, A c)
{
    return (a + c) + (b + b);
}

__device__ __forceinline__ int32_t merge_sample(int32_t s, int32_t r, int32_t m) { return (s * (256 - m) + r * m + 128) >> 8; }

__device__ __forceinline__ float merge_sample(float s, float r, int32_t m)
{
    if (m == 0) return s;
    if (m == 256) return r;
    return s + (r - s) * ((float)m * 0.00390625f);
}

__device__ __forceinline__ int32_t mask_sample(int32_t m, int32_t maxv, int32_t) { return (m * maxv + 128) >> 8; }
__device__ __forceinline__ float mask_sample(int32_t m, int32_t, float) { return (float)m * 0.00390625f; }

// The tile's geometry in LDS, shared by the kernels of this file (steps 1 and 2 are mask_tile below)
template <class T, int E>
struct MaskTile {
    static constexpr int V = 16 / (int)sizeof(T);  // samples per 16 bytes
    static constexpr int TW = kMaskTileBytes / (int)sizeof(T), TH = kMaskTileH;
    static constexpr int HS = 1 + E;                // halo of S
    static constexpr int LW = TW + 2 * V;           // samples per staged row: LDS column c is S column x0 - V + c
    static constexpr int LR = TH + 2 * HS;          // staged rows: LDS row j is S row y0 - HS + j
    static constexpr int G = 256 / TW;              // groups of rows the walkers of one column share: 1 / 2 / 4
    static constexpr int RG = TH / G;               // output rows per walker
    static constexpr int MW = TW + 8;               // 16-bit values per mask row: column c is plane column x0 - E + c; rows 16-byte aligned
    static constexpr bool kTable = sizeof(T) == 1;  // 8-bit samples: every e >= 256 is above Tlo and at or above Thi, so m0 is a table of 257 entries
};

// Steps 1 and 2 for the tile at (x0, y0) of the plane `s` (w x h): S to lds4 with the edge clamp, then the mask's vertical
// half to vm32 (with E = 0 the mask itself).  Ends behind the barrier after step 2.
template <class T, int E>
__device__ __forceinline__ void mask_tile(const uint8_t* s, int spitch, int src16, int w, int h, int x0, int y0, int tw, int th, const MaskThresholds& t,
                                          uint4* lds4, uint32_t* vm32, uint16_t* m0_of)
{
    using A = typename std::conditional<std::is_same<T, float>::value, float, int32_t>::type;
    using M = MaskTile<T, E>;
    constexpr int V = M::V, TW = M::TW, TH = M::TH, HS = M::HS, LW = M::LW, RG = M::RG, MW = M::MW;
    constexpr bool kTable = M::kTable;
    T* lds = reinterpret_cast<T*>(lds4);
    uint16_t* vm = reinterpret_cast<uint16_t*>(vm32);

    if (kTable) {
        m0_of[threadIdx.x] = (uint16_t)((int)threadIdx.x <= t.tlo ? 0 : (int)threadIdx.x >= t.thi ? 256 : (((int)threadIdx.x - t.tlo) << 8) / t.span);
        if (threadIdx.x == 0) m0_of[256] = 256;
    }

    // 1. the rows and 16-byte units this tile reads: LDS columns V - HS .. V + tw + HS - 1, rows 0 .. th + 2 HS - 1
    constexpr int NV = LW / V;
    const int nrows = th + 2 * HS, nvec = (V + tw + HS - 1) / V + 1;
    for (int i = threadIdx.x; i < nrows * NV; i += 256) {
        const int j = i / NV, q = i % NV;
        if (q >= nvec) continue;
        int sy = y0 - HS + j;
        sy = sy < 0 ? 0 : sy > h - 1 ? h - 1 : sy;
        const int sc = x0 - V + q * V;
        const T* row = reinterpret_cast<const T*>(s + (int64_t)sy * spitch);
        if (src16 && sc >= 0 && sc + V <= w) {
            lds4[j * (LW / V) + q] = *reinterpret_cast<const uint4*>(row + sc);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                int c = sc + k;
                c = c < 0 ? 0 : c > w - 1 ? w - 1 : c;
                lds[j * LW + q * V + k] = row[c];
            }
        }
    }
    __syncthreads();

    // 2. mask column lc, output rows r0 .. r0 + nr - 1 of the tile: m0 of rows r0 - E .. r0 + nr - 1 + E, its maximum over
    // three rows with expand.  Every thread walks one of the tile's columns (G groups of RG rows); the 2 E columns right of
    // them go row by row.  (Rows of a ragged tile that were not staged are read, in bounds of the array, and never used.)
    auto walk = [&](int lc, int r0, auto rows) {
        constexpr int nr = decltype(rows)::value;
        const int x = x0 - E + lc;
        if (x < 0 || x >= w) {
#pragma unroll
            for (int r = r0; r < r0 + nr; ++r) vm[r * MW + lc] = 0;
            return;
        }
        const T* p = lds + r0 * LW + V - E + lc - 1;  // S(y0 + r0 - E - 1, x - 1)
        A a0 = (A)p[0], a2 = (A)p[2], b0 = (A)p[LW], b2 = (A)p[LW + 2];
        A ra = smooth3(a0, (A)p[1], a2), rb = smooth3(b0, (A)p[LW + 1], b2);
        int32_t m1 = 0, m2 = 0;  // m0 of the two rows above
#pragma unroll
        for (int k = 0; k < nr + 2 * E; ++k) {
            const int r = r0 - E + k;
            const T* pc = p + (k + 2) * LW;
            const A c0 = (A)pc[0], c2 = (A)pc[2];
            const A rc = smooth3(c0, (A)pc[1], c2);
            const A xp = smooth3(a2, b2, c2), xm = smooth3(a0, b0, c0);
            const int y = y0 + r;
            int32_t m;
            if constexpr (std::is_same<T, float>::value) {
                m = mask_of(xp - xm, rc - ra, t);
            } else if constexpr (kTable) {  // the sums stay below 2^16: both differences in one packed instruction
                const uint32_t e = __builtin_amdgcn_sad_u16((uint32_t)xp | ((uint32_t)rc << 16), (uint32_t)xm | ((uint32_t)ra << 16), 0u) >> 2;
                m = m0_of[e < 256 ? e : 256];
            } else {
                m = mask_of(edge_of(xp, xm, rc, ra), t);
            }
            m = y >= 0 && y < h ? m : 0;
            if (E) {
                if (k >= 2) {
                    const int32_t mm = m > m1 ? m : m1;
                    vm[(r - 1) * MW + lc] = (uint16_t)(mm > m2 ? mm : m2);
                }
                m2 = m1, m1 = m;
            } else {
                vm[r * MW + lc] = (uint16_t)m;
            }
            ra = rb, rb = rc;
            a0 = b0, a2 = b2, b0 = c0, b2 = c2;
        }
    };
    walk((int)threadIdx.x % TW, (int)threadIdx.x / TW * RG, std::integral_constant<int, RG>());
    if (E && threadIdx.x < 2 * TH) walk(TW + (int)threadIdx.x / TH, (int)threadIdx.x % TH, std::integral_constant<int, 1>());
    __syncthreads();
}

template <class T, int E>
__global__ void __launch_bounds__(256) k_mask_merge(const uint8_t* src, int64_t sfs, int spitch, const uint8_t* aa, int64_t afs, int apitch, uint8_t* dst,
                                                    int64_t dfs, int dpitch, int w, int h, MaskThresholds t, int maxv, int src16, int aa16, int dst16)
{
    using A = typename std::conditional<std::is_same<T, float>::value, float, int32_t>::type;
    using M = MaskTile<T, E>;
    constexpr int V = M::V, TW = M::TW, TH = M::TH, HS = M::HS, LW = M::LW, LR = M::LR, MW = M::MW;
    __shared__ uint4 lds4[LR * LW / V];
    __shared__ uint32_t vm32[TH * MW / 2];
    __shared__ uint16_t m0_of[M::kTable ? 258 : 2];

    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int tw = w - x0 < TW ? w - x0 : TW, th = h - y0 < TH ? h - y0 : TH;
    mask_tile<T, E>(src + (int64_t)blockIdx.z * sfs, spitch, src16, w, h, x0, y0, tw, th, t, lds4, vm32, m0_of);

    // 3. 16 bytes of one row per thread
    const int r = threadIdx.x / (TW / V), q = threadIdx.x % (TW / V);
    const int xs = x0 + q * V, y = y0 + r;
    if (r >= th || xs >= w) return;
    const int n = w - xs < V ? w - xs : V;
    int32_t m[V];
    {
        const uint32_t* vp = vm32 + (r * MW + q * V) / 2;
        uint32_t u[V / 2 + 1];
#pragma unroll
        for (int k = 0; k < V / 2 + E; ++k) u[k] = vp[k];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            auto at = [&](int c) { return (int32_t)((u[c / 2] >> (16 * (c & 1))) & 0xFFFF); };
            if (E) {
                const int32_t mm = at(k) > at(k + 1) ? at(k) : at(k + 1);
                m[k] = mm > at(k + 2) ? mm : at(k + 2);
            } else {
                m[k] = at(k);
            }
        }
    }
    union Unit {
        uint4 v;
        T t[V];
    };
    Unit out;
    T* drow = reinterpret_cast<T*>(dst + (int64_t)blockIdx.z * dfs + (int64_t)y * dpitch) + xs;
    if (!aa) {
#pragma unroll
        for (int k = 0; k < V; ++k) out.t[k] = (T)mask_sample(m[k], maxv, A());
    } else {
        Unit sv, rv;
        sv.v = lds4[(r + HS) * (LW / V) + 1 + q];
        int32_t any = 0;
#pragma unroll
        for (int k = 0; k < V; ++k) any |= k < n ? m[k] : 0;
        if (any) {  // where every m is 0 the result is S and R is not read
            const T* arow = reinterpret_cast<const T*>(aa + (int64_t)blockIdx.z * afs + (int64_t)y * apitch) + xs;
            if (aa16 && n == V) {
                rv.v = *reinterpret_cast<const uint4*>(arow);
            } else {
#pragma unroll
                for (int k = 0; k < V; ++k) rv.t[k] = k < n ? arow[k] : sv.t[k];
            }
        } else {
            rv = sv;
        }
#pragma unroll
        for (int k = 0; k < V; ++k) out.t[k] = (T)merge_sample((A)sv.t[k], (A)rv.t[k], m[k]);
    }
    if (dst16 && n == V) {
        *reinterpret_cast<uint4*>(drow) = out.v;
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (k < n) drow[k] = out.t[k];
    }
}

template <class T>
static void mask_launch(hipStream_t st, int expand, int nframes, const uint8_t* src, int64_t sfs, int spitch, const uint8_t* aa, int64_t afs, int apitch,
                        uint8_t* dst, int64_t dfs, int dpitch, int w, int h, const MaskThresholds& t, int maxv, int src16, int aa16, int dst16)
{
    constexpr int TW = kMaskTileBytes / (int)sizeof(T);
    const dim3 grid((w + TW - 1) / TW, (h + kMaskTileH - 1) / kMaskTileH, nframes);
    if (expand)
        hipLaunchKernelGGL((k_mask_merge<T, 1>), grid, dim3(256), 0, st, src, sfs, spitch, aa, afs, apitch, dst, dfs, dpitch, w, h, t, maxv, src16, aa16, dst16);
    else
        hipLaunchKernelGGL((k_mask_merge<T, 0>), grid, dim3(256), 0, st, src, sfs, spitch, aa, afs, apitch, dst, dfs, dpitch, w, h, t, maxv, src16, aa16, dst16);
}

static MaskThresholds thresholds_of(int bytes, int bits, int lo, int hi)
{
    MaskThresholds t{};
    if (bytes == 4) {
        t.flo = (float)lo / 255.0f;
        t.fhi = (float)hi / 255.0f;
        t.k = hi > lo ? 256.0f / (t.fhi - t.flo) : 0.0f;
    } else {
        t.tlo = lo << (bits - 8);
        t.thi = hi << (bits - 8);
        t.span = hi > lo ? t.thi - t.tlo : 1;
        t.rspan = 1.0f / (float)t.span;
    }
    return t;
}

hipError_t launch_mask_merge(hipStream_t st, int bytes, int bits, int lo, int hi, int expand, int nframes, PlaneView s, PlaneView a, int w, int h,
                             PlaneViewW d)
{
    const uint8_t *const src = s.base, *const aa = a.base;
    uint8_t* const dst = d.base;
    const int64_t sfs = s.fs, afs = a.fs, dfs = d.fs;
    const int spitch = s.pitch, apitch = a.pitch, dpitch = d.pitch;
    if (nframes <= 0 || w <= 0 || h <= 0) return hipSuccess;
    if (lo < 0 || hi > 255 || lo > hi || expand < 0 || expand > 1) return hipErrorInvalidValue;
    const int src16 = (uintptr_t)src % 16 == 0 && spitch % 16 == 0 && sfs % 16 == 0;
    const int aa16 = (uintptr_t)aa % 16 == 0 && apitch % 16 == 0 && afs % 16 == 0;
    const int dst16 = (uintptr_t)dst % 16 == 0 && dpitch % 16 == 0 && dfs % 16 == 0;
    const MaskThresholds t = thresholds_of(bytes, bits, lo, hi);
    const int maxv = bytes == 4 ? 0 : (1 << bits) - 1;
    switch (bytes) {
    case 1: mask_launch<uint8_t>(st, expand, nframes, src, sfs, spitch, aa, afs, apitch, dst, dfs, dpitch, w, h, t, maxv, src16, aa16, dst16); break;
    case 2: mask_launch<uint16_t>(st, expand, nframes, src, sfs, spitch, aa, afs, apitch, dst, dfs, dpitch, w, h, t, maxv, src16, aa16, dst16); break;
    default: mask_launch<float>(st, expand, nframes, src, sfs, spitch, aa, afs, apitch, dst, dfs, dpitch, w, h, t, maxv, src16, aa16, dst16); break;
    }
    return hipGetLastError();
}

// ---- chroma merged through the LUMA plane's mask (sangnom_hip.h, "Edge mask": mc) ----------------------------------------------
// One launch serves one or two chroma planes (U and V) of w x h samples under a luma plane of (w << sw) x (h << sh).  A
// workgroup owns the same LUMA tile as k_mask_merge, 256 bytes of a row x 16 rows, and with it the chroma tile of
// (TW >> sw) x (16 >> sh) samples of each plane.  Steps 1 and 2 are mask_tile on the luma plane.  Step 3: a thread owns 16
// bytes of one chroma row of one plane; it reads the (V << sw) + 2 E values of each of its 2^sh rows of vm once, takes the
// horizontal half of the maximum and sums the block: mc = (sum + half) >> (sw + sh).  S and R of the chroma plane come from
// memory (R not where all mc of the unit are 0; each thread reads exactly the R samples it overwrites, so dst may be R's
// plane), one store.  The units of both planes are dealt to the 256 threads in turn, (16 >> sw) * (16 >> sh) per plane:
// 4:2:0 keeps 128 threads busy with two planes, 4:4:4 gives every thread one unit of each plane and reduces vm once for both.
// No LDS beyond k_mask_merge's.  A side is luma, or src / aa / dst of one plane, each with its own 16-byte flag.
struct LumaMergeArgs {
    const uint8_t* luma;
    int64_t lfs;
    int lpitch, luma16;
    const uint8_t* src[2];
    const uint8_t* aa[2];
    uint8_t* dst[2];
    int64_t sfs[2], afs[2], dfs[2];
    int spitch[2], apitch[2], dpitch[2];
    int src16[2], aa16[2], dst16[2];
    int planes, w, h, sh, maxv;  // w x h: a chroma plane
};

template <class T, int E, int SW>
__global__ void __launch_bounds__(256) k_mask_merge_luma(LumaMergeArgs g, MaskThresholds t)
{
    using A = typename std::conditional<std::is_same<T, float>::value, float, int32_t>::type;
    using M = MaskTile<T, E>;
    constexpr int V = M::V, TW = M::TW, TH = M::TH, LW = M::LW, LR = M::LR, MW = M::MW;
    __shared__ uint4 lds4[LR * LW / V];
    __shared__ uint32_t vm32[TH * MW / 2];
    __shared__ uint16_t m0_of[M::kTable ? 258 : 2];

    const int sh = g.sh, n = SW + sh;
    const int wl = g.w << SW, hl = g.h << sh;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int tw = wl - x0 < TW ? wl - x0 : TW, th = hl - y0 < TH ? hl - y0 : TH;
    mask_tile<T, E>(g.luma + (int64_t)blockIdx.z * g.lfs, g.lpitch, g.luma16, wl, hl, x0, y0, tw, th, t, lds4, vm32, m0_of);

    // 3. 16 bytes of one chroma row of one plane per thread and turn
    constexpr int UR = (TW / V) >> SW;  // units per chroma row of the tile: 16 / 8 / 4
    constexpr int NL = V << SW;         // luma columns under a unit
    const int units = UR * (TH >> sh);
    int32_t m[V];
    int have = -1;
    for (int i = threadIdx.x; i < units * g.planes; i += 256) {
        const int p = i / units, u = i % units;
        const int r = u / UR, q = u % UR;
        const int xs = (x0 >> SW) + q * V, y = (y0 >> sh) + r;
        if (y >= g.h || xs >= g.w) continue;
        const int nv = g.w - xs < V ? g.w - xs : V;
        if (u != have) {
            have = u;
#pragma unroll
            for (int k = 0; k < V; ++k) m[k] = 0;
            for (int j = 0; j < (1 << sh); ++j) {
                const uint32_t* vp = vm32 + (((r << sh) + j) * MW + q * NL) / 2;
                uint32_t w2[NL / 2 + 1];
#pragma unroll
                for (int k = 0; k < NL / 2 + E; ++k) w2[k] = vp[k];
                auto at = [&](int c) { return (int32_t)((w2[c / 2] >> (16 * (c & 1))) & 0xFFFF); };
#pragma unroll
                for (int k = 0; k < NL; ++k) {
                    int32_t v = at(k);
                    if (E) {
                        v = v > at(k + 1) ? v : at(k + 1);
                        v = v > at(k + 2) ? v : at(k + 2);
                    }
                    m[k >> SW] += v;
                }
            }
#pragma unroll
            for (int k = 0; k < V; ++k) m[k] = (m[k] + ((1 << n) >> 1)) >> n;
        }
        union Unit {
            uint4 v;
            T t[V];
        };
        Unit out;
        T* drow = reinterpret_cast<T*>(g.dst[p] + (int64_t)blockIdx.z * g.dfs[p] + (int64_t)y * g.dpitch[p]) + xs;
        if (!g.aa[p]) {
#pragma unroll
            for (int k = 0; k < V; ++k) out.t[k] = (T)mask_sample(m[k], g.maxv, A());
        } else {
            Unit sv, rv;
            const T* srow = reinterpret_cast<const T*>(g.src[p] + (int64_t)blockIdx.z * g.sfs[p] + (int64_t)y * g.spitch[p]) + xs;
            if (g.src16[p] && nv == V) {
                sv.v = *reinterpret_cast<const uint4*>(srow);
            } else {
#pragma unroll
                for (int k = 0; k < V; ++k) sv.t[k] = k < nv ? srow[k] : (T)0;
            }
            int32_t any = 0;
#pragma unroll
            for (int k = 0; k < V; ++k) any |= k < nv ? m[k] : 0;
            if (any) {  // where every mc is 0 the result is S and R is not read
                const T* arow = reinterpret_cast<const T*>(g.aa[p] + (int64_t)blockIdx.z * g.afs[p] + (int64_t)y * g.apitch[p]) + xs;
                if (g.aa16[p] && nv == V) {
                    rv.v = *reinterpret_cast<const uint4*>(arow);
                } else {
#pragma unroll
                    for (int k = 0; k < V; ++k) rv.t[k] = k < nv ? arow[k] : sv.t[k];
                }
            } else {
                rv = sv;
            }
#pragma unroll
            for (int k = 0; k < V; ++k) out.t[k] = (T)merge_sample((A)sv.t[k], (A)rv.t[k], m[k]);
        }
        if (g.dst16[p] && nv == V) {
            *reinterpret_cast<uint4*>(drow) = out.v;
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (k < nv) drow[k] = out.t[k];
        }
    }
}

template <class T>
static void mask_luma_launch(hipStream_t st, int expand, int sw, int nframes, const LumaMergeArgs& g, const MaskThresholds& t)
{
    constexpr int TW = kMaskTileBytes / (int)sizeof(T);
    const dim3 grid(((g.w << sw) + TW - 1) / TW, ((g.h << g.sh) + kMaskTileH - 1) / kMaskTileH, nframes);
#define SN_LUMA_MERGE(E, SW) hipLaunchKernelGGL((k_mask_merge_luma<T, E, SW>), grid, dim3(256), 0, st, g, t)
    switch (sw * 2 + (expand ? 1 : 0)) {
    case 0: SN_LUMA_MERGE(0, 0); break;
    case 1: SN_LUMA_MERGE(1, 0); break;
    case 2: SN_LUMA_MERGE(0, 1); break;
    case 3: SN_LUMA_MERGE(1, 1); break;
    case 4: SN_LUMA_MERGE(0, 2); break;
    default: SN_LUMA_MERGE(1, 2); break;
    }
#undef SN_LUMA_MERGE
}

hipError_t launch_mask_merge_luma(hipStream_t st, int bytes, int bits, int lo, int hi, int expand, int nframes, PlaneView luma, int sub_w, int sub_h,
                                  int planes, const PlaneView s[2], const PlaneView a[2], int w, int h, const PlaneViewW d[2])
{
    if (nframes <= 0 || w <= 0 || h <= 0) return hipSuccess;
    if (lo < 0 || hi > 255 || lo > hi || expand < 0 || expand > 1 || sub_w < 0 || sub_w > 2 || sub_h < 0 || sub_h > 2 || planes < 1 || planes > 2)
        return hipErrorInvalidValue;
    auto fast = [](const uint8_t* base, int pitch, int64_t fs) { return (int)((uintptr_t)base % 16 == 0 && pitch % 16 == 0 && fs % 16 == 0); };
    LumaMergeArgs g{};
    g.luma = luma.base, g.lfs = luma.fs, g.lpitch = luma.pitch, g.luma16 = fast(luma.base, luma.pitch, luma.fs);
    for (int p = 0; p < planes; ++p) {
        g.src[p] = s[p].base, g.sfs[p] = s[p].fs, g.spitch[p] = s[p].pitch, g.src16[p] = fast(s[p].base, s[p].pitch, s[p].fs);
        g.aa[p] = a[p].base, g.afs[p] = a[p].fs, g.apitch[p] = a[p].pitch, g.aa16[p] = fast(a[p].base, a[p].pitch, a[p].fs);
        g.dst[p] = d[p].base, g.dfs[p] = d[p].fs, g.dpitch[p] = d[p].pitch, g.dst16[p] = fast(d[p].base, d[p].pitch, d[p].fs);
    }
    g.planes = planes, g.w = w, g.h = h, g.sh = sub_h, g.maxv = bytes == 4 ? 0 : (1 << bits) - 1;
    const MaskThresholds t = thresholds_of(bytes, bits, lo, hi);
    switch (bytes) {
    case 1: mask_luma_launch<uint8_t>(st, expand, sub_w, nframes, g, t); break;
    case 2: mask_luma_launch<uint16_t>(st, expand, sub_w, nframes, g, t); break;
    default: mask_luma_launch<float>(st, expand, sub_w, nframes, g, t); break;
    }
    return hipGetLastError();
}

}  // namespace sn
