// sn_repair.hip -- the rank repair of the anti-aliasing call: each sample of the call's result R is clamped into the range
// spanned by the rank-th smallest and the rank-th largest of the nine source samples around it, which is what scripts do with
// Repair(filtered, source, mode) behind an edge-directed interpolator (include/sangnom_hip.h, "Rank repair", has the contract).
//
//   a[1] <= ... <= a[9]: S(y+j, x+i), j, i in {-1, 0, 1}, coordinates clamped to the plane's edge
//   out = min(max(R(y,x), a[rank]), a[10 - rank])           float: R where it or one of the nine is a NaN; a zero bound is +0.0
//
// Tile constants: a workgroup of 256 threads owns kRepairTileBytes / B x kRepairTileH output samples of one frame -- 256 bytes
// of a row x 16 rows whatever the sample type, as k_contra_sharpen, k_mask_merge and k_reduce do.  Two steps, LDS between them:
//   1. S rows y0 - 1 .. y0 + 16, from one 16-byte unit left of the tile to one unit right of it, go to LDS with the edge clamp
//      applied.  R is needed at the centre only: the thread that writes a unit loads it straight from memory, ahead of the
//      barrier, which is also what lets dst be the plane R lies in.
//   2. A thread owns 16 bytes of one output row, in blocks of at most eight samples.  It sorts each of the block's U + 2
//      columns of three once (min3 / med3 / max3); a sample takes its two bounds from the three sorted columns around it:
//      sorting the three minima, the three medians and the three maxima leaves a 3 x 3 matrix ordered along rows and columns,
//      in which a[k] has few places to be (bounds_of() has them).  Only what the rank needs is computed: the rank is a
//      template argument.
// Float samples are staged as keys: sign-magnitude -> two's complement, so that both zeros are key 0, the order of the keys
// is the order of `<`, and a bound that is a zero decodes to +0.0 without anybody asking which zero the network delivered.
// A NaN has a key beyond either infinity's.  The file has no float arithmetic at all.
// HBM-bound by design: 2 W H B read, W H B written.  A side (src, aa, dst) whose base, pitch and frame stride are multiples of
// 16 moves 16 bytes per lane and access (a unit that crosses the plane's edge goes sample by sample); any other side takes
// sample-wide accesses.  Nothing outside width * B bytes of a destination row is written.  dst must not overlap src: other
// workgroups read its neighbours.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "sn_internal.h"

namespace sn {

constexpr int kRepairTileBytes = 256, kRepairTileH = 16;  // the tile is kRepairTileBytes / sizeof(sample) columns wide

template <class T>
struct RepairTile {
    static constexpr int V = 16 / (int)sizeof(T);  // samples per 16 bytes
    static constexpr int TW = kRepairTileBytes / (int)sizeof(T), TH = kRepairTileH;
    static constexpr int LW = TW + 2 * V;  // samples per staged row: LDS column c is plane column x0 - V + c
    static constexpr int LR = TH + 2;      // staged rows: LDS row j is plane row y0 - 1 + j
    static constexpr int NV = LW / V;      // 16-byte units per staged row
};

constexpr int32_t kRepairInfKey = 0x7F800000;  // |key| above it: a NaN

// float bits <-> key (an involution up to the sign of zero: both zeros are key 0, and key 0 is +0.0)
__device__ __forceinline__ uint32_t repair_key(uint32_t b)
{
    const int32_t m = (int32_t)(b & 0x7FFFFFFFu);
    return (uint32_t)((int32_t)b < 0 ? -m : m);
}
__device__ __forceinline__ uint32_t repair_bits(int32_t k) { return k < 0 ? 0x80000000u - (uint32_t)k : (uint32_t)k; }

template <class T>
__device__ __forceinline__ uint4 repair_keys(uint4 v)
{
    if constexpr (std::is_same<T, float>::value) v.x = repair_key(v.x), v.y = repair_key(v.y), v.z = repair_key(v.z), v.w = repair_key(v.w);
    return v;
}

__device__ __forceinline__ int32_t min2(int32_t a, int32_t b) { return a < b ? a : b; }
__device__ __forceinline__ int32_t max2(int32_t a, int32_t b) { return a > b ? a : b; }
__device__ __forceinline__ int32_t min3(int32_t a, int32_t b, int32_t c) { return min2(min2(a, b), c); }  // (one v_min3_i32)
__device__ __forceinline__ int32_t max3(int32_t a, int32_t b, int32_t c) { return max2(max2(a, b), c); }
__device__ __forceinline__ int32_t med3(int32_t a, int32_t b, int32_t c)
{
    int32_t d;  // (the compiler forms v_med3 only around constants)
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}

// a[RANK] and a[10 - RANK] of nine values given as three columns sorted in themselves: lo[i] <= mi[i] <= hi[i], i = 0..2.
// With L = sorted(lo), M = sorted(mi), H = sorted(hi), rows and columns of [L; M; H] ascend, and counting who is surely below
// and surely above whom leaves
//   a[1] = L0                                    a[9] = H2
//   a[2] = min(L1, M0)                           a[8] = max(H1, M2)
//   a[3] = min(max(L1, M0), L2, H0)              a[7] = max(min(H1, M2), H0, L2)
//   a[4] = min(max(u, max(L1, M0)), v, M1)       a[6] = max(min(v, min(H1, M2)), u, M1),   u = min(L2, H0), v = max(L2, H0)
// (tests/test_aa_repair_cpu.py walks every 0-1 input through these lines.)
template <int RANK>
__device__ __forceinline__ void bounds_of(const int32_t* lo, const int32_t* mi, const int32_t* hi, int32_t& a_lo, int32_t& a_hi)
{
    if constexpr (RANK == 1) {
        a_lo = min3(lo[0], lo[1], lo[2]);
        a_hi = max3(hi[0], hi[1], hi[2]);
    } else {
        const int32_t L1 = med3(lo[0], lo[1], lo[2]), M0 = min3(mi[0], mi[1], mi[2]);
        const int32_t H1 = med3(hi[0], hi[1], hi[2]), M2 = max3(mi[0], mi[1], mi[2]);
        if constexpr (RANK == 2) {
            a_lo = min2(L1, M0);
            a_hi = max2(H1, M2);
        } else {
            const int32_t L2 = max3(lo[0], lo[1], lo[2]), H0 = min3(hi[0], hi[1], hi[2]);
            const int32_t q = max2(L1, M0), p = min2(H1, M2);
            if constexpr (RANK == 3) {
                a_lo = min3(q, L2, H0);
                a_hi = max3(p, H0, L2);
            } else {
                const int32_t M1 = med3(mi[0], mi[1], mi[2]);
                const int32_t u = min2(L2, H0), v = max2(L2, H0);
                a_lo = min3(max2(u, q), v, M1);
                a_hi = max3(min2(v, p), u, M1);
            }
        }
    }
}

// Step 1: rows y0 - 1 .. y0 + th, units 0 .. nvec - 1 of each, coordinates clamped to the plane (float: as keys).  A tile whose
// staged units all lie inside the plane, on an aligned side -- every tile but those on the plane's left and right edge --, has
// at most two units per thread: both loads are issued before the first LDS store.
template <class T>
__device__ __forceinline__ void repair_stage(const uint8_t* p, int pitch, int fast, int w, int h, int x0, int y0, int tw, int th, uint4* lds4)
{
    using M = RepairTile<T>;
    constexpr int V = M::V, LW = M::LW, NV = M::NV;
    static_assert(M::LR * NV <= 512, "two units per thread");
    const int nrows = th + 2, nvec = (V + tw) / V + 1;  // LDS columns V - 1 .. V + tw are read
    auto row_of = [&](int j) {
        const int sy = y0 - 1 + j;
        return sy < 0 ? 0 : sy > h - 1 ? h - 1 : sy;
    };
    if (fast && x0 >= V && x0 - V + nvec * V <= w) {
        const int i0 = (int)threadIdx.x, i1 = i0 + 256;
        const int j0 = i0 / NV, q0 = i0 % NV, j1 = i1 / NV, q1 = i1 % NV;
        const bool ok0 = i0 < nrows * NV && q0 < nvec, ok1 = i1 < nrows * NV && q1 < nvec;
        uint4 v0 = {}, v1 = {};
        if (ok0) v0 = *reinterpret_cast<const uint4*>(p + (int64_t)row_of(j0) * pitch + (int64_t)(x0 - V + q0 * V) * (int)sizeof(T));
        if (ok1) v1 = *reinterpret_cast<const uint4*>(p + (int64_t)row_of(j1) * pitch + (int64_t)(x0 - V + q1 * V) * (int)sizeof(T));
        if (ok0) lds4[j0 * NV + q0] = repair_keys<T>(v0);
        if (ok1) lds4[j1 * NV + q1] = repair_keys<T>(v1);
        return;
    }
    using E = typename std::conditional<std::is_same<T, float>::value, uint32_t, T>::type;
    E* lds = reinterpret_cast<E*>(lds4);
    for (int i = threadIdx.x; i < nrows * NV; i += 256) {
        const int j = i / NV, q = i % NV;
        if (q >= nvec) continue;
        const int sc = x0 - V + q * V;
        const E* row = reinterpret_cast<const E*>(p + (int64_t)row_of(j) * pitch);
        if (fast && sc >= 0 && sc + V <= w) {
            lds4[j * NV + q] = repair_keys<T>(*reinterpret_cast<const uint4*>(row + sc));
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                int c = sc + k;
                c = c < 0 ? 0 : c > w - 1 ? w - 1 : c;
                E s = row[c];
                if constexpr (std::is_same<T, float>::value) s = repair_key(s);
                lds[j * LW + q * V + k] = s;
            }
        }
    }
}

template <class T, int RANK>
__global__ void __launch_bounds__(256) k_repair(const uint8_t* src, int64_t sfs, int spitch, const uint8_t* aa, int64_t afs, int apitch, uint8_t* dst,
                                                int64_t dfs, int dpitch, int w, int h, int src16, int aa16, int dst16)
{
    constexpr bool kFloat = std::is_same<T, float>::value;
    using E = typename std::conditional<kFloat, int32_t, T>::type;  // what LDS holds: samples, or a float's key
    using R = typename std::conditional<kFloat, uint32_t, T>::type;  // what memory holds, as bits
    using M = RepairTile<T>;
    constexpr int V = M::V, TW = M::TW, TH = M::TH, LW = M::LW, LR = M::LR, NV = M::NV;
    __shared__ uint4 s4[LR * NV];

    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int tw = w - x0 < TW ? w - x0 : TW, th = h - y0 < TH ? h - y0 : TH;
    // 16 bytes of one row per thread
    const int r = threadIdx.x / (TW / V), q = threadIdx.x % (TW / V);
    const int xs = x0 + q * V, y = y0 + r;
    const bool mine = r < th && xs < w;
    const int n = w - xs < V ? w - xs : V;
    union Unit {
        uint4 v;
        R t[V];
    };
    // R at the centre, ahead of the barrier (dst == aa: this thread alone reads and writes these samples)
    Unit rv;
    rv.v = uint4{};
    if (mine) {
        const R* arow = reinterpret_cast<const R*>(aa + (int64_t)blockIdx.z * afs + (int64_t)y * apitch) + xs;
        if (aa16 && n == V) {
            rv.v = *reinterpret_cast<const uint4*>(arow);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (k < n) rv.t[k] = arow[k];
        }
    }
    repair_stage<T>(src + (int64_t)blockIdx.z * sfs, spitch, src16, w, h, x0, y0, tw, th, s4);
    __syncthreads();
    if (!mine) return;

    // 2. the unit in blocks of U samples, one after the other (8-bit: two blocks of eight, as in k_contra_sharpen)
    constexpr int U = V > 8 ? 8 : V;
    struct alignas(U * sizeof(E)) Block {
        E t[U];
    };
    const E* sl = reinterpret_cast<const E*>(s4);
    Unit out;
#pragma unroll
    for (int o = 0; o < V; o += U) {
        if (o) __builtin_amdgcn_sched_barrier(0);  // (keeps the blocks apart: nothing of the next one is started early)
        int32_t c[3][U + 2];  // columns xs + o - 1 .. xs + o + U of LDS rows r .. r + 2 (plane rows y - 1 .. y + 1)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int at = (r + j) * LW + V + q * V + o;  // column xs + o
            const Block b = *reinterpret_cast<const Block*>(sl + at);
            c[j][0] = (int32_t)sl[at - 1];
            c[j][U + 1] = (int32_t)sl[at + U];
#pragma unroll
            for (int k = 0; k < U; ++k) c[j][k + 1] = (int32_t)b.t[k];
        }
        int32_t lo[U + 2], mi[U + 2], hi[U + 2];  // each column sorted, once for the three samples that use it
#pragma unroll
        for (int k = 0; k < U + 2; ++k) {
            lo[k] = min3(c[0][k], c[1][k], c[2][k]);
            mi[k] = med3(c[0][k], c[1][k], c[2][k]);
            hi[k] = max3(c[0][k], c[1][k], c[2][k]);
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            int32_t a_lo, a_hi;
            bounds_of<RANK>(lo + k, mi + k, hi + k, a_lo, a_hi);
            if constexpr (kFloat) {
                const int32_t rk = (int32_t)repair_key(rv.t[o + k]);
                // a NaN among the ten: a key beyond an infinity's (a[1] and a[9] say it for the nine)
                const int32_t least = RANK == 1 ? a_lo : min3(lo[k], lo[k + 1], lo[k + 2]), most = RANK == 1 ? a_hi : max3(hi[k], hi[k + 1], hi[k + 2]);
                const bool nan = min2(least, rk) < -kRepairInfKey || max2(most, rk) > kRepairInfKey;
                const int32_t ok = med3(rk, a_lo, a_hi);  // a_lo <= a_hi: the clamp
                out.t[o + k] = (nan || ok == rk) ? rv.t[o + k] : repair_bits(ok);  // inside, bounds included: R bit for bit
            } else {
                out.t[o + k] = (R)med3((int32_t)rv.t[o + k], a_lo, a_hi);
            }
        }
    }
    R* drow = reinterpret_cast<R*>(dst + (int64_t)blockIdx.z * dfs + (int64_t)y * dpitch) + xs;
    if (dst16 && n == V) {
        *reinterpret_cast<uint4*>(drow) = out.v;
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (k < n) drow[k] = out.t[k];
    }
}

template <class T>
static void repair_launch(hipStream_t st, int rank, int nframes, PlaneView s, PlaneView a, PlaneViewW d, int w, int h, int src16, int aa16, int dst16)
{
    constexpr int TW = kRepairTileBytes / (int)sizeof(T);
    const dim3 grid((w + TW - 1) / TW, (h + kRepairTileH - 1) / kRepairTileH, nframes);
    switch (rank) {  // uniform over a launch: the kernel has no rank in its sample loop
    case 1: hipLaunchKernelGGL((k_repair<T, 1>), grid, dim3(256), 0, st, s.base, s.fs, s.pitch, a.base, a.fs, a.pitch, d.base, d.fs, d.pitch, w, h, src16, aa16, dst16); break;
    case 2: hipLaunchKernelGGL((k_repair<T, 2>), grid, dim3(256), 0, st, s.base, s.fs, s.pitch, a.base, a.fs, a.pitch, d.base, d.fs, d.pitch, w, h, src16, aa16, dst16); break;
    case 3: hipLaunchKernelGGL((k_repair<T, 3>), grid, dim3(256), 0, st, s.base, s.fs, s.pitch, a.base, a.fs, a.pitch, d.base, d.fs, d.pitch, w, h, src16, aa16, dst16); break;
    default: hipLaunchKernelGGL((k_repair<T, 4>), grid, dim3(256), 0, st, s.base, s.fs, s.pitch, a.base, a.fs, a.pitch, d.base, d.fs, d.pitch, w, h, src16, aa16, dst16); break;
    }
}

hipError_t launch_repair(hipStream_t st, int bytes, int rank, int nframes, PlaneView s, PlaneView a, int w, int h, PlaneViewW d)
{
    if (nframes <= 0 || w <= 0 || h <= 0) return hipSuccess;
    if (rank < 1 || rank > 4) return hipErrorInvalidValue;
    auto fast = [](const uint8_t* base, int pitch, int64_t fs) { return (int)((uintptr_t)base % 16 == 0 && pitch % 16 == 0 && fs % 16 == 0); };
    const int src16 = fast(s.base, s.pitch, s.fs), aa16 = fast(a.base, a.pitch, a.fs), dst16 = fast(d.base, d.pitch, d.fs);
    switch (bytes) {
    case 1: repair_launch<uint8_t>(st, rank, nframes, s, a, d, w, h, src16, aa16, dst16); break;
    case 2: repair_launch<uint16_t>(st, rank, nframes, s, a, d, w, h, src16, aa16, dst16); break;
    default: repair_launch<float>(st, rank, nframes, s, a, d, w, h, src16, aa16, dst16); break;
    }
    return hipGetLastError();
}

}  // namespace sn
