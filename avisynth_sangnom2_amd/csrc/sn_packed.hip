// sn_packed.hip -- packed 4:2:2 on the device: ONE plane that holds Y, U and V (what SDI / HDMI capture and uncompressed
// intermediates hand over) unpacked into a Y, a U and a V plane for the passes, and packed again.
//   YUYV (YUY2; Y210 / Y212 / Y216 with 16-bit words):  Y0 U0 Y1 V0  Y2 U1 Y3 V1 ...
//   UYVY (v216 with 16-bit words):                      U0 Y0 V0 Y1  U1 Y2 V1 Y3 ...
//   v210: blocks of four little-endian 32-bit words for six pixels, three 10-bit fields per word at bits 0, 10 and 20:
//         U0 Y0 V0 | Y1 U1 Y2 | V1 Y3 U2 | Y4 V2 Y5;  the planes are 16-bit words (a 10-bit context)
// Memory-bound, no reuse, so no LDS; the shape of k_uv (sn_uv.hip): rows with 64-bit offsets, blockIdx.z over frames with a loop,
// the field form (only the lines row0 + rstep r), vec_ok per launch.
// YUYV / UYVY: a lane of the vector path moves 64 packed bytes -- four 16-byte loads, de-interleaved by v_perm_b32 (byte selectors
// for 8-bit samples, half-word selectors for 16-bit) into two 16-byte stores of Y and one each of U and V; the pack is the
// inverse.  The pixel pairs of a row behind its last whole vector, and every pair of a launch that is not 16-byte aligned, move
// one sample per access.  MSB-aligned words (Y210, Y212) go through (x >> ss) << ds as in k_uv: the unpack shifts what it loads
// down by ss, the pack what it loads up by ds.
// v210: a lane of the vector path moves one 128-byte group of 48 pixels -- eight 16-byte loads into six 16-byte stores of Y and
// three each of U and V; the pack is the inverse.  The blocks behind the last whole group, and every block of an unaligned
// launch, go one block per lane as four 4-byte words, their samples one at a time: pixels at or beyond w are not stored by the
// unpack and are zero fields in the pack.  Bits 30..31 of a word are ignored on input and zero on output; a packed field is
// sample & 0x3FF.
// Never a byte beyond the row size of a packed row (2 w B; 16 ceil(w / 6)), w B of a Y row, (w / 2) B of a U or V row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sn_internal.h"

namespace sn {

constexpr int kPkLanes = 64;  // lanes along a row: one wave
constexpr int kPkRows = 4;    // rows per workgroup

struct PkPlane {  // frame f's line y starts at base + f * fs + y * pitch
    uint8_t* base;
    int64_t fs;
    int32_t pitch;
};

typedef uint16_t PkU16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk_shift(uint32_t x, int ss, int ds)
{
    PkU16x2 v = __builtin_bit_cast(PkU16x2, x);
    v = (v >> (uint16_t)ss) << (uint16_t)ds;
    return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ uint4 pk_shift(uint4 a, int ss, int ds)
{
    return make_uint4(pk_shift(a.x, ss, ds), pk_shift(a.y, ss, ds), pk_shift(a.z, ss, ds), pk_shift(a.w, ss, ds));
}

// v_perm_b32 takes bytes 0..3 from its second operand and 4..7 from its first
template <int B>
struct PkSel;
template <>
struct PkSel<1> {
    static constexpr uint32_t even = 0x06040200u, odd = 0x07050301u;  // (d1, d0) -> bytes 0 2 4 6 / 1 3 5 7
    static constexpr uint32_t lo = 0x05010400u, hi = 0x07030602u;     // (b, a)   -> a0 b0 a1 b1 / a2 b2 a3 b3
};
template <>
struct PkSel<2> {
    static constexpr uint32_t even = 0x05040100u, odd = 0x07060302u;  // (d1, d0) -> halves 0 2 / 1 3
    static constexpr uint32_t lo = 0x05040100u, hi = 0x07060302u;     // (b, a)   -> a0 b0 / a1 b1
};

// 16 packed bytes -> 8 bytes of Y (y0, y1), 4 of U, 4 of V
template <int B, bool kUyvy>
__device__ __forceinline__ void yuyv_split(uint4 a, uint32_t& y0, uint32_t& y1, uint32_t& u, uint32_t& v)
{
    constexpr uint32_t sy = kUyvy ? PkSel<B>::odd : PkSel<B>::even, sc = kUyvy ? PkSel<B>::even : PkSel<B>::odd;
    y0 = __builtin_amdgcn_perm(a.y, a.x, sy), y1 = __builtin_amdgcn_perm(a.w, a.z, sy);
    const uint32_t c0 = __builtin_amdgcn_perm(a.y, a.x, sc), c1 = __builtin_amdgcn_perm(a.w, a.z, sc);  // U V U V
    u = __builtin_amdgcn_perm(c1, c0, PkSel<B>::even), v = __builtin_amdgcn_perm(c1, c0, PkSel<B>::odd);
}

template <int B, bool kUyvy>
__device__ __forceinline__ uint4 yuyv_join(uint32_t y0, uint32_t y1, uint32_t u, uint32_t v)
{
    const uint32_t c0 = __builtin_amdgcn_perm(v, u, PkSel<B>::lo), c1 = __builtin_amdgcn_perm(v, u, PkSel<B>::hi);  // U V U V
    uint4 a;
    if constexpr (kUyvy) {
        a.x = __builtin_amdgcn_perm(y0, c0, PkSel<B>::lo), a.y = __builtin_amdgcn_perm(y0, c0, PkSel<B>::hi);
        a.z = __builtin_amdgcn_perm(y1, c1, PkSel<B>::lo), a.w = __builtin_amdgcn_perm(y1, c1, PkSel<B>::hi);
    } else {
        a.x = __builtin_amdgcn_perm(c0, y0, PkSel<B>::lo), a.y = __builtin_amdgcn_perm(c0, y0, PkSel<B>::hi);
        a.z = __builtin_amdgcn_perm(c1, y1, PkSel<B>::lo), a.w = __builtin_amdgcn_perm(c1, y1, PkSel<B>::hi);
    }
    return a;
}

// vec_ok: vectors i < nvec of a row are 64 packed bytes (32 / B pixels); the lanes behind them take the row's remaining pixel
// pairs.  Otherwise every lane walks pairs.  kMsb (uint16_t only): every sample read goes through (x >> ss) << ds.
template <class T, bool kUyvy, bool kPack, bool kMsb>
__global__ void __launch_bounds__(kPkLanes* kPkRows) k_yuyv(PkPlane pk, PkPlane py, PkPlane pu, PkPlane pv, int w, int row0, int rstep, int nrows,
                                                            int nframes, int vec_ok, int ss, int ds)
{
    static_assert(!kMsb || sizeof(T) == 2, "MSB-aligned samples are 16-bit words");
    [[maybe_unused]] auto conv4 = [=](uint4 a) { if constexpr (kMsb) return pk_shift(a, ss, ds); else return a; };
    [[maybe_unused]] auto conv1 = [=](T x) { if constexpr (kMsb) return (T)(((uint32_t)x >> ss) << ds); else return x; };
    constexpr int B = (int)sizeof(T);
    constexpr int ppv = 32 / B;  // pixels per vector
    constexpr int iy = kUyvy ? 1 : 0, ic = kUyvy ? 0 : 1;  // where Y0 and U stand among the four samples of a pair
    const int nvec = vec_ok ? w / ppv : 0, npairs = w / 2;
    const int i = blockIdx.x * kPkLanes + threadIdx.x;
    const int lanes = gridDim.x * kPkLanes;
    for (int f = blockIdx.z; f < nframes; f += gridDim.z) {
        for (int r = blockIdx.y * kPkRows + threadIdx.y; r < nrows; r += gridDim.y * kPkRows) {
            const int64_t y = row0 + (int64_t)rstep * r;
            uint8_t* const pp = pk.base + (int64_t)f * pk.fs + y * pk.pitch;
            uint8_t* const pyb = py.base + (int64_t)f * py.fs + y * py.pitch;
            uint8_t* const pub = pu.base + (int64_t)f * pu.fs + y * pu.pitch;
            uint8_t* const pvb = pv.base + (int64_t)f * pv.fs + y * pv.pitch;
            if (i < nvec) {
                uint4 ya, yb, u, v;
                if constexpr (!kPack) {
                    const uint4* const q = reinterpret_cast<const uint4*>(pp) + 4 * (int64_t)i;
                    const uint4 a = conv4(q[0]), b = conv4(q[1]), c = conv4(q[2]), d = conv4(q[3]);
                    yuyv_split<B, kUyvy>(a, ya.x, ya.y, u.x, v.x);
                    yuyv_split<B, kUyvy>(b, ya.z, ya.w, u.y, v.y);
                    yuyv_split<B, kUyvy>(c, yb.x, yb.y, u.z, v.z);
                    yuyv_split<B, kUyvy>(d, yb.z, yb.w, u.w, v.w);
                    reinterpret_cast<uint4*>(pyb)[2 * i] = ya;
                    reinterpret_cast<uint4*>(pyb)[2 * i + 1] = yb;
                    reinterpret_cast<uint4*>(pub)[i] = u;
                    reinterpret_cast<uint4*>(pvb)[i] = v;
                } else {
                    ya = conv4(reinterpret_cast<const uint4*>(pyb)[2 * i]), yb = conv4(reinterpret_cast<const uint4*>(pyb)[2 * i + 1]);
                    u = conv4(reinterpret_cast<const uint4*>(pub)[i]), v = conv4(reinterpret_cast<const uint4*>(pvb)[i]);
                    uint4* const q = reinterpret_cast<uint4*>(pp) + 4 * (int64_t)i;
                    q[0] = yuyv_join<B, kUyvy>(ya.x, ya.y, u.x, v.x);
                    q[1] = yuyv_join<B, kUyvy>(ya.z, ya.w, u.y, v.y);
                    q[2] = yuyv_join<B, kUyvy>(yb.x, yb.y, u.z, v.z);
                    q[3] = yuyv_join<B, kUyvy>(yb.z, yb.w, u.w, v.w);
                }
            } else {
                // the ragged tail of an aligned row, or the whole row of a launch that is not: one sample per access
                T* const q = reinterpret_cast<T*>(pp);
                T* const qy = reinterpret_cast<T*>(pyb);
                T* const qu = reinterpret_cast<T*>(pub);
                T* const qv = reinterpret_cast<T*>(pvb);
                for (int x = nvec * (ppv / 2) + (i - nvec); x < npairs; x += lanes - nvec) {
                    if constexpr (!kPack) {
                        qy[2 * x] = conv1(q[4 * x + iy]), qy[2 * x + 1] = conv1(q[4 * x + iy + 2]);
                        qu[x] = conv1(q[4 * x + ic]), qv[x] = conv1(q[4 * x + ic + 2]);
                    } else {
                        q[4 * x + iy] = conv1(qy[2 * x]), q[4 * x + iy + 2] = conv1(qy[2 * x + 1]);
                        q[4 * x + ic] = conv1(qu[x]), q[4 * x + ic + 2] = conv1(qv[x]);
                    }
                }
            }
        }
    }
}

// ---- v210 ---------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t f10(uint32_t word, int k) { return (word >> (10 * k)) & 0x3FFu; }
__device__ __forceinline__ uint32_t w10(uint32_t a, uint32_t b, uint32_t c) { return (a & 0x3FFu) | (b & 0x3FFu) << 10 | (c & 0x3FFu) << 20; }
__device__ __forceinline__ uint32_t lo16(uint32_t x) { return x & 0xFFFFu; }
__device__ __forceinline__ uint32_t hi16(uint32_t x) { return x >> 16; }

// vec_ok: groups i < ngroups of a row are 128 packed bytes (48 pixels); the lanes behind them take the row's remaining blocks,
// one each.  Otherwise every lane walks blocks.
template <bool kPack>
__global__ void __launch_bounds__(kPkLanes* kPkRows) k_v210(PkPlane pk, PkPlane py, PkPlane pu, PkPlane pv, int w, int row0, int rstep, int nrows,
                                                            int nframes, int vec_ok)
{
    const int ngroups = vec_ok ? w / 48 : 0, nblocks = (w + 5) / 6, cw = w / 2;
    const int i = blockIdx.x * kPkLanes + threadIdx.x;
    const int lanes = gridDim.x * kPkLanes;
    for (int f = blockIdx.z; f < nframes; f += gridDim.z) {
        for (int r = blockIdx.y * kPkRows + threadIdx.y; r < nrows; r += gridDim.y * kPkRows) {
            const int64_t y = row0 + (int64_t)rstep * r;
            uint8_t* const pp = pk.base + (int64_t)f * pk.fs + y * pk.pitch;
            uint8_t* const pyb = py.base + (int64_t)f * py.fs + y * py.pitch;
            uint8_t* const pub = pu.base + (int64_t)f * pu.fs + y * pu.pitch;
            uint8_t* const pvb = pv.base + (int64_t)f * pv.fs + y * pv.pitch;
            if (i < ngroups) {
                uint4* const q = reinterpret_cast<uint4*>(pp) + 8 * (int64_t)i;
                uint4* const qy = reinterpret_cast<uint4*>(pyb) + 6 * (int64_t)i;
                uint4* const qu = reinterpret_cast<uint4*>(pub) + 3 * (int64_t)i;
                uint4* const qv = reinterpret_cast<uint4*>(pvb) + 3 * (int64_t)i;
                uint32_t yd[24], ud[12], vd[12];  // the group's planes as dwords of two samples
                if constexpr (!kPack) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {  // two blocks: 12 Y, 6 U, 6 V
                        const uint4 a = q[2 * j], b = q[2 * j + 1];
                        yd[6 * j + 0] = f10(a.x, 1) | f10(a.y, 0) << 16, yd[6 * j + 1] = f10(a.y, 2) | f10(a.z, 1) << 16;
                        yd[6 * j + 2] = f10(a.w, 0) | f10(a.w, 2) << 16, yd[6 * j + 3] = f10(b.x, 1) | f10(b.y, 0) << 16;
                        yd[6 * j + 4] = f10(b.y, 2) | f10(b.z, 1) << 16, yd[6 * j + 5] = f10(b.w, 0) | f10(b.w, 2) << 16;
                        ud[3 * j + 0] = f10(a.x, 0) | f10(a.y, 1) << 16, ud[3 * j + 1] = f10(a.z, 2) | f10(b.x, 0) << 16;
                        ud[3 * j + 2] = f10(b.y, 1) | f10(b.z, 2) << 16;
                        vd[3 * j + 0] = f10(a.x, 2) | f10(a.z, 0) << 16, vd[3 * j + 1] = f10(a.w, 1) | f10(b.x, 2) << 16;
                        vd[3 * j + 2] = f10(b.z, 0) | f10(b.w, 1) << 16;
                    }
#pragma unroll
                    for (int k = 0; k < 6; ++k) qy[k] = make_uint4(yd[4 * k], yd[4 * k + 1], yd[4 * k + 2], yd[4 * k + 3]);
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        qu[k] = make_uint4(ud[4 * k], ud[4 * k + 1], ud[4 * k + 2], ud[4 * k + 3]);
                        qv[k] = make_uint4(vd[4 * k], vd[4 * k + 1], vd[4 * k + 2], vd[4 * k + 3]);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 6; ++k) {
                        const uint4 a = qy[k];
                        yd[4 * k] = a.x, yd[4 * k + 1] = a.y, yd[4 * k + 2] = a.z, yd[4 * k + 3] = a.w;
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const uint4 a = qu[k], b = qv[k];
                        ud[4 * k] = a.x, ud[4 * k + 1] = a.y, ud[4 * k + 2] = a.z, ud[4 * k + 3] = a.w;
                        vd[4 * k] = b.x, vd[4 * k + 1] = b.y, vd[4 * k + 2] = b.z, vd[4 * k + 3] = b.w;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t* const Y = yd + 6 * j;
                        const uint32_t* const U = ud + 3 * j;
                        const uint32_t* const V = vd + 3 * j;
                        uint4 a, b;
                        a.x = w10(lo16(U[0]), lo16(Y[0]), lo16(V[0])), a.y = w10(hi16(Y[0]), hi16(U[0]), lo16(Y[1]));
                        a.z = w10(hi16(V[0]), hi16(Y[1]), lo16(U[1])), a.w = w10(lo16(Y[2]), lo16(V[1]), hi16(Y[2]));
                        b.x = w10(hi16(U[1]), lo16(Y[3]), hi16(V[1])), b.y = w10(hi16(Y[3]), lo16(U[2]), lo16(Y[4]));
                        b.z = w10(lo16(V[2]), hi16(Y[4]), hi16(U[2])), b.w = w10(lo16(Y[5]), hi16(V[2]), hi16(Y[5]));
                        q[2 * j] = a, q[2 * j + 1] = b;
                    }
                }
            } else {
                // the blocks behind the last whole group, or every block of a launch that is not aligned: four 4-byte words,
                // the samples one at a time; pixels at or beyond w are left alone (unpack) or zero (pack)
                uint16_t* const qy = reinterpret_cast<uint16_t*>(pyb);
                uint16_t* const qu = reinterpret_cast<uint16_t*>(pub);
                uint16_t* const qv = reinterpret_cast<uint16_t*>(pvb);
                for (int b = ngroups * 8 + (i - ngroups); b < nblocks; b += lanes - ngroups) {
                    uint32_t* const q = reinterpret_cast<uint32_t*>(pp) + 4 * (int64_t)b;
                    const int x = 6 * b, c = 3 * b;
                    if constexpr (!kPack) {
                        const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
                        const uint32_t ys[6] = {f10(w0, 1), f10(w1, 0), f10(w1, 2), f10(w2, 1), f10(w3, 0), f10(w3, 2)};
                        const uint32_t us[3] = {f10(w0, 0), f10(w1, 1), f10(w2, 2)}, vs[3] = {f10(w0, 2), f10(w2, 0), f10(w3, 1)};
#pragma unroll
                        for (int k = 0; k < 6; ++k)
                            if (x + k < w) qy[x + k] = (uint16_t)ys[k];
#pragma unroll
                        for (int k = 0; k < 3; ++k)
                            if (c + k < cw) qu[c + k] = (uint16_t)us[k], qv[c + k] = (uint16_t)vs[k];
                    } else {
                        uint32_t ys[6], us[3], vs[3];
#pragma unroll
                        for (int k = 0; k < 6; ++k) ys[k] = x + k < w ? qy[x + k] : 0u;
#pragma unroll
                        for (int k = 0; k < 3; ++k) us[k] = c + k < cw ? qu[c + k] : 0u, vs[k] = c + k < cw ? qv[c + k] : 0u;
                        q[0] = w10(us[0], ys[0], vs[0]), q[1] = w10(ys[1], us[1], ys[2]);
                        q[2] = w10(vs[1], ys[3], us[2]), q[3] = w10(ys[4], vs[2], ys[5]);
                    }
                }
            }
        }
    }
}

static bool pk_aligned(const PkPlane& p) { return (uintptr_t)p.base % 16 == 0 && p.pitch % 16 == 0 && p.fs % 16 == 0; }

// `want` lanes along a row -- aligned: one per vector and one per unit of the tail; otherwise up to 16 waves walk a row's units
static dim3 pk_grid(int64_t want, int nrows, int nframes)
{
    const unsigned gx = (unsigned)((want + kPkLanes - 1) / kPkLanes);
    const int gy = (nrows + kPkRows - 1) / kPkRows;
    return dim3(gx < 1 ? 1 : gx, gy > 65535 ? 65535 : gy, nframes > 65535 ? 65535 : nframes);
}

template <class T, bool kUyvy, bool kMsb>
static void launch_yuyv_as(bool pack, dim3 grid, hipStream_t st, const PkPlane& pk, const PkPlane& y, const PkPlane& u, const PkPlane& v, int w, int row0,
                           int rstep, int nrows, int nframes, int vec_ok, int ss, int ds)
{
    const dim3 block(kPkLanes, kPkRows);
    if (pack) hipLaunchKernelGGL((k_yuyv<T, kUyvy, true, kMsb>), grid, block, 0, st, pk, y, u, v, w, row0, rstep, nrows, nframes, vec_ok, ss, ds);
    else hipLaunchKernelGGL((k_yuyv<T, kUyvy, false, kMsb>), grid, block, 0, st, pk, y, u, v, w, row0, rstep, nrows, nframes, vec_ok, ss, ds);
}

static hipError_t launch_packed(hipStream_t st, bool pack, int packing, int bytes, int nframes, const PkPlane& pk, const PkPlane& y, const PkPlane& u,
                                const PkPlane& v, int w, int h, int line_parity, int ss, int ds)
{
    if (nframes <= 0 || w <= 0 || h <= 0) return hipSuccess;
    if ((bytes != 1 && bytes != 2) || (w & 1) || packing < 1 || packing > 3) return hipErrorInvalidValue;
    const bool msb = ss != 0 || ds != 0;
    if (msb && (bytes != 2 || packing == 3 || ss < 0 || ss > 15 || ds < 0 || ds > 15)) return hipErrorInvalidValue;
    if (packing == 3 && bytes != 2) return hipErrorInvalidValue;
    const int row0 = line_parity < 0 ? 0 : line_parity & 1, rstep = line_parity < 0 ? 1 : 2;
    const int nrows = (h - row0 + rstep - 1) / rstep;
    if (nrows <= 0) return hipSuccess;
    const int vec_ok = pk_aligned(pk) && pk_aligned(y) && pk_aligned(u) && pk_aligned(v) ? 1 : 0;
    if (packing == 3) {
        const int nblocks = (w + 5) / 6;
        const int64_t want = vec_ok ? w / 48 + (nblocks - w / 48 * 8) : (nblocks < 16 * kPkLanes ? nblocks : 16 * kPkLanes);
        const dim3 grid = pk_grid(want, nrows, nframes), block(kPkLanes, kPkRows);
        if (pack) hipLaunchKernelGGL(k_v210<true>, grid, block, 0, st, pk, y, u, v, w, row0, rstep, nrows, nframes, vec_ok);
        else hipLaunchKernelGGL(k_v210<false>, grid, block, 0, st, pk, y, u, v, w, row0, rstep, nrows, nframes, vec_ok);
        return hipGetLastError();
    }
    const int ppv = 32 / bytes, npairs = w / 2;
    const int64_t want = vec_ok ? w / ppv + (npairs - w / ppv * (ppv / 2)) : (npairs < 16 * kPkLanes ? npairs : 16 * kPkLanes);
    const dim3 grid = pk_grid(want, nrows, nframes);
    const bool uyvy = packing == 2;
#define SN_PK(T, M)                                                                                                         \
    do {                                                                                                                    \
        if (uyvy) launch_yuyv_as<T, true, M>(pack, grid, st, pk, y, u, v, w, row0, rstep, nrows, nframes, vec_ok, ss, ds);  \
        else launch_yuyv_as<T, false, M>(pack, grid, st, pk, y, u, v, w, row0, rstep, nrows, nframes, vec_ok, ss, ds);      \
    } while (0)
    if (bytes == 1) SN_PK(uint8_t, false);
    else if (!msb) SN_PK(uint16_t, false);
    else SN_PK(uint16_t, true);
#undef SN_PK
    return hipGetLastError();
}

static PkPlane pk_plane(const PlaneView& p) { return PkPlane{const_cast<uint8_t*>(p.base), p.fs, p.pitch}; }

hipError_t launch_unpack(hipStream_t st, int packing, int bytes, int nframes, PlaneView pk, int w, int h, PlaneViewW y, PlaneViewW u, PlaneViewW v,
                         int line_parity, int ss)
{
    return launch_packed(st, false, packing, bytes, nframes, pk_plane(pk), pk_plane(y), pk_plane(u), pk_plane(v), w, h, line_parity, ss, 0);
}

hipError_t launch_pack(hipStream_t st, int packing, int bytes, int nframes, PlaneView y, PlaneView u, PlaneView v, int w, int h, PlaneViewW pk, int ds)
{
    return launch_packed(st, true, packing, bytes, nframes, pk_plane(pk), pk_plane(y), pk_plane(u), pk_plane(v), w, h, -1, 0, ds);
}

}  // namespace sn
