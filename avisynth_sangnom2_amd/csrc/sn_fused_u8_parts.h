// sn_fused_u8_parts.h -- the pieces of the 8-bit fused sweeps that do not depend on the sweep's mode: a kept line in
// packed form (two pixels per register), stage 1's operands (and the plain sweep's vertical byte pairs), the 7-tap box with the line buffer's clamps, and stage 3 in
// the byte domain.  Shared by sn_fused_u8_v3.hip (a register's halves = two column strips of one plane) and
// sn_fused_u8_uv.hip (a register's halves = the same strip of the U pass and of the V pass of a 4:2:0 frame).
// Reference semantics: /root/reference/src/SangNom2.cpp:25-34 (loadPixel), :60-65 (calculateSangNom), :74-124
// (prepareBuffers_c), :144-150 (the box of processBuffers_c), :204-249 (finalizePlane_c's ladder).
#pragma once

#include <type_traits>

#include "sn_fused_v3_common.h"

namespace sn {
namespace v3 {

using namespace v3c;

constexpr unsigned kLo = 0x0000ffffu, kHi = 0xffff0000u, kByte = 0x00ff00ffu;

// One kept line: P[i] = pixel (x0 - 3 + i) of both strips, F / B = the two SangNom values per pixel
// (calculateSangNom, SangNom2.cpp:60-65), all packed lo | hi << 16.
struct Line {
    unsigned P[PXL + 6];
    unsigned FB[PXL];  // F | B << 8 in each 16-bit half (both are 8-bit values)
    __device__ __forceinline__ unsigned F(int j) const { return FB[j] & kByte; }
    __device__ __forceinline__ unsigned B(int j) const { return pk_lshr8(FB[j]); }  // F < 256: one packed shift, no mask
    // [lo j, lo j+1, hi j, hi j+1] of F / of B: one byte permute
    __device__ __forceinline__ unsigned F2(int j) const { return __builtin_amdgcn_perm(FB[j + 1], FB[j], 0x06020400u); }
    __device__ __forceinline__ unsigned B2(int j) const { return __builtin_amdgcn_perm(FB[j + 1], FB[j], 0x07030501u); }
};
// The same with F and B in registers of their own: eight registers more per line, no extraction per use.  For the
// sweeps whose stage 3 runs in the byte domain: there a line in this form only serves stage 1, two of them are live,
// and the kernel has the registers.
struct WideLine {
    unsigned P[PXL + 6];
    unsigned Fv[PXL], Bv[PXL];
    __device__ __forceinline__ unsigned F(int j) const { return Fv[j]; }
    __device__ __forceinline__ unsigned B(int j) const { return Bv[j]; }
    __device__ __forceinline__ unsigned F2(int j) const { return Fv[j] | (Fv[j + 1] << 8); }
    __device__ __forceinline__ unsigned B2(int j) const { return Bv[j] | (Bv[j + 1] << 8); }
};

// A WideLine with the VERTICAL PAIRS that stage 1 of the plain sweep reads (round 9).  For the kept line k,
//   Z[h][i] = pixel (x0 - 3 + i) of strip h:  byte 0 = line k - 1, byte 1 = line k, bytes 2 and 3 = zero.
// The seven pixel-difference buffers (every buffer but the two SangNom ones) put
//   S[r] = O[r-1] + |c_r(x+d) - c_{r+1}(x-d)| + |c_{r+1}(x+d) - c_{r+2}(x-d)|      (d = -3 .. 3 by buffer, c_r = kept line r - 1)
// into the box, and that is ONE v_sad_u8 per strip on two such pairs with O as the accumulator: the pair (r, r+1) of
// column x + d against the pair (r+1, r+2) of column x - d -- the pairs of the row's line n and of its line nn.  The low
// strip's sum goes into bits 0..15 (v_sad_u8), the high strip's on top of it into bits 16..31 (v_sad_hi_u8); a half is
// at most 255 + 2 * 255 = 765, so nothing carries from one into the other.  Bytes 2 and 3 of every pair are zero and add
// nothing.  A row brings one new line: its pairs are the previous line's moved down a byte with the new pixel on top
// (pair_down, one v_perm_b32 per pair, 28 per row), written over the pairs of the line that has just left -- the two
// sets swap roles like the two line registers do.
// The dead-half invariant of box7 holds as before: a half that is not live loads zeros for every line, so its pairs are
// zero and both SADs add zero there; its O is zero through key_mask; so S = O + 0 + 0 stays zero in every row.
struct PairLine : WideLine {
    unsigned Z[2][PXL + 6];
};
template <class LineT>
constexpr bool kWideForm = std::is_base_of<WideLine, LineT>::value;

struct RawHalf {  // left dword, own 8 bytes, right dword of one strip
    uint32_t l, m0, m1, r;
};
struct Raw {
    RawHalf h[2];
};


// One 16-byte buffer load per strip and line: bytes [x0 - 4, x0 + 12) = left dword, own 8 bytes,
// right dword.  Row base in soffset (wave-uniform), column in voffset; dead lanes carry an
// out-of-range voffset and read zeros, so there is no branch around memory operations.
// The lane that owns column 0 loads from column 0 instead (unpack() shifts its dwords).
__device__ __forceinline__ RawHalf load_half(__amdgpu_buffer_rsrc_t rs, int voff, int soff)
{
    const u32x4 q = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0);
    return RawHalf{q.x, q.y, q.z, q.w};
}

struct LaneRole {
    bool edge_wave;      // wave holds column 0 or column w-1: clamps needed
    unsigned first_mask; // 0xffff in the half that owns column 0 (else 0)
    unsigned last_mask;  // 0xffff (shifted) in the half that owns column w-1 of the sweep
    unsigned line_last_mask;  // ... that owns the last column of the source lines (kChroma: region_w - 1)
    unsigned inside_mask;     // kChroma: halves whose columns lie inside the chroma region
    unsigned key_mask;        // 0x0ff0 in each live half, 0 in the others (operand of the and-or that forms the ladder
                              // keys; zero keeps S zero where the half is not live, see box7)
};

// byte k of the lo word -> bits 0..7, byte k of the hi word -> bits 16..23
__device__ __forceinline__ unsigned pair_byte(uint32_t hi_word, uint32_t lo_word, int k)
{
    return __builtin_amdgcn_perm(hi_word, lo_word, 0x0c040c00u + (unsigned)k * 0x00010001u);
}

// loadPixel's clamp (SangNom2.cpp:25-34) for the two image-edge lanes: afterwards l / m0 m1 / r are the four pixels
// left of the lane's eight, the eight, and the four right of them in every lane
__device__ __forceinline__ Raw clamp_edges(Raw q, const LaneRole& role)
{
    if (role.edge_wave) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (role.first_mask & (h ? kHi : kLo)) {  // loaded from column 0: dwords are one slot early
                q.h[h].r = q.h[h].m1;
                q.h[h].m1 = q.h[h].m0;
                q.h[h].m0 = q.h[h].l;
                q.h[h].l = (q.h[h].m0 & 0xff) * 0x01010101u;
            }
            if (role.line_last_mask & (h ? kHi : kLo)) q.h[h].r = (q.h[h].m1 >> 24) * 0x01010101u;
        }
    }
    return q;
}

// 32a + c with a wave-uniform c, and 4 (a + b): ONE instruction each (left to itself the compiler splits these sums into
// two-operand adds and shifts)
__device__ __forceinline__ unsigned lshl5_add_s(unsigned a, unsigned c)
{
    unsigned r;
    asm("v_lshl_add_u32 %0, %1, 5, %2" : "=v"(r) : "v"(a), "s"(c));
    return r;
}
__device__ __forceinline__ unsigned add_lshl2(unsigned a, unsigned b)
{
    unsigned r;
    asm("v_add_lshl_u32 %0, %1, %2, 2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// The SangNom value of the SSE2 arithmetic (SN_ARITH_SSE2, sn_pixel.h PxA) on packed pairs: 4a + 5b - c in clean 16-bit
// halves, a LOGICAL >> 3, an unsigned minimum against 255 -- as _mm_srli_epi16 + _mm_packus_epi16 give it
// (src/SangNom2_SSE2.cpp:446-516): a negative half is at least 0x1fe0 after the shift, so the one minimum covers it and
// the values above 255 alike.  The borrows the default form lets travel between the halves (below) would be wrong here:
// every operation is a packed 16-bit one.
__device__ __forceinline__ unsigned sg_sat(unsigned a, unsigned b, unsigned c)
{
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const u16x2 va = __builtin_bit_cast(u16x2, a), vb = __builtin_bit_cast(u16x2, b), vc = __builtin_bit_cast(u16x2, c);
    const u16x2 five = {5, 5}, lim = {255, 255};
    const u16x2 s = (u16x2)((u16x2)(va << 2) + vb * five - vc) >> 3;
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(s, lim));
}

// q: after clamp_edges().  ARITH: SN_ARITH_* (0: the reference's C++ arithmetic)
template <class LineT, int ARITH = 0>
__device__ __forceinline__ void unpack(LineT& L, const Raw& q)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        L.P[k] = pair_byte(q.h[1].l, q.h[0].l, k + 1);
        L.P[PXL + 3 + k] = pair_byte(q.h[1].r, q.h[0].r, k);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        L.P[3 + k] = pair_byte(q.h[1].m0, q.h[0].m0, k);
        L.P[7 + k] = pair_byte(q.h[1].m1, q.h[0].m1, k);
    }
    if constexpr (ARITH == 1) {  // the SSE2 arithmetic: F and B saturate (sg_sat), nothing of the form below applies
#pragma unroll
        for (int j = 0; j < PXL; ++j) {
            const unsigned f = sg_sat(L.P[j + 2], L.P[j + 3], L.P[j + 4]), b = sg_sat(L.P[j + 4], L.P[j + 3], L.P[j + 2]);
            if constexpr (kWideForm<LineT>) {
                L.Fv[j] = f;
                L.Bv[j] = b;
            } else {
                L.FB[j] = f | (b << 8);  // F | B << 8 in each half
            }
        }
        return;
    }
    // The C++ arithmetic: F = ((4a + 5b - c) >> 3) mod 256, B = ((4c + 5b - a) >> 3) mod 256 (a, b, c = P[j + 2 .. j + 4]), computed 32 times
    // over with a bias of 2048 per half: X = 32 (4 (a + b + 512) + (b - c)) for F and 32 (4 (b + c + 512) + (b - a)) for
    // B.  Neighbouring pixels share every term: with Q[i] = 32 P[i + 2] + 0x2000 per half (one v_lshl_add_u32, the bias
    // in an SGPR), T[i] = 4 (Q[i] + Q[i + 1]) (one v_add_lshl_u32: the pair sum with its bias of 4 x 0x4000) and
    // e[i] = Q[i] - Q[i + 1] (the bias cancels), F is T[j] + e[j + 1] and B is T[j + 1] - e[j] -- the pair sum of B at j
    // is that of F at j + 1, and the difference of B at j + 1 is minus that of F at j.  44 instructions per line where a
    // shift, a pair sum, a difference and a v_lshl_add per value took 51.  The
    // value then sits in bits 8..15 of each half, and one byte permute extracts it (no shift and mask).  32 (x + 2048) is
    // in [57 376, 138 976]: the low half carries at most 2 into the high half, whose own value is a multiple of 32, so its
    // bits 8..15 stay its own; differences may borrow from the high half, and the sums return it (32-bit adds are exact
    // modulo 2^32).
    unsigned Q[PXL + 2], T[PXL + 1], e[PXL + 1];
#pragma unroll
    for (int i = 0; i < PXL + 2; ++i) Q[i] = lshl5_add_s(L.P[i + 2], 0x20002000u);
#pragma unroll
    for (int i = 0; i < PXL + 1; ++i) {
        T[i] = add_lshl2(Q[i], Q[i + 1]);
        e[i] = Q[i] - Q[i + 1];
    }
#pragma unroll
    for (int j = 0; j < PXL; ++j) {
        const unsigned xf = T[j] + e[j + 1];  // 4 (a + b) + (b - c)
        const unsigned xb = T[j + 1] - e[j];  // 4 (b + c) + (b - a)
        if constexpr (kWideForm<LineT>) {
            L.Fv[j] = __builtin_amdgcn_perm(0u, xf, 0x0c030c01u);
            L.Bv[j] = __builtin_amdgcn_perm(0u, xb, 0x0c030c01u);
        } else {
            L.FB[j] = __builtin_amdgcn_perm(xb, xf, 0x07030501u);  // F | B << 8 in each half
        }
    }
}

// byte 1 of a pair moves to byte 0, byte k of the new line's dword `raw` becomes byte 1; bytes 2 and 3 stay zero
__device__ __forceinline__ unsigned pair_down(unsigned old, uint32_t raw, int k)
{
    return __builtin_amdgcn_perm(raw, old, 0x0c0c0401u + ((unsigned)k << 8));
}
// The pairs of the line in q (after clamp_edges(), so loadPixel's clamp is inherited) from those of the line above it.
// `L.Z` and `above` are different registers: the line above is still the row's n.
__device__ __forceinline__ void make_pairs(PairLine& L, const Raw& q, const unsigned (&above)[2][PXL + 6])
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            L.Z[h][k] = pair_down(above[h][k], q.h[h].l, k + 1);
            L.Z[h][PXL + 3 + k] = pair_down(above[h][PXL + 3 + k], q.h[h].r, k);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            L.Z[h][3 + k] = pair_down(above[h][3 + k], q.h[h].m0, k);
            L.Z[h][7 + k] = pair_down(above[h][7 + k], q.h[h].m1, k);
        }
    }
}
// The plane's last pool row has no line pair below it: S = O + |c_r(x+d) - c_{r+1}(x-d)| alone.  The same two SADs give it
// on pairs whose byte 1 is zero: `n` keeps its upper pixels only, `nn` (the line register that is free by then) gets n's
// lower pixels in byte 0.  Once per plane.
__device__ __forceinline__ void last_pairs(PairLine& n, PairLine& nn)
{
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < PXL + 6; ++i) {
            nn.Z[h][i] = n.Z[h][i] >> 8;
            n.Z[h][i] &= 0xffu;
        }
}
// S of a pixel-difference buffer (BUF = 0, 1, 2, 4, 6, 7, 8) at packed position j from the state O = O[r-1]: see PairLine
template <int BUF>
__device__ __forceinline__ unsigned sad_pairs_sum(const PairLine& n, const PairLine& nn, int j, unsigned o)
{
    static_assert(BUF != 3 && BUF != 5, "the SangNom buffers have no byte pairs");
    constexpr int d = BUF < 3 ? BUF - 3 : BUF == 4 ? 0 : BUF - 5;  // cost_operands: c.P[i + d] against n.P[i - d]
    const int a = j + 3 + d, b = j + 3 - d;
    return __builtin_amdgcn_sad_hi_u8(n.Z[1][a], nn.Z[1][b], __builtin_amdgcn_sad_u8(n.Z[0][a], nn.Z[0][b], o));
}

// Stage 1, buffer BUF, packed position j, pair (c, n): the two values whose difference is the cost; Buffers enum of
// SangNom2.h:8-20.
template <int BUF, class LineT>
__device__ __forceinline__ void cost_operands(const LineT& c, const LineT& n, int j, unsigned& x, unsigned& y)
{
    const int i = j + 3;
    if constexpr (BUF == 0) { x = c.P[i - 3]; y = n.P[i + 3]; }
    else if constexpr (BUF == 1) { x = c.P[i - 2]; y = n.P[i + 2]; }
    else if constexpr (BUF == 2) { x = c.P[i - 1]; y = n.P[i + 1]; }
    else if constexpr (BUF == 3) { x = c.F(j); y = n.B(j); }  // |forwardSangNom1 - forwardSangNom2|
    else if constexpr (BUF == 4) { x = c.P[i]; y = n.P[i]; }
    else if constexpr (BUF == 5) { x = c.B(j); y = n.F(j); }  // |backwardSangNom1 - backwardSangNom2|
    else if constexpr (BUF == 6) { x = c.P[i + 1]; y = n.P[i - 1]; }
    else if constexpr (BUF == 7) { x = c.P[i + 2]; y = n.P[i - 2]; }
    else { x = c.P[i + 3]; y = n.P[i - 3]; }
}
template <int BUF, class LineT>
__device__ __forceinline__ unsigned cost(const LineT& c, const LineT& n, int j)
{
    unsigned x, y;
    cost_operands<BUF>(c, n, j, x, y);
    return pk_absdiff(x, y);
}

// ---- Stage 3 in the byte domain ---------------------------------------------------------------
// The ladder's winner picks, per pixel, ONE byte of the upper line and ONE byte of the lower line (SangNom2.cpp:214-249:
// c(k) and n(-k) for k = -3 .. 3, or the two SangNom values), and the result is their rounded average.  In the packed
// pair layout that is nine tap sums and an eight-select tree per register (31 instructions per pixel pair).  On the
// lines as they lie in memory -- four pixels per dword -- it is a handful of byte permutes whose SELECTORS are data:
//   * the rank code of the winner (low nibble of the minimum key) indexes a byte table through v_perm_b32
//     (selector 0..7 -> table byte, 12 -> 0x00): sel_c = 3 + k;  the lower line's selector is 6 - sel_c;
//   * two neighbouring pixels x, x+1 find all their candidates c(x-3) .. c(x+4) in ONE 8-byte window, so a v_perm_b32
//     over that window with selectors (3 + k0, 4 + k1) fetches both; the windows of a lane's eight pixels are six
//     dwords per strip, cut with v_alignbyte_b32 once per line and kept in LDS for the two rows that use the line;
//   * the SangNom candidates are two more byte permutes (take the F / B byte where the code says so);
//   * v_lerp_u8 with 0x01010101 is (a + b + 1) >> 1 on four pixels at once.
// 18 instructions per four pixels of a strip instead of 124, and the result is already in memory order.
struct RawLine {
    unsigned W[2][6];  // per strip: [p-3..p0] [p1..p4] [p-1..p2] [p3..p6] [p5..p8] [p7..p10] (p0 = the lane's first pixel)
    unsigned F[2][2], B[2][2];  // forward / backward SangNom values of p0..p3 and p4..p7, one byte each
};
// rank codes: P4 (and the `minBuf > aaf` arm, same result) 0, P5 1, P3 2, P6 3, P2 4, P7 5, P1 6, P8 7, P0 12
constexpr unsigned kLutLo = 0x04030303u, kLutHi = 0x06010502u;  // code -> 3 + k; code 12 reads 0x00 = 3 + (-3)

template <class LineT>
__device__ __forceinline__ void make_raw(RawLine& R, const Raw& q, const LineT& L)
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const RawHalf& x = q.h[h];
        R.W[h][0] = __builtin_amdgcn_alignbyte(x.m0, x.l, 1);
        R.W[h][1] = __builtin_amdgcn_alignbyte(x.m1, x.m0, 1);
        R.W[h][2] = __builtin_amdgcn_alignbyte(x.m0, x.l, 3);
        R.W[h][3] = __builtin_amdgcn_alignbyte(x.m1, x.m0, 3);
        R.W[h][4] = __builtin_amdgcn_alignbyte(x.r, x.m1, 1);
        R.W[h][5] = __builtin_amdgcn_alignbyte(x.r, x.m1, 3);
    }
    // F[j] = [lo strip, 0, hi strip, 0]: pixels j, j+1 side by side, then the four of a strip into one dword
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const unsigned f01 = L.F2(4 * g), f23 = L.F2(4 * g + 2);  // [lo0 lo1 hi0 hi1]
        const unsigned b01 = L.B2(4 * g), b23 = L.B2(4 * g + 2);
        R.F[0][g] = __builtin_amdgcn_perm(f23, f01, 0x05040100u);
        R.F[1][g] = __builtin_amdgcn_perm(f23, f01, 0x07060302u);
        R.B[0][g] = __builtin_amdgcn_perm(b23, b01, 0x05040100u);
        R.B[1][g] = __builtin_amdgcn_perm(b23, b01, 0x07060302u);
    }
}

// four interpolated pixels of strip h, group g (pixels 4g .. 4g+3), from the rank codes of their winners
__device__ __forceinline__ unsigned interpolate4(const RawLine& c, const RawLine& n, int h, int g, unsigned codes)
{
    const unsigned sc = __builtin_amdgcn_perm(kLutHi, kLutLo, codes) + 0x01000100u;  // [3 + k0, 4 + k1, 3 + k2, 4 + k3]
    const unsigned sn = 0x08060806u - sc;                                          // [3 - k0, 4 - k1, 3 - k2, 4 - k3]
    const int a = g == 0 ? 0 : 1, b = g == 0 ? 1 : 4;  // window of pixels 0, 1 of the group: dwords W[a], W[b]
    const int d = g == 0 ? 2 : 3, e = g == 0 ? 3 : 5;  // ... of pixels 2, 3
    unsigned cc = bfi(0x0000ffffu, __builtin_amdgcn_perm(c.W[h][b], c.W[h][a], sc), __builtin_amdgcn_perm(c.W[h][e], c.W[h][d], sc));
    unsigned nn = bfi(0x0000ffffu, __builtin_amdgcn_perm(n.W[h][b], n.W[h][a], sn), __builtin_amdgcn_perm(n.W[h][e], n.W[h][d], sn));
    // P5 (code 1): avg(backwardSangNom1, backwardSangNom2) = c.B, n.F;  P3 (code 2): avg(forward1, forward2) = c.F, n.B
    const unsigned sb = __builtin_amdgcn_perm(0u, 0x00000400u, codes) + 0x03020100u;  // byte i: i, or 4 + i where the code is 1
    const unsigned sf = __builtin_amdgcn_perm(0u, 0x00040000u, codes) + 0x03020100u;  // ... where the code is 2
    cc = __builtin_amdgcn_perm(c.B[h][g], cc, sb);
    nn = __builtin_amdgcn_perm(n.F[h][g], nn, sb);
    cc = __builtin_amdgcn_perm(c.F[h][g], cc, sf);
    nn = __builtin_amdgcn_perm(n.B[h][g], nn, sf);
    return __builtin_amdgcn_lerp(cc, nn, 0x01010101u);  // (a + b + 1) >> 1 per byte, SangNom2.cpp:48-52
}

// the code of buffer BUF in the ladder keys (see RawLine): the reference's order P4, P5, P3, P6, P2, P7, P1, P8, P0
// (SangNom2.cpp:214-249) as 0, 1, 2, 3, 4, 5, 6, 7, 12 -- smaller wins a tie
template <int BUF, int MODE>
constexpr unsigned rank_of()
{
    constexpr unsigned code[9] = {12, 6, 4, 2, 0, 1, 3, 5, 7};
    return code[BUF] * 0x00010001u;
}

// The 7-tap box over S with the line buffer's clamps (SangNom2.cpp:144-150), the same instructions in every wave.
// Windows 3 and 4 hold only the lane's own pixels and share S[1..6]: with P = S1 + S2 + S3 and Q = S4 + S5 + S6 they are
// P + Q + S0 and P + Q + S7.  From there the box walks outwards, so that every neighbour tap enters exactly one
// instruction and that instruction is the DPP form of an operation the walk needs anyway -- the same form on both sides:
//   left:  Bx[j] = Bx[j+1] + (L - S[j+4]) + z      L - S[j+4] = v_sub_u32_dpp (wave_shr:1, lane 0 reads 0)
//   right: Bx[j] = Bx[j-1] + (R - S[j-4]) + m      R - S[j-4] = v_sub_u32_dpp (wave_shl:1, lane 63 reads 0)
//   * column 0 is lane 0 of the first strip, and lane 0 has no left neighbour: its tap reads 0 and z = S[0] there (the
//     clamp; z = 0 elsewhere).  Lane 0 of every other strip is the outermost ghost lane, whose value is wrong by design:
//     its tap reads 0.
//   * column w - 1 sits in some lane of the last strip, and its right-hand tap must read 0 too, so that m = S[PXL-1]
//     there (m = 0 elsewhere) adds the clamp.  It does, by an invariant of both 8-bit kernels: S is ZERO in every half
//     that is not live.  Every fused width is a multiple of 32, so w - 1 is pixel 7 of its lane, and that lane is 3 mod 4
//     in its strip (kFirst = 62, kInner = 60); the last strip has no right ghosts, so the lane after it is lane 64 (the
//     DPP reads 0) or a half that is not live.  There the lines, the previous pass's rows and the luma pass's rows all
//     load from an out-of-range voffset (zeros: every cost and every stale value is 0), and key_mask = 0 makes the key
//     the bare rank code, so O = key >> 4 = 0 and A' = O + costs = 0 in every row: S = A + costs stays 0.  (The class-S
//     waves of the one-sweep chroma kernel, which form no keys, mask O the same way.)  Before this the right walk paid
//     for the clamp in every wave: R & ~m as a v_and_b32_dpp, and m S7 - S[j-4] apart, three instructions per window.
// 18 instructions per buffer step (4 for windows 3 and 4, 1 + 6 left, 1 + 6 right); 22 before, and the box that started
// at window 0 took 29 (each left tap in two sums, a move to preset every DPP `old`).  All sums stay below 2^16 per half;
// the differences may borrow across the halves, which the later adds return (32-bit arithmetic is exact modulo 2^32).
// Round 2 branched on "this wave holds an image edge" around two whole variants of the box: the edge waves paid 29
// instructions per buffer instead of 20, the branch cut every buffer step into three scheduling regions, and the seam
// refresh made every wave wait for the slowest (knocking the edge variant out -- wrong at the edges -- ran 12 % faster).
// In the SSE2 arithmetic the window sum saturates: min(sum >> 4, 255) (src/SangNom2_SSE2.cpp:748-761).  The key is
// (Bx & 0x0ff00ff0) | rank, so a half of 4096 or more has to become 4095, whose bits 4..11 are 255: ONE v_pk_min_u16 in
// front of the v_and_or (Bx holds the true sums, below 2^16 per half: the borrows have been returned by then).  A
// minimum never turns a zero half into something else, so S stays zero in every half that is not live.  The bound holds
// in the pool-coupled sweeps too: what they take from a pool is a saturated O of the previous pass, at most 255 like a
// cost, and where a stale value enters the sum the cost beside it is zero -- S <= 3 * 255 and a window <= 5 355 per half.
template <int ARITH>
__device__ __forceinline__ unsigned box_sat(unsigned bx)
{
    if constexpr (ARITH == 1) return pk_min(bx, 0x0fff0fffu);
    return bx;
}

__device__ __forceinline__ void box7(const unsigned (&S)[PXL], unsigned (&Bx)[PXL], const LaneRole& role)
{
    const unsigned p = add3(S[1], S[2], S[3]), q = add3(S[4], S[5], S[6]);
    Bx[3] = add3(p, q, S[0]);
    Bx[4] = add3(p, q, S[PXL - 1]);
    const unsigned z = S[0] & role.first_mask;
#pragma unroll
    for (int j = 2; j >= 0; --j) Bx[j] = add3(Bx[j + 1], dpp_from_left(S[j + 5]) - S[j + 4], z);
    const unsigned m = S[PXL - 1] & role.last_mask;
#pragma unroll
    for (int j = 5; j < PXL; ++j) Bx[j] = add3(Bx[j - 1], dpp_from_right(S[j - 5]) - S[j - 4], m);
}

// A RawLine parked in LDS for the two rows that use it: five uint4 per thread and line, `nthreads` apart (each thread
// reads back exactly what it wrote, so no barrier is involved); `v` = the line's slot.
__device__ __forceinline__ void park_raw_at(uint4* v, int nthreads, int tid, const RawLine& R)
{
    uint4* to = v + tid;
    to[0 * nthreads] = make_uint4(R.W[0][0], R.W[0][1], R.W[0][2], R.W[0][3]);
    to[1 * nthreads] = make_uint4(R.W[0][4], R.W[0][5], R.W[1][0], R.W[1][1]);
    to[2 * nthreads] = make_uint4(R.W[1][2], R.W[1][3], R.W[1][4], R.W[1][5]);
    to[3 * nthreads] = make_uint4(R.F[0][0], R.F[0][1], R.B[0][0], R.B[0][1]);
    to[4 * nthreads] = make_uint4(R.F[1][0], R.F[1][1], R.B[1][0], R.B[1][1]);
}
__device__ __forceinline__ void unpark_raw_at(const uint4* v, int nthreads, int tid, RawLine& R)
{
    const uint4* from = v + tid;
    const uint4 a = from[0 * nthreads], b = from[1 * nthreads], c = from[2 * nthreads], d = from[3 * nthreads], e = from[4 * nthreads];
    R.W[0][0] = a.x; R.W[0][1] = a.y; R.W[0][2] = a.z; R.W[0][3] = a.w;
    R.W[0][4] = b.x; R.W[0][5] = b.y; R.W[1][0] = b.z; R.W[1][1] = b.w;
    R.W[1][2] = c.x; R.W[1][3] = c.y; R.W[1][4] = c.z; R.W[1][5] = c.w;
    R.F[0][0] = d.x; R.F[0][1] = d.y; R.B[0][0] = d.z; R.B[0][1] = d.w;
    R.F[1][0] = e.x; R.F[1][1] = e.y; R.B[1][0] = e.z; R.B[1][1] = e.w;
}

struct Out {
    uint32_t lo[2], hi[2];  // 8 interpolated bytes of each half's strip
};

}  // namespace v3
}  // namespace sn
