// sn_fused_v3_common.h -- the device side shared by the fused sweep kernels (sn_fused_u8_v3.hip and sn_fused_u8_uv.hip: two
// 8-bit strips per register; sn_fused_u16_v3.hip and sn_fused_f32_v3.hip: one strip per register).  The argument block,
// the modes and the geometry of a sweep are in sn_sweep_args.h, which a host compiler takes too.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "sn_sweep_args.h"

namespace sn {
namespace v3c {

constexpr int kOutOfRange = 0x7fffffff;  // voffset that the buffer range check always rejects

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned dpp_from_left(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, true);
}
// ... where lane 0, which has no left neighbour, gets `edge` instead
__device__ __forceinline__ unsigned dpp_from_left_or(unsigned edge, unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp((int)edge, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}
__device__ __forceinline__ unsigned dpp_from_right(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x130 /* wave_shl:1 */, 0xf, 0xf, true);
}
__device__ __forceinline__ unsigned pk_max(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ unsigned pk_min(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
// Instruction selection the compiler cannot be talked into (it splits vector shifts into per-half selects, and its
// demanded-bits analysis undoes a shared and-or): spelled out.  Plain `asm` (not volatile), so they are scheduled and
// CSE'd like any other pure operation.
// bit BIT of each 16-bit half spread over that half
template <int BIT>
__device__ __forceinline__ unsigned pk_bit_mask(unsigned v)
{
    unsigned m;
    asm("v_pk_lshlrev_b16 %0, %2, %1 op_sel_hi:[0,1]\n\tv_pk_ashrrev_i16 %0, 15, %0 op_sel_hi:[0,1]" : "=v"(m) : "v"(v), "n"(15 - BIT));
    return m;
}
// (s + 1) >> 1 in both halves (s < 65535)
__device__ __forceinline__ unsigned pk_avg_from_sum(unsigned s)
{
    unsigned r;
    asm("v_pk_add_u16 %0, %1, 1 op_sel_hi:[1,0]\n\tv_pk_lshrrev_b16 %0, 1, %0 op_sel_hi:[0,1]" : "=v"(r) : "v"(s));
    return r;
}
// both halves shifted right by 4 (nothing crosses from the high half into the low one)
__device__ __forceinline__ unsigned pk_lshr4(unsigned v)
{
    const u16x2 four = {4, 4};
    return __builtin_bit_cast(unsigned, (u16x2)(__builtin_bit_cast(u16x2, v) >> four));  // v_pk_lshrrev_b16
}
// both halves shifted right by 8
__device__ __forceinline__ unsigned pk_lshr8(unsigned v)
{
    const u16x2 eight = {8, 8};
    return __builtin_bit_cast(unsigned, (u16x2)(__builtin_bit_cast(u16x2, v) >> eight));  // v_pk_lshrrev_b16
}
// max(a - b, 0) in both halves: v_pk_sub_u16 with clamp
__device__ __forceinline__ unsigned pk_sub_sat(unsigned a, unsigned b)
{
    unsigned r;
    asm("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// a + b + c as ONE instruction (left to itself the compiler forms b + c first where two such sums share it)
__device__ __forceinline__ unsigned add3(unsigned a, unsigned b, unsigned c)
{
    unsigned r;
    asm("v_add3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// (a & m) | c with a wave-uniform c (the one scalar operand the encoding allows)
__device__ __forceinline__ unsigned and_or(unsigned a, unsigned m, unsigned c)
{
    unsigned r;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(m), "s"(c));
    return r;
}
// ... with a per-lane c
__device__ __forceinline__ unsigned and_or_v(unsigned a, unsigned m, unsigned c)
{
    unsigned r;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(m), "v"(c));
    return r;
}
// min(a, b, c) of ladder keys in both halves as ONE v_pk_minimum3_f16 (same issue class as v_pk_min_u16, which has no
// three-input form).  A float minimum is the unsigned minimum of the bit patterns only because of what a key is:
//   * key < 0x1000 per half -- (sum & 0x0ff0) | rank through LaneRole::key_mask (the bare rank, < 16, in a half that is
//     not live), and the threshold key (thr + 1) << 4 with thr <= 168, at most 0x0a90.  So the sign bit and the
//     exponent's top bit are clear: a non-negative finite f16, never a NaN or Inf pattern, no -0, and non-negative f16
//     patterns order like the unsigned integers they are;
//   * keys below 0x0400 are denormal patterns: the instruction must hand them on as they are.  Every 8-bit kernel runs
//     with f16 denormals kept (csrc/Makefile: -fno-gpu-flush-denormals-to-zero, .amdhsa_float_denorm_mode_16_64 3).
// A minimum returns one of its operands bit for bit, so the rank in the low nibble comes through.
__device__ __forceinline__ unsigned pk_min3_keys(unsigned a, unsigned b, unsigned c)
{
    unsigned r;
    asm("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// One buffer's keys into the ladder's running minimum, five instructions per register and row where one per buffer took
// nine: buffers 0, 2, 4, 6 hand their key on (`held`, live for one buffer step), buffers 1, 3, 5, 7 fold it with their
// own, buffer 8 folds alone.
template <int BUF>
__device__ __forceinline__ void fold_key(unsigned& kmin, unsigned& held, unsigned key)
{
    if constexpr (BUF == kBuffers - 1) kmin = pk_min(kmin, key);
    else if constexpr (BUF % 2 == 0) held = key;
    else kmin = pk_min3_keys(kmin, held, key);
}
// |a - b| in both halves (values < 32768 per half)
__device__ __forceinline__ unsigned pk_absdiff(unsigned a, unsigned b) { return pk_max(a, b) - pk_min(a, b); }
// (m & x) | (~m & y): v_bfi_b32
__device__ __forceinline__ unsigned bfi(unsigned m, unsigned x, unsigned y) { return (m & x) | (~m & y); }

// A lane's place in a row cut into strips (sn_sweep_args.h: GH, kFirst, kInner, K): strip `wave` of `nw`, `nl` lanes of
// PXL columns in the row.  Strip 0 starts at the image edge; every inner side of a strip has GH ghost lanes that repeat
// the neighbouring strip's seam columns and, every K rows, take the seam lanes' state from a mailbox in LDS laid out
// [copy][strip][side][slot] (records of whatever a lane hands over: the index counts records).
struct StripLane {
    int wave, lane, nw;
    int gl;      // the lane among all of the row's
    bool ghost;  // repeats columns another strip owns
    bool live;   // has columns at all: dead lanes shadow column 0 and store nothing
    bool real;   // stores its columns
    int x0;      // its first column
    unsigned first_mask, last_mask;  // all ones in the lane that holds the row's first / last columns
    bool pub_right;  // feeds the next strip's left ghosts
    bool pub_left;   // ... the previous strip's right ghosts
    bool recv;       // a ghost that takes a record in
    int slot;        // which of the GH records of its side
    __device__ __forceinline__ StripLane(int wave_, int lane_, int nw_, int nl) : wave(wave_), lane(lane_), nw(nw_)
    {
        if (wave == 0) {
            gl = lane;
            ghost = nw > 1 && lane >= 64 - GH;
        } else {
            gl = kFirst + kInner * (wave - 1) + (lane - GH);
            ghost = lane < GH || (lane >= 64 - GH && wave < nw - 1);
        }
        live = gl < nl;
        real = live && !ghost;
        x0 = live ? gl * PXL : 0;
        first_mask = live && gl == 0 ? 0xffffffffu : 0u;
        last_mask = live && gl == nl - 1 ? 0xffffffffu : 0u;
        pub_right = lane >= 64 - 2 * GH && lane < 64 - GH && wave < nw - 1;
        pub_left = lane >= GH && lane < 2 * GH && wave > 0;
        recv = ghost && live;
        slot = lane < GH ? lane : lane >= 64 - GH ? lane - (64 - GH) : pub_right ? lane - (64 - 2 * GH) : lane - GH;
    }
    __device__ __forceinline__ int mailbox(int copy, int w, int side, int s) const { return ((copy * nw + w) * 2 + side) * GH + s; }
    __device__ __forceinline__ int recv_from(int copy) const { return mailbox(copy, wave, lane < GH ? 0 : 1, slot); }  // recv lanes
    __device__ __forceinline__ int publish_to(int copy) const  // pub_right / pub_left lanes
    {
        return pub_right ? mailbox(copy, wave + 1, 0, slot) : mailbox(copy, wave - 1, 1, slot);
    }
};

// Two workgroups share every SIMD (one wave each), and the issue arbiter serves equal priorities oldest first:
// left alone, the wave dispatched first runs at nearly its solo speed and the other one on the leftovers, so the
// first finishes a 2160p sweep after 3.6 ms and the second only after 5.7 ms -- the last 2.1 ms with one wave per
// SIMD (measured with per-wave timestamps; MI355X_MICROARCH.md, "Two waves per SIMD", item 2).  Taking turns at
// s_setprio 1 in slices of the free-running 100 MHz clock, the wave in the odd hardware slot during odd slices
// and vice versa, makes both advance at the same average rate and finish together.  Slices of about a quarter
// of a sweep measured best (short ones cost throughput); the slice length comes from the host.
struct TurnTaking {
    unsigned slot_parity;
    int shift;  // > 0: time slices of 2^shift ticks of the 100 MHz clock; kLadder: by rows since the last seam barrier; 0: off
    static constexpr int kLadder = kTurnLadder;
    __device__ __forceinline__ void init(int turn_shift)
    {
        slot_parity = __builtin_amdgcn_s_getreg((3 << 11) | 4) & 1u;  // HW_REG_HW_ID, wave_id bit 0
        shift = turn_shift;
    }
    // once per row: a few scalar instructions.  `block_row`: rows this wave has done since the last seam barrier (0 .. K - 1).
    __device__ __forceinline__ void update(int block_row) const
    {
        if (shift == 0) return;
        if (shift == kLadder) {
            // Workgroups of eight waves: the two waves a SIMD holds belong to the SAME workgroup and meet at its seam barrier.
            // The priority FALLS with the rows done since that barrier -- 3, 3, 2, 1, 0 -- so whichever of the two is behind
            // has the higher one and they reach the next barrier together.  No communication: the barrier itself is the
            // common clock (see turn_shift_for).
            switch (block_row) {
            case 0:
            case 1: __builtin_amdgcn_s_setprio(3); break;
            case 2: __builtin_amdgcn_s_setprio(2); break;
            case 3: __builtin_amdgcn_s_setprio(1); break;
            default: __builtin_amdgcn_s_setprio(0); break;
            }
            return;
        }
        const unsigned turn = (unsigned)(__builtin_amdgcn_s_memrealtime() >> shift) & 1u;
        if (turn != slot_parity) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
    }
};

// 16-byte buffer store with the whole offset in voffset and soffset = 0.  With an SGPR soffset hipcc pads no wait
// state after a >8-byte store, and gfx950 was seen still reading the last data register while the next VALU
// instruction overwrote it (stale words in the spilled rows of 3840-wide 16-bit sweeps); in this form the
// compiler's hazard recogniser adds the s_nop itself where one is needed.  `voff` may be kOutOfRange: adding
// an offset below 2^31 keeps it out of range.
__device__ __forceinline__ void store_b128(const u32x4& d, __amdgpu_buffer_rsrc_t r, int voff, int off)
{
    __builtin_amdgcn_raw_buffer_store_b128(d, r, (int)((unsigned)voff + (unsigned)off), 0, 0);
}

}  // namespace v3c

// sn_fused_u8_v3.hip compiled with -DSN_TU_PLAIN: the 8-bit sweeps of planes on their own (mode kPlain / kPadded)
hipError_t launch_fused_u8_v3_plain(hipStream_t st, const v3c::Sweep& s);

}  // namespace sn
