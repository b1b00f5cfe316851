// sn_pixel.h -- per-sample-type arithmetic of the SangNom2 path, device side.
//
// Semantics follow the reference's opt=0 helpers (/root/reference/src/SangNom2.cpp:25-72):
// integer narrowing wraps modulo 2^(8*sizeof T), `>>` on the SangNom sum is arithmetic, float
// code keeps the reference's operation order (the library is built with -ffp-contract=off so
// no multiply-add is fused).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sn {

template <class T>
struct Px;

template <>
struct Px<uint8_t> {
    using W = int32_t;  // working type (the reference uses int16_t; the values are identical)
    static __device__ __forceinline__ W narrow(W v) { return v & 0xFF; }
    static __device__ __forceinline__ W sg(W p1, W p2, W p3) { return ((4 * p1 + 5 * p2 - p3) >> 3) & 0xFF; }
    static __device__ __forceinline__ W adiff(W a, W b) { W d = a - b; return d < 0 ? -d : d; }
    static __device__ __forceinline__ W avg(W a, W b) { return (a + b + 1) >> 1; }
    static __device__ __forceinline__ W div16(W s) { return (s >> 4) & 0xFF; }  // s >= 0
    static __device__ __forceinline__ W sum3(W a, W b, W c) { return a + b + c; }
};

template <>
struct Px<uint16_t> {
    using W = int32_t;
    static __device__ __forceinline__ W narrow(W v) { return v & 0xFFFF; }
    static __device__ __forceinline__ W sg(W p1, W p2, W p3) { return ((4 * p1 + 5 * p2 - p3) >> 3) & 0xFFFF; }
    static __device__ __forceinline__ W adiff(W a, W b) { W d = a - b; return d < 0 ? -d : d; }
    static __device__ __forceinline__ W avg(W a, W b) { return (a + b + 1) >> 1; }
    static __device__ __forceinline__ W div16(W s) { return (s >> 4) & 0xFFFF; }
    static __device__ __forceinline__ W sum3(W a, W b, W c) { return a + b + c; }
};

template <>
struct Px<float> {
    using W = float;
    static __device__ __forceinline__ W narrow(W v) { return v; }
    static __device__ __forceinline__ W sg(W p1, W p2, W p3)
    {
        float s = (p1 * 4.0f + p2 * 5.0f) - p3;  // SangNom2.cpp:70
        return s * 0.125f;
    }
    static __device__ __forceinline__ W adiff(W a, W b) { return __builtin_fabsf(a - b); }
    static __device__ __forceinline__ W avg(W a, W b) { return (a + b) * 0.5f; }
    static __device__ __forceinline__ W div16(W s) { return s * 0.0625f; }  // == s / 16 exactly
    static __device__ __forceinline__ W sum3(W a, W b, W c) { return (a + b) + c; }
};

// The arithmetic of a context (sangnom_hip.h, SN_ARITH_*).  A = 0: the reference's C++ path, Px<T> as it is.  A = 1: its
// SSE2 path (src/SangNom2_SSE2.cpp), which differs in two narrowing steps of the integer types, both saturating to the
// container (MAXT = 255 / 65535, whatever the bit depth) where the C++ path wraps:
//   sg     the sum in a lane twice as wide, a LOGICAL >> 3, an unsigned-saturating pack (:446-516): a negative sum
//          has its top bits set after the shift, so it packs to MAXT like a value above MAXT does
//   div16  min(sum >> 4, MAXT) (:748-761); sums are never negative
// Float is the same in both paths.
template <class T, int A>
struct PxA : Px<T> {};

template <>
struct PxA<uint8_t, 1> : Px<uint8_t> {
    static __device__ __forceinline__ W sg(W p1, W p2, W p3)
    {
        const uint32_t q = (uint32_t)((4 * p1 + 5 * p2 - p3) & 0xFFFF) >> 3;  // the 16-bit lane of _mm_srli_epi16
        return (W)(q < 255u ? q : 255u);
    }
    static __device__ __forceinline__ W div16(W s) { const W q = s >> 4; return q < 255 ? q : 255; }
};

template <>
struct PxA<uint16_t, 1> : Px<uint16_t> {
    static __device__ __forceinline__ W sg(W p1, W p2, W p3)
    {
        const uint32_t q = (uint32_t)(4 * p1 + 5 * p2 - p3) >> 3;  // the 32-bit lane of _mm_srli_epi32
        return (W)(q < 65535u ? q : 65535u);
    }
    static __device__ __forceinline__ W div16(W s) { const W q = s >> 4; return q < 65535 ? q : 65535; }
};

// The same narrowing on the packed forms of the 8-bit and 16-bit stage-2 kernels.  box8: two 16-bit window sums per
// register (at most 5 355 each in the default arithmetic; in the SSE2 arithmetic a sum stays below 7 * 3 * 255 too, the
// costs being bytes); a half of 4096 or more becomes 4095, whose bits 4..11 are 255: one v_pk_min_u16 in front of the
// shift and mask.  box16: one 32-bit sum per register.
template <int A>
__device__ __forceinline__ unsigned box8(unsigned t)
{
    if constexpr (A == 1) {
        typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
        const u16x2 lim = {0x0fff, 0x0fff};
        t = __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(u16x2, t), lim));
    }
    return (t >> 4) & 0x00ff00ffu;  // (sum / 16) wraps to uint8_t, SangNom2.cpp:152
}
template <int A>
__device__ __forceinline__ unsigned box16(unsigned t)
{
    if constexpr (A == 1) {
        const unsigned q = t >> 4;
        return q < 0xffffu ? q : 0xffffu;
    }
    return (t >> 4) & 0xffffu;  // (sum / 16) wraps to uint16_t, SangNom2.cpp:152
}

}  // namespace sn
