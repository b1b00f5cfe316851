// sn_avg.h -- avg(a, b) of the both-fields call (sangnom_hip.h, "Both fields"), for device code: sn_merge.hip and the
// turn with a second source (sn_turn.hip).  Integers: (a + b + 1) >> 1 without overflow; float: (a + b) * 0.5f in that order,
// any NaN result as 0x7FC00000.  B is the sample size in bytes; a dword holds 4 / B samples.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sn {

template <int B>
__device__ __forceinline__ uint32_t avg_dword(uint32_t a, uint32_t b)
{
    if constexpr (B == 1) {
        return __builtin_amdgcn_lerp(a, b, 0x01010101u);  // per byte (a + b + 1) >> 1, the rounding the sweeps use it for
    } else if constexpr (B == 2) {
        // the ceiling of the mean is (a | b) - ((a ^ b) >> 1); the mask keeps the high half's low bit out of the low half,
        // and no half borrows: a | b >= (a ^ b) >> 1 in each
        return (a | b) - (((a ^ b) >> 1) & 0x7FFF7FFFu);
    } else {
        const float s = __uint_as_float(a) + __uint_as_float(b);
        const float r = s * 0.5f;
        return r != r ? 0x7FC00000u : __float_as_uint(r);
    }
}

// one sample, in the low bits of the word
template <int B>
__device__ __forceinline__ uint32_t avg_sample(uint32_t a, uint32_t b)
{
    if constexpr (B == 4) return avg_dword<4>(a, b);
    else return (a + b + 1u) >> 1;  // a, b < 2^16
}

}  // namespace sn
