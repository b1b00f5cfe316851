// sn_pool_dispatch.h -- which stage-2 kernel a pool of the pool path gets (sn_pool_kernels.hip), as a pure rule over
// bytes per sample, the pool's row stride, its rows and the frames of the launch; and which pools the chain of a
// history-carrying stream takes, over how many workgroups per buffer.  No device code: a host compiler takes this header as
// it is (tests/c/pool_dispatch_check.cpp walks the rules against boundaries written out by hand, and answers queries for
// tests/test_pool_geometry_cpu.py, which holds the restatement of tests/pool_geometry_cases.py against them).
#pragma once

#include <stddef.h>

#include "sn_sweep_args.h"

namespace sn {

constexpr int kSmoothThreads = 1024;  // the launch bound of every stage-2 kernel of a plane

// The schedules of stage 2.  A lane of the x8 and strips kernels owns eight columns of a pool row.
//   kStrided  one column per thread, a barrier per row: pools narrower than 256 columns (k_smooth_strided)
//   kX8       a barrier per row, the neighbours' three-row sums through a double-buffered LDS line
//   kStrips   one wave per strip of the row as in the fused sweeps: DPP inside a wave, ghost lanes refreshed from an LDS
//             mailbox every v3c::K rows
enum class PoolSchedule { kNone, kStrided, kX8, kStrips, kRefused };

struct PoolStage2 {
    PoolSchedule schedule;  // kNone: the pool has no row to smooth.  kRefused: wider than any kernel (create_impl refuses it first)
    int threads;            // of the workgroup
    size_t lds;             // dynamic LDS bytes
    bool lds_attr;          // more than the 48 KiB a kernel gets unasked: hipFuncAttributeMaxDynamicSharedMemorySize first
};

inline PoolStage2 pool_stage2_for(int bytes, int stride_e, int bh, int frames)
{
    if (bh <= 1) return {PoolSchedule::kNone, 0, 0, false};
    const int nl = stride_e / 8;                       // lanes that own columns
    const size_t lane_bytes = bytes == 1 ? 16 : 32;    // a lane's eight sums: 8-bit pools pack two columns per register
    // float, launches of more than eight frames: bound by HBM, where the ghost lanes' second fetch of the seam columns
    // costs more than the barriers saved (sixteen 2160p frames: 6.3 k frames/s with k_smooth_f32x8, 5.9 k in strips)
    const bool strips_pay = bytes != 4 || frames <= 8;
    if (stride_e >= 512 && v3c::strips_for(nl) <= kSmoothThreads / 64 && strips_pay) {
        const int nw = v3c::strips_for(nl);
        // mailbox: [copy][wave][side][ghost lane][a lane's sums]
        return {PoolSchedule::kStrips, nw * 64, (size_t)2 * nw * 2 * v3c::GH * lane_bytes, false};
    }
    if (stride_e >= 256 && stride_e <= 8 * kSmoothThreads) {
        const size_t lds = (size_t)2 * nl * lane_bytes;  // two lines of every lane's sums
        return {PoolSchedule::kX8, (nl + 63) / 64 * 64, lds, lds > 48 * 1024};
    }
    if (stride_e < 256) return {PoolSchedule::kStrided, kSmoothThreads, (size_t)2 * stride_e * 4, false};  // two lines of 32-bit sums
    return {PoolSchedule::kRefused, 0, 0, false};
}

// ---- the chain of a history-carrying stream (k_smooth_{u8,u16,f32}_chain): which pools it takes, over how many workgroups ----
// The workgroup of the 8-bit chain's two-pass body; kChainMaxGroups, the most workgroups per buffer, is sn_internal.h's.
#ifndef SN_CHAIN8_THREADS
#define SN_CHAIN8_THREADS 1024  // sixteen waves, four per SIMD: the two-pass body fits 128 registers (512 threads measured slower)
#endif
constexpr int kChain8Threads = SN_CHAIN8_THREADS;

// passes one workgroup keeps in flight; 0: no chain for this pool
inline int pool_chain_lanes(int bytes, int stride_e)
{
    if (stride_e < 64) return 0;
    const int nw = v3c::strips_for(stride_e / 8);
    if (bytes == 1) return nw <= kChain8Threads / 64 ? 2 * (kChain8Threads / 64 / nw) : 0;  // two passes per set of nw waves (k_smooth_u8_chain)
    return nw <= kSmoothThreads / 128 ? kSmoothThreads / 64 / nw : 0;                     // at least two passes in flight
}

// Workgroups per buffer a chain can be spread over (`want` or fewer).  8-bit: each gets 1 / groups of the sixteen waves
// and needs at least one pair of passes (nw waves).  16-bit and float (one pass per wave): thirty-two waves in all, sixteen
// per workgroup at most, and a workgroup needs a pass (nw waves).
inline int chain_waves(int bytes, int groups)
{
    const int all = bytes == 1 ? kChain8Threads / 64 : 2 * (kSmoothThreads / 64);
    const int w = all / groups;
    return w > kSmoothThreads / 64 ? kSmoothThreads / 64 : w;
}
// workgroups per buffer the chain kernel can run for `want`
inline int pool_chain_groups(int bytes, int stride_e, int want)
{
    if (want <= 1) return 1;
    const int nw = v3c::strips_for(stride_e / 8);
    int g = 1;
    while (g * 2 <= want && g * 2 <= kChainMaxGroups && chain_waves(bytes, g * 2) >= nw) g *= 2;
    return g;
}

}  // namespace sn
