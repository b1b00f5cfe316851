// pool_dispatch_check.cpp -- sn::pool_stage2_for (csrc/sn_pool_dispatch.h) on a host compiler, no GPU: which stage-2 kernel a
// pool of the pool path gets, its workgroup and its dynamic LDS, for every pool stride a context can have (create_impl
// refuses strides above 8192) against boundaries written out by hand, and against the if-ladder the launcher had before the
// rule was a function of its own -- restated below -- which also shows that the ladder's last branch, the kernels with NC
// consecutive columns per thread (k_smooth<T, NC, A>, NC = 2, 4, 8), was never taken.
//
// The chain's rules of the same header -- pool_chain_lanes, chain_waves, pool_chain_groups -- against values written out by hand
// on both sides of every boundary they have.
//
// `pool_dispatch_check query` reads lines of "bytes stride bh frames want" from stdin and prints, per line,
// "schedule threads lds lds_attr lanes groups waves": pool_stage2_for(bytes, stride, bh, frames), pool_chain_lanes(bytes, stride),
// pool_chain_groups(bytes, stride, want) and chain_waves(bytes, that answer) -- tests/test_pool_geometry_cpu.py holds the
// restatement of tests/pool_geometry_cases.py against it.
#include <stdio.h>
#include <string.h>

#include "sn_pool_dispatch.h"

using namespace sn;

static int failures = 0;
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond)) {                                                                                       \
            if (failures < 20) printf("%s:%d: %s (bytes %d stride %d bh %d frames %d)\n", __FILE__, __LINE__, #cond, bytes, se, bh, frames); \
            ++failures;                                                                                      \
        }                                                                                                    \
    } while (0)

// strips of a row of nl lanes by hand: one strip up to 64 lanes, else 62 real lanes in the first and 60 in every later one
static int strips_by_hand(int nl)
{
    if (nl <= 64) return 1;
    int n = 1, covered = 62;
    while (covered < nl) {
        covered += 60;
        ++n;
    }
    return n;
}

// The launcher's ladder as it stood (launch_pool_plane_t, eight branches), kernel by kernel.  nc > 0: k_smooth<T, nc, A>.
struct Old {
    PoolSchedule schedule;
    int threads;
    size_t lds;
    bool attr;
    int nc;
};
static Old old_ladder(int bytes, int stride_e, int bh, int nframes)
{
    const int kThreads = 1024, GH = 2;
    const bool u8 = bytes == 1, u16 = bytes == 2, f32 = bytes == 4;
    if (u8 && bh > 1 && stride_e >= 512 && strips_by_hand(stride_e / 8) <= kThreads / 64) {
        const int nw = strips_by_hand(stride_e / 8);
        return {PoolSchedule::kStrips, nw * 64, (size_t)2 * nw * 2 * GH * 4 * 4, false, 0};
    } else if (u8 && bh > 1 && stride_e >= 256 && stride_e <= 8 * kThreads) {
        return {PoolSchedule::kX8, ((stride_e / 8) + 63) / 64 * 64, (size_t)2 * (stride_e / 8) * 16, false, 0};
    } else if (u16 && bh > 1 && stride_e >= 512 && strips_by_hand(stride_e / 8) <= kThreads / 64) {
        const int nw = strips_by_hand(stride_e / 8);
        return {PoolSchedule::kStrips, nw * 64, (size_t)2 * nw * 2 * GH * 8 * 4, false, 0};
    } else if (u16 && bh > 1 && stride_e >= 256 && stride_e <= 8 * kThreads) {
        const size_t lds = (size_t)2 * 2 * (stride_e / 8) * 16;
        return {PoolSchedule::kX8, ((stride_e / 8) + 63) / 64 * 64, lds, lds > 48 * 1024, 0};
    } else if (f32 && bh > 1 && stride_e >= 512 && strips_by_hand(stride_e / 8) <= kThreads / 64 && nframes <= 8) {
        const int nw = strips_by_hand(stride_e / 8);
        return {PoolSchedule::kStrips, nw * 64, (size_t)2 * nw * 2 * GH * 8 * 4, false, 0};
    } else if (f32 && bh > 1 && stride_e >= 256 && stride_e <= 8 * kThreads) {
        const size_t lds = (size_t)2 * 2 * (stride_e / 8) * 16;
        return {PoolSchedule::kX8, ((stride_e / 8) + 63) / 64 * 64, lds, lds > 48 * 1024, 0};
    } else if (bh > 1) {
        int nc = (stride_e + kThreads - 1) / kThreads;
        nc = nc <= 1 ? 1 : nc <= 2 ? 2 : nc <= 4 ? 4 : 8;
        if (nc < 4 && stride_e >= 1024) nc = 4;
        const size_t lds = (size_t)2 * stride_e * 4;
        if (nc <= 1) return {PoolSchedule::kStrided, kThreads, lds, false, 0};
        return {PoolSchedule::kX8, ((stride_e / nc) + 63) / 64 * 64, lds, lds > 48 * 1024, nc};
    }
    return {PoolSchedule::kNone, 0, 0, false, 0};
}

static int query()
{
    static const char* const names[] = {"none", "strided", "x8", "strips", "refused"};
    int bytes, se, bh, frames, want;
    while (scanf("%d %d %d %d %d", &bytes, &se, &bh, &frames, &want) == 5) {
        const PoolStage2 r = pool_stage2_for(bytes, se, bh, frames);
        const int g = pool_chain_groups(bytes, se, want);
        printf("%s %d %zu %d %d %d %d\n", names[(int)r.schedule], r.threads, r.lds, (int)r.lds_attr, pool_chain_lanes(bytes, se), g, chain_waves(bytes, g));
    }
    return 0;
}

// the chain's rules, by hand
static void chain_rules()
{
    int bytes = 0, se = 0, bh = 0, frames = 0;
    static_assert(kChain8Threads == 1024 && kSmoothThreads == 1024 && kChainMaxGroups == 8, "the values below are written for these");
    // pool_chain_lanes.  Below 64 columns no chain, whatever the type
    for (int b : {1, 2, 4}) {
        bytes = b;
        se = 32;
        CHECK(pool_chain_lanes(b, 32) == 0);
    }
    // 8-bit: sixteen waves in sets of nw, two passes a set.  64 and 512 columns: one strip, 32 passes; 544: two strips, 16
    CHECK(pool_chain_lanes(1, 64) == 32 && pool_chain_lanes(1, 512) == 32 && pool_chain_lanes(1, 544) == 16 && pool_chain_lanes(1, 960) == 16);
    CHECK(pool_chain_lanes(1, 992) == 10 && pool_chain_lanes(1, 1472) == 8 && pool_chain_lanes(1, 1952) == 6);   // 3, 4, 5 strips: 5, 4, 3 sets
    CHECK(pool_chain_lanes(1, 2432) == 4 && pool_chain_lanes(1, 2912) == 4 && pool_chain_lanes(1, 3840) == 4);     // 6, 7, 8 strips: two sets
    CHECK(pool_chain_lanes(1, 3872) == 2 && pool_chain_lanes(1, 7232) == 2 && pool_chain_lanes(1, 7680) == 2);     // 9 .. 16 strips: one set
    CHECK(pool_chain_lanes(1, 7712) == 0 && pool_chain_lanes(1, 8192) == 0);                                       // seventeen strips: none
    // 16-bit and float: sixteen waves, one pass each, at least two passes: up to eight strips
    for (int b : {2, 4}) {
        bytes = b;
        CHECK(pool_chain_lanes(b, 64) == 16 && pool_chain_lanes(b, 512) == 16 && pool_chain_lanes(b, 544) == 8 && pool_chain_lanes(b, 992) == 5);
        CHECK(pool_chain_lanes(b, 1472) == 4 && pool_chain_lanes(b, 1952) == 3 && pool_chain_lanes(b, 2400) == 3 && pool_chain_lanes(b, 2432) == 2);
        CHECK(pool_chain_lanes(b, 3392) == 2 && pool_chain_lanes(b, 3840) == 2 && pool_chain_lanes(b, 3872) == 0 && pool_chain_lanes(b, 8192) == 0);
    }
    // chain_waves: 8-bit sixteen waves shared out; the others thirty-two, sixteen a workgroup at most
    bytes = 1;
    CHECK(chain_waves(1, 1) == 16 && chain_waves(1, 2) == 8 && chain_waves(1, 4) == 4 && chain_waves(1, 8) == 2);
    for (int b : {2, 4}) {
        bytes = b;
        CHECK(chain_waves(b, 1) == 16 && chain_waves(b, 2) == 16 && chain_waves(b, 4) == 8 && chain_waves(b, 8) == 4);
    }
    // pool_chain_groups: the largest power of two <= want, <= 8, whose workgroups still hold a set of nw waves
    for (int b : {1, 2, 4}) {
        bytes = b;
        for (int want : {-1, 0, 1}) CHECK(pool_chain_groups(b, 512, want) == 1);
        CHECK(pool_chain_groups(b, 512, 2) == 2 && pool_chain_groups(b, 512, 3) == 2 && pool_chain_groups(b, 512, 4) == 4);
        CHECK(pool_chain_groups(b, 512, 7) == 4 && pool_chain_groups(b, 512, 8) == 8 && pool_chain_groups(b, 512, 9) == 8 && pool_chain_groups(b, 512, 64) == 8);
    }
    bytes = 1;  // 8-bit: 2 strips -> 8 (two waves each), 3 and 4 strips -> 4, 5 .. 8 strips -> 2, 9 and more -> 1
    CHECK(pool_chain_groups(1, 544, 8) == 8 && pool_chain_groups(1, 960, 8) == 8 && pool_chain_groups(1, 992, 8) == 4 && pool_chain_groups(1, 1920, 8) == 4);
    CHECK(pool_chain_groups(1, 1952, 8) == 2 && pool_chain_groups(1, 3840, 8) == 2 && pool_chain_groups(1, 3872, 8) == 1 && pool_chain_groups(1, 7680, 8) == 1);
    CHECK(pool_chain_groups(1, 992, 2) == 2 && pool_chain_groups(1, 1952, 4) == 2 && pool_chain_groups(1, 3872, 2) == 1);
    for (int b : {2, 4}) {  // 16-bit and float: up to 4 strips -> 8 (four waves each), 5 .. 8 strips -> 4
        bytes = b;
        CHECK(pool_chain_groups(b, 544, 8) == 8 && pool_chain_groups(b, 1472, 8) == 8 && pool_chain_groups(b, 1920, 8) == 8);
        CHECK(pool_chain_groups(b, 1952, 8) == 4 && pool_chain_groups(b, 3840, 8) == 4 && pool_chain_groups(b, 3840, 2) == 2);
    }
}

int main(int argc, char** argv)
{
    if (argc > 1 && strcmp(argv[1], "query") == 0) return query();
    chain_rules();
    int reached[5][3] = {};  // [schedule][sample type]
    for (int bytes : {1, 2, 4}) {
        const int ti = bytes == 1 ? 0 : bytes == 2 ? 1 : 2;
        const size_t lane_bytes = bytes == 1 ? 16 : 32;  // eight columns: four registers of two 16-bit sums, or eight of one 32-bit sum
        for (int se = 32; se <= 8192; se += 32) {
            for (int bh : {1, 2, 16}) {
                for (int frames : {1, 8, 9}) {
                    const PoolStage2 r = pool_stage2_for(bytes, se, bh, frames);
                    const Old o = old_ladder(bytes, se, bh, frames);
                    // the ladder never reached its last branch's k_smooth<T, NC, A>, and the rule is the ladder
                    CHECK(o.nc == 0);
                    CHECK(r.schedule == o.schedule && r.threads == o.threads && r.lds == o.lds && r.lds_attr == o.attr);
                    CHECK(r.threads <= 1024);
                    reached[(int)r.schedule][ti]++;
                    const int nl = se / 8;
                    if (bh <= 1) {  // no row between the first and the last: no stage 2
                        CHECK(r.schedule == PoolSchedule::kNone && r.threads == 0 && r.lds == 0 && !r.lds_attr);
                    } else if (se < 256) {  // one column per thread, two lines of 32-bit sums
                        CHECK(r.schedule == PoolSchedule::kStrided && r.threads == 1024 && r.lds == (size_t)se * 8 && !r.lds_attr);
                    } else if (se >= 512 && se <= 7680 && !(bytes == 4 && frames > 8)) {
                        // 7680 columns: 960 lanes = 62 + 14 x 60 + 58, sixteen strips; 7712: 964 lanes, seventeen
                        const int nw = strips_by_hand(nl);
                        CHECK(nw >= 1 && nw <= 16);
                        CHECK(r.schedule == PoolSchedule::kStrips && r.threads == 64 * nw && !r.lds_attr);
                        CHECK(r.lds == (size_t)2 /* copies */ * nw * 2 /* sides */ * 2 /* ghost lanes */ * lane_bytes);
                    } else {  // 256-480, 7712-8192, and float launches of more than eight frames
                        CHECK(r.schedule == PoolSchedule::kX8 && r.threads == (nl + 63) / 64 * 64);
                        CHECK(r.lds == (size_t)2 /* lines */ * nl * lane_bytes);
                        CHECK(r.lds_attr == (r.lds > 48 * 1024));
                    }
                }
            }
        }
    }
    {
        int bytes = 0, se = 0, bh = 0, frames = 0;
        // spot values by hand
        PoolStage2 r = pool_stage2_for(1, 512, 16, 1);  // 64 lanes: one strip, one wave, 2 x 1 x 2 x 2 x 16 bytes
        CHECK(r.schedule == PoolSchedule::kStrips && r.threads == 64 && r.lds == 128);
        r = pool_stage2_for(2, 544, 16, 1);  // 68 lanes: two strips
        CHECK(r.schedule == PoolSchedule::kStrips && r.threads == 128 && r.lds == 512);
        r = pool_stage2_for(4, 7680, 2, 8);
        CHECK(r.schedule == PoolSchedule::kStrips && r.threads == 1024 && r.lds == 4096);
        r = pool_stage2_for(4, 7680, 2, 9);  // 960 lanes x 32 bytes x 2 lines = 61 440: above 48 KiB
        CHECK(r.schedule == PoolSchedule::kX8 && r.threads == 960 && r.lds == 61440 && r.lds_attr);
        r = pool_stage2_for(2, 8192, 2, 1);  // 64 KiB
        CHECK(r.schedule == PoolSchedule::kX8 && r.threads == 1024 && r.lds == 65536 && r.lds_attr);
        r = pool_stage2_for(1, 8192, 2, 1);  // 8-bit: 32 KiB, no attribute
        CHECK(r.schedule == PoolSchedule::kX8 && r.threads == 1024 && r.lds == 32768 && !r.lds_attr);
        r = pool_stage2_for(2, 6144, 2, 1);  // 768 lanes = 62 + 11 x 60 + 46: thirteen strips
        CHECK(r.schedule == PoolSchedule::kStrips && r.threads == 13 * 64);
        r = pool_stage2_for(1, 480, 2, 9);
        CHECK(r.schedule == PoolSchedule::kX8 && r.threads == 64 && r.lds == 1920 && !r.lds_attr);
        r = pool_stage2_for(4, 224, 2, 9);
        CHECK(r.schedule == PoolSchedule::kStrided && r.threads == 1024 && r.lds == 1792);
        r = pool_stage2_for(4, 8224, 2, 1);  // wider than any kernel (and than any context)
        CHECK(r.schedule == PoolSchedule::kRefused);
        // every schedule is reached by every sample type
        for (int s = 0; s < 4; ++s)
            for (int t = 0; t < 3; ++t) CHECK(reached[s][t] > 0);
        for (int t = 0; t < 3; ++t) CHECK(reached[(int)PoolSchedule::kRefused][t] == 0);
    }
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
