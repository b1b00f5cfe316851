// route_check.cpp -- csrc/sn_route.h: the clip's plan and the decision of a launch against values written out by hand, at each
// boundary of the rules and on both sides of it; the pause after failed frames; prefer_pool against the answers of the function
// it replaced.  Stand-alone host program (no device code, no GPU): without arguments it prints "ok" or what differs.
// With arguments it answers queries, kQuery integers each, one line per query (tests/test_small_planes_cpu.py):
//   bytes bits planes sub_w sub_h width height dh luma chroma mode isolated fresh arith column_parts sse2_sweeps
//   n slot0 slots parts_slots seam_record sweeps_always band_force band_warm parts_force ghost_force chroma_sweeps chain_lanes
//   bands_paused parts_paused
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "sn_route.h"

static int failures = 0;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            ++failures;                                                  \
        }                                                                \
    } while (0)

using namespace sn;

static sn_config clip(int bytes, int planes, int sub_w, int sub_h, int w, int h, int mode = SN_MODE_AUTO)
{
    sn_config c{};
    c.struct_size = (int32_t)sizeof c;
    c.width = w;
    c.height = h;
    c.bytes_per_sample = bytes;
    c.bits_per_sample = 8 * bytes;
    c.num_planes = planes;
    c.sub_w = sub_w;
    c.sub_h = sub_h;
    c.order = 1;
    c.aa = 48;
    c.aac = 48;
    c.luma = c.chroma = 1;
    c.max_batch = 1;
    c.mode = mode;
    return c;
}

static ClipPlan plan_of(const sn_config& c, int arith = SN_ARITH_CXX, bool parts = false, int sse2_sweeps = 0)
{
    sn_policy pol{};
    pol.sse2_sweeps = sse2_sweeps;
    return clip_plan(c, arith, parts, pol);
}

static LaunchInput launch(int n, int slots)
{
    LaunchInput in;
    in.n = n;
    in.slots = slots;
    return in;
}

static void refused(const ClipPlan& p, const char* text)
{
    if (p.refusal != SN_ERR_UNSUPPORTED || p.refusal_text != text) {
        std::printf("refusal: got %d '%s'\n         want %d '%s'\n", p.refusal, p.refusal_text.c_str(), SN_ERR_UNSUPPORTED, text);
        ++failures;
    }
}

// ---- creation ---------------------------------------------------------------------------------------------------------------
static void check_refusals()
{
    // width: the pool stride, not the width, is what is bounded
    CHECK(plan_of(clip(1, 1, 0, 0, 8192, 4)).refusal == SN_OK);
    CHECK(plan_of(clip(1, 1, 0, 0, 8192, 4)).stride_e == 8192);
    refused(plan_of(clip(1, 1, 0, 0, 8224, 4)), "width 8224 exceeds the supported maximum of 8192");
    refused(plan_of(clip(1, 1, 0, 0, 8193, 4)), "width 8193 exceeds the supported maximum of 8192");
    // height: out_height / 2 <= 65535
    CHECK(plan_of(clip(1, 1, 0, 0, 64, 131070)).refusal == SN_OK);
    refused(plan_of(clip(1, 1, 0, 0, 64, 131072)), "height 131072 exceeds the supported maximum");
    sn_config dh = clip(1, 1, 0, 0, 64, 65536);
    dh.dh = 1;
    refused(plan_of(dh), "height 65536 exceeds the supported maximum");
    // SN_ARITH_SSE2: two vectors, 32 / 16 / 8 samples, every processed plane
    CHECK(plan_of(clip(1, 1, 0, 0, 32, 4), SN_ARITH_SSE2).refusal == SN_OK);
    refused(plan_of(clip(1, 1, 0, 0, 31, 4), SN_ARITH_SSE2),
            "SN_ARITH_SSE2: plane 0 is 31 samples wide; the reference's SSE2 path is defined from 32 samples (two vectors) on");
    CHECK(plan_of(clip(2, 1, 0, 0, 16, 4), SN_ARITH_SSE2).refusal == SN_OK);
    refused(plan_of(clip(2, 1, 0, 0, 15, 4), SN_ARITH_SSE2),
            "SN_ARITH_SSE2: plane 0 is 15 samples wide; the reference's SSE2 path is defined from 16 samples (two vectors) on");
    CHECK(plan_of(clip(4, 1, 0, 0, 8, 4), SN_ARITH_SSE2).refusal == SN_OK);
    refused(plan_of(clip(4, 1, 0, 0, 7, 4), SN_ARITH_SSE2),
            "SN_ARITH_SSE2: plane 0 is 7 samples wide; the reference's SSE2 path is defined from 8 samples (two vectors) on");
    CHECK(plan_of(clip(1, 3, 1, 1, 64, 4), SN_ARITH_SSE2).refusal == SN_OK);  // chroma 32 wide
    refused(plan_of(clip(1, 3, 1, 1, 62, 4), SN_ARITH_SSE2),
            "SN_ARITH_SSE2: plane 1 is 31 samples wide; the reference's SSE2 path is defined from 32 samples (two vectors) on");
    sn_config copied = clip(1, 3, 1, 1, 62, 4);
    copied.chroma = 0;  // a plane that is only copied may be as narrow as it likes
    CHECK(plan_of(copied, SN_ARITH_SSE2).refusal == SN_OK);
    // SN_MODE_FUSED in SN_ARITH_SSE2 without sse2_sweeps: 8-bit planes on their own only
    CHECK(plan_of(clip(1, 1, 0, 0, 256, 4, SN_MODE_FUSED), SN_ARITH_SSE2).refusal == SN_OK);
    refused(plan_of(clip(2, 1, 0, 0, 256, 4, SN_MODE_FUSED), SN_ARITH_SSE2),
            "SN_MODE_FUSED requested but in SN_ARITH_SSE2 only 8-bit planes on their own have fused sweeps; this clip (9..16-bit samples) runs on the "
            "pool path in that mode");
    refused(plan_of(clip(1, 3, 1, 1, 256, 4, SN_MODE_FUSED), SN_ARITH_SSE2),
            "SN_MODE_FUSED requested but in SN_ARITH_SSE2 only 8-bit planes on their own have fused sweeps; this clip (subsampled chroma sharing the luma "
            "pool) runs on the pool path in that mode");
    CHECK(plan_of(clip(2, 1, 0, 0, 256, 4, SN_MODE_FUSED), SN_ARITH_SSE2, false, 1).refusal == SN_OK);
    CHECK(plan_of(clip(1, 3, 1, 1, 256, 4, SN_MODE_FUSED), SN_ARITH_SSE2, false, 1).refusal == SN_OK);
    CHECK(plan_of(clip(4, 1, 0, 0, 256, 4, SN_MODE_FUSED), SN_ARITH_SSE2).refusal == SN_OK);  // float has one arithmetic
    // ... in SN_MODE_AUTO the same clips run, on the pool path
    const ClipPlan sat = plan_of(clip(2, 1, 0, 0, 256, 4), SN_ARITH_SSE2);
    CHECK(sat.refusal == SN_OK && sat.saturating && !sat.saturating_sweeps && !sat.use_fused && !sat.parts_eligible && sat.pool.arith == SN_ARITH_SSE2);
    // SN_MODE_FUSED on a clip the sweeps do not serve
    CHECK(plan_of(clip(1, 1, 0, 0, 64, 4, SN_MODE_FUSED)).refusal == SN_OK);
    refused(plan_of(clip(1, 1, 0, 0, 40, 4, SN_MODE_FUSED)), "SN_MODE_FUSED requested but this configuration is not eligible");
    refused(plan_of(clip(2, 1, 0, 0, 3872, 4, SN_MODE_FUSED)), "SN_MODE_FUSED requested but this configuration is not eligible");
    CHECK(plan_of(clip(2, 1, 0, 0, 3872, 4, SN_MODE_FUSED), SN_ARITH_CXX, true).refusal == SN_OK);  // column parts serve it
}

static void check_plan_fields()
{
    const ClipPlan y = plan_of(clip(1, 1, 0, 0, 40, 6));
    CHECK(y.out_height == 6 && y.stride_e == 64 && y.bh == 3 && !y.history_free && !y.isolated && !y.use_fused && !y.fused420);
    CHECK(y.pool.stride_e == 64 && y.pool.bh == 3 && y.pool.slot_bytes == ((9 * 4 * 64 + 255) & ~255) && y.pool.base == nullptr);
    CHECK(y.aaf[0] == 63.0f && y.process[0]);
    sn_config d = clip(2, 1, 0, 0, 64, 5 * 2);
    d.dh = 1;
    d.bits_per_sample = 10;
    const ClipPlan dh = plan_of(d);
    CHECK(dh.out_height == 20 && dh.bh == 10 && dh.history_free && dh.use_fused && dh.aaf[0] == 252.0f);
    CHECK(plan_of(clip(4, 1, 0, 0, 64, 4)).aaf[0] == 63.0f / 256.0f);
    // bh = 1 and 2
    CHECK(plan_of(clip(1, 1, 0, 0, 64, 2)).bh == 1 && plan_of(clip(1, 1, 0, 0, 64, 4)).bh == 2);
    // SN_MODE_POOL: nothing is marked for the sweeps or the parts
    const ClipPlan pp = plan_of(clip(4, 1, 0, 0, 6144, 4, SN_MODE_POOL), SN_ARITH_CXX, true);
    CHECK(pp.refusal == SN_OK && !pp.plane_parts[0] && pp.parts_eligible && !pp.use_fused);
    const ClipPlan pa = plan_of(clip(4, 1, 0, 0, 6144, 4), SN_ARITH_CXX, true);
    CHECK(pa.plane_parts[0] && pa.parts_eligible && pa.use_fused);
    CHECK(!plan_of(clip(4, 1, 0, 0, 6144, 4)).use_fused);  // without the option: the pool path
    sn_config iso = clip(1, 3, 1, 1, 256, 64);
    iso.isolated_planes = 1;
    const ClipPlan ia = plan_of(iso);
    CHECK(ia.isolated && ia.plane_fused[0] && ia.plane_fused[1] && ia.plane_fused[2] && ia.use_fused && !ia.fused420);
    CHECK(ia.plane_pool[1].stride_e == 128 && ia.plane_pool[1].bh == 16 && ia.plane_pool[0].bh == 32);
    iso.mode = SN_MODE_POOL;
    const ClipPlan ip = plan_of(iso);
    CHECK(ip.isolated && !ip.plane_fused[0] && !ip.plane_fused[1] && !ip.plane_fused[2] && !ip.use_fused);
    // fresh_pool: 8 and 24 columns take the padded sweep, 9 the pool path
    for (int w : {8, 24, 9}) {
        sn_config f = clip(1, 1, 0, 0, w, 4);
        f.fresh_pool = 1;
        const ClipPlan fp = plan_of(f);
        CHECK(fp.fresh && fp.isolated && fp.history_free && fp.plane_padded[0] == (w != 9) && fp.plane_fused[0] == (w != 9) && fp.use_fused == (w != 9));
    }
    // widths: the widest whole-plane sweep and the next width
    CHECK(sweep_plane_ok(1, 7680) && !sweep_plane_ok(1, 7712) && sweep_plane_ok(2, 3840) && !sweep_plane_ok(2, 3872) && sweep_plane_ok(4, 3840) && !sweep_plane_ok(4, 3872));
    CHECK(sweep_waves(1, 7680) == 8 && sweep_waves(2, 3840) == 8 && sweep_waves(1, 1024) == 2 && sweep_waves(2, 1024) == 3);
    CHECK(!fused_parts_plane_eligible(1, 7712) && fused_parts_plane_eligible(2, 3872) && fused_parts_plane_eligible(4, 8192) && !fused_parts_plane_eligible(4, 3840) &&
          !fused_parts_plane_eligible(2, 3880));
    // fields
    CHECK(field_offset(0, 1) == 0 && field_offset(0, 0) == 1 && field_offset(1, 0) == 0 && field_offset(1, 1) == 0 && field_offset(2, 0) == 1 && field_offset(2, 1) == 1);
    const KeptLines k = kept_lines(plan_of(clip(1, 1, 0, 0, 64, 8)), 0, 0), kd = kept_lines(dh, 0, 0);
    CHECK(k.first == 0 && k.step == 2 && k.rows == 4 && kd.first == 0 && kd.step == 1 && kd.rows == 10);
    sn_config o2 = clip(1, 1, 0, 0, 64, 8);
    o2.order = 2;
    CHECK(kept_lines(plan_of(o2), 0, 0).first == 1);
}

// ---- coupled sweeps ---------------------------------------------------------------------------------------------------------
static void check_coupled()
{
    // reach = min(nr_c + 2, bh - 1): the bh - 1 arm, both arms equal, the nr_c + 2 arm
    CHECK(coupled_reach(0, 2) == 1 && coupled_reach(1, 4) == 3 && coupled_reach(2, 6) == 4);
    CHECK(coupled_sweep_u(0, 2) == 1 && coupled_sweep_u(1, 4) == 2 && coupled_sweep_u(2, 6) == 3 && coupled_sweep_u(5, 6) == 5);
    const int want_rows[3] = {2, 4, 5};
    for (int i = 0; i < 3; ++i) {
        const ClipPlan p = plan_of(clip(1, 3, 1, 1, 1024, 4 + 4 * i, SN_MODE_FUSED));
        CHECK(p.fused420 && p.fpool_rows == want_rows[i] && !p.uv_geometry);
        const LaunchDecision d = decide_launch(p, launch(3, 1), false, false);
        CHECK(d.route == Route::kCoupled && d.fused[0] && d.fused[1] && d.fused[2] && d.nbands == 0);
    }
    const ClipPlan p422 = plan_of(clip(1, 3, 1, 0, 1024, 2, SN_MODE_FUSED));  // reach 0: a hand-off pool of row 0 alone
    CHECK(p422.fused420 && p422.fpool_rows == 1);
    // U and V as one sweep: nr_c = 5, 6, 7 (4:2:0 heights 24, 28, 32)
    CHECK(!plan_of(clip(1, 3, 1, 1, 256, 24, SN_MODE_FUSED)).uv_geometry);
    CHECK(plan_of(clip(1, 3, 1, 1, 256, 28, SN_MODE_FUSED)).uv_geometry);
    CHECK(plan_of(clip(1, 3, 1, 1, 256, 32, SN_MODE_FUSED)).uv_geometry);
    CHECK(!plan_of(clip(2, 3, 1, 1, 256, 32, SN_MODE_FUSED)).uv_geometry);  // 8-bit only
    CHECK(!fused_uv_ok(256, 128, 6, 12) && fused_uv_ok(256, 128, 7, 14) && fused_uv_ok(256, 128, 8, 16));
    CHECK(fused_uv_ok(3840, 1920, 7, 14) && !fused_uv_ok(3872, 1936, 7, 14) && !fused_uv_ok(256, 256, 7, 14) && !fused_uv_ok(256, 124, 7, 14));
    CHECK(!fused_uv_ok(256, 128, 16, 14));  // nr_c <= bh - 1
    // a plane whose layout the sweeps do not take: the clip leaves the coupled route
    const ClipPlan p = plan_of(clip(1, 3, 1, 1, 1024, 64, SN_MODE_FUSED));
    LaunchInput in = launch(3, 1);
    in.layout_ok[1] = false;
    const LaunchDecision d = decide_launch(p, in, false, false);
    CHECK(d.route == Route::kPlanes && d.fused[0] && !d.fused[1] && d.fused[2]);
    // stops of a 4:2:0 frame: chroma own rows 16, luma 32
    CHECK(d.stop[2] == 16 && d.stop[1] == 17 && d.stop[0] == 32);
}

// ---- row bands --------------------------------------------------------------------------------------------------------------
static void check_bands()
{
    // nr = 15, 16, 24, 25 (heights 32, 34, 50, 52), forced and chosen: bands per frame for 8-bit, 16-bit and float planes.  Chosen,
    // a band has at least a quarter of the run-up (32 / 40 / 48 rows) of rows of its own: 24 rows are three bands of 8 or two of 12
    struct { int h, force, want[3]; } const rows[] = {{32, 2, {0, 0, 0}}, {34, 2, {2, 2, 2}}, {50, 3, {3, 3, 3}}, {52, 3, {3, 3, 3}}, {52, 4, {3, 3, 3}},
                                                      {34, 1, {0, 0, 0}}, {32, 0, {0, 0, 0}}, {34, 0, {0, 0, 0}}, {50, 0, {3, 2, 2}}, {52, 0, {3, 2, 2}},
                                                      {50, -1, {0, 0, 0}}};
    for (const auto& r : rows)
        for (int t = 0; t < 3; ++t) {
            const int bytes = 1 << t, want = r.want[t];
            const ClipPlan p = plan_of(clip(bytes, 1, 0, 0, 512, r.h));
            LaunchInput in = launch(1, 4);
            in.band_force = r.force;
            const LaunchDecision d = decide_launch(p, in, false, false);
            CHECK(d.nbands == want && launch_bands(p, in) == want);
            CHECK(d.route == (want ? Route::kBandedPlanes : Route::kPlanes));
            // not cut, the estimate decides: 16 or 17 rows of a sweep take 42 - 48 us (8-bit, 16-bit) or 69 - 73 us (float), 25 rows
            // 65 / 70 / 108 us, the pool path 60 us and 0.26 - 0.37 us a row
            CHECK(d.fused[0] == (want != 0 || bytes == 1 || (bytes == 2 && r.h < 50)));
            CHECK(decide_launch(p, in, true, false).nbands == 0);  // paused
            CHECK(band_rows_available(p, r.force, 0) == (r.h / 2 - 1 >= 16 && r.force >= 0 ? r.h / 2 - 1 : 0));
        }
    // the run-up bounds the chosen count: 8-bit run-up 32 -> bands of at least 8 rows, float 48 -> 12
    CHECK(band_count(plan_of(clip(1, 1, 0, 0, 512, 400)), launch(1, 4)) == 24);  // nr 199: 199 / 8 = 24
    CHECK(band_count(plan_of(clip(4, 1, 0, 0, 512, 400)), launch(1, 4)) == 16);  // 199 / 24 = 8 < 12: 199 / 12
    CHECK(band_count(plan_of(clip(1, 1, 0, 0, 512, 400)), launch(171, 256)) == 0);  // 512 / 171 = 2 bands: not worth it
    CHECK(band_count(plan_of(clip(1, 1, 0, 0, 512, 400)), launch(170, 256)) == 3);
    CHECK(band_count(plan_of(clip(1, 1, 0, 0, 512, 400)), launch(2, 1)) == 0);      // no pool slots for the fallback
    CHECK(band_count(plan_of(clip(1, 1, 0, 0, 512, 400)), launch(193, 256)) == 0);  // kMaxBandSlots
    LaunchInput sw = launch(1, 4);
    sw.sweeps_always = true;
    CHECK(band_count(plan_of(clip(1, 1, 0, 0, 512, 400)), sw) == 0);
    sw.band_force = 200;
    CHECK(band_count(plan_of(clip(1, 1, 0, 0, 512, 2100)), sw) == 128);  // kMaxBands
    CHECK(band_warm_rows(1, 0) == 32 && band_warm_rows(2, 0) == 40 && band_warm_rows(4, 0) == 48 && band_warm_rows(4, 1) == 1);
    // never with column parts, never in the other modes, never with history
    CHECK(band_rows_available(plan_of(clip(1, 1, 0, 0, 512, 400)), 0, 2) == 0);
    CHECK(band_rows_available(plan_of(clip(1, 1, 0, 0, 512, 400, SN_MODE_FUSED)), 0, 0) == 0);
    CHECK(band_rows_available(plan_of(clip(1, 1, 0, 0, 520, 400)), 0, 0) == 0);
    CHECK(band_rows_available(plan_of(clip(1, 3, 1, 1, 512, 400)), 0, 0) == 99);  // the shortest processed plane
    // the geometry of a sweep's bands
    const BandGeometry a = band_geometry(2, 16), b = band_geometry(3, 25), c = band_geometry(2, 15), e = band_geometry(67, 539);
    CHECK(a.band_rows == 8 && a.nbands == 2 && b.band_rows == 9 && b.nbands == 3 && c.band_rows == 8 && c.nbands == 2 && e.band_rows == 9 && e.nbands == 60);
    // a small 4:2:0 launch: luma in bands
    const LaunchDecision d = decide_launch(plan_of(clip(1, 3, 1, 1, 256, 400)), launch(1, 4), false, false);
    CHECK(d.route == Route::kCoupledBanded && d.nbands == 12 && d.stop[0] == 200 && d.stop[1] == 101 && d.stop[2] == 100);
}

// ---- column parts -----------------------------------------------------------------------------------------------------------
static void check_parts()
{
    LaunchInput in = launch(3, 3);
    in.parts_slots = 3;
    in.seam_record = true;
    // nr = 0: marked, never cut, off the sweeps
    const ClipPlan p0 = plan_of(clip(4, 1, 0, 0, 6144, 2, SN_MODE_FUSED), SN_ARITH_CXX, true);
    PartsPlan pl;
    CHECK(p0.plane_parts[0] && !plan_parts(p0, 0, 0, 0, pl) && pl.n == 0);
    const LaunchDecision d0 = decide_launch(p0, in, false, false);
    CHECK(!d0.fused[0] && !d0.parts_cut && d0.plan[0].n == 0 && d0.route == Route::kPlanes && d0.stop[0] == 1);
    // nr = 1: four windows of 1728 columns, ghosts of 96
    const ClipPlan p1 = plan_of(clip(4, 1, 0, 0, 6144, 4, SN_MODE_FUSED), SN_ARITH_CXX, true);
    CHECK(plan_parts(p1, 0, 0, 0, pl) && pl.n == 4 && pl.win_w == 1728);
    const int seams[5] = {0, 1536, 3072, 4608, 6144}, wins[4] = {0, 1440, 2976, 4416};
    for (int k = 0; k < 4; ++k) CHECK(pl.seam[k] == seams[k] && pl.win_x[k] == wins[k]);
    CHECK(pl.seam[4] == 6144);
    const LaunchDecision d1 = decide_launch(p1, in, false, false);
    CHECK(d1.fused[0] && d1.parts_cut && d1.plan[0].n == 4 && d1.route == Route::kPlanes && d1.stop[0] == 2);
    const LaunchDecision dp = decide_launch(p1, in, false, true);  // paused: the pool path
    CHECK(!dp.fused[0] && dp.parts_cut && dp.plan[0].n == 0);
    LaunchInput none = in;
    none.seam_record = false;
    CHECK(!decide_launch(p1, none, false, false).parts_cut && !decide_launch(p1, none, false, false).fused[0]);
    none = in;
    none.slot0 = 3;
    CHECK(!decide_launch(p1, none, false, false).parts_cut);
    // SN_MODE_AUTO: launches small enough for row bands (512 / n >= 3) go to the pool path unless SN_SMALL_SWEEP
    const ClipPlan pa = plan_of(clip(4, 1, 0, 0, 6144, 4), SN_ARITH_CXX, true);
    LaunchInput big = launch(171, 256);
    big.parts_slots = 256;
    big.seam_record = true;
    LaunchInput small = big;
    small.n = 170;
    CHECK(decide_launch(pa, big, false, false).parts_cut && !decide_launch(pa, small, false, false).parts_cut);
    small.sweeps_always = true;
    CHECK(decide_launch(pa, small, false, false).parts_cut);
    // Y16 3872: three parts; forced parts on a plane the whole-plane sweep takes: paused, it goes to that sweep
    CHECK(plan_parts(plan_of(clip(2, 1, 0, 0, 3872, 4, SN_MODE_FUSED), SN_ARITH_CXX, true), 0, 0, 0, pl) && pl.n == 3);
    const ClipPlan pf = plan_of(clip(2, 1, 0, 0, 512, 4, SN_MODE_FUSED), SN_ARITH_CXX, true);
    CHECK(!pf.plane_parts[0] && !plan_parts(pf, 0, 0, 0, pl) && plan_parts(pf, 0, 2, 0, pl) && pl.n == 2 && pl.seam[1] == 256);
    CHECK(plan_parts(pf, 0, 8, 0, pl) && pl.n == 8 && pl.win_w == 192);  // 64 columns a part and ghosts of 64: windows of 128 and 192
    CHECK(!plan_parts(plan_of(clip(4, 1, 0, 0, 512, 4, SN_MODE_FUSED), SN_ARITH_CXX, true), 0, 8, 0, pl));  // ... no room for ghosts of 96
    CHECK(!plan_parts(pf, 0, 9, 0, pl));
    in.parts_force = 2;
    CHECK(decide_launch(pf, in, false, false).plan[0].n == 2);
    const LaunchDecision df = decide_launch(pf, in, false, true);
    CHECK(df.fused[0] && df.plan[0].n == 0);
    in.parts_ghost_force = 8;  // the seam eight columns from the end of the window left of it
    const LaunchDecision dg = decide_launch(pf, in, false, false);
    CHECK(dg.plan[0].n == 2 && dg.plan[0].seam[1] == dg.plan[0].win_x[0] + dg.plan[0].win_w - 8);
    CHECK(!plan_parts(plan_of(clip(1, 1, 0, 0, 512, 4, SN_MODE_FUSED), SN_ARITH_CXX, true), 0, 2, 0, pl));  // 8-bit: no instance
    CHECK(parts_ghost(2) == 64 && parts_ghost(4) == 96 && kPartsWindow == 1936);
}

// ---- chains -----------------------------------------------------------------------------------------------------------------
static void check_chains()
{
    int planes[3];
    CHECK(chain_planes(plan_of(clip(1, 1, 0, 0, 40, 2)), 2, planes) == 0);  // bh = 1, nr = 0
    CHECK(chain_planes(plan_of(clip(1, 1, 0, 0, 40, 4)), 2, planes) == 1 && planes[0] == 0);  // bh = 2, nr = 1
    CHECK(chain_planes(plan_of(clip(1, 1, 0, 0, 40, 4)), 1, planes) == 0);   // the pool has no chain kernel
    CHECK(chain_planes(plan_of(clip(1, 1, 0, 0, 64, 4)), 2, planes) == 0);   // history-free
    CHECK(chain_planes(plan_of(clip(1, 1, 0, 0, 44, 4)), 2, planes) == 0);   // not a whole number of lanes
    CHECK(chain_planes(plan_of(clip(1, 3, 1, 1, 720, 4)), 2, planes) == 0);  // bh = 2, chroma without a row
    CHECK(chain_planes(plan_of(clip(1, 3, 1, 1, 720, 8)), 2, planes) == 3 && planes[2] == 2);
    sn_config c = clip(1, 3, 1, 1, 720, 8);
    c.luma = 0;
    CHECK(chain_planes(plan_of(c), 2, planes) == 2 && planes[0] == 1 && planes[1] == 2);
}

// ---- the pause --------------------------------------------------------------------------------------------------------------
static void check_pause()
{
    FallbackPause p;
    for (int i = 0; i < 100; ++i) CHECK(!p.paused(0));
    for (int i = 0; i < 8; ++i) CHECK(p.paused(1));  // a failed frame: eight launches
    CHECK(!p.paused(1));
    for (int i = 0; i < 16; ++i) CHECK(p.paused(2));  // another: sixteen
    for (int i = 0; i < 63; ++i) CHECK(!p.paused(2));
    for (int i = 0; i < 32; ++i) CHECK(p.paused(3));  // 63 good launches do not forget
    for (int i = 0; i < 64; ++i) CHECK(!p.paused(3));
    for (int i = 0; i < 8; ++i) CHECK(p.paused(4));   // 64 do
    CHECK(!p.paused(4));
    FallbackPause q;
    int64_t seen = 0;
    int longest = 0;
    for (int k = 0; k < 10; ++k) {  // 8, 16, ... up to 1024
        int run = 0;
        ++seen;
        while (q.paused(seen)) ++run;
        longest = run;
        CHECK(run == (k < 7 ? 8 << k : 1024));
    }
    CHECK(longest == 1024);
    q.forget();
    CHECK(!q.paused(seen) && q.pause == 0 && q.next == 0);
}

// ---- prefer_pool ------------------------------------------------------------------------------------------------------------
// The answers of the function this header's prefer_pool replaced (sn_api.hip before the move), recorded from its body as it was:
// {width, height, bytes per sample, 4:2:0, bit i: the pool path for a launch of 1 << i frames on 256 slots}
static const int kPreferPool[18][5] = {
    {1920, 1080, 1, 0, 0x7f}, {1920, 1080, 1, 1, 0x7f}, {1920, 1080, 2, 0, 0x7f}, {1920, 1080, 2, 1, 0x7f}, {1920, 1080, 4, 0, 0x3f}, {1920, 1080, 4, 1, 0x3f},
    {3840, 2160, 1, 0, 0x3f}, {3840, 2160, 1, 1, 0x3f}, {3840, 2160, 2, 0, 0x1f}, {3840, 2160, 2, 1, 0x3f}, {3840, 2160, 4, 0, 0x1f}, {3840, 2160, 4, 1, 0x1f},
    {7680, 4320, 1, 0, 0x3f}, {7680, 4320, 1, 1, 0x1f}, {7680, 4320, 2, 0, 0x0f}, {7680, 4320, 2, 1, 0x0f}, {7680, 4320, 4, 0, 0x0f}, {7680, 4320, 4, 1, 0x0f},
};

static void check_prefer_pool()
{
    for (const auto& r : kPreferPool) {
        const ClipPlan p = plan_of(clip(r[2], r[3] ? 3 : 1, r[3], r[3], r[0], r[1]));
        CHECK(p.refusal == SN_OK && p.history_free);
        for (int i = 0; i < 8; ++i) {
            const bool got = prefer_pool(p, launch(1 << i, 256));
            if (got != (((r[4] >> i) & 1) != 0)) {
                std::printf("prefer_pool %dx%d bytes %d 420 %d n %d: got %d\n", r[0], r[1], r[2], r[3], 1 << i, got);
                ++failures;
            }
        }
        // ... and never outside SN_MODE_AUTO, with SN_SMALL_SWEEP, or without the slots
        LaunchInput in = launch(1, 256);
        in.sweeps_always = true;
        CHECK(!prefer_pool(p, in) && !prefer_pool(p, launch(2, 1)));
        CHECK(!prefer_pool(plan_of(clip(r[2], r[3] ? 3 : 1, r[3], r[3], r[0], r[1], SN_MODE_POOL)), launch(1, 256)));
    }
    // the one-sweep form of U and V is what makes the sweeps cheaper for 8-bit 4:2:0: with a sweep each the estimate moves
    const ClipPlan p = plan_of(clip(1, 3, 1, 1, 3840, 2160));
    CHECK(p.uv_geometry);
    // a launch too large for bands that the estimate sends to the pool path leaves the sweeps altogether
    const ClipPlan y = plan_of(clip(1, 1, 0, 0, 1920, 1080));
    LaunchInput in = launch(1, 4);
    in.band_force = -1;
    const LaunchDecision d = decide_launch(y, in, false, false);
    CHECK(d.nbands == 0 && !d.fused[0] && d.route == Route::kPlanes && d.stop[0] == 540);
    CHECK(decide_launch(y, launch(1, 4), false, false).nbands == 67);  // with bands: those first
    CHECK(!decide_launch(y, launch(1, 4), true, false).fused[0]);      // bands paused: the estimate decides
}

// ---- queries ----------------------------------------------------------------------------------------------------------------
constexpr int kQuery = 30;

static void answer(const int* q)
{
    sn_config c = clip(q[0], q[2], q[3], q[4], q[5], q[6], q[10]);
    c.bits_per_sample = q[1];
    c.dh = q[7];
    c.luma = q[8];
    c.chroma = q[9];
    c.isolated_planes = q[11];
    c.fresh_pool = q[12];
    const ClipPlan p = plan_of(c, q[13], q[14] != 0, q[15]);
    std::printf("refusal=%d", p.refusal);
    if (p.refusal != SN_OK) {
        std::printf(" text=%s\n", p.refusal_text.c_str());
        return;
    }
    LaunchInput in;
    in.n = q[16];
    in.slot0 = q[17];
    in.slots = q[18];
    in.parts_slots = q[19];
    in.seam_record = q[20] != 0;
    in.sweeps_always = q[21] != 0;
    in.band_force = q[22];
    in.band_warm = q[23];
    in.parts_force = q[24];
    in.parts_ghost_force = q[25];
    in.chroma_sweeps = q[26];
    std::printf(" out_height=%d stride_e=%d bh=%d history_free=%d isolated=%d fresh=%d use_fused=%d fused420=%d uv_geometry=%d fpool_rows=%d parts_eligible=%d",
                p.out_height, p.stride_e, p.bh, p.history_free, p.isolated, p.fresh, p.use_fused, p.fused420, p.uv_geometry, p.fpool_rows, p.parts_eligible);
    std::printf(" reach=%d slot_bytes=%lld", coupled_reach(p.plane_h_out(p.nplanes() - 1) / 2 - 1, p.bh), (long long)p.pool.slot_bytes);
    for (int i = 0; i < p.nplanes(); ++i)
        std::printf(" plane%d=%d,%d,%d,%d,%d,%d,%d,%d,%d", i, p.plane_w(i), p.plane_h_out(i), p.enabled(i), p.plane_fused[i], p.plane_padded[i], p.plane_parts[i],
                    sweep_plane_ok(c.bytes_per_sample, p.plane_w(i)), p.plane_pool[i].stride_e, p.plane_pool[i].bh);
    int planes[3];
    std::printf(" chain=%d band_rows=%d warm=%d prefer_pool=%d", chain_planes(p, q[27], planes), band_rows_available(p, in.band_force, in.parts_force),
                band_warm_rows(c.bytes_per_sample, in.band_warm), prefer_pool(p, in));
    const LaunchDecision d = decide_launch(p, in, q[28] != 0, q[29] != 0);
    static const char* const routes[] = {"planes", "banded_planes", "coupled", "coupled_banded"};
    std::printf(" route=%s nbands=%d parts_cut=%d fused=%d,%d,%d stop=%d,%d,%d", routes[(int)d.route], d.nbands, d.parts_cut, d.fused[0], d.fused[1], d.fused[2],
                d.stop[0], d.stop[1], d.stop[2]);
    for (int i = 0; i < p.nplanes(); ++i) {
        // what sn_get_parts_info reports (the plan of a plane the sweeps serve), then what this launch runs
        PartsPlan pl;
        const bool cut = (p.isolated ? p.plane_fused[i] : p.use_fused) && plan_parts(p, i, in.parts_force, in.parts_ghost_force, pl);
        std::printf(" parts%d=%d,%d,%d", i, cut ? pl.n : 0, d.plan[i].n, cut ? pl.win_w : 0);
        for (int k = 0; cut && k < pl.n; ++k) std::printf(",%d:%d", pl.win_x[k], pl.seam[k]);
    }
    std::printf("\n");
}

int main(int argc, char** argv)
{
    if (argc > 1) {
        if ((argc - 1) % kQuery != 0) {
            std::fprintf(stderr, "route_check: %d integers per query\n", kQuery);
            return 2;
        }
        int q[kQuery];
        for (int i = 1; i < argc; i += kQuery) {
            for (int k = 0; k < kQuery; ++k) q[k] = std::atoi(argv[i + k]);
            answer(q);
        }
        return 0;
    }
    check_refusals();
    check_plan_fields();
    check_coupled();
    check_bands();
    check_parts();
    check_chains();
    check_pause();
    check_prefer_pool();
    if (failures == 0) std::printf("ok\n");
    return failures ? 1 : 0;
}
