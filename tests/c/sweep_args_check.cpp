// sweep_args_check.cpp -- v3c::build_sweep (csrc/sn_sweep_args.h) on a host compiler, no GPU: the geometry of a sweep, the
// fields each mode's kernel reads, and every refusal.  Every expected value below is written out by hand from the definitions
// (8 pixels per lane; strip 0 holds 62 real lanes of 64, later strips 60; a plane of at most 64 lanes is one strip).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sn_sweep_args.h"

using namespace sn;
using namespace sn::v3c;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);               \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

static uint8_t mem[64];  // addresses to tell apart; nothing is read or written through them
static uint8_t* const kSrc = mem, * const kDst = mem + 8, * const kPoolIn = mem + 16, * const kPoolOut = mem + 24, * const kRec = mem + 32;
static uint32_t* const kBandState = reinterpret_cast<uint32_t*>(mem + 40);
static int32_t* const kBandFlags = reinterpret_cast<int32_t*>(mem + 48);

static PlaneArgs plane(int bytes, int w, int h_out)
{
    PlaneArgs p{};
    p.src = kSrc;
    p.dst = kDst;
    p.src_pitch = w * bytes + 64;
    p.dst_pitch = w * bytes + 128;
    p.w = w;
    p.h_in = h_out / 2;
    p.h_out = h_out;
    p.src_frame_stride = (int64_t)p.src_pitch * p.h_in + 4096;
    p.dst_frame_stride = (int64_t)p.dst_pitch * p.h_out + 8192;
    p.offset = 1;
    p.dh = 0;
    p.enabled = 1;
    p.arith = SN_ARITH_CXX;
    return p;
}

// the fields of the hand-off that a caller of the coupled sweeps fills in (values chosen to be told apart)
static FusedPool coupling(int mode, int sweep_w)
{
    FusedPool fp{};
    fp.mode = mode;
    fp.sweep_w = sweep_w;
    fp.pool_in = kPoolIn;
    fp.pool_out = kPoolOut;
    fp.frame_stride = 123456;
    fp.pool_rows = 11;
    fp.pool_row_bytes = 2048;
    fp.rows_in = 9;
    fp.rows_out = 7;
    fp.sweep_rows = 8;
    fp.cone_w = 128;
    fp.cone_nr = 6;
    fp.cone_in = 6;
    fp.cone_out = 3;
    return fp;
}

static void bands(FusedPool& fp)
{
    fp.band_rows = 5;
    fp.band_warm = 32;
    fp.nbands = 3;
    fp.band_reset = 1;
    fp.band_state = kBandState;
    fp.band_flags = kBandFlags;
}

// float, 3872 x 32 as two windows of 2048 columns at 0 and 1824 with the seam at column 1936
static FusedPool two_parts()
{
    FusedPool fp{};
    fp.mode = kParts;
    fp.nparts = 2;
    fp.win_w = 2048;
    fp.win_x[0] = 0;
    fp.win_x[1] = 1824;
    fp.store_lo[0] = 0;
    fp.store_hi[0] = 1936;
    fp.store_lo[1] = 112;  // 1936 - 1824
    fp.store_hi[1] = 2048;
    fp.seam_x[0][0] = -1;
    fp.seam_x[0][1] = 1936;
    fp.seam_x[1][0] = 112;
    fp.seam_x[1][1] = -1;
    fp.seam_off[0][1] = 0;
    fp.seam_off[1][0] = 8640;  // one side: 15 rows x 9 buffers x 16 samples x 4 bytes
    fp.seam_rec = kRec;
    fp.seam_frame_stride = 20000;
    fp.seam_bytes = 17280;
    return fp;
}

static bool pool_fields_zero(const Args& a)
{
    return !a.pool_in && !a.pool_out && a.pool_frame_stride == 0 && a.pool_rows == 0 && a.pool_row_bytes == 0 && a.rows_in == 0 && a.rows_out == 0 &&
           a.sweep_rows == 0 && a.cone_w == 0 && a.cone_nr == 0 && a.cone_in == 0 && a.cone_out == 0;
}
static bool band_fields_zero(const Args& a)
{
    return a.band_rows == 0 && a.band_warm == 0 && a.nbands == 0 && !a.band_state && !a.band_flags && a.band_reset == 0;
}
static bool parts_fields_zero(const Args& a)
{
    Args z{};
    return a.nparts == 0 && !a.seam_rec && a.seam_frame_stride == 0 && a.seam_bytes == 0 && !memcmp(a.part_x, z.part_x, sizeof z.part_x) &&
           !memcmp(a.part_store_lo, z.part_store_lo, sizeof z.part_store_lo) && !memcmp(a.part_store_hi, z.part_store_hi, sizeof z.part_store_hi) &&
           !memcmp(a.part_seam_x, z.part_seam_x, sizeof z.part_seam_x) && !memcmp(a.part_seam_off, z.part_seam_off, sizeof z.part_seam_off);
}

static void geometry()
{
    Sweep s;
    // 8-bit, 256 x 16: 32 lanes, one strip, one wave; four frames share a workgroup of four waves; 128 * 8 kept lines >> 11 == 0
    PlaneArgs p = plane(1, 256, 16);
    CHECK(build_sweep(kSweepU8, p, 10.0, 5, nullptr, s) == hipSuccess);
    CHECK(s.mode == kPlain && !s.band);
    CHECK(s.args.w == 256 && s.args.nl == 32 && s.args.nvw == 1 && s.args.nw == 1);
    CHECK(group_of(s.args.nw) == 4);
    CHECK(s.args.turn_shift == 10);
    // everything a plain sweep reads
    CHECK(s.args.src == kSrc && s.args.dst == kDst);
    CHECK(s.args.src_pitch == 320 && s.args.dst_pitch == 384);
    CHECK(s.args.src_frame_stride == 320 * 8 + 4096 && s.args.dst_frame_stride == 384 * 16 + 8192);
    CHECK(s.args.src_bytes == 320 * 8 && s.args.dst_bytes == 384 * 16);
    CHECK(s.args.nk == 8 && s.args.offset == 1 && s.args.dh == 0 && s.args.thr == 10 && s.args.nframes == 5 && s.args.arith == SN_ARITH_CXX);
    CHECK(s.args.region_w == 256);
    CHECK(pool_fields_zero(s.args) && band_fields_zero(s.args) && parts_fields_zero(s.args));
    // 8-bit, 7680 wide: 960 lanes = 62 + 14 * 60 + 58 -> 16 strips, two to a wave: 8 waves, and the ladder instead of time slices
    p = plane(1, 7680, 4320);
    CHECK(build_sweep(kSweepU8, p, 0.0, 1, nullptr, s) == hipSuccess);
    CHECK(s.args.nl == 960 && s.args.nvw == 16 && s.args.nw == 8 && group_of(8) == 1);
    CHECK(s.args.turn_shift == kTurnLadder && kTurnLadder == -1);
    // 8-bit, 3840 x 2160: 480 lanes = 62 + 6 * 60 + 58 -> 8 strips, 4 waves; 128 * 1080 = 138240 < 2^18: slices of 2^17 ticks
    p = plane(1, 3840, 2160);
    CHECK(build_sweep(kSweepU8, p, 0.0, 1, nullptr, s) == hipSuccess);
    CHECK(s.args.nvw == 8 && s.args.nw == 4 && s.args.turn_shift == 17);
    // 8-bit, 7712 wide: 964 lanes, 17 strips, 9 waves: refused
    p = plane(1, 7712, 64);
    CHECK(build_sweep(kSweepU8, p, 0.0, 1, nullptr, s) == hipErrorInvalidValue);
    // 16-bit, 3840 wide: 8 strips = 8 waves, time slices of 2^10 ticks
    p = plane(2, 3840, 2160);
    p.arith = SN_ARITH_SSE2;
    p.dh = 1;
    CHECK(build_sweep(kSweepU16, p, 3.0, 2, nullptr, s) == hipSuccess);
    CHECK(s.args.nl == 480 && s.args.nvw == 8 && s.args.nw == 8 && s.args.turn_shift == 10);
    CHECK(s.args.arith == SN_ARITH_SSE2 && s.args.dh == 1 && s.args.thr == 3);
    // 16-bit, 1024 wide: 128 lanes = 62 + 60 + 6 -> 3 strips, 3 waves: a workgroup per frame, no turns
    p = plane(2, 1024, 64);
    CHECK(build_sweep(kSweepU16, p, 0.0, 1, nullptr, s) == hipSuccess);
    CHECK(s.args.nw == 3 && group_of(3) == 1 && s.args.turn_shift == 0);
    // ... and 960 wide: 120 lanes <= 122 -> 2 strips, two frames per workgroup: 4 waves, 128 * 32 >> 11 == 2, >> 12 == 1, >> 13 == 0
    p = plane(2, 960, 64);
    CHECK(build_sweep(kSweepU16, p, 0.0, 1, nullptr, s) == hipSuccess);
    CHECK(s.args.nw == 2 && group_of(2) == 2 && s.args.turn_shift == 12);
    // float, 3872 wide: 484 lanes = 62 + 7 * 60 + 2 -> nine strips: refused as a plain sweep ...
    p = plane(4, 3872, 32);
    CHECK(strips_for(484) == 9);
    CHECK(build_sweep(kSweepF32, p, 0.0, 1, nullptr, s) == hipErrorInvalidValue);
    // ... and accepted as two parts of a window of 2048 columns (256 lanes = 62 + 3 * 60 + 14 -> 5 strips, no turns)
    FusedPool fp = two_parts();
    CHECK(build_sweep(kSweepF32, p, 0.0, 3, &fp, s) == hipSuccess);
    CHECK(s.mode == kParts && !s.band);
    CHECK(s.args.w == 2048 && s.args.nl == 256 && s.args.nvw == 5 && s.args.nw == 5 && s.args.turn_shift == 0);
    CHECK(s.args.nk == 16 && s.args.nframes == 3);
    CHECK(s.args.src == kSrc && s.args.dst == kDst && s.args.src_bytes == (3872 * 4 + 64) * 16 && s.args.dst_bytes == (3872 * 4 + 128) * 32);  // the whole plane's
    CHECK(s.args.nparts == 2 && s.args.part_x[0] == 0 && s.args.part_x[1] == 1824);
    CHECK(s.args.part_store_lo[0] == 0 && s.args.part_store_hi[0] == 1936 && s.args.part_store_lo[1] == 112 && s.args.part_store_hi[1] == 2048);
    CHECK(s.args.part_seam_x[0][0] == -1 && s.args.part_seam_x[0][1] == 1936 && s.args.part_seam_x[1][0] == 112 && s.args.part_seam_x[1][1] == -1);
    CHECK(s.args.part_seam_off[0][1] == 0 && s.args.part_seam_off[1][0] == 8640);
    CHECK(s.args.seam_rec == kRec && s.args.seam_frame_stride == 20000 && s.args.seam_bytes == 17280);
    CHECK(pool_fields_zero(s.args) && band_fields_zero(s.args));
}

static void modes()
{
    Sweep s;
    // 4:2:0, luma 512 x 64 and chroma 256 x 32, in each sample size: 64 lanes -> one strip
    for (const SweepTraits* t : {&kSweepU8, &kSweepU16, &kSweepF32}) {
        const PlaneArgs luma = plane(t->bytes, 512, 64), chroma = plane(t->bytes, 256, 32);
        // kLumaSpill: the plane is the sweep; pool_out and what goes with it, pool_row_bytes as given
        FusedPool fp = coupling(kLumaSpill, 512);
        CHECK(build_sweep(*t, luma, 0.0, 1, &fp, s) == hipSuccess);
        CHECK(s.mode == kLumaSpill && !s.band);
        CHECK(s.args.w == 512 && s.args.nl == 64 && s.args.nw == 1 && s.args.nk == 32);
        CHECK(s.args.pool_out == kPoolOut && s.args.pool_frame_stride == 123456 && s.args.pool_rows == 11 && s.args.pool_row_bytes == 2048 && s.args.rows_out == 7);
        CHECK(s.args.cone_w == 128 && s.args.cone_nr == 6 && s.args.cone_in == 6 && s.args.cone_out == 3);
        CHECK(band_fields_zero(s.args) && parts_fields_zero(s.args));
        // ... with no pool to leave rows in: rows_out = 0
        fp.pool_out = nullptr;
        CHECK(build_sweep(*t, luma, 0.0, 1, &fp, s) == hipSuccess);
        CHECK(s.mode == kLumaSpill && !s.args.pool_out && s.args.rows_out == 0);
        // kChroma: the sweep covers the luma width, the plane is the region; both pools; pool_row_bytes only for kLumaSpill
        fp = coupling(kChroma, 512);
        CHECK(build_sweep(*t, chroma, 0.0, 1, &fp, s) == hipSuccess);
        CHECK(s.mode == kChroma && !s.band);
        CHECK(s.args.w == 512 && s.args.nl == 64 && s.args.region_w == 256 && s.args.nk == 16);
        CHECK(s.args.src_bytes == chroma.src_pitch * 16 && s.args.dst_bytes == chroma.dst_pitch * 32);
        CHECK(s.args.pool_in == kPoolIn && s.args.pool_out == kPoolOut && s.args.pool_frame_stride == 123456 && s.args.pool_rows == 11);
        CHECK(s.args.pool_row_bytes == 0);
        CHECK(s.args.rows_in == 9 && s.args.rows_out == 7 && s.args.sweep_rows == 8);
        CHECK(s.args.cone_w == 128 && s.args.cone_nr == 6 && s.args.cone_in == 6 && s.args.cone_out == 3);
        // kChromaLast: a chroma sweep that hands nothing on
        fp.pool_out = nullptr;
        CHECK(build_sweep(*t, chroma, 0.0, 1, &fp, s) == hipSuccess);
        CHECK(s.mode == kChromaLast && !s.band);
        CHECK(s.args.pool_in == kPoolIn && !s.args.pool_out && s.args.rows_in == 9 && s.args.rows_out == 0 && s.args.sweep_rows == 8 && s.args.region_w == 256);
        // kPadded: a plane of 1000 columns over its pool stride of 1024 (128 lanes: 3 strips); no pools
        const PlaneArgs narrow = plane(t->bytes, 1000, 64);
        fp = FusedPool{};
        fp.mode = kPadded;
        fp.sweep_w = 1024;
        CHECK(build_sweep(*t, narrow, 0.0, 1, &fp, s) == hipSuccess);
        CHECK(s.mode == kPadded && !s.band);
        CHECK(s.args.w == 1024 && s.args.nl == 128 && s.args.nvw == 3 && s.args.nw == (t->packed ? 2 : 3) && s.args.region_w == 1000);
        CHECK(pool_fields_zero(s.args) && band_fields_zero(s.args) && parts_fields_zero(s.args));
        // bands: a plane on its own (sweep_w does not matter) ...
        fp = FusedPool{};
        fp.mode = kPlain;
        fp.sweep_w = 4096;
        bands(fp);
        CHECK(build_sweep(*t, luma, 0.0, 1, &fp, s) == hipSuccess);
        CHECK(s.mode == kPlain && s.band);
        CHECK(s.args.w == 512);
        CHECK(s.args.band_rows == 5 && s.args.band_warm == 32 && s.args.nbands == 3 && s.args.band_reset == 1 && s.args.band_state == kBandState &&
              s.args.band_flags == kBandFlags);
        CHECK(pool_fields_zero(s.args));
        // ... one band is "not cut"
        fp.nbands = 1;
        CHECK(build_sweep(*t, luma, 0.0, 1, &fp, s) == hipSuccess);
        CHECK(s.mode == kPlain && !s.band && band_fields_zero(s.args));
        // ... and the luma sweep of the coupling
        fp = coupling(kLumaSpill, 512);
        bands(fp);
        CHECK(build_sweep(*t, luma, 0.0, 1, &fp, s) == hipSuccess);
        CHECK(s.mode == kLumaSpill && s.band);
        CHECK(s.args.band_rows == 5 && s.args.band_warm == 32 && s.args.nbands == 3 && s.args.band_reset == 1 && s.args.band_state == kBandState &&
              s.args.band_flags == kBandFlags);
        CHECK(s.args.pool_out == kPoolOut && s.args.pool_row_bytes == 2048 && s.args.rows_out == 7);
        // bands with any other mode: refused
        for (int mode : {(int)kChroma, (int)kPadded}) {
            fp = coupling(mode, 512);
            bands(fp);
            CHECK(build_sweep(*t, chroma, 0.0, 1, &fp, s) == hipErrorInvalidValue);
        }
        fp = coupling(kChroma, 512);  // (kChromaLast)
        fp.pool_out = nullptr;
        bands(fp);
        CHECK(build_sweep(*t, chroma, 0.0, 1, &fp, s) == hipErrorInvalidValue);
        // arithmetic 2: refused, alone and with a coupling; a mode that does not exist too
        PlaneArgs odd = luma;
        odd.arith = 2;
        CHECK(build_sweep(*t, odd, 0.0, 1, nullptr, s) == hipErrorInvalidValue);
        fp = coupling(kLumaSpill, 512);
        CHECK(build_sweep(*t, odd, 0.0, 1, &fp, s) == hipErrorInvalidValue);
        fp = coupling(kModes, 512);
        CHECK(build_sweep(*t, luma, 0.0, 1, &fp, s) == hipErrorInvalidValue);
    }
}

static void parts_refusals()
{
    Sweep s;
    const PlaneArgs p = plane(4, 3872, 32);
    const PlaneArgs p16 = plane(2, 3872, 32);
    FusedPool ok = two_parts();
    CHECK(build_sweep(kSweepF32, p, 0.0, 1, &ok, s) == hipSuccess);
    ok.seam_off[1][0] = 4320;  // 16-bit: a side is 15 x 9 x 16 x 2 bytes
    ok.seam_bytes = 8640;
    CHECK(build_sweep(kSweepU16, p16, 0.0, 1, &ok, s) == hipSuccess && s.mode == kParts);
    ok = two_parts();
#define REFUSED(edit)                                                                  \
    do {                                                                               \
        FusedPool fp = ok;                                                             \
        edit;                                                                          \
        CHECK(build_sweep(kSweepF32, p, 0.0, 1, &fp, s) == hipErrorInvalidValue);      \
    } while (0)
    // the window: a multiple of 8 columns, inside the plane
    REFUSED(fp.win_x[1] = 1828);
    REFUSED(fp.win_x[0] = -8);
    REFUSED(fp.win_x[1] = 1832);  // 1832 + 2048 > 3872
    REFUSED(fp.win_w = 2040);     // not a multiple of 32
    REFUSED(fp.win_w = 3872);     // nine strips
    // the stored columns: multiples of 8, inside the window
    REFUSED(fp.store_lo[1] = 116);
    REFUSED(fp.store_hi[0] = 1940);
    REFUSED(fp.store_lo[0] = -8);
    REFUSED(fp.store_hi[1] = 2056);
    // a seam: a multiple of 8, both lanes next to it inside the window
    REFUSED(fp.seam_x[1][0] = 116);
    REFUSED(fp.seam_x[1][0] = 0);
    REFUSED(fp.seam_x[0][1] = 2048);  // 2048 + 8 > 2048
    // its record: inside the frame's
    REFUSED(fp.seam_bytes = 17279);
    REFUSED(fp.seam_off[1][0] = 8641);
    REFUSED(fp.seam_off[0][1] = -1);
    REFUSED(fp.seam_rec = nullptr);
    // the number of parts
    REFUSED(fp.nparts = 1);
    REFUSED(fp.nparts = 9);
    // never in bands
    REFUSED(bands(fp));
    // arithmetic 2
    PlaneArgs odd = p;
    odd.arith = 2;
    CHECK(build_sweep(kSweepF32, odd, 0.0, 1, &ok, s) == hipErrorInvalidValue);
    // the 8-bit sweep has no parts
    FusedPool fp8 = ok;
    fp8.seam_off[1][0] = 2160;
    CHECK(build_sweep(kSweepU8, plane(1, 3872, 32), 0.0, 1, &fp8, s) == hipErrorInvalidValue);
    // eight parts are taken (windows of 512 at multiples of 480: 7 * 480 + 512 = 3872; seams at 496 + 480 k)
    FusedPool many{};
    many.mode = kParts;
    many.nparts = 8;
    many.win_w = 512;
    many.seam_rec = kRec;
    many.seam_bytes = 7 * 2 * 8640;
    for (int k = 0; k < 8; ++k) {
        many.win_x[k] = 480 * k;
        many.store_lo[k] = k == 0 ? 0 : 16;
        many.store_hi[k] = k == 7 ? 512 : 496;
        many.seam_x[k][0] = k == 0 ? -1 : 16;
        many.seam_x[k][1] = k == 7 ? -1 : 496;
        many.seam_off[k][0] = k == 0 ? 0 : (2 * (k - 1) + 1) * 8640;
        many.seam_off[k][1] = k == 7 ? 0 : 2 * k * 8640;
    }
    CHECK(build_sweep(kSweepF32, p, 0.0, 1, &many, s) == hipSuccess);
    CHECK(s.args.nparts == 8 && s.args.part_x[7] == 3360 && s.args.part_seam_off[7][0] == 13 * 8640 && s.args.nw == 1);
}

// `sweep_args_check bytes width[:sweep_w] ...`: one line "nvw nw" per plane, from build_sweep -- a plane on its own, or
// (width:sweep_w) the padded sweep of a plane over its pool stride; "refused" where build_sweep has no instance.
// tests/test_sweep_geometry_cpu.py holds the table of tests/sweep_geometry_cases.py against it.
static int query(int argc, char** argv)
{
    const int bytes = atoi(argv[1]);
    if (bytes != 1 && bytes != 2 && bytes != 4) return 2;
    for (int i = 2; i < argc; ++i) {
        int w = 0, sweep_w = 0;
        const int n = sscanf(argv[i], "%d:%d", &w, &sweep_w);
        if (n < 1 || w <= 0) return 2;
        FusedPool fp{};
        fp.mode = kPadded;
        fp.sweep_w = sweep_w;
        Sweep s;
        if (build_sweep(sweep_traits(bytes), plane(bytes, w, 16), 0.0, 1, n == 2 ? &fp : nullptr, s) != hipSuccess) printf("refused\n");
        else printf("%d %d\n", s.args.nvw, s.args.nw);
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 2) return query(argc, argv);
    geometry();
    modes();
    parts_refusals();
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
