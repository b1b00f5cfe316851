// surface_layout_check.cpp -- csrc/sn_surface_layout.h against values written out by hand: what each value of sn_surfaces.layout
// is, the row bytes of its planes, the alignment unit, the planes that must be NULL and the contexts that are refused.
// Stand-alone host program (no device code, no GPU): prints "ok" or what differs.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "sn_surface_layout.h"

static int failures = 0;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            ++failures;                                                  \
        }                                                                \
    } while (0)

int main()
{
    using namespace sn;
    // ---- which values are layouts
    for (int v = -2; v <= 16; ++v) {
        const bool want = (v >= 0 && v <= 3) || (v >= 8 && v <= 12);
        CHECK(surface_layout(v).valid == want);
    }
    struct Kind { int value; bool semi, msb; int packing; };
    const Kind kinds[] = {{SN_LAYOUT_PLANAR, false, false, 0},         {SN_LAYOUT_SEMIPLANAR, true, false, 0},
                          {SN_LAYOUT_PLANAR_MSB, false, true, 0},      {SN_LAYOUT_SEMIPLANAR_MSB, true, true, 0},
                          {SN_LAYOUT_PACKED_YUYV, false, false, 1},    {SN_LAYOUT_PACKED_UYVY, false, false, 2},
                          {SN_LAYOUT_PACKED_YUYV_MSB, false, true, 1}, {SN_LAYOUT_PACKED_UYVY_MSB, false, true, 2},
                          {SN_LAYOUT_PACKED_V210, false, false, 3}};
    CHECK(SN_LAYOUT_PACKED_YUYV == 8 && SN_LAYOUT_PACKED_UYVY == 9 && SN_LAYOUT_PACKED_YUYV_MSB == 10 && SN_LAYOUT_PACKED_UYVY_MSB == 11 &&
          SN_LAYOUT_PACKED_V210 == 12);
    for (const Kind& k : kinds) {
        const SurfaceLayout L = surface_layout(k.value);
        CHECK(L.valid && L.semi == k.semi && L.msb == k.msb && L.packing == k.packing);
        // planes described, and the first that must be NULL
        CHECK(surface_planes(L, 3) == (k.packing ? 1 : k.semi ? 2 : 3));
        CHECK(surface_null_from(L) == (k.packing ? 1 : k.semi ? 2 : 3));
        // the shift of the _MSB forms
        CHECK(surface_shift(L, 10) == (k.msb ? 6 : 0) && surface_shift(L, 12) == (k.msb ? 4 : 0) && surface_shift(L, 16) == 0);
    }
    CHECK(surface_planes(surface_layout(SN_LAYOUT_PLANAR), 1) == 1);

    // ---- row bytes of a packed plane: 2 w B; v210 16 ceil(w / 6)
    const int widths[7] = {2, 6, 8, 96, 98, 100, 3840};
    const long yuyv1[7] = {4, 12, 16, 192, 196, 200, 7680};
    const long yuyv2[7] = {8, 24, 32, 384, 392, 400, 15360};
    const long v210[7] = {16, 16, 32, 256, 272, 272, 10240};
    for (int i = 0; i < 7; ++i) {
        const int w = widths[i];
        for (int value : {SN_LAYOUT_PACKED_YUYV, SN_LAYOUT_PACKED_UYVY, SN_LAYOUT_PACKED_YUYV_MSB, SN_LAYOUT_PACKED_UYVY_MSB}) {
            CHECK(surface_row_bytes(surface_layout(value), 0, w, w / 2, 1) == yuyv1[i]);
            CHECK(surface_row_bytes(surface_layout(value), 0, w, w / 2, 2) == yuyv2[i]);
        }
        for (int B = 1; B <= 2; ++B) {
            CHECK(surface_row_bytes(surface_layout(SN_LAYOUT_PACKED_V210), 0, w, w / 2, B) == v210[i]);
            // the planar and semi-planar rows the walk always had
            CHECK(surface_row_bytes(surface_layout(SN_LAYOUT_PLANAR), 0, w, w / 2, B) == (long)w * B);
            CHECK(surface_row_bytes(surface_layout(SN_LAYOUT_PLANAR_MSB), 2, w, w / 2, B) == (long)(w / 2) * B);
            CHECK(surface_row_bytes(surface_layout(SN_LAYOUT_SEMIPLANAR), 0, w, w / 2, B) == (long)w * B);
            CHECK(surface_row_bytes(surface_layout(SN_LAYOUT_SEMIPLANAR), 1, w, w / 2, B) == (long)w * B);
            CHECK(surface_row_bytes(surface_layout(SN_LAYOUT_SEMIPLANAR_MSB), 1, w, w, B) == 2L * w * B);  // NV24
        }
    }

    // ---- alignment units
    for (const Kind& k : kinds)
        for (int B : {1, 2, 4}) CHECK(surface_align(surface_layout(k.value), B) == (k.packing == 3 ? 4 : B));

    // ---- refusals over (planes, sub_w, sub_h, B, bits)
    struct Ctx { int planes, sub_w, sub_h, B, bits; };
    const Ctx c422_8{3, 1, 0, 1, 8}, c422_10{3, 1, 0, 2, 10}, c422_12{3, 1, 0, 2, 12}, c422_16{3, 1, 0, 2, 16}, c422_f{3, 1, 0, 4, 32};
    const Ctx c420_8{3, 1, 1, 1, 8}, c444_8{3, 0, 0, 1, 8}, c440_8{3, 0, 1, 1, 8}, c411_8{3, 2, 0, 1, 8}, y8{1, 0, 0, 1, 8}, y10{1, 0, 0, 2, 10};
    auto refused = [](int value, const Ctx& c) { return surface_refusal(surface_layout(value), c.planes, c.sub_w, c.sub_h, c.B, c.bits); };
    auto names_layout = [&](int value, const Ctx& c) { const char* t = refused(value, c); return t && std::strstr(t, "layout"); };
    // YUYV / UYVY: every 4:2:2 context with integer samples
    for (int value : {SN_LAYOUT_PACKED_YUYV, SN_LAYOUT_PACKED_UYVY}) {
        for (const Ctx& c : {c422_8, c422_10, c422_12, c422_16}) CHECK(refused(value, c) == nullptr);
        for (const Ctx& c : {c422_f, c420_8, c444_8, c440_8, c411_8, y8, y10}) CHECK(names_layout(value, c));
    }
    // the _MSB forms: 16-bit words only (shift 0 on a 16-bit context)
    for (int value : {SN_LAYOUT_PACKED_YUYV_MSB, SN_LAYOUT_PACKED_UYVY_MSB}) {
        for (const Ctx& c : {c422_10, c422_12, c422_16}) CHECK(refused(value, c) == nullptr);
        for (const Ctx& c : {c422_8, c422_f, c420_8, c444_8, y8, y10}) CHECK(names_layout(value, c));
    }
    // v210: 10 bits only
    CHECK(refused(SN_LAYOUT_PACKED_V210, c422_10) == nullptr);
    for (const Ctx& c : {c422_8, c422_12, c422_16, c422_f, c420_8, c444_8, y8, y10}) CHECK(names_layout(SN_LAYOUT_PACKED_V210, c));
    const Ctx c420_10{3, 1, 1, 2, 10};
    CHECK(names_layout(SN_LAYOUT_PACKED_V210, c420_10));
    // the layouts the walk always had keep their rules and the words their callers look for
    for (const Ctx& c : {c422_8, c422_10, c422_f, c420_8, c444_8, y8, y10}) CHECK(refused(SN_LAYOUT_PLANAR, c) == nullptr);
    CHECK(refused(SN_LAYOUT_SEMIPLANAR, c420_8) == nullptr && refused(SN_LAYOUT_SEMIPLANAR, c422_16) == nullptr);
    CHECK(refused(SN_LAYOUT_SEMIPLANAR_MSB, c422_10) == nullptr && refused(SN_LAYOUT_PLANAR_MSB, y10) == nullptr);
    CHECK(refused(SN_LAYOUT_SEMIPLANAR, y8) && std::strstr(refused(SN_LAYOUT_SEMIPLANAR, y8), "num_planes"));
    CHECK(refused(SN_LAYOUT_SEMIPLANAR, c422_f) && std::strstr(refused(SN_LAYOUT_SEMIPLANAR, c422_f), "bytes_per_sample"));
    CHECK(names_layout(SN_LAYOUT_PLANAR_MSB, c422_8) && names_layout(SN_LAYOUT_SEMIPLANAR_MSB, c422_f) && names_layout(SN_LAYOUT_PLANAR_MSB, y8));

    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
