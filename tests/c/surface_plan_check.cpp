// surface_plan_check.cpp -- csrc/sn_surface_plan.h: the plan of a surface call against lines written out by hand (from the two
// walks the plan replaced: which launches, where the passes read and write, which counters move), invariants of the plan over
// every combination the library accepts, and the cutter of runs of frames on parity sequences written out by hand.
// Stand-alone host program (no device code, no GPU): prints "ok" or what differs.
#include <cstdio>
#include <string>
#include <vector>

#include "sn_surface_plan.h"

static int failures = 0;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            ++failures;                                                  \
        }                                                                \
    } while (0)

using namespace sn;

// the side classes: shift 6 is a 10-bit clip's
static const PlanSide kPlanar{false, 0, 0}, kPlanarMsb{false, 0, 6}, kSemi{true, 0, 0}, kSemiMsb{true, 0, 6}, kYuyv{false, 1, 0}, kY210{false, 1, 6},
    kV210{false, 3, 0};

static void expect(const char* what, const PlanSide& s, const PlanSide& d, int planes, bool lp, bool cp, bool all, const char* want)
{
    const std::string got = surface_plan_text(surface_plan(s, d, planes, lp, cp, all));
    if (got != want) {
        std::printf("%s:\n  got  %s\n  want %s\n", what, got.c_str(), want);
        ++failures;
    }
}

static bool scratch(const PlaneRef& r) { return r.buf != kBufSrc && r.buf != kBufDst; }

// what a step writes (source stage: planes of read[]) or reads (after stage: planes of result[]) besides the one plane it names
static std::vector<int> planes_of(const PlanStep& s, bool source)
{
    if (s.op == (source ? kOpUvSplit : kOpUvMerge)) return {1, 2};
    if (s.op == (source ? kOpUnpack : kOpPack)) return {0, 1, 2};
    return {s.plane};
}

static void invariants(const PlanSide& s, const PlanSide& d, int planes, bool lp, bool cp, bool all)
{
    const SurfacePlan P = surface_plan(s, d, planes, lp, cp, all);
    const std::string what = surface_plan_text(P);
    const bool packed = s.packing || d.packing, msb = s.shift || d.shift;
    auto fail = [&](const char* why) {
        std::printf("%s: src(%d %d %d) dst(%d %d %d) planes %d lp %d cp %d all %d: %s\n", why, s.semi, s.packing, s.shift, d.semi, d.packing, d.shift, planes, lp,
                    cp, all, what.c_str());
        ++failures;
    };
    if (P.nonce > 3 || P.nsource > 3 || P.nafter > 4) fail("too many steps");

    // ---- a scratch part is needed exactly when a route or a step touches it (without a packed side the two chroma geometries
    // are one part: both are allocated when either is touched, as ever)
    bool t_in = false, t_out = false, t_y = false, t_yo = false;
    auto touch = [&](const PlaneRef& r) {
        t_in = t_in || r.buf == kBufIn, t_out = t_out || r.buf == kBufOut, t_y = t_y || r.buf == kBufY, t_yo = t_yo || r.buf == kBufYo;
    };
    for (int p = 0; p < 3; ++p) touch(P.read[p]), touch(P.write[p]);
    for (int i = 0; i < P.nafter; ++i)
        for (int p : planes_of(P.after[i], false)) touch(P.result[p]);
    if (!packed) t_in = t_out = t_in || t_out;
    if (P.need.in != t_in || P.need.out != t_out || P.need.y != t_y || P.need.yo != t_yo) fail("scratch needed and scratch touched differ");
    // chunks of what the scratch holds as soon as there is scratch; a call without scratch runs in one piece unless it has a packed side
    const bool any = P.need.in || P.need.out || P.need.y || P.need.yo;
    if (P.chunked != (any || packed)) fail("scratch but no chunks, or chunks without scratch");

    // ---- the source stage writes scratch only, and every scratch plane the passes or the destination read is written by it
    bool brought[3] = {false, false, false};
    for (int i = 0; i < P.nsource; ++i)
        for (int p : planes_of(P.source[i], true)) {
            if (!scratch(P.read[p]) || P.read[p].buf == kBufOut || P.read[p].buf == kBufYo) fail("a source step writes outside the source scratch");
            if (brought[p]) fail("a source plane brought twice");
            brought[p] = true;
        }
    for (int p = 0; p < 3; ++p) {
        if (scratch(P.read[p]) != brought[p]) fail("source scratch read but not written, or written but not read");
        if (P.read[p].buf == kBufOut || P.read[p].buf == kBufYo || P.read[p].buf == kBufDst) fail("the passes read the destination's side");
        if (P.write[p].buf == kBufIn || P.write[p].buf == kBufY || P.write[p].buf == kBufSrc) fail("the passes write the source's side");
    }

    // ---- a plane that is not processed is not a real plane of the passes -- but for luma without an MSB-aligned or packed
    // side, which the passes copy themselves, as in the planar call
    for (int p = 0; p < 3; ++p) {
        const bool processed = p == 0 ? lp : planes >= 3 && cp;
        const bool copied_by_passes = p == 0 && !lp && !msb && !packed;
        if (P.read[p].live != P.write[p].live) fail("a plane the passes read but do not write, or the reverse");
        if (P.read[p].live != (processed || copied_by_passes)) fail("a plane that is not processed is routed as a real plane, or the reverse");
        if (P.read[p].live && p < planes && !scratch(P.read[p]) && P.read[p].idx != p) fail("a real plane routed to another plane");
        const PlaneRef& want = processed ? P.write[p] : P.read[p];
        if (P.result[p].buf != want.buf || P.result[p].idx != want.idx) fail("result is neither what the passes wrote nor the source's planar form");
    }

    // ---- every plane the context has reaches the destination exactly once per frame
    int written[3] = {0, 0, 0};
    for (int i = 0; i < P.nonce; ++i) {
        const PlanStep& st = P.once[i];
        if (st.op == kOpUvSplit || st.op == kOpUvMerge || st.uv_row) ++written[1], ++written[2];
        else if (st.op == kOpShift16 || st.op == kOpCopy) ++written[st.plane];
        else fail("a step before the chunks that is none of theirs");
    }
    for (int p = 0; p < 3; ++p)
        if (P.write[p].live && P.write[p].buf == kBufDst) ++written[p];
    for (int i = 0; i < P.nafter; ++i) {
        const PlanStep& st = P.after[i];
        if (st.op == kOpUnpack || st.op == kOpUvSplit || st.op == kOpCopy || st.uv_row) fail("a step after the passes that is none of theirs");
        for (int p : planes_of(st, false)) {
            const bool in_place = P.result[p].buf == kBufDst;  // shifted up where the passes wrote it: no second write
            if (in_place && !(st.op == kOpShift16 && P.write[p].live && P.result[p].idx == p && d.shift != 0)) fail("a destination plane read back");
            if (!in_place) ++written[p];
            if (scratch(P.result[p]) && (P.result[p].buf == kBufOut || P.result[p].buf == kBufYo) && !P.write[p].live) fail("output scratch read but never written");
        }
    }
    for (int p = 0; p < planes && p < 3; ++p)
        if (written[p] != 1) fail("a plane written to the destination not exactly once");
    for (int p = planes; p < 3; ++p)
        if (written[p] != 0) fail("a plane the context does not have is written");
    // an MSB-aligned destination: what the passes wrote in place is shifted up
    for (int p = 0; p < planes && p < 3 && d.shift != 0; ++p) {
        const bool processed = p == 0 ? lp : cp;
        bool shifted = false;
        for (int i = 0; i < P.nafter; ++i) shifted = shifted || (P.after[i].op == kOpShift16 && P.after[i].plane == p);
        if (processed && P.write[p].buf == kBufDst && !shifted) fail("LSB-aligned samples left in an MSB-aligned destination");
    }

    // ---- the counters
    const bool chroma = planes >= 3;
    if ((P.count_split != kCountNever) != (chroma && (cp || packed) && (s.packing || s.semi))) fail("split_frames");
    if ((P.count_merged != kCountNever) != (chroma && (cp || packed) && (d.packing || d.semi))) fail("merged_frames");
    if ((P.count_copied != kCountNever) != (chroma && !cp)) fail("copied_frames");
}

static void runs()
{
    auto order0 = [](int parity) { return parity ? 0 : 1; };  // a field offset that depends on the parity
    auto fixed = [](int) { return 1; };                        // ... and one that does not
    auto cut = [&](const std::vector<int32_t>& par, int m, bool extend, bool by_parity) {
        std::string s;
        for (int f = 0; f < m;) {
            const FieldRun r = by_parity ? field_run(par.empty() ? nullptr : par.data(), f, m, order0, extend)
                                         : field_run(par.empty() ? nullptr : par.data(), f, m, fixed, extend);
            if (r.end <= f || r.end > m) {
                CHECK(!"a run that does not advance or leaves the batch");
                break;
            }
            s += std::to_string(f) + "-" + std::to_string(r.end) + "@" + std::to_string(r.offset) + " ";
            f = r.end;
        }
        return s;
    };
    CHECK(cut({}, 5, true, true) == "0-5@0 ");          // no parity array: parity 1 for every frame
    CHECK(cut({}, 1, true, true) == "0-1@0 ");
    CHECK(cut({0}, 1, true, true) == "0-1@1 ");         // a single frame
    CHECK(cut({0, 1, 0}, 3, true, true) == "0-1@1 1-2@0 2-3@1 ");  // alternating
    CHECK(cut({0, 0, 1, 1, 1, 0}, 6, true, true) == "0-2@1 2-5@0 5-6@1 ");
    CHECK(cut({0, 1, 0, 1}, 4, true, false) == "0-4@1 ");  // the offset ignores the parity: one run
    CHECK(cut({1, 1, 1}, 2, true, true) == "0-2@0 ");      // m below the array's length
    // run_batch on a history-carrying clip without a chain: one frame at a time, the offset still the frame's own
    CHECK(cut({0, 0, 1, 1}, 4, false, true) == "0-1@1 1-2@1 2-3@0 3-4@0 ");
    CHECK(cut({}, 3, false, true) == "0-1@0 1-2@0 2-3@0 ");
    CHECK(cut({}, 0, true, true).empty());
}

int main()
{
    // ---- semi-planar and MSB-aligned sides: planes that are processed pass through scratch where the caller's plane is not
    // planar and LSB-aligned; the merge comes before the shift-up of what the passes wrote in place
    expect("NV12 -> NV12", kSemi, kSemi, 3, true, true, false,
           "need in out | once - | chunks | source uv_split:1 kept | read src0,in0,in1 | write dst0,out0,out1 | after uv_merge:1 from dst0,out0,out1 | "
           "split chunk merged chunk copied -");
    expect("NV12 -> planar", kSemi, kPlanar, 3, true, true, false,
           "need in out | once - | chunks | source uv_split:1 kept | read src0,in0,in1 | write dst0,dst1,dst2 | after - from dst0,dst1,dst2 | "
           "split chunk merged - copied -");
    expect("planar -> NV12", kPlanar, kSemi, 3, true, true, false,
           "need in out | once - | chunks | source - | read src0,src1,src2 | write dst0,out0,out1 | after uv_merge:1 from dst0,out0,out1 | "
           "split - merged chunk copied -");
    expect("P010 -> P010", kSemiMsb, kSemiMsb, 3, true, true, false,
           "need in out y | once - | chunks | source shift16:0,uv_split:1 kept | read y,in0,in1 | write dst0,out0,out1 | "
           "after uv_merge:1,shift16:0 from dst0,out0,out1 | split chunk merged chunk copied -");
    expect("planar-MSB -> planar, Y only", kPlanarMsb, kPlanar, 1, true, true, false,
           "need y | once - | chunks | source shift16:0 kept | read y,src0~,src0~ | write dst0,dst0~,dst0~ | after - from dst0,src0,src0 | "
           "split - merged - copied -");
    expect("P010 -> planar-MSB", kSemiMsb, kPlanarMsb, 3, true, true, false,
           "need in out y | once - | chunks | source shift16:0,uv_split:1 kept | read y,in0,in1 | write dst0,dst1,dst2 | "
           "after shift16:0,shift16:1,shift16:2 from dst0,dst1,dst2 | split chunk merged - copied -");
    // ---- chroma that is not processed, no packed side: once, before the chunks, never through scratch; the five forms
    expect("NV12 -> NV12, chroma off", kSemi, kSemi, 3, true, false, false,
           "need - | once copy:1x2 | whole | source - | read src0,src0~,src0~ | write dst0,dst0~,dst0~ | after - from dst0,src0,src0 | "
           "split - merged - copied call");
    expect("P010 -> P010, chroma off", kSemiMsb, kSemiMsb, 3, true, false, false,
           "need y | once shift16:1x2 | chunks | source shift16:0 kept | read y,src0~,src0~ | write dst0,dst0~,dst0~ | after shift16:0 from dst0,src0,src0 | "
           "split - merged - copied call");
    expect("NV12 -> planar, chroma off", kSemi, kPlanar, 3, true, false, false,
           "need - | once uv_split:1 | whole | source - | read src0,src0~,src0~ | write dst0,dst0~,dst0~ | after - from dst0,src0,src0 | "
           "split - merged - copied call");
    expect("planar -> P010, chroma off", kPlanar, kSemiMsb, 3, true, false, false,
           "need - | once uv_merge:1 | whole | source - | read src0,src0~,src0~ | write dst0,dst0~,dst0~ | after shift16:0 from dst0,src0,src0 | "
           "split - merged - copied call");
    expect("planar-MSB -> planar, chroma off", kPlanarMsb, kPlanar, 3, true, false, false,
           "need y | once shift16:1,shift16:2 | chunks | source shift16:0 kept | read y,src0~,src0~ | write dst0,dst0~,dst0~ | after - from dst0,src0,src0 | "
           "split - merged - copied call");
    // ---- luma that is not processed: with an MSB-aligned side it goes once, before the chunks; without one the passes copy it
    expect("P010 -> P010, luma off", kSemiMsb, kSemiMsb, 3, false, true, false,
           "need in out | once shift16:0 | chunks | source uv_split:1 kept | read src0~,in0,in1 | write dst0~,out0,out1 | "
           "after uv_merge:1 from src0,out0,out1 | split chunk merged chunk copied -");
    expect("NV12 -> NV12, luma off", kSemi, kSemi, 3, false, true, false,
           "need in out | once - | chunks | source uv_split:1 kept | read src0,in0,in1 | write dst0,out0,out1 | after uv_merge:1 from src0,out0,out1 | "
           "split chunk merged chunk copied -");
    // ---- a packed side: every plane through its planar form; the merge comes last
    expect("YUY2 -> YUY2", kYuyv, kYuyv, 3, true, true, false,
           "need in out y yo | once - | chunks | source unpack:0 kept | read y,in0,in1 | write yo,out0,out1 | after pack:0 from yo,out0,out1 | "
           "split chunk merged chunk copied -");
    expect("v210 -> Y210", kV210, kY210, 3, true, true, false,
           "need in out y yo | once - | chunks | source unpack:0 kept | read y,in0,in1 | write yo,out0,out1 | after pack:0 from yo,out0,out1 | "
           "split chunk merged chunk copied -");
    expect("Y210 -> planar", kY210, kPlanar, 3, true, true, false,
           "need in y | once - | chunks | source unpack:0 kept | read y,in0,in1 | write dst0,dst1,dst2 | after - from dst0,dst1,dst2 | "
           "split chunk merged - copied -");
    expect("planar-MSB -> v210", kPlanarMsb, kV210, 3, true, true, false,
           "need in out y yo | once - | chunks | source shift16:0,shift16:1,shift16:2 kept | read y,in0,in1 | write yo,out0,out1 | "
           "after pack:0 from yo,out0,out1 | split - merged chunk copied -");
    expect("YUY2 -> NV16", kYuyv, kSemi, 3, true, true, false,
           "need in out y | once - | chunks | source unpack:0 kept | read y,in0,in1 | write dst0,out0,out1 | after uv_merge:1 from dst0,out0,out1 | "
           "split chunk merged chunk copied -");
    expect("NV16 -> v210", kSemi, kV210, 3, true, true, false,
           "need in out yo | once - | chunks | source uv_split:1 kept | read src0,in0,in1 | write yo,out0,out1 | after pack:0 from yo,out0,out1 | "
           "split chunk merged chunk copied -");
    expect("planar -> Y210", kPlanar, kY210, 3, true, true, false,
           "need out yo | once - | chunks | source - | read src0,src1,src2 | write yo,out0,out1 | after pack:0 from yo,out0,out1 | "
           "split - merged chunk copied -");
    expect("Y210 -> planar-MSB", kY210, kPlanarMsb, 3, true, true, false,
           "need in y | once - | chunks | source unpack:0 kept | read y,in0,in1 | write dst0,dst1,dst2 | after shift16:0,shift16:1,shift16:2 from dst0,dst1,dst2 | "
           "split chunk merged - copied -");
    // ... with a plane that is not processed: the source in every line, the plane out of where the source's planar form lies
    expect("Y210 -> Y210, chroma off", kY210, kY210, 3, true, false, false,
           "need in out y yo | once - | chunks | source unpack:0 all | read y,in0~,in1~ | write yo,out0~,out1~ | after pack:0 from yo,in0,in1 | "
           "split chunk merged chunk copied chunk");
    expect("v210 -> planar, chroma off", kV210, kPlanar, 3, true, false, false,
           "need in y | once - | chunks | source unpack:0 all | read y,in0~,in1~ | write dst0,dst1~,dst2~ | "
           "after copy|shift16:1,copy|shift16:2 from dst0,in0,in1 | split chunk merged - copied chunk");
    expect("planar -> YUY2, luma off", kPlanar, kYuyv, 3, false, true, false,
           "need out yo | once - | chunks | source - | read src0~,src1,src2 | write yo~,out0,out1 | after pack:0 from src0,out0,out1 | "
           "split - merged chunk copied -");
    expect("Y210 -> P010, luma off", kY210, kSemiMsb, 3, false, true, false,
           "need in out y | once - | chunks | source unpack:0 all | read y~,in0,in1 | write dst0~,out0,out1 | "
           "after copy|shift16:0,uv_merge:1 from y,out0,out1 | split chunk merged chunk copied -");
    expect("NV16 -> Y210, chroma off", kSemi, kY210, 3, true, false, false,
           "need in out yo | once - | chunks | source uv_split:1 all | read src0,in0~,in1~ | write yo,out0~,out1~ | after pack:0 from yo,in0,in1 | "
           "split chunk merged chunk copied chunk");
    // ---- passes that read every line of their source (dh; the anti-aliasing call)
    expect("NV12 -> NV12, all lines", kSemi, kSemi, 3, true, true, true,
           "need in out | once - | chunks | source uv_split:1 all | read src0,in0,in1 | write dst0,out0,out1 | after uv_merge:1 from dst0,out0,out1 | "
           "split chunk merged chunk copied -");
    expect("YUY2 -> YUY2, all lines", kYuyv, kYuyv, 3, true, true, true,
           "need in out y yo | once - | chunks | source unpack:0 all | read y,in0,in1 | write yo,out0,out1 | after pack:0 from yo,out0,out1 | "
           "split chunk merged chunk copied -");

    // ---- invariants over everything the library accepts: a Y clip takes planar sides only (sn_surface_layout.h)
    const PlanSide sides[] = {kPlanar, kPlanarMsb, kSemi, kSemiMsb, kYuyv, kY210, kV210};
    int plans = 0;
    for (int planes : {1, 3})
        for (const PlanSide& s : sides)
            for (const PlanSide& d : sides) {
                if (planes == 1 && (s.semi || s.packing || d.semi || d.packing)) continue;
                for (int flags = 0; flags < 8; ++flags) invariants(s, d, planes, flags & 1, flags & 2, flags & 4), ++plans;
            }
    CHECK(plans == (4 + 49) * 8);

    runs();
    if (failures == 0) std::printf("ok\n");
    return failures ? 1 : 0;
}
