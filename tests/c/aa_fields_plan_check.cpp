// aa_fields_plan_check.cpp -- the both-fields part of the anti-aliasing call's plan (csrc/sn_aa_plan.h), on the host compiler:
// the steps of SN_AA_FIELDS_BOTH against lines written out by hand, the intermediates' byte sums, every refusal of sn_aa_fields,
// and for every combination of the other options that the plan with fields = NULL, the plan with mode ONE and the plan of the
// seven-parameter aa_check are one and the same.  Prints "ok" and returns 0, or says what differs.
#include <cstdio>
#include <cstring>
#include <string>

#include "sn_aa_plan.h"

using namespace sn;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) std::printf("line %d: %s\n", __LINE__, #cond), ++failures; \
    } while (0)

static sn_config config(int planes, int w, int h, int bytes, int bits, int sub_w, int sub_h, int dh = 0)
{
    sn_config c{};
    c.struct_size = (int32_t)sizeof(sn_config);
    c.width = w, c.height = h, c.bytes_per_sample = bytes, c.bits_per_sample = bits, c.num_planes = planes, c.sub_w = sub_w, c.sub_h = sub_h;
    c.order = 1, c.aa = 48, c.aac = 0, c.dh = dh, c.luma = 1, c.chroma = 1, c.max_batch = 1, c.mode = SN_MODE_AUTO;
    return c;
}

static sn_aa_fields fields_of(int mode)
{
    sn_aa_fields f{};
    f.struct_size = (int32_t)sizeof f, f.mode = mode;
    return f;
}

static AaPlan plan_of(const sn_config& c, const sn_aa_fields* f, const sn_aa_mask* m = nullptr, const sn_aa_mask_ex* e = nullptr, const sn_aa_sharpen* s = nullptr)
{
    AaOptions opt;
    std::string msg;
    const int rc = aa_check(c, nullptr, m, e, s, f, opt, msg);
    if (rc != SN_OK) std::printf("refused (%d): %s\n", rc, msg.c_str()), ++failures;
    AaPlan P = aa_geometry(c, opt);
    aa_steps(P);
    return P;
}

// The steps as one line of text: stage, planes, reads>writes (per plane where they differ), cut, :argument.
static std::string steps_text(const AaPlan& P)
{
    static const char* const kinds[] = {"TurnLeft", "Pass1", "TurnRight", "Pass2", "Reduce", "Sharpen", "MaskLuma", "Mask", "Pass1B", "TurnRightMerge",
                                        "Pass2B", "Merge"};
    static const char* const bufs[] = {"src", "dst", "t1", "u1", "t2", "e", "s", "u1b", "d2"};
    static const char* const cuts[] = {"chunk", "run1", "run2"};
    std::string t;
    for (int i = 0; i < P.nsteps; ++i) {
        const AaStep& s = P.step[i];
        std::string planes, writes;
        bool same = true;
        int first = -1;
        for (int p = 0; p < 3; ++p) {
            if (!s.on(p)) continue;
            if (first < 0) first = p;
            planes += std::to_string(p);
            writes += std::string(writes.empty() ? "" : ",") + bufs[s.write[p]];
            same = same && s.write[p] == s.write[first];
        }
        if (same && first >= 0) writes = bufs[s.write[first]];
        t += std::string(i ? " | " : "") + kinds[s.kind] + " " + (planes.empty() ? "-" : planes) + " " + bufs[s.read[0]] +
             (s.read[1] != kAaNoBuf ? std::string("+") + bufs[s.read[1]] : "") + ">" + (writes.empty() ? "-" : writes) + " " + cuts[s.cut] +
             (s.arg ? ":" + std::to_string(s.arg) : "");
    }
    return t;
}

static void expect_steps(const char* what, const AaPlan& P, const char* want)
{
    const std::string got = steps_text(P);
    if (got != want) std::printf("%s:\n  got  %s\n  want %s\n", what, got.c_str(), want), ++failures;
}

// ---- the steps of both fields, written out by hand -----------------------------------------------------------------------------
static void steps()
{
    const sn_aa_fields both = fields_of(SN_AA_FIELDS_BOTH);
    {  // Y8 64x32: every pitch is 256; T1, U1 and U1B are 256 x 64, T2 and D2 256 x 32
        const AaPlan P = plan_of(config(1, 64, 32, 1, 8, 0, 0), &both);
        expect_steps("Y8", P,
                     "TurnLeft 0 src>t1 chunk | Pass1 0 t1>u1 chunk | Pass1B 0 t1>u1b chunk | TurnRightMerge 0 u1+u1b>t2 chunk | Pass2 0 t2>dst chunk | "
                     "Pass2B 0 t2>d2 chunk | Merge 0 d2>dst chunk");
        CHECK(P.nsteps == 7 && P.nsteps <= kAaMaxSteps && kAaMaxSteps >= 10);
        CHECK(aa_frame_bytes(P) == 16384 + 16384 + 16384 + 8192 + 8192);  // five plane sizes where one field takes three
        CHECK(aa_frame_bytes(plan_of(config(1, 64, 32, 1, 8, 0, 0), nullptr)) == 16384 + 16384 + 8192);
        CHECK(aa_buf_needed(P, 0, kAaU1B) && aa_buf_needed(P, 0, kAaD2) && !aa_buf_needed(P, 0, kAaS) && !aa_buf_needed(P, 0, kAaE));
        CHECK(aa_buf_frame_bytes(P, 0, kAaU1B) == 16384 && aa_buf_frame_bytes(P, 0, kAaD2) == 8192);
        CHECK(aa_buf_pitch(P, 0, kAaU1B) == 256 && aa_buf_pitch(P, 0, kAaD2) == 256);
        const int64_t f = 65536;
        CHECK(aa_chunk_frames(P, 2 * f, 5) == 2 && aa_chunk_frames(P, 2 * f - 1, 5) == 1 && aa_chunk_frames(P, 0, 5) == 1 && aa_chunk_frames(P, 9 * f, 5) == 5);
        // the twins: orders 1 and 2, nothing else differs
        CHECK(P.c1.order == 1 && P.c2.order == 1 && P.c1b.order == 2 && P.c2b.order == 2);
        CHECK(P.c1b.width == P.c1.width && P.c1b.height == P.c1.height && P.c2b.width == 64 && P.c2b.height == 32 && P.c1b.max_batch == P.c1.max_batch);
    }
    {  // YUV420P8 64x32, chroma only: luma is in no step and has no intermediate; chroma 32 x 16
        sn_config c = config(3, 64, 32, 1, 8, 1, 1);
        c.luma = 0;
        const AaPlan P = plan_of(c, &both);
        expect_steps("420P8 chroma", P,
                     "TurnLeft 12 src>t1 chunk | Pass1 12 t1>u1 chunk | Pass1B 12 t1>u1b chunk | TurnRightMerge 12 u1+u1b>t2 chunk | Pass2 12 t2>dst chunk | "
                     "Pass2B 12 t2>d2 chunk | Merge 12 d2>dst chunk");
        CHECK(aa_frame_bytes(P) == 2 * (8192 + 8192 + 8192 + 4096 + 4096));
        CHECK(!aa_buf_needed(P, 0, kAaU1B) && !aa_buf_needed(P, 0, kAaD2) && !aa_buf_needed(P, 0, kAaT1));
        // the passes name a buffer for every plane (run_batch wants pointers), the other steps only for theirs
        CHECK(P.step[2].write[0] == kAaU1B && P.step[5].write[0] == kAaD2 && P.step[6].write[0] == kAaNoBuf && P.step[3].write[0] == kAaNoBuf);
    }
    {  // ... every plane, luma sharpened, chroma through luma's mask: the order-1 pass and the average write S for plane 0
        sn_config c = config(3, 64, 32, 1, 8, 1, 1);
        sn_aa_mask m{};
        m.struct_size = (int32_t)sizeof m, m.kind = SN_AA_MASK_SOBEL, m.lo = 16, m.hi = 96, m.expand = 1;
        sn_aa_mask_ex e{};
        e.struct_size = (int32_t)sizeof e, e.chroma = SN_AA_MASK_CHROMA_LUMA;
        sn_aa_sharpen s{};
        s.struct_size = (int32_t)sizeof s, s.amount = 64;
        const AaPlan P = plan_of(c, &both, &m, &e, &s);
        expect_steps("420P8 sharpen + luma mask", P,
                     "TurnLeft 012 src>t1 chunk | Pass1 012 t1>u1 chunk | Pass1B 012 t1>u1b chunk | TurnRightMerge 012 u1+u1b>t2 chunk | "
                     "Pass2 012 t2>s,dst,dst chunk | Pass2B 012 t2>d2 chunk | Merge 012 d2>s,dst,dst chunk | Sharpen 0 src+s>dst chunk:64 | "
                     "MaskLuma 12 src+dst>dst chunk | Mask 0 src+dst>dst chunk");
        CHECK(P.nsteps == 10 && P.nsteps <= kAaMaxSteps);
        CHECK(aa_frame_bytes(P) == (16384 * 3 + 8192 * 2 + 8192) + 2 * (8192 * 3 + 4096 * 2));  // six plane sizes for luma, five for U and V
    }
    // order has no influence on the plan, and no step is cut by parity
    for (int order = 0; order <= 2; ++order) {
        sn_config c = config(1, 64, 32, 1, 8, 0, 0);
        c.order = order;
        const AaPlan P = plan_of(c, &both);
        CHECK(P.c1.order == 1 && P.c2.order == 1 && P.c1b.order == 2 && P.c2b.order == 2);
        for (int i = 0; i < P.nsteps; ++i) CHECK(P.step[i].cut == kAaCutChunk);
        const int32_t parity[4] = {0, 1, 1, 0};
        const FieldRun r = aa_step_run(P, P.step[0], parity, 0, 4);
        CHECK(r.end == 4 && r.offset == -1);
    }
}

// ---- refusals ------------------------------------------------------------------------------------------------------------------
static void refused(int line, const sn_config& c, const sn_aa_options* o, const sn_aa_fields* f, int code, const char* text)
{
    AaOptions opt;
    std::string msg;
    const int rc = aa_check(c, o, nullptr, nullptr, nullptr, f, opt, msg);
    if (rc != code || msg != text) std::printf("line %d: %d \"%s\", expected %d \"%s\"\n", line, rc, msg.c_str(), code, text), ++failures;
}

static void refusals()
{
    const sn_config c = config(1, 64, 32, 1, 8, 0, 0), dh = config(1, 64, 32, 1, 8, 0, 0, 1);
    sn_aa_fields f = fields_of(SN_AA_FIELDS_BOTH);
    f.struct_size = 28;
    refused(__LINE__, c, nullptr, &f, SN_ERR_INVALID_ARG, "sn_aa_fields.struct_size mismatch");
    f.mode = SN_AA_FIELDS_ONE;  // with one field only struct_size is looked at -- and it is
    refused(__LINE__, c, nullptr, &f, SN_ERR_INVALID_ARG, "sn_aa_fields.struct_size mismatch");
    for (int mode : {-1, 2, 77}) {
        f = fields_of(mode);
        refused(__LINE__, c, nullptr, &f, SN_ERR_INVALID_ARG, "sn_aa_fields.mode must be 0 (one) or 1 (both)");
    }
    for (int word = 0; word < 6; ++word) {
        f = fields_of(SN_AA_FIELDS_BOTH);
        f.reserved[word] = 1;
        refused(__LINE__, c, nullptr, &f, SN_ERR_INVALID_ARG, "sn_aa_fields.reserved must be zero");
    }
    f = fields_of(SN_AA_FIELDS_BOTH);
    refused(__LINE__, dh, nullptr, &f, SN_ERR_CONFIG, "SangNomAA: both fields needs dh=false");
    sn_aa_options o{};
    o.struct_size = (int32_t)sizeof o, o.reduce = SN_AA_REDUCE_HALFBAND;
    refused(__LINE__, dh, &o, &f, SN_ERR_CONFIG, "SangNomAA: both fields needs dh=false");  // reduce needs dh, and falls with it
    refused(__LINE__, c, &o, &f, SN_ERR_CONFIG, "SangNomAA: reduce needs dh=true");
    // one field with junk in the other words passes, with and without dh
    f = fields_of(SN_AA_FIELDS_ONE);
    for (int32_t& r : f.reserved) r = -5;
    AaOptions opt;
    std::string msg = "x";
    CHECK(aa_check(c, nullptr, nullptr, nullptr, nullptr, &f, opt, msg) == SN_OK && msg.empty() && opt.fields == SN_AA_FIELDS_ONE);
    CHECK(aa_check(dh, nullptr, nullptr, nullptr, nullptr, &f, opt, msg) == SN_OK && opt.fields == SN_AA_FIELDS_ONE);
    f = fields_of(SN_AA_FIELDS_BOTH);
    CHECK(aa_check(c, nullptr, nullptr, nullptr, nullptr, &f, opt, msg) == SN_OK && opt.fields == SN_AA_FIELDS_BOTH);
}

// ---- fields off: today's plan --------------------------------------------------------------------------------------------------
static bool same_config(const sn_config& a, const sn_config& b)
{
    return a.width == b.width && a.height == b.height && a.bytes_per_sample == b.bytes_per_sample && a.bits_per_sample == b.bits_per_sample &&
           a.num_planes == b.num_planes && a.sub_w == b.sub_w && a.sub_h == b.sub_h && a.order == b.order && a.aa == b.aa && a.aac == b.aac && a.dh == b.dh &&
           a.luma == b.luma && a.chroma == b.chroma && a.max_batch == b.max_batch && a.mode == b.mode && a.host_depth == b.host_depth &&
           a.isolated_planes == b.isolated_planes && a.fresh_pool == b.fresh_pool && a.stream == b.stream;
}

static bool same_plan(const AaPlan& a, const AaPlan& b)
{
    bool same = a.nsteps == b.nsteps && a.planes == b.planes && a.dh == b.dh && a.B == b.B && a.bits == b.bits && a.max_batch == b.max_batch &&
                a.depth == b.depth && a.ring_groups == b.ring_groups && a.per_group == b.per_group && a.inner_batch == b.inner_batch &&
                a.opt.fields == b.opt.fields && a.opt.reduce == b.opt.reduce && a.opt.mask_chroma == b.opt.mask_chroma &&
                a.opt.mask.kind == b.opt.mask.kind && a.opt.sharpen.amount == b.opt.sharpen.amount && same_config(a.c1, b.c1) && same_config(a.c2, b.c2) &&
                aa_frame_bytes(a) == aa_frame_bytes(b);
    for (int i = 0; same && i < a.nsteps; ++i) {
        const AaStep &s = a.step[i], &t = b.step[i];
        same = s.kind == t.kind && s.planes == t.planes && s.cut == t.cut && s.arg == t.arg && !memcmp(s.read, t.read, sizeof s.read) &&
               !memcmp(s.write, t.write, sizeof s.write);
    }
    for (int p = 0; same && p < 3; ++p)
        for (int buf = 0; same && buf < kAaBuffers; ++buf)
            same = aa_buf_needed(a, p, buf) == aa_buf_needed(b, p, buf) && aa_buf_frame_bytes(a, p, buf) == aa_buf_frame_bytes(b, p, buf) &&
                   aa_buf_pitch(a, p, buf) == aa_buf_pitch(b, p, buf);
    return same;
}

// the combinations tests/c/aa_plan_check.cpp walks
static void every_combination()
{
    const sn_config clips[3] = {config(1, 64, 32, 1, 8, 0, 0), config(3, 64, 32, 1, 8, 1, 1), config(3, 64, 32, 1, 8, 0, 0)};
    int accepted = 0, refused_n = 0;
    for (const sn_config& clip : clips)
        for (int bits = 0; bits < 256; ++bits)
            for (int kernel = SN_AA_REDUCE_NONE; kernel <= SN_AA_REDUCE_HALFBAND; ++kernel) {
                sn_config c = clip;
                c.dh = bits & 1, c.luma = (bits >> 1) & 1, c.chroma = (bits >> 2) & 1;
                sn_aa_options o{};
                o.struct_size = (int32_t)sizeof o, o.reduce = kernel;
                sn_aa_mask m{};
                m.struct_size = (int32_t)sizeof m, m.kind = (bits >> 3) & 1, m.lo = 16, m.hi = 96, m.expand = 1;
                sn_aa_mask_ex e{};
                e.struct_size = (int32_t)sizeof e, e.chroma = (bits >> 4) & 1;
                sn_aa_sharpen s{};
                s.struct_size = (int32_t)sizeof s, s.amount = ((bits >> 5) & 1) * 64, s.chroma = (bits >> 6) & 1;
                c.order = (bits >> 7) & 1 ? 0 : 1;
                sn_aa_fields one = fields_of(SN_AA_FIELDS_ONE);
                one.reserved[2] = 123;  // ignored
                AaOptions o7, o8, o1;
                std::string m7, m8, m1;
                const int r7 = aa_check(c, &o, &m, &e, &s, o7, m7);
                const int r8 = aa_check(c, &o, &m, &e, &s, nullptr, o8, m8);
                const int r1 = aa_check(c, &o, &m, &e, &s, &one, o1, m1);
                CHECK(r7 == r8 && r7 == r1 && m7 == m8 && m7 == m1);
                if (r7 != SN_OK) {
                    ++refused_n;
                    continue;
                }
                ++accepted;
                AaPlan P7 = aa_geometry(c, o7), P8 = aa_geometry(c, o8), P1 = aa_geometry(c, o1);
                aa_steps(P7), aa_steps(P8), aa_steps(P1);
                if (!same_plan(P7, P8) || !same_plan(P7, P1)) std::printf("plans differ: %s / %s / %s\n", steps_text(P7).c_str(), steps_text(P8).c_str(), steps_text(P1).c_str()), ++failures;
                // ... and no step or buffer of both fields stands in it
                for (int i = 0; i < P7.nsteps; ++i) CHECK(P7.step[i].kind <= kAaMask);
                for (int p = 0; p < 3; ++p) CHECK(!aa_buf_needed(P7, p, kAaU1B) && !aa_buf_needed(P7, p, kAaD2));
                CHECK(P7.c1.order == c.order && P7.c2.order == c.order);
            }
    CHECK(accepted == 2 * (208 + 204 + 204));  // as there
    CHECK(accepted + refused_n == 3 * 256 * 3);
}

int main()
{
    steps();
    refusals();
    every_combination();
    if (failures) return std::printf("%d failures\n", failures), 1;
    std::printf("ok\n");
    return 0;
}
