// aa_repair_plan_check.cpp -- the rank-repair part of the anti-aliasing call's plan (csrc/sn_aa_plan.h), on the host compiler:
// the steps with sn_aa_repair against lines written out by hand, that the repair step reads the source and the destination
// and writes the destination, that it adds nothing to the intermediates, every refusal of sn_aa_repair, and that rank 0 and
// repair = NULL give the plan of the eight-parameter aa_check, step for step.  Prints "ok" and returns 0, or says what differs.
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

static sn_aa_repair repair_of(int rank, int chroma = 0)
{
    sn_aa_repair r{};
    r.struct_size = (int32_t)sizeof r, r.rank = rank, r.chroma = chroma;
    return r;
}

struct Options {
    const sn_aa_options* o = nullptr;
    const sn_aa_mask* m = nullptr;
    const sn_aa_mask_ex* e = nullptr;
    const sn_aa_sharpen* s = nullptr;
    const sn_aa_fields* f = nullptr;
};

static AaPlan plan_of(const sn_config& c, const Options& k, const sn_aa_repair* r)
{
    AaOptions opt;
    std::string msg;
    const int rc = aa_check(c, k.o, k.m, k.e, k.s, k.f, r, opt, msg);
    if (rc != SN_OK) std::printf("refused (%d): %s\n", rc, msg.c_str()), ++failures;
    AaPlan P = aa_geometry(c, opt);
    aa_steps(P);
    return P;
}

// today's plan: the eight-parameter aa_check, which knows no repair
static AaPlan plan_without(const sn_config& c, const Options& k)
{
    AaOptions opt;
    std::string msg;
    const int rc = aa_check(c, k.o, k.m, k.e, k.s, k.f, opt, msg);
    if (rc != SN_OK) std::printf("refused (%d): %s\n", rc, msg.c_str()), ++failures;
    AaPlan P = aa_geometry(c, opt);
    aa_steps(P);
    return P;
}

// The steps as one line of text: stage, planes, reads>writes (per plane where they differ), cut, :argument.
static std::string steps_text(const AaPlan& P)
{
    static const char* const kinds[] = {"TurnLeft", "Pass1", "TurnRight", "Pass2", "Reduce", "Sharpen", "MaskLuma", "Mask", "Pass1B", "TurnRightMerge",
                                        "Pass2B", "Merge", "Repair"};
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

static bool same_step(const AaStep& s, const AaStep& t)
{
    return s.kind == t.kind && s.planes == t.planes && s.cut == t.cut && s.arg == t.arg && !memcmp(s.read, t.read, sizeof s.read) &&
           !memcmp(s.write, t.write, sizeof s.write);
}

static bool same_plan(const AaPlan& a, const AaPlan& b)
{
    bool same = a.nsteps == b.nsteps && aa_frame_bytes(a) == aa_frame_bytes(b) && a.opt.repair.rank == b.opt.repair.rank;
    for (int i = 0; same && i < a.nsteps; ++i) same = same_step(a.step[i], b.step[i]);
    for (int p = 0; same && p < 3; ++p)
        for (int buf = 0; same && buf < kAaBuffers; ++buf) same = aa_buf_needed(a, p, buf) == aa_buf_needed(b, p, buf);
    return same;
}

// One plan with repair against the line written out by hand, and what holds for every one of them: exactly one repair step
// that reads src and dst and writes dst for its planes only, in one piece, with the rank as its argument; every other step as
// without repair, in the same order; nothing added to the intermediates; rank 0 and NULL: today's plan, step for step.
static void expect(const char* what, const sn_config& c, const Options& k, int rank, int chroma, uint8_t planes, int nsteps, const char* want)
{
    const sn_aa_repair r = repair_of(rank, chroma), off = repair_of(0, 1);
    const AaPlan P = plan_of(c, k, &r), T = plan_without(c, k);
    const std::string got = steps_text(P);
    if (got != want) std::printf("%s:\n  got  %s\n  want %s\n", what, got.c_str(), want), ++failures;
    CHECK(P.nsteps == nsteps && P.nsteps == T.nsteps + 1 && P.nsteps <= kAaMaxSteps);
    CHECK(P.opt.repair.rank == rank && P.opt.repair.chroma == chroma && P.opt.repair.struct_size == 32);
    int at = -1, count = 0;
    for (int i = 0; i < P.nsteps; ++i)
        if (P.step[i].kind == kAaRepair) at = i, ++count;
    CHECK(count == 1);
    if (count != 1) return;
    const AaStep& s = P.step[at];
    CHECK(s.planes == planes && s.cut == kAaCutChunk && s.arg == rank && s.read[0] == kAaSrc && s.read[1] == kAaDst);
    for (int p = 0; p < 3; ++p) {
        CHECK(s.write[p] == (s.on(p) ? kAaDst : kAaNoBuf));
        CHECK(P.plane[p].repaired == s.on(p));
    }
    for (int i = 0; i < T.nsteps; ++i) CHECK(same_step(T.step[i], P.step[i < at ? i : i + 1]));
    // behind the sharpening, before the masks
    for (int i = 0; i < at; ++i) CHECK(P.step[i].kind != kAaMask && P.step[i].kind != kAaMaskLuma);
    for (int i = at + 1; i < P.nsteps; ++i) CHECK(P.step[i].kind == kAaMask || P.step[i].kind == kAaMaskLuma);
    CHECK(aa_frame_bytes(P) == aa_frame_bytes(T));
    for (int p = 0; p < 3; ++p)
        for (int buf = kAaT1; buf < kAaBuffers; ++buf) CHECK(aa_buf_needed(P, p, buf) == aa_buf_needed(T, p, buf));
    CHECK(aa_chunk_frames(P, 1 << 20, 64) == aa_chunk_frames(T, 1 << 20, 64));
    const AaPlan Z = plan_of(c, k, &off), N = plan_of(c, k, nullptr);
    CHECK(same_plan(Z, T) && same_plan(N, T) && Z.opt.repair.rank == 0 && Z.opt.repair.chroma == 0);
    for (int i = 0; i < T.nsteps; ++i) CHECK(T.step[i].kind != kAaRepair);
}

static void steps()
{
    sn_aa_mask m{};
    m.struct_size = (int32_t)sizeof m, m.kind = SN_AA_MASK_SOBEL, m.lo = 16, m.hi = 96, m.expand = 1;
    sn_aa_mask_ex luma{};
    luma.struct_size = (int32_t)sizeof luma, luma.chroma = SN_AA_MASK_CHROMA_LUMA;
    sn_aa_sharpen s{};
    s.struct_size = (int32_t)sizeof s, s.amount = 64;
    sn_aa_options half{};
    half.struct_size = (int32_t)sizeof half, half.reduce = SN_AA_REDUCE_HALFBAND;
    sn_aa_fields both{};
    both.struct_size = (int32_t)sizeof both, both.mode = SN_AA_FIELDS_BOTH;
    {  // repair alone, Y8 without dh
        Options k;
        expect("Y8", config(1, 64, 32, 1, 8, 0, 0), k, 2, 0, 1, 5,
               "TurnLeft 0 src>t1 run1 | Pass1 0 t1>u1 chunk | TurnRight 0 u1>t2 run1 | Pass2 0 t2>dst chunk | Repair 0 src+dst>dst chunk:2");
        CHECK(aa_frame_bytes(plan_of(config(1, 64, 32, 1, 8, 0, 0), k, nullptr)) == 16384 + 16384 + 8192);
    }
    {  // with sharpen and mask: the sharpening writes the destination, the repair runs in place on it, the mask last
        Options k;
        k.m = &m, k.s = &s;
        expect("Y8 sharpen + mask", config(1, 64, 32, 1, 8, 0, 0), k, 1, 0, 1, 7,
               "TurnLeft 0 src>t1 run1 | Pass1 0 t1>u1 chunk | TurnRight 0 u1>t2 run1 | Pass2 0 t2>s chunk | Sharpen 0 src+s>dst chunk:64 | "
               "Repair 0 src+dst>dst chunk:1 | Mask 0 src+dst>dst chunk");
    }
    {  // dh + reduce + chroma = 1 on 4:2:0: every plane is processed and repaired
        Options k;
        k.o = &half;
        expect("420P8 dh + reduce", config(3, 64, 32, 1, 8, 1, 1, 1), k, 3, 1, 7, 6,
               "TurnLeft 012 src>t1 chunk | Pass1 012 t1>u1 chunk | TurnRight 012 u1>t2 chunk | Pass2 012 t2>e chunk | Reduce 012 e>dst run2:2 | "
               "Repair 012 src+dst>dst chunk:3");
        // ... and with chroma = 0 plane 0 alone
        const sn_aa_repair r = repair_of(3, 0);
        const AaPlan P = plan_of(config(3, 64, 32, 1, 8, 1, 1, 1), k, &r);
        CHECK(P.step[5].kind == kAaRepair && P.step[5].planes == 1 && P.plane[0].repaired && !P.plane[1].repaired && !P.plane[2].repaired);
    }
    {  // both fields + sharpen + luma mask + own mask: as many steps as a plan can have
        Options k;
        k.m = &m, k.e = &luma, k.s = &s, k.f = &both;
        expect("420P8 both fields, every stage", config(3, 64, 32, 1, 8, 1, 1), k, 4, 1, 7, 11,
               "TurnLeft 012 src>t1 chunk | Pass1 012 t1>u1 chunk | Pass1B 012 t1>u1b chunk | TurnRightMerge 012 u1+u1b>t2 chunk | "
               "Pass2 012 t2>s,dst,dst chunk | Pass2B 012 t2>d2 chunk | Merge 012 d2>s,dst,dst chunk | Sharpen 0 src+s>dst chunk:64 | "
               "Repair 012 src+dst>dst chunk:4 | MaskLuma 12 src+dst>dst chunk | Mask 0 src+dst>dst chunk");
        CHECK(kAaMaxSteps == 11);
    }
    {  // a plane that is not processed is not repaired: luma = 0 without dh, chroma = 1
        sn_config c = config(3, 64, 32, 1, 8, 1, 1);
        c.luma = 0;
        Options k;
        expect("420P8 chroma only", c, k, 1, 1, 6, 5,
               "TurnLeft 12 src>t1 run1 | Pass1 12 t1>u1 chunk | TurnRight 12 u1>t2 run1 | Pass2 12 t2>dst chunk | Repair 12 src+dst>dst chunk:1");
        // ... and with chroma = 0 nothing is: no step at all
        const sn_aa_repair r = repair_of(1, 0);
        const AaPlan P = plan_of(c, k, &r);
        CHECK(P.nsteps == 4 && P.opt.repair.rank == 1);
    }
    CHECK(kAaRepair == kAaMerge + 1 && kAaMerge == 11 && kAaMask == 7);  // appended: no earlier value moved
}

// ---- refusals ------------------------------------------------------------------------------------------------------------------
static void refused(int line, const sn_config& c, const sn_aa_options* o, const sn_aa_repair* r, int code, const char* text)
{
    AaOptions opt;
    std::string msg;
    const int rc = aa_check(c, o, nullptr, nullptr, nullptr, nullptr, r, opt, msg);
    if (rc != code || msg != text) std::printf("line %d: %d \"%s\", expected %d \"%s\"\n", line, rc, msg.c_str(), code, text), ++failures;
}

static void refusals()
{
    const sn_config c = config(1, 64, 32, 1, 8, 0, 0), dh = config(1, 64, 32, 1, 8, 0, 0, 1);
    sn_aa_repair r = repair_of(2);
    r.struct_size = 28;
    refused(__LINE__, c, nullptr, &r, SN_ERR_INVALID_ARG, "sn_aa_repair.struct_size mismatch");
    r.rank = 0;  // with rank 0 only struct_size is looked at -- and it is
    refused(__LINE__, c, nullptr, &r, SN_ERR_INVALID_ARG, "sn_aa_repair.struct_size mismatch");
    for (int rank : {-1, 5, 77}) {
        r = repair_of(rank);
        refused(__LINE__, c, nullptr, &r, SN_ERR_INVALID_ARG, "sn_aa_repair.rank must be 0 (off) or 1..4");
    }
    for (int chroma : {-1, 2}) {
        r = repair_of(1, chroma);
        refused(__LINE__, c, nullptr, &r, SN_ERR_INVALID_ARG, "sn_aa_repair.chroma must be 0 or 1");
    }
    for (int word = 0; word < 5; ++word) {
        r = repair_of(4);
        r.reserved[word] = 1;
        refused(__LINE__, c, nullptr, &r, SN_ERR_INVALID_ARG, "sn_aa_repair.reserved must be zero");
    }
    for (int rank = 1; rank <= 4; ++rank) {
        r = repair_of(rank, rank & 1);
        refused(__LINE__, dh, nullptr, &r, SN_ERR_CONFIG, "SangNomAA: repair needs the frame at source size (dh=false, or dh=true with reduce)");
    }
    sn_aa_options o{};
    o.struct_size = (int32_t)sizeof o;
    for (int kernel : {SN_AA_REDUCE_TENT, SN_AA_REDUCE_HALFBAND}) {  // with a reduction dh is fine
        o.reduce = kernel;
        AaOptions opt;
        std::string msg = "x";
        r = repair_of(2, 1);
        CHECK(aa_check(dh, &o, nullptr, nullptr, nullptr, nullptr, &r, opt, msg) == SN_OK && msg.empty() && opt.repair.rank == 2 && opt.repair.chroma == 1);
    }
    // rank 0 with junk in the other words passes, with and without dh, and is reported as off
    r = repair_of(0, 7);
    for (int32_t& w : r.reserved) w = -5;
    AaOptions opt;
    std::string msg = "x";
    CHECK(aa_check(c, nullptr, nullptr, nullptr, nullptr, nullptr, &r, opt, msg) == SN_OK && msg.empty() && opt.repair.rank == 0 && opt.repair.chroma == 0);
    CHECK(aa_check(dh, nullptr, nullptr, nullptr, nullptr, nullptr, &r, opt, msg) == SN_OK && opt.repair.rank == 0);
    CHECK(opt.repair.struct_size == (int32_t)sizeof(sn_aa_repair) && sizeof(sn_aa_repair) == 32);
}

int main()
{
    steps();
    refusals();
    if (failures) return std::printf("%d failures\n", failures), 1;
    std::printf("ok\n");
    return 0;
}
