// aa_plan_check.cpp -- csrc/sn_aa_plan.h: the geometry of an anti-aliasing call against numbers written out by hand, its step
// lists against lines written out by hand (from the aa_run the plan replaced: which stage, on which planes, from where to where,
// cut how), invariants of the steps and the buffers over every combination of options the library accepts, the chunk size at the
// budgets where it changes, and every refusal of the option structs with its code and text.
// Stand-alone host program (no device code, no GPU): prints "ok" or what differs.
#include <cstdio>
#include <string>
#include <vector>

#include "sn_aa_plan.h"

static int failures = 0;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            ++failures;                                                  \
        }                                                                \
    } while (0)

using namespace sn;

static sn_config config(int planes, int w, int h, int B, int bits, int sub_w, int sub_h, int dh = 0)
{
    sn_config c{};
    c.struct_size = (int32_t)sizeof(sn_config);
    c.width = w, c.height = h, c.bytes_per_sample = B, c.bits_per_sample = bits, c.num_planes = planes, c.sub_w = sub_w, c.sub_h = sub_h;
    c.order = 1, c.aa = 48, c.dh = dh, c.luma = 1, c.chroma = 1;
    return c;
}
static sn_config yuv420p8(int dh = 0) { return config(3, 64, 32, 1, 8, 1, 1, dh); }

static sn_aa_options reduce_of(int kernel)
{
    sn_aa_options o{};
    o.struct_size = (int32_t)sizeof(o), o.reduce = kernel;
    return o;
}
static sn_aa_mask mask_of(int lo = 16, int hi = 96, int expand = 1, int kind = SN_AA_MASK_SOBEL)
{
    sn_aa_mask m{};
    m.struct_size = (int32_t)sizeof(m), m.kind = kind, m.lo = lo, m.hi = hi, m.expand = expand;
    return m;
}
static sn_aa_mask_ex ex_of(int chroma = SN_AA_MASK_CHROMA_LUMA)
{
    sn_aa_mask_ex e{};
    e.struct_size = (int32_t)sizeof(e), e.chroma = chroma;
    return e;
}
static sn_aa_sharpen sharpen_of(int amount = 64, int chroma = 0)
{
    sn_aa_sharpen s{};
    s.struct_size = (int32_t)sizeof(s), s.amount = amount, s.chroma = chroma;
    return s;
}

// the plan of a clip and its option structs as creation builds it; the structs must pass
static AaPlan plan_of(const sn_config& c, const sn_aa_options* o = nullptr, const sn_aa_mask* m = nullptr, const sn_aa_mask_ex* e = nullptr,
                      const sn_aa_sharpen* s = nullptr)
{
    AaOptions opt;
    std::string msg;
    const int rc = aa_check(c, o, m, e, s, opt, msg);
    if (rc != SN_OK) std::printf("refused (%d): %s\n", rc, msg.c_str()), ++failures;
    AaPlan P = aa_geometry(c, opt);
    aa_steps(P);
    return P;
}

// ---- geometry ------------------------------------------------------------------------------------------------------------------
struct PlaneNumbers {  // in AaPlane's order
    int w, h, pitch, tpitch;
    int64_t cbytes, tbytes;
    int ow, oh, opitch;
    int64_t obytes, u1bytes;
    int t2pitch;
    int64_t t2bytes;
    int dstw, dsth, dstpitch;
    int64_t dstbytes;
};

static void expect_plane(const char* what, const AaPlan& P, int p, const PlaneNumbers& n)
{
    const AaPlane& a = P.plane[p];
    const bool same = a.w == n.w && a.h == n.h && a.pitch == n.pitch && a.tpitch == n.tpitch && a.cbytes == n.cbytes && a.tbytes == n.tbytes && a.ow == n.ow &&
                      a.oh == n.oh && a.opitch == n.opitch && a.obytes == n.obytes && a.u1bytes == n.u1bytes && a.t2pitch == n.t2pitch &&
                      a.t2bytes == n.t2bytes && a.dstw == n.dstw && a.dsth == n.dsth && a.dstpitch == n.dstpitch && a.dstbytes == n.dstbytes;
    if (!same) {
        std::printf("%s, plane %d: %d %d %d %d %lld %lld | %d %d %d %lld %lld | %d %lld | %d %d %d %lld\n", what, p, a.w, a.h, a.pitch, a.tpitch,
                    (long long)a.cbytes, (long long)a.tbytes, a.ow, a.oh, a.opitch, (long long)a.obytes, (long long)a.u1bytes, a.t2pitch, (long long)a.t2bytes,
                    a.dstw, a.dsth, a.dstpitch, (long long)a.dstbytes);
        ++failures;
    }
}

static void geometry()
{
    {  // YUV420P8 64x32: every row of every form is padded to 256 bytes
        const AaPlan P = plan_of(yuv420p8());
        expect_plane("420P8 plain", P, 0, {64, 32, 256, 256, 8192, 16384, 64, 32, 256, 8192, 16384, 256, 8192, 64, 32, 256, 8192});
        for (int p : {1, 2}) expect_plane("420P8 plain", P, p, {32, 16, 256, 256, 4096, 8192, 32, 16, 256, 4096, 8192, 256, 4096, 32, 16, 256, 4096});
        CHECK(P.planes == 3 && P.max_batch == 1 && !P.dh && P.B == 1 && P.bits == 8);
        CHECK(P.depth == 4 && P.ring_groups == 2 && P.per_group == 2 && P.inner_batch == 2);  // host_depth 0: four slots in two groups
        CHECK(P.c1.width == 32 && P.c1.height == 64 && P.c1.sub_w == 1 && P.c1.sub_h == 1 && P.c1.max_batch == 2 && P.c1.mode == SN_MODE_AUTO);
        CHECK(P.c2.width == 64 && P.c2.height == 32 && P.c2.max_batch == 2 && P.c2.mode == SN_MODE_AUTO && !P.c1.stream && !P.c2.stream);
        CHECK(P.plane[0].process && P.plane[1].process && P.plane[2].process && !P.plane[0].sharpened);
        CHECK(aa_frame_bytes(P) == (16384 + 16384 + 8192) + 2 * (8192 + 8192 + 4096));
    }
    {  // ... with dh: the first pass's output twice as high, the second pass 128 wide and its output 128 x 64
        const AaPlan P = plan_of(yuv420p8(1));
        expect_plane("420P8 dh", P, 0, {64, 32, 256, 256, 8192, 16384, 128, 64, 256, 16384, 32768, 256, 8192, 128, 64, 256, 16384});
        for (int p : {1, 2}) expect_plane("420P8 dh", P, p, {32, 16, 256, 256, 4096, 8192, 64, 32, 256, 8192, 16384, 256, 4096, 64, 32, 256, 8192});
        CHECK(P.dh && P.c1.width == 32 && P.c1.height == 64 && P.c1.dh == 1 && P.c2.width == 128 && P.c2.height == 32 && P.c2.dh == 1);
        CHECK(aa_frame_bytes(P) == (16384 + 32768 + 8192) + 2 * (8192 + 16384 + 4096));
    }
    {  // ... and a reduction: the same intermediates and E, the destination of source size again
        const sn_aa_options o = reduce_of(SN_AA_REDUCE_HALFBAND);
        const AaPlan P = plan_of(yuv420p8(1), &o);
        expect_plane("420P8 dh reduce", P, 0, {64, 32, 256, 256, 8192, 16384, 128, 64, 256, 16384, 32768, 256, 8192, 64, 32, 256, 8192});
        for (int p : {1, 2}) expect_plane("420P8 dh reduce", P, p, {32, 16, 256, 256, 4096, 8192, 64, 32, 256, 8192, 16384, 256, 4096, 32, 16, 256, 4096});
        CHECK(P.opt.reduce == SN_AA_REDUCE_HALFBAND && P.c2.width == 128);
        CHECK(aa_frame_bytes(P) == (16384 + 32768 + 8192 + 16384) + 2 * (8192 + 16384 + 4096 + 8192));
    }
    {  // YUV422P16 72x40, dh and a reduction: no pitch is the row's bytes, and the turn swaps the subsampling (chroma 36 x 40)
        sn_config c = config(3, 72, 40, 2, 16, 1, 0, 1);
        c.max_batch = 6, c.host_depth = 5;
        const sn_aa_options o = reduce_of(SN_AA_REDUCE_TENT);
        const AaPlan P = plan_of(c, &o);
        expect_plane("422P16 dh reduce", P, 0, {72, 40, 256, 256, 10240, 18432, 144, 80, 512, 40960, 36864, 512, 20480, 72, 40, 256, 10240});
        for (int p : {1, 2}) expect_plane("422P16 dh reduce", P, p, {36, 40, 256, 256, 10240, 9216, 72, 80, 256, 20480, 18432, 256, 10240, 36, 40, 256, 10240});
        CHECK(P.c1.width == 40 && P.c1.height == 72 && P.c1.sub_w == 0 && P.c1.sub_h == 1);
        CHECK(P.c2.width == 144 && P.c2.height == 40 && P.c2.sub_w == 1 && P.c2.sub_h == 0);
        CHECK(P.max_batch == 6 && P.depth == 4 && P.ring_groups == 2 && P.per_group == 2 && P.inner_batch == 6 && P.c1.max_batch == 6 && P.c2.max_batch == 6);
        CHECK(P.B == 2 && P.bits == 16);
        // what the library's own buffers of each kind hold, and their pitches
        CHECK(aa_buf_frame_bytes(P, 0, kAaSrc) == 10240 && aa_buf_frame_bytes(P, 0, kAaDst) == 10240 && aa_buf_frame_bytes(P, 0, kAaT1) == 18432);
        CHECK(aa_buf_frame_bytes(P, 0, kAaU1) == 36864 && aa_buf_frame_bytes(P, 0, kAaT2) == 20480 && aa_buf_frame_bytes(P, 0, kAaE) == 40960);
        CHECK(aa_buf_frame_bytes(P, 0, kAaS) == 10240);
        CHECK(aa_buf_pitch(P, 0, kAaSrc) == 256 && aa_buf_pitch(P, 0, kAaDst) == 256 && aa_buf_pitch(P, 0, kAaT1) == 256 && aa_buf_pitch(P, 0, kAaU1) == 256);
        CHECK(aa_buf_pitch(P, 0, kAaT2) == 512 && aa_buf_pitch(P, 0, kAaE) == 512 && aa_buf_pitch(P, 0, kAaS) == 256 && aa_buf_pitch(P, 1, kAaE) == 256);
    }
    {  // the ring's split: one slot is one group, an odd depth loses a slot, a group larger than max_batch sets the passes' batch
        sn_config c = yuv420p8();
        c.host_depth = 1;
        AaPlan P = plan_of(c);
        CHECK(P.depth == 1 && P.ring_groups == 1 && P.per_group == 1 && P.inner_batch == 1);
        c.host_depth = 9, c.max_batch = 3;
        P = plan_of(c);
        CHECK(P.depth == 8 && P.ring_groups == 2 && P.per_group == 4 && P.inner_batch == 4 && P.max_batch == 3);
    }
    {  // planes that are not selected: processed only with dh; a width whose double does not fit is left for creation to refuse
        sn_config c = yuv420p8();
        c.chroma = 0;
        AaPlan P = plan_of(c);
        CHECK(P.plane[0].process && !P.plane[1].process && !P.plane[2].process && aa_frame_bytes(P) == 16384 + 16384 + 8192);
        c.dh = 1;
        P = plan_of(c);
        CHECK(P.plane[0].process && P.plane[1].process && P.plane[2].process);
        c.width = INT32_MAX / 2 + 1;
        CHECK(aa_geometry(c, AaOptions()).c2.width == c.width);
    }
}

// ---- steps ---------------------------------------------------------------------------------------------------------------------
// The steps as one line of text: stage, planes, reads>writes (per plane where they differ), cut, :argument.
static std::string aa_steps_text(const AaPlan& P)
{
    static const char* const kinds[] = {"TurnLeft", "Pass1", "TurnRight", "Pass2", "Reduce", "Sharpen", "MaskLuma", "Mask"};
    static const char* const bufs[] = {"src", "dst", "t1", "u1", "t2", "e", "s"};
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
    const std::string got = aa_steps_text(P);
    if (got != want) {
        std::printf("%s:\n  got  %s\n  want %s\n", what, got.c_str(), want);
        ++failures;
    }
}

static void steps()
{
    const sn_aa_options half = reduce_of(SN_AA_REDUCE_HALFBAND), tent = reduce_of(SN_AA_REDUCE_TENT);
    const sn_aa_mask mask = mask_of();
    const sn_aa_mask_ex by_luma = ex_of();
    const sn_aa_sharpen luma_only = sharpen_of(64, 0), every_plane = sharpen_of(64, 1);
    // the turns write the lines the next pass keeps: per run of the first pass's field offsets
    expect_steps("plain", plan_of(yuv420p8()), "TurnLeft 012 src>t1 run1 | Pass1 012 t1>u1 chunk | TurnRight 012 u1>t2 run1 | Pass2 012 t2>dst chunk");
    // a dh pass reads every line: the whole chunk in one launch
    expect_steps("dh", plan_of(yuv420p8(1)), "TurnLeft 012 src>t1 chunk | Pass1 012 t1>u1 chunk | TurnRight 012 u1>t2 chunk | Pass2 012 t2>dst chunk");
    // the second pass fills E; the reduction is cut by the second pass's field offsets
    expect_steps("dh reduce", plan_of(yuv420p8(1), &half),
                 "TurnLeft 012 src>t1 chunk | Pass1 012 t1>u1 chunk | TurnRight 012 u1>t2 chunk | Pass2 012 t2>e chunk | Reduce 012 e>dst run2:2");
    expect_steps("mask", plan_of(yuv420p8(), nullptr, &mask),
                 "TurnLeft 012 src>t1 run1 | Pass1 012 t1>u1 chunk | TurnRight 012 u1>t2 run1 | Pass2 012 t2>dst chunk | Mask 012 src+dst>dst chunk");
    // a sharpened plane: the last step writes S, the sharpening the destination; the other planes go straight there
    expect_steps("sharpen luma, mask", plan_of(yuv420p8(), nullptr, &mask, nullptr, &luma_only),
                 "TurnLeft 012 src>t1 run1 | Pass1 012 t1>u1 chunk | TurnRight 012 u1>t2 run1 | Pass2 012 t2>s,dst,dst chunk | Sharpen 0 src+s>dst chunk:64 | "
                 "Mask 012 src+dst>dst chunk");
    // every stage: the reduction is the last step, chroma goes through luma's mask in one launch and luma through its own
    expect_steps("dh reduce, sharpen all, mask by luma", plan_of(yuv420p8(1), &tent, &mask, &by_luma, &every_plane),
                 "TurnLeft 012 src>t1 chunk | Pass1 012 t1>u1 chunk | TurnRight 012 u1>t2 chunk | Pass2 012 t2>e chunk | Reduce 012 e>s run2:1 | "
                 "Sharpen 012 src+s>dst chunk:64 | MaskLuma 12 src+dst>dst chunk | Mask 0 src+dst>dst chunk");
    {  // the same without dh (so without the reduction) and with luma = 0: plane 0 is in no step, and no Mask step follows MaskLuma.
        // (aa_check refuses this combination -- the host routes never upload the luma plane -- so the options are set by hand.)
        sn_config c = yuv420p8();
        c.luma = 0;
        AaOptions opt;
        std::string msg;
        CHECK(aa_check(c, nullptr, &mask, &by_luma, &every_plane, opt, msg) == SN_ERR_CONFIG);
        opt.mask = mask, opt.mask_chroma = SN_AA_MASK_CHROMA_LUMA, opt.sharpen = every_plane;
        AaPlan P = aa_geometry(c, opt);
        aa_steps(P);
        expect_steps("luma off, sharpen all, mask by luma", P,
                     "TurnLeft 12 src>t1 run1 | Pass1 12 t1>u1 chunk | TurnRight 12 u1>t2 run1 | Pass2 12 t2>s chunk | Sharpen 12 src+s>dst chunk:64 | "
                     "MaskLuma 12 src+dst>dst chunk");
        CHECK(!aa_buf_needed(P, 0, kAaT1) && !aa_buf_needed(P, 0, kAaS) && aa_buf_needed(P, 1, kAaS));
        // ... and with chroma's own mask, which aa_check accepts: one Mask step, planes 1 and 2
        expect_steps("luma off, sharpen all, own masks", plan_of(c, nullptr, &mask, nullptr, &every_plane),
                     "TurnLeft 12 src>t1 run1 | Pass1 12 t1>u1 chunk | TurnRight 12 u1>t2 run1 | Pass2 12 t2>s chunk | Sharpen 12 src+s>dst chunk:64 | "
                     "Mask 12 src+dst>dst chunk");
    }
    {  // nothing selected: the two passes still see the batch (they count its frames), nothing else runs and nothing is allocated
        sn_config c = yuv420p8();
        c.luma = c.chroma = 0;
        const AaPlan P = plan_of(c, nullptr, &mask, nullptr, &every_plane);
        expect_steps("nothing processed", P, "Pass1 - t1>- chunk | Pass2 - t2>- chunk");
        CHECK(aa_frame_bytes(P) == 0);
    }
    // how a step is cut: the chunk with offset -1, or runs of the first / the second pass's order
    {
        sn_config c = yuv420p8();
        c.order = 0;
        const AaPlan P = plan_of(c);
        const int32_t par[5] = {1, 1, 0, 0, 1};
        FieldRun r = aa_step_run(P, P.step[0], par, 0, 5);  // TurnLeft
        CHECK(r.end == 2 && r.offset == 0);
        r = aa_step_run(P, P.step[0], par, 2, 5);
        CHECK(r.end == 4 && r.offset == 1);
        r = aa_step_run(P, P.step[0], par, 4, 5);
        CHECK(r.end == 5 && r.offset == 0);
        r = aa_step_run(P, P.step[0], nullptr, 1, 5);  // no parity array: parity 1 throughout
        CHECK(r.end == 5 && r.offset == 0);
        r = aa_step_run(P, P.step[1], par, 0, 5);  // Pass1: the chunk
        CHECK(r.end == 5 && r.offset == -1);
        c.order = 2, c.dh = 1;
        const AaPlan Q = plan_of(c, &half);
        r = aa_step_run(Q, Q.step[4], par, 0, 5);  // Reduce, keep bottom: one run
        CHECK(Q.step[4].kind == kAaReduce && r.end == 5 && r.offset == 1);
        r = aa_step_run(Q, Q.step[0], par, 0, 5);  // a dh turn: the chunk
        CHECK(r.end == 5 && r.offset == -1);
    }
}

// ---- invariants ----------------------------------------------------------------------------------------------------------------
static void invariants(const AaPlan& P, const std::string& what)
{
    auto fail = [&](const char* why) {
        std::printf("%s: %s: %s\n", why, what.c_str(), aa_steps_text(P).c_str());
        ++failures;
    };
    if (P.nsteps > kAaMaxSteps) fail("too many steps");
    bool written[3][kAaBuffers] = {}, named[3][kAaBuffers] = {}, read_later[3][kAaBuffers] = {};
    for (int i = 0; i < P.nsteps; ++i) {
        const AaStep& s = P.step[i];
        const bool masks = s.kind == kAaMask || s.kind == kAaMaskLuma;
        for (int p = 0; p < 3; ++p) {
            if (!s.on(p)) continue;
            if (p >= P.planes || !P.plane[p].process) fail("a plane that is not processed stands in a step");
            for (int8_t buf : s.read) {
                if (buf == kAaNoBuf) continue;
                if (buf != kAaSrc && !written[p][buf]) fail("a step reads what no earlier step of the chunk wrote on that plane");
                if (buf == kAaDst && !masks) fail("a step other than the masks reads the destination");
                named[p][buf] = read_later[p][buf] = true;
            }
            if (s.write[p] == kAaNoBuf || s.write[p] == kAaSrc) fail("a step writes nowhere, or the source");
            else written[p][s.write[p]] = named[p][s.write[p]] = true, read_later[p][s.write[p]] = false;
        }
        if (s.kind == kAaMaskLuma && (s.planes != 6 || P.planes != 3)) fail("MaskLuma on planes other than 1 and 2");  // (it reads plane 0 of the source)
        if ((s.kind == kAaSharpen || masks) && s.read[0] != kAaSrc) fail("sharpening and masks take the source first");
        if ((s.cut != kAaCutChunk) != (s.kind == kAaReduce || (!P.dh && (s.kind == kAaTurnLeft || s.kind == kAaTurnRight)))) fail("cut");
    }
    int64_t sum = 0;
    for (int p = 0; p < 3; ++p) {
        if (p < P.planes && P.plane[p].process && !written[p][kAaDst]) fail("a processed plane never reaches the destination");
        for (int buf = kAaT1; buf < kAaBuffers; ++buf) {
            if (aa_buf_needed(P, p, buf) != named[p][buf]) fail("an intermediate needed but in no step, or in a step but not needed");
            if (read_later[p][buf] != written[p][buf]) fail("an intermediate written and never read");
            if (aa_buf_needed(P, p, buf)) sum += aa_buf_frame_bytes(P, p, buf);
        }
        if (aa_buf_needed(P, p, kAaSrc) || aa_buf_needed(P, p, kAaDst)) fail("the caller's planes are not the library's to allocate");
    }
    // the chunk is the budget over that sum
    if (sum != aa_frame_bytes(P)) fail("frame bytes");
    if (sum > 0 && (aa_chunk_frames(P, 3 * sum, 1000) != 3 || aa_chunk_frames(P, 3 * sum - 1, 1000) != 2 || aa_chunk_frames(P, sum - 1, 1000) != 1))
        fail("the chunk is not the budget over the needed buffers' bytes");
    if (sum == 0 && aa_chunk_frames(P, 0, 1000) != 1000) fail("no intermediates: the chunk is the batch");
}

static void every_combination()
{
    const sn_config clips[3] = {config(1, 64, 32, 1, 8, 0, 0), config(3, 64, 32, 1, 8, 1, 1), config(3, 64, 32, 1, 8, 0, 0)};
    int accepted = 0, refused = 0;
    for (const sn_config& clip : clips)
        for (int bits = 0; bits < 256; ++bits)
            for (int kernel = SN_AA_REDUCE_NONE; kernel <= SN_AA_REDUCE_HALFBAND; ++kernel) {
                sn_config c = clip;
                c.dh = bits & 1, c.luma = (bits >> 1) & 1, c.chroma = (bits >> 2) & 1;
                const sn_aa_options o = reduce_of(kernel);
                const sn_aa_mask m = mask_of(16, 96, 1, (bits >> 3) & 1);
                const sn_aa_mask_ex e = ex_of((bits >> 4) & 1);
                const sn_aa_sharpen s = sharpen_of(((bits >> 5) & 1) * 64, (bits >> 6) & 1);
                c.order = (bits >> 7) & 1 ? 0 : 1;
                AaOptions opt;
                std::string msg;
                if (aa_check(c, &o, &m, &e, &s, opt, msg) != SN_OK) {
                    ++refused;
                    continue;
                }
                ++accepted;
                AaPlan P = aa_geometry(c, opt);
                aa_steps(P);
                invariants(P, "planes " + std::to_string(c.num_planes) + " sub " + std::to_string(c.sub_w) + " dh " + std::to_string(c.dh) + " luma " +
                                  std::to_string(c.luma) + " chroma " + std::to_string(c.chroma));
            }
    // per clip, order and the flags a refusal does not look at aside: without dh no reduction, 2^6 combinations of (mask, mask
    // chroma, amount, sharpen chroma, luma, chroma), less the 4 a 3-plane clip is refused for a luma-derived mask without luma;
    // with dh and no reduction neither mask nor sharpening, 2^4; with dh and either reduction all 2^6: 208 for Y, 204 for YUV
    CHECK(accepted == 2 * (208 + 204 + 204));
    CHECK(accepted + refused == 3 * 256 * 3);
}

// ---- chunks --------------------------------------------------------------------------------------------------------------------
static void chunks()
{
    const sn_aa_options o = reduce_of(SN_AA_REDUCE_HALFBAND);
    const AaPlan P = plan_of(yuv420p8(1), &o);
    const int64_t f = 147456;  // geometry(): 73728 for luma, 36864 for U and for V
    CHECK(aa_frame_bytes(P) == f);
    CHECK(aa_chunk_frames(P, 0, 5) == 1);  // at least one frame, whatever the budget
    CHECK(aa_chunk_frames(P, f - 1, 5) == 1 && aa_chunk_frames(P, f, 5) == 1);
    CHECK(aa_chunk_frames(P, 2 * f - 1, 5) == 1 && aa_chunk_frames(P, 2 * f, 5) == 2);
    CHECK(aa_chunk_frames(P, 5 * f - 1, 5) == 4 && aa_chunk_frames(P, 5 * f, 5) == 5);
    CHECK(aa_chunk_frames(P, 100 * f, 5) == 5);  // never more than asked for
    sn_config c = yuv420p8();
    c.luma = c.chroma = 0;  // no plane is processed: no intermediates, the chunk is the batch
    CHECK(aa_chunk_frames(plan_of(c), 0, 7) == 7);
}

// ---- refusals ------------------------------------------------------------------------------------------------------------------
static void refused(int line, const sn_config& c, const sn_aa_options* o, const sn_aa_mask* m, const sn_aa_mask_ex* e, const sn_aa_sharpen* s, int code,
                    const char* text)
{
    AaOptions opt;
    std::string msg;
    const int rc = aa_check(c, o, m, e, s, opt, msg);
    if (rc != code || msg != text) {
        std::printf("%s:%d: got (%d) \"%s\", want (%d) \"%s\"\n", __FILE__, line, rc, msg.c_str(), code, text);
        ++failures;
    }
}
#define REFUSED(...) refused(__LINE__, __VA_ARGS__)

static void refusals()
{
    const sn_config plain = yuv420p8(), dh = yuv420p8(1);
    const char* const at_source_size[2] = {"SangNomAA: mask needs the frame at source size (dh=false, or dh=true with reduce)",
                                           "SangNomAA: sharpen needs the frame at source size (dh=false, or dh=true with reduce)"};
    // sn_config's own fields
    sn_config c = plain;
    c.struct_size -= 4;
    REFUSED(c, nullptr, nullptr, nullptr, nullptr, SN_ERR_INVALID_ARG, "sn_config.struct_size mismatch");
    c = plain, c.max_batch = -1;
    REFUSED(c, nullptr, nullptr, nullptr, nullptr, SN_ERR_INVALID_ARG, "max_batch must be >= 0");
    for (int depth : {-1, 257}) {
        c = plain, c.host_depth = depth;
        REFUSED(c, nullptr, nullptr, nullptr, nullptr, SN_ERR_INVALID_ARG, "host_depth must be 0..256");
    }
    // sn_aa_options
    sn_aa_options o = reduce_of(SN_AA_REDUCE_TENT);
    REFUSED(plain, &o, nullptr, nullptr, nullptr, SN_ERR_CONFIG, "SangNomAA: reduce needs dh=true");
    for (int kernel : {3, -1}) {
        o = reduce_of(kernel);
        REFUSED(dh, &o, nullptr, nullptr, nullptr, SN_ERR_INVALID_ARG, "sn_aa_options.reduce must be 0 (none), 1 (tent) or 2 (half-band)");
    }
    for (int word = 0; word < 6; ++word) {
        o = reduce_of(SN_AA_REDUCE_TENT), o.reserved[word] = 1;
        REFUSED(dh, &o, nullptr, nullptr, nullptr, SN_ERR_INVALID_ARG, "sn_aa_options.reserved must be zero");
    }
    o = reduce_of(SN_AA_REDUCE_TENT), o.struct_size -= 4;
    REFUSED(dh, &o, nullptr, nullptr, nullptr, SN_ERR_INVALID_ARG, "sn_aa_options.struct_size mismatch");
    // sn_aa_mask
    sn_aa_mask m;
    for (int size : {28, 0}) {
        m = mask_of(), m.struct_size = size;
        REFUSED(plain, nullptr, &m, nullptr, nullptr, SN_ERR_INVALID_ARG, "sn_aa_mask.struct_size mismatch");
    }
    for (int kind : {2, -1}) {
        m = mask_of(16, 96, 1, kind);
        REFUSED(plain, nullptr, &m, nullptr, nullptr, SN_ERR_INVALID_ARG, "sn_aa_mask.kind must be 0 (none) or 1 (Sobel)");
    }
    m = mask_of(-1);
    REFUSED(plain, nullptr, &m, nullptr, nullptr, SN_ERR_INVALID_ARG, "sn_aa_mask.lo must be 0..255");
    m = mask_of(256, 256);
    REFUSED(plain, nullptr, &m, nullptr, nullptr, SN_ERR_INVALID_ARG, "sn_aa_mask.lo must be 0..255");
    m = mask_of(16, 256);
    REFUSED(plain, nullptr, &m, nullptr, nullptr, SN_ERR_INVALID_ARG, "sn_aa_mask.hi must be 0..255");
    m = mask_of(0, -1);
    REFUSED(plain, nullptr, &m, nullptr, nullptr, SN_ERR_INVALID_ARG, "sn_aa_mask.hi must be 0..255");
    m = mask_of(97, 96);
    REFUSED(plain, nullptr, &m, nullptr, nullptr, SN_ERR_INVALID_ARG, "sn_aa_mask.lo must not be above sn_aa_mask.hi");
    for (int expand : {2, -1}) {
        m = mask_of(16, 96, expand);
        REFUSED(plain, nullptr, &m, nullptr, nullptr, SN_ERR_INVALID_ARG, "sn_aa_mask.expand must be 0 or 1");
    }
    for (int word = 0; word < 3; ++word) {
        m = mask_of(), m.reserved[word] = 1;
        REFUSED(plain, nullptr, &m, nullptr, nullptr, SN_ERR_INVALID_ARG, "sn_aa_mask.reserved must be zero");
    }
    m = mask_of();
    REFUSED(dh, nullptr, &m, nullptr, nullptr, SN_ERR_CONFIG, at_source_size[0]);
    // sn_aa_mask_ex
    sn_aa_mask_ex e;
    for (int size : {28, 0}) {
        e = ex_of(), e.struct_size = size;
        REFUSED(plain, nullptr, &m, &e, nullptr, SN_ERR_INVALID_ARG, "sn_aa_mask_ex.struct_size mismatch");
    }
    for (int chroma : {2, -1}) {
        e = ex_of(chroma);
        REFUSED(plain, nullptr, &m, &e, nullptr, SN_ERR_INVALID_ARG, "sn_aa_mask_ex.chroma must be 0 (own) or 1 (luma)");
    }
    for (int word = 0; word < 6; ++word) {
        e = ex_of(), e.reserved[word] = 1;
        REFUSED(plain, nullptr, &m, &e, nullptr, SN_ERR_INVALID_ARG, "sn_aa_mask_ex.reserved must be zero");
    }
    e = ex_of();
    c = plain, c.luma = 0;
    REFUSED(c, nullptr, &m, &e, nullptr, SN_ERR_CONFIG, "SangNomAA: a luma-derived chroma mask needs luma processed (luma=true)");
    // sn_aa_sharpen
    sn_aa_sharpen s;
    for (int size : {28, 0}) {
        s = sharpen_of(), s.struct_size = size;
        REFUSED(plain, nullptr, nullptr, nullptr, &s, SN_ERR_INVALID_ARG, "sn_aa_sharpen.struct_size mismatch");
    }
    for (int amount : {-1, 256}) {
        s = sharpen_of(amount);
        REFUSED(plain, nullptr, nullptr, nullptr, &s, SN_ERR_INVALID_ARG, "sn_aa_sharpen.amount must be 0 (off) or 1..255");
    }
    for (int chroma : {2, -1}) {
        s = sharpen_of(64, chroma);
        REFUSED(plain, nullptr, nullptr, nullptr, &s, SN_ERR_INVALID_ARG, "sn_aa_sharpen.chroma must be 0 or 1");
    }
    for (int word = 0; word < 5; ++word) {
        s = sharpen_of(), s.reserved[word] = 1;
        REFUSED(plain, nullptr, nullptr, nullptr, &s, SN_ERR_INVALID_ARG, "sn_aa_sharpen.reserved must be zero");
    }
    for (int chroma : {0, 1}) {
        s = sharpen_of(64, chroma);
        REFUSED(dh, nullptr, nullptr, nullptr, &s, SN_ERR_CONFIG, at_source_size[1]);
    }

    // ---- ignored when off: a mask of kind 0, mask_ex without a mask, a sharpening of amount 0 -- but for a bad struct_size
    AaOptions opt;
    std::string msg = "stale";
    m = mask_of(999, -5, 7, SN_AA_MASK_NONE), m.reserved[1] = 3;
    e = ex_of(7), e.reserved[2] = 1;
    s = sharpen_of(0, 7), s.reserved[3] = 9;
    CHECK(aa_check(dh, nullptr, &m, &e, &s, opt, msg) == SN_OK && msg.empty());
    CHECK(opt.reduce == 0 && opt.mask.kind == 0 && opt.mask.lo == 0 && opt.mask_chroma == SN_AA_MASK_CHROMA_OWN && opt.sharpen.amount == 0 && opt.sharpen.chroma == 0);
    CHECK(opt.mask.struct_size == (int32_t)sizeof(sn_aa_mask) && opt.sharpen.struct_size == (int32_t)sizeof(sn_aa_sharpen));  // (what the getters hand out)
    CHECK(aa_check(dh, nullptr, nullptr, &e, nullptr, opt, msg) == SN_OK);
    e.struct_size = 28;
    REFUSED(plain, nullptr, nullptr, &e, nullptr, SN_ERR_INVALID_ARG, "sn_aa_mask_ex.struct_size mismatch");
    REFUSED(plain, nullptr, &m, &e, nullptr, SN_ERR_INVALID_ARG, "sn_aa_mask_ex.struct_size mismatch");
    s.struct_size = 28;
    REFUSED(plain, nullptr, nullptr, nullptr, &s, SN_ERR_INVALID_ARG, "sn_aa_sharpen.struct_size mismatch");
    // what is kept of structs that pass
    o = reduce_of(SN_AA_REDUCE_HALFBAND), m = mask_of(8, 32, 0), e = ex_of(), s = sharpen_of(200, 1);
    CHECK(aa_check(dh, &o, &m, &e, &s, opt, msg) == SN_OK);
    CHECK(opt.reduce == 2 && opt.mask.kind == 1 && opt.mask.lo == 8 && opt.mask.hi == 32 && opt.mask.expand == 0 && opt.mask_chroma == 1);
    CHECK(opt.sharpen.amount == 200 && opt.sharpen.chroma == 1);
    // luma off and a luma-derived mask: fine with dh (every plane is processed), on a Y clip, and where chroma is off too
    c = dh, c.luma = 0;
    CHECK(aa_check(c, &o, &m, &e, nullptr, opt, msg) == SN_OK);
    c = config(1, 64, 32, 1, 8, 0, 0), c.luma = 0;
    CHECK(aa_check(c, nullptr, &m, &e, nullptr, opt, msg) == SN_OK);
    c = plain, c.luma = 0, c.chroma = 0;
    CHECK(aa_check(c, nullptr, &m, &e, nullptr, opt, msg) == SN_OK);

    // ---- of two faults the earlier one is reported
    o = reduce_of(7), s = sharpen_of(999);
    REFUSED(dh, &o, nullptr, nullptr, &s, SN_ERR_INVALID_ARG, "sn_aa_options.reduce must be 0 (none), 1 (tent) or 2 (half-band)");
    m = mask_of(), s = sharpen_of();
    REFUSED(dh, nullptr, &m, nullptr, &s, SN_ERR_CONFIG, at_source_size[0]);
    e = ex_of(5);  // the mask's source-size rule comes before mask_ex's fields are looked at, reduce's dh rule before the mask is
    REFUSED(dh, nullptr, &m, &e, nullptr, SN_ERR_CONFIG, at_source_size[0]);
    o = reduce_of(SN_AA_REDUCE_TENT), m = mask_of(300);
    REFUSED(plain, &o, &m, nullptr, nullptr, SN_ERR_CONFIG, "SangNomAA: reduce needs dh=true");
}

int main()
{
    geometry();
    steps();
    every_combination();
    chunks();
    refusals();
    if (failures == 0) std::printf("ok\n");
    return failures ? 1 : 0;
}
