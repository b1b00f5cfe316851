// sn_aa_plan.h -- what an anti-aliasing call (sn_aa_*) does, decided once at creation, on the host only (no HIP header and no
// pointers: a host compiler takes this header as it is, tests/c/aa_plan_check.cpp checks it against lines written out by hand).
//   aa_check():    what sn_aa_create_ex7 refuses of its option structs, and the options it keeps.
//   aa_geometry(): every plane size and pitch of the call, the host ring's split and the passes' configurations.
//   AaBuf:         the caller's planes and the intermediates, which of them a plane needs and how large a frame of each is.
//   aa_steps():    the stages of a chunk in order -- which planes, what each reads and writes, how it is cut into launches.
// aa_run (sn_api.hip) executes plan.step[] and decides nothing itself; aa_ensure_intermediates allocates what aa_buf_needed
// names, in chunks of aa_chunk_frames.  The next stage of the call is a step kind here and a case there.
// What a processed plane costs in intermediates, in plane sizes per frame: three (T1, U1, T2); with dh five, with a reduction
// nine; with both fields (sn_aa_fields, never with dh) five (T1, U1, U1B, T2, D2); one more where the plane is sharpened.
#pragma once
#include <stdint.h>

#include <string>

#include "sangnom_hip.h"
#include "sn_surface_plan.h"

namespace sn {

// ---- the options ---------------------------------------------------------------------------------------------------------------
// sn_aa_mask as sn_aa_create_ex3 and sn_mask_merge_device take it: empty when it is fine, otherwise the message, naming the field
inline std::string mask_problem(const sn_aa_mask* m)
{
    if (m->struct_size != (int32_t)sizeof(sn_aa_mask)) return "sn_aa_mask.struct_size mismatch";
    if (m->kind < SN_AA_MASK_NONE || m->kind > SN_AA_MASK_SOBEL) return "sn_aa_mask.kind must be 0 (none) or 1 (Sobel)";
    if (m->kind == SN_AA_MASK_NONE) return "";
    if (m->lo < 0 || m->lo > 255) return "sn_aa_mask.lo must be 0..255";
    if (m->hi < 0 || m->hi > 255) return "sn_aa_mask.hi must be 0..255";
    if (m->lo > m->hi) return "sn_aa_mask.lo must not be above sn_aa_mask.hi";
    if (m->expand < 0 || m->expand > 1) return "sn_aa_mask.expand must be 0 or 1";
    for (int32_t r : m->reserved)
        if (r) return "sn_aa_mask.reserved must be zero";
    return "";
}

// The checked options of a context (what the getters report).
struct AaOptions {
    int reduce = SN_AA_REDUCE_NONE;           // dh only: the second pass's output goes through sn_reduce.hip on its way out
    sn_aa_mask mask{};                        // kind != 0: the result is merged into the source through an edge mask (sn_mask.hip), last
    int mask_chroma = SN_AA_MASK_CHROMA_OWN;  // ... SN_AA_MASK_CHROMA_LUMA: planes 1 and 2 through the source luma plane's mask
    sn_aa_sharpen sharpen{};                  // amount != 0: the result is contra-sharpened (sn_sharpen.hip) behind the last step, before the mask
    int fields = SN_AA_FIELDS_ONE;            // SN_AA_FIELDS_BOTH: every pass twice (order 1, order 2) and the average of the two (sn_merge.hip)
    sn_aa_repair repair{};                    // rank != 0: the result is clamped into the source's 3 x 3 rank range (sn_repair.hip), before the mask
    AaOptions()
    {
        mask.struct_size = (int32_t)sizeof(sn_aa_mask), sharpen.struct_size = (int32_t)sizeof(sn_aa_sharpen);
        repair.struct_size = (int32_t)sizeof(sn_aa_repair);
    }
};

// Every refusal sn_aa_create_ex7 makes of cfg's own fields and of the option structs (NULL: defaults), in the order it makes
// them: SN_OK and `out`, or the code and `msg`.  What the two passes refuse of cfg follows at their creation.
inline int aa_check(const sn_config& cfg, const sn_aa_options* aa_options, const sn_aa_mask* mask, const sn_aa_mask_ex* mask_ex, const sn_aa_sharpen* sharpen,
                    const sn_aa_fields* fields, const sn_aa_repair* repair, AaOptions& out, std::string& msg)
{
    auto refuse = [&msg](int code, const char* text) {
        msg = text;
        return code;
    };
    out = AaOptions();
    if (cfg.struct_size != (int32_t)sizeof(sn_config)) return refuse(SN_ERR_INVALID_ARG, "sn_config.struct_size mismatch");
    if (cfg.max_batch < 0) return refuse(SN_ERR_INVALID_ARG, "max_batch must be >= 0");
    if (cfg.host_depth < 0 || cfg.host_depth > 256) return refuse(SN_ERR_INVALID_ARG, "host_depth must be 0..256");
    if (aa_options) {
        if (aa_options->struct_size != (int32_t)sizeof(sn_aa_options)) return refuse(SN_ERR_INVALID_ARG, "sn_aa_options.struct_size mismatch");
        if (aa_options->reduce < SN_AA_REDUCE_NONE || aa_options->reduce > SN_AA_REDUCE_HALFBAND)
            return refuse(SN_ERR_INVALID_ARG, "sn_aa_options.reduce must be 0 (none), 1 (tent) or 2 (half-band)");
        for (int32_t r : aa_options->reserved)
            if (r) return refuse(SN_ERR_INVALID_ARG, "sn_aa_options.reserved must be zero");
        out.reduce = aa_options->reduce;
    }
    if (out.reduce && !cfg.dh) return refuse(SN_ERR_CONFIG, "SangNomAA: reduce needs dh=true");
    if (mask) {
        msg = mask_problem(mask);
        if (!msg.empty()) return SN_ERR_INVALID_ARG;
        if (mask->kind != SN_AA_MASK_NONE) out.mask = *mask;
    }
    if (out.mask.kind && cfg.dh && !out.reduce)
        return refuse(SN_ERR_CONFIG, "SangNomAA: mask needs the frame at source size (dh=false, or dh=true with reduce)");
    if (mask_ex) {
        if (mask_ex->struct_size != (int32_t)sizeof(sn_aa_mask_ex)) return refuse(SN_ERR_INVALID_ARG, "sn_aa_mask_ex.struct_size mismatch");
        if (out.mask.kind) {  // without a mask the fields below are ignored
            if (mask_ex->chroma < SN_AA_MASK_CHROMA_OWN || mask_ex->chroma > SN_AA_MASK_CHROMA_LUMA)
                return refuse(SN_ERR_INVALID_ARG, "sn_aa_mask_ex.chroma must be 0 (own) or 1 (luma)");
            for (int32_t r : mask_ex->reserved)
                if (r) return refuse(SN_ERR_INVALID_ARG, "sn_aa_mask_ex.reserved must be zero");
            out.mask_chroma = mask_ex->chroma;
        }
    }
    // the source luma plane reaches the device only where it is processed (the host routes upload no other plane)
    if (out.mask_chroma == SN_AA_MASK_CHROMA_LUMA && cfg.num_planes >= 3 && !cfg.dh && !cfg.luma && cfg.chroma)
        return refuse(SN_ERR_CONFIG, "SangNomAA: a luma-derived chroma mask needs luma processed (luma=true)");
    if (sharpen) {
        if (sharpen->struct_size != (int32_t)sizeof(sn_aa_sharpen)) return refuse(SN_ERR_INVALID_ARG, "sn_aa_sharpen.struct_size mismatch");
        if (sharpen->amount < 0 || sharpen->amount > 255) return refuse(SN_ERR_INVALID_ARG, "sn_aa_sharpen.amount must be 0 (off) or 1..255");
        if (sharpen->amount) {  // with amount 0 the fields below it are ignored
            if (sharpen->chroma < 0 || sharpen->chroma > 1) return refuse(SN_ERR_INVALID_ARG, "sn_aa_sharpen.chroma must be 0 or 1");
            for (int32_t r : sharpen->reserved)
                if (r) return refuse(SN_ERR_INVALID_ARG, "sn_aa_sharpen.reserved must be zero");
            out.sharpen.amount = sharpen->amount, out.sharpen.chroma = sharpen->chroma;
        }
    }
    if (out.sharpen.amount && cfg.dh && !out.reduce)
        return refuse(SN_ERR_CONFIG, "SangNomAA: sharpen needs the frame at source size (dh=false, or dh=true with reduce)");
    if (fields) {
        if (fields->struct_size != (int32_t)sizeof(sn_aa_fields)) return refuse(SN_ERR_INVALID_ARG, "sn_aa_fields.struct_size mismatch");
        if (fields->mode != SN_AA_FIELDS_ONE) {  // with one field the words below it are ignored
            if (fields->mode != SN_AA_FIELDS_BOTH) return refuse(SN_ERR_INVALID_ARG, "sn_aa_fields.mode must be 0 (one) or 1 (both)");
            for (int32_t r : fields->reserved)
                if (r) return refuse(SN_ERR_INVALID_ARG, "sn_aa_fields.reserved must be zero");
            out.fields = SN_AA_FIELDS_BOTH;
        }
    }
    // the two dh results place the source on different lines: their average is a half-line blur (reduce needs dh and falls with it)
    if (out.fields == SN_AA_FIELDS_BOTH && cfg.dh) return refuse(SN_ERR_CONFIG, "SangNomAA: both fields needs dh=false");
    if (repair) {
        if (repair->struct_size != (int32_t)sizeof(sn_aa_repair)) return refuse(SN_ERR_INVALID_ARG, "sn_aa_repair.struct_size mismatch");
        if (repair->rank < 0 || repair->rank > 4) return refuse(SN_ERR_INVALID_ARG, "sn_aa_repair.rank must be 0 (off) or 1..4");
        if (repair->rank) {  // with rank 0 the fields below it are ignored
            if (repair->chroma < 0 || repair->chroma > 1) return refuse(SN_ERR_INVALID_ARG, "sn_aa_repair.chroma must be 0 or 1");
            for (int32_t r : repair->reserved)
                if (r) return refuse(SN_ERR_INVALID_ARG, "sn_aa_repair.reserved must be zero");
            out.repair.rank = repair->rank, out.repair.chroma = repair->chroma;
        }
    }
    if (out.repair.rank && cfg.dh && !out.reduce)
        return refuse(SN_ERR_CONFIG, "SangNomAA: repair needs the frame at source size (dh=false, or dh=true with reduce)");
    msg.clear();
    return SN_OK;
}

// ... as sn_aa_create_ex6 makes them: no rank repair
inline int aa_check(const sn_config& cfg, const sn_aa_options* aa_options, const sn_aa_mask* mask, const sn_aa_mask_ex* mask_ex, const sn_aa_sharpen* sharpen,
                    const sn_aa_fields* fields, AaOptions& out, std::string& msg)
{
    return aa_check(cfg, aa_options, mask, mask_ex, sharpen, fields, nullptr, out, msg);
}

// ... as sn_aa_create_ex5 makes them: one field per pass
inline int aa_check(const sn_config& cfg, const sn_aa_options* aa_options, const sn_aa_mask* mask, const sn_aa_mask_ex* mask_ex, const sn_aa_sharpen* sharpen,
                    AaOptions& out, std::string& msg)
{
    return aa_check(cfg, aa_options, mask, mask_ex, sharpen, nullptr, nullptr, out, msg);
}

// ---- buffers and steps ---------------------------------------------------------------------------------------------------------
// Where a plane of a chunk lies: the caller's source and destination, and the intermediates (one per processed plane each).
//   T1  turned: input of the first pass (only its kept lines are written; dh and both fields: every line)
//   U1  turned: its output (dh: twice as high)
//   T2  turned back: input of the second pass (kept lines only; dh: every line, twice as wide; both fields: every line)
//   E   reduce: the second pass's output, opitch x oh
//   S   sharpen: the last step's output of a sharpened plane, dstpitch x dsth
//   U1B both fields: the first pass's order-2 output, as U1
//   D2  both fields: the second pass's order-2 output, dstpitch x dsth (the order-1 output lies where the average goes)
enum AaBuf : int8_t { kAaSrc, kAaDst, kAaT1, kAaU1, kAaT2, kAaE, kAaS, kAaU1B, kAaD2, kAaBuffers, kAaNoBuf = -1 };

enum AaStepKind : int8_t {
    kAaTurnLeft, kAaPass1, kAaTurnRight, kAaPass2, kAaReduce, kAaSharpen, kAaMaskLuma, kAaMask,
    kAaPass1B, kAaTurnRightMerge, kAaPass2B, kAaMerge,  // both fields
    kAaRepair                                           // (appended: no earlier value moves)
};
inline bool aa_is_pass(int kind) { return kind == kAaPass1 || kind == kAaPass2 || kind == kAaPass1B || kind == kAaPass2B; }

// How a step's frames are cut into launches: the chunk in one piece (a turn then writes every line: line parity -1), or one
// launch per run of frames with the same field offset (field_run), the offset being that of the first or the second pass's order.
enum AaCut : int8_t { kAaCutChunk, kAaCutRun1, kAaCutRun2 };

// One stage of a chunk.  Within a step a run's planes come before the next run, the planes in ascending order.
//   TurnLeft / TurnRight / Reduce / Sharpen / Repair / Mask  one launch per run and plane of `planes`: read[] -> write[p]
//   Pass1 / Pass2 / Pass1B / Pass2B   one run_batch for the chunk (B: of the order-2 twin); a plane outside `planes` is not
//                   touched, its pointers only have to be there
//   TurnRightMerge  one launch per plane: the turn of avg(read[0], read[1]) -> write[p]
//   Merge           one launch per plane, in place: write[p] = avg(write[p], read[0])
//   MaskLuma        one launch for planes 1 and 2, which also reads plane 0 of read[0]
struct AaStep {
    int8_t kind = kAaTurnLeft;
    uint8_t planes = 0;  // bit p: the step works on plane p
    int8_t cut = kAaCutChunk;
    int8_t read[2] = {kAaNoBuf, kAaNoBuf};
    int8_t write[3] = {kAaNoBuf, kAaNoBuf, kAaNoBuf};  // per plane
    int32_t arg = 0;  // Reduce: the kernel (SN_AA_REDUCE_*); Sharpen: the amount; Repair: the rank
    bool on(int p) const { return (planes >> p) & 1; }
};
constexpr int kAaMaxSteps = 11;  // both fields + sharpen + repair + luma mask + own mask

// ---- the plan ------------------------------------------------------------------------------------------------------------------
struct AaPlane {
    bool process = false;    // the passes work on it (dh forces every plane); otherwise it is copied from source to destination elsewhere
    bool sharpened = false;  // processed, and plane 0 unless sharpen.chroma
    bool repaired = false;   // processed, and plane 0 unless repair.chroma
    int w = 0, h = 0;        // clip geometry
    int pitch = 0, tpitch = 0;
    int64_t cbytes = 0, tbytes = 0;  // one frame of the plane: clip geometry / turned
    int ow = 0, oh = 0;              // the second pass's output (dh: 2w x 2h)
    int opitch = 0;
    int64_t obytes = 0;
    int64_t u1bytes = 0;  // the first pass's output: tpitch x ow lines
    int t2pitch = 0;      // the second pass's input: ow wide, h high
    int64_t t2bytes = 0;
    int dstw = 0, dsth = 0;  // the destination's geometry: ow x oh, with reduce w x h
    int dstpitch = 0;        // ... of the library's own buffers of that geometry (host groups)
    int64_t dstbytes = 0;
};

struct AaPlan {
    AaOptions opt;
    bool dh = false;
    int B = 1, bits = 8;  // bytes and bits per sample
    int planes = 1;
    int max_batch = 1;
    // the host ring: two groups, so that one group uploads while the other is worked on; a group's frames are one batch
    int depth = 0, ring_groups = 0, per_group = 1;
    int inner_batch = 1;  // max_batch of both passes
    sn_config c1{}, c2{};  // the passes' configurations, stream left null: the turned clip (subsampling swapped), the clip (dh: 2W wide)
    sn_config c1b{}, c2b{};  // both fields: their twins -- c1 and c2 have order 1 then, these order 2, and nothing else differs
    AaPlane plane[3];
    int nsteps = 0;
    AaStep step[kAaMaxSteps];
};

inline AaPlan aa_geometry(const sn_config& cfg, const AaOptions& opt)
{
    AaPlan P;
    P.opt = opt;
    P.dh = cfg.dh != 0;
    P.B = cfg.bytes_per_sample, P.bits = cfg.bits_per_sample;
    P.max_batch = cfg.max_batch > 1 ? cfg.max_batch : 1;
    P.depth = cfg.host_depth > 0 ? cfg.host_depth : 4;
    P.ring_groups = P.depth < 2 ? 1 : 2;
    P.per_group = P.depth / P.ring_groups;
    P.depth = P.ring_groups * P.per_group;
    P.inner_batch = P.max_batch > P.per_group ? P.max_batch : P.per_group;
    P.c1 = cfg;  // TurnLeft: width <-> height, the chroma subsampling turns with it
    P.c1.width = cfg.height;
    P.c1.height = cfg.width;
    P.c1.sub_w = cfg.sub_h;
    P.c1.sub_h = cfg.sub_w;
    P.c2 = cfg;  // TurnRight of the first pass's output: with dh that is twice as wide as the clip
    if (cfg.dh && cfg.width <= INT32_MAX / 2) P.c2.width = 2 * cfg.width;  // (a wider clip: creation refuses it between the passes' own checks)
    for (sn_config* c : {&P.c1, &P.c2}) c->max_batch = P.inner_batch, c->mode = SN_MODE_AUTO, c->stream = nullptr;
    if (opt.fields == SN_AA_FIELDS_BOTH) {  // cfg.order has no influence: the twins are orders 1 and 2, which take no parity
        P.c1.order = P.c2.order = 1;
        P.c1b = P.c1, P.c2b = P.c2;
        P.c1b.order = P.c2b.order = 2;
    }
    P.planes = cfg.num_planes < 3 ? cfg.num_planes : 3;
    const int B = P.B;
    for (int p = 0; p < P.planes; ++p) {
        AaPlane& a = P.plane[p];
        a.process = cfg.dh || plane_selected(cfg, p);  // dh forces every plane, as in the reference (SangNom2.cpp:361-366)
        a.w = p ? cfg.width >> cfg.sub_w : cfg.width;
        a.h = p ? cfg.height >> cfg.sub_h : cfg.height;
        a.pitch = (a.w * B + 255) & ~255;
        a.tpitch = (a.h * B + 255) & ~255;
        a.cbytes = (int64_t)a.pitch * a.h;
        a.tbytes = (int64_t)a.tpitch * a.w;
        a.ow = cfg.dh ? (p ? P.c2.width >> cfg.sub_w : P.c2.width) : a.w;
        a.oh = cfg.dh ? 2 * a.h : a.h;
        a.opitch = (a.ow * B + 255) & ~255;
        a.obytes = (int64_t)a.opitch * a.oh;
        a.u1bytes = (int64_t)a.tpitch * a.ow;
        a.t2pitch = a.opitch;
        a.t2bytes = (int64_t)a.t2pitch * a.h;
        a.dstw = opt.reduce ? a.w : a.ow;
        a.dsth = opt.reduce ? a.h : a.oh;
        a.dstpitch = opt.reduce ? a.pitch : a.opitch;
        a.dstbytes = opt.reduce ? a.cbytes : a.obytes;
        a.sharpened = opt.sharpen.amount && a.process && (p == 0 || opt.sharpen.chroma);
        a.repaired = opt.repair.rank && a.process && (p == 0 || opt.repair.chroma);
    }
    return P;
}

// A plane's own intermediate `buf`: the library allocates it (the caller's planes are the caller's).
inline bool aa_buf_needed(const AaPlan& P, int p, int buf)
{
    const AaPlane& a = P.plane[p];
    if (p >= P.planes || !a.process) return false;  // copied from source to destination: no turn, no pass, no intermediate
    if ((buf == kAaU1B || buf == kAaD2) && P.opt.fields == SN_AA_FIELDS_BOTH) return true;
    return buf == kAaT1 || buf == kAaU1 || buf == kAaT2 || (buf == kAaE && P.opt.reduce) || (buf == kAaS && a.sharpened);
}

// One frame of plane p in `buf`, and its pitch; for the caller's planes what the library's own buffers of that geometry have.
inline int64_t aa_buf_frame_bytes(const AaPlan& P, int p, int buf)
{
    const AaPlane& a = P.plane[p];
    const int64_t nb[kAaBuffers] = {a.cbytes, a.dstbytes, a.tbytes, a.u1bytes, a.t2bytes, a.obytes, a.dstbytes, a.u1bytes, a.dstbytes};
    return nb[buf];
}
inline int aa_buf_pitch(const AaPlan& P, int p, int buf)
{
    const AaPlane& a = P.plane[p];
    const int pitch[kAaBuffers] = {a.pitch, a.dstpitch, a.tpitch, a.tpitch, a.t2pitch, a.opitch, a.dstpitch, a.tpitch, a.dstpitch};
    return pitch[buf];
}

// The intermediates of one frame: nine plane sizes per processed plane with a reduction instead of five (dh), five instead of
// three with both fields, one more per sharpened plane.
inline int64_t aa_frame_bytes(const AaPlan& P)
{
    int64_t per_frame = 0;
    for (int p = 0; p < P.planes; ++p)
        for (int buf = kAaT1; buf < kAaBuffers; ++buf)
            if (aa_buf_needed(P, p, buf)) per_frame += aa_buf_frame_bytes(P, p, buf);
    return per_frame;
}

// The frames of a chunk: what `budget_bytes` of intermediates holds, at least one and at most `frames`.
inline int aa_chunk_frames(const AaPlan& P, int64_t budget_bytes, int frames)
{
    const int64_t per_frame = aa_frame_bytes(P);
    const int64_t fit = per_frame > 0 ? budget_bytes / per_frame : frames;
    return (int)(fit < 1 ? 1 : fit < frames ? fit : frames);
}

// The stages of a chunk, filled once at creation.  Planes that are not processed stay out of every step: the strided call, the
// surface walk and the host staging copy them.
inline void aa_steps(AaPlan& P)
{
    uint8_t processed = 0, sharpened = 0, repaired = 0;
    for (int p = 0; p < P.planes; ++p) {
        processed |= (uint8_t)(P.plane[p].process << p), sharpened |= (uint8_t)(P.plane[p].sharpened << p);
        repaired |= (uint8_t)(P.plane[p].repaired << p);
    }
    P.nsteps = 0;
    auto add = [&P](AaStepKind kind, uint8_t planes, AaCut cut, AaBuf r0, AaBuf r1, AaBuf w) -> AaStep& {
        AaStep& s = P.step[P.nsteps++] = AaStep();
        s.kind = kind, s.planes = planes, s.cut = cut, s.read[0] = r0, s.read[1] = r1;
        for (int p = 0; p < P.planes; ++p)
            if (s.on(p) || aa_is_pass(kind)) s.write[p] = w;
        return s;
    };
    const bool both = P.opt.fields == SN_AA_FIELDS_BOTH;
    // a turn writes the lines its pass keeps: one launch per run of frames with the same field offset, as run_batch cuts them;
    // a dh pass reads every line of its source, and so do the two passes of both fields together: the whole form, one launch
    // for the chunk
    const AaCut turn = P.dh || both ? kAaCutChunk : kAaCutRun1;
    if (processed) add(kAaTurnLeft, processed, turn, kAaSrc, kAaNoBuf, kAaT1);  // the clip's plane -> h wide, w high
    add(kAaPass1, processed, kAaCutChunk, kAaT1, kAaNoBuf, kAaU1);
    if (both) add(kAaPass1B, processed, kAaCutChunk, kAaT1, kAaNoBuf, kAaU1B);
    if (processed && !both) add(kAaTurnRight, processed, turn, kAaU1, kAaNoBuf, kAaT2);
    if (processed && both) add(kAaTurnRightMerge, processed, kAaCutChunk, kAaU1, kAaU1B, kAaT2);  // the average never reaches memory
    // the last step -- the second pass, the reduction, or the average of both fields -- writes the destination, or S where the
    // plane is contra-sharpened
    auto to_last = [&](AaStep& s) {
        for (int p = 0; p < P.planes; ++p)
            if ((sharpened >> p) & 1) s.write[p] = kAaS;
    };
    AaStep& pass2 = add(kAaPass2, processed, kAaCutChunk, kAaT2, kAaNoBuf, P.opt.reduce ? kAaE : kAaDst);
    if (!P.opt.reduce) to_last(pass2);
    if (both) {  // the order-1 pass has written where the average goes: the average runs in place on it
        add(kAaPass2B, processed, kAaCutChunk, kAaT2, kAaNoBuf, kAaD2);
        if (processed) to_last(add(kAaMerge, processed, kAaCutChunk, kAaD2, kAaNoBuf, kAaDst));
    }
    if (P.opt.reduce) {  // (dh: every plane is processed) one launch per run: the field offset is where the source samples lie in E
        AaStep& s = add(kAaReduce, processed, kAaCutRun2, kAaE, kAaNoBuf, kAaDst);
        s.arg = P.opt.reduce;
        to_last(s);
    }
    // the contra-sharpening: the destination from the source and the last step's output
    if (sharpened) add(kAaSharpen, sharpened, kAaCutChunk, kAaSrc, kAaS, kAaDst).arg = P.opt.sharpen.amount;
    // the rank repair: the result so far is clamped into the source's 3 x 3 rank range, in place on the destination (which has
    // the source's size: aa_check has seen to it); no intermediate
    if (repaired) add(kAaRepair, repaired, kAaCutChunk, kAaSrc, kAaDst, kAaDst).arg = P.opt.repair.rank;
    // the edge mask, last: the chunk's result is merged into the source through the source's own mask, in place on the destination
    // (which has the source's size: aa_check has seen to it) -- chroma through the source luma plane's mask: U and V in one launch
    const bool by_luma = P.opt.mask.kind && P.opt.mask_chroma == SN_AA_MASK_CHROMA_LUMA && P.planes == 3 && P.plane[1].process;
    if (by_luma) add(kAaMaskLuma, 6, kAaCutChunk, kAaSrc, kAaDst, kAaDst);
    const uint8_t own = P.opt.mask.kind ? (by_luma ? processed & 1 : processed) : 0;
    if (own) add(kAaMask, own, kAaCutChunk, kAaSrc, kAaDst, kAaDst);
}

// The run of a step's frames that starts at frame g0 of the chunk's m (kAaCutChunk: the chunk, offset -1).
inline FieldRun aa_step_run(const AaPlan& P, const AaStep& s, const int32_t* parity, int g0, int m)
{
    if (s.cut == kAaCutChunk) return FieldRun{m, -1};
    const int order = s.cut == kAaCutRun1 ? P.c1.order : P.c2.order;
    return field_run(parity, g0, m, [order](int q) { return field_offset(order, q); });
}

}  // namespace sn
