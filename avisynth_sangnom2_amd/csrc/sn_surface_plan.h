// sn_surface_plan.h -- what a surface call does, decided once, on the host only (no HIP header and no pointers: a host compiler
// takes this header as it is, tests/c/surface_plan_check.cpp checks it against lines written out by hand).
//   surface_plan(): from the two sides' layouts and what the context processes to the scratch parts the call needs, the launches
//   that turn the source into planar LSB-aligned planes, where the passes read and write, and the launches that finish the
//   destination.  surface_walk (sn_api.hip) executes a plan and decides nothing itself; surface_scratch allocates plan.need.
//   field_run(): a batch cut into runs of frames with the same field offset; field_offset() and plane_selected(): what a clip's
//   configuration says of a frame's field and of a plane (here so that every host-only header has the one definition).
#pragma once
#include <stdint.h>

#include <string>

#include "sangnom_hip.h"

namespace sn {

// ---- fields and planes ---------------------------------------------------------------------------------------------------------
// GetFrame's field choice, SangNom2.cpp:336-341.
inline int field_offset(int order, int parity)
{
    switch (order) {
    case 0: return parity ? 0 : 1;
    case 1: return 0;
    default: return 1;
    }
}

// processPlane[p]: cfg.luma / cfg.chroma select the plane (dh forces every plane on top of this: ClipPlan::enabled)
inline bool plane_selected(const sn_config& cfg, int p) { return p == 0 ? cfg.luma != 0 : cfg.chroma != 0; }

// ---- runs of frames ------------------------------------------------------------------------------------------------------------
// The run of frames with the same field offset that starts at frame f of [0, m): parity == nullptr means parity 1 for every
// frame, offset_of(parity) is the field offset.  extend == false: the run is that one frame, whatever follows (run_batch on a
// history-carrying clip without a chain).
struct FieldRun {
    int end;     // one past the run's last frame
    int offset;  // the run's field offset
};

template <class OffsetOf>
inline FieldRun field_run(const int32_t* parity, int f, int m, OffsetOf offset_of, bool extend = true)
{
    FieldRun r{f + 1, offset_of(parity ? parity[f] : 1)};
    while (extend && r.end < m && offset_of(parity ? parity[r.end] : 1) == r.offset) ++r.end;
    return r;
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------
struct PlanSide {  // of a checked sn_surfaces (sn_surface_layout.h)
    bool semi;
    int packing;  // sn::Packing
    int shift;    // zero bits below every sample (an _MSB layout on a clip of fewer than 16 bits), else 0
};

// What a call needs of the scratch (UvScratch): U and V in the source's / the destination's geometry, luma likewise.
struct SurfaceNeeds {
    bool in = false, out = false;
    bool y = false, yo = false;
};

// Where a plane lies: plane idx of the caller's source or destination, or a scratch part (kIn / kOut: idx 0 = U, 1 = V).
enum PlanBuf : int8_t { kBufSrc, kBufDst, kBufIn, kBufOut, kBufY, kBufYo };
struct PlaneRef {
    int8_t buf = kBufSrc, idx = 0;
    bool live = false;  // the passes touch it; otherwise the pointer only has to be there
};

// One launch (kOpCopy: one 2-D copy per frame).  Which planes it reads and writes follows from the stage it stands in:
//   once    caller's source -> caller's destination, every frame of the call, every line, shifts (ss, ds)
//   source  caller's source -> read[], per run of frames with the same field offset, the run's kept lines or every line, (ss, 0)
//   after   result[] -> caller's destination, per chunk, every line, (0, ds)
// kOpShift16 / kOpCopy / kOpCopyOrShift16 move plane `plane`; kOpUvSplit reads plane 1 and writes planes 1 and 2, kOpUvMerge the
// reverse; kOpUnpack reads plane 0 and writes all three, kOpPack the reverse.
enum PlanOp : int8_t {
    kOpCopy,           // 2-D copies
    kOpCopyOrShift16,  // 16-bit samples: shift16 (which also shifts up); 8-bit: 2-D copies
    kOpShift16,
    kOpUvSplit,
    kOpUvMerge,
    kOpUnpack,
    kOpPack,
};
struct PlanStep {
    int8_t op = kOpCopy, plane = 0;
    bool uv_row = false;  // the UV plane moved as one plane of 2 w samples a row
};

enum PlanCount : int8_t { kCountNever, kCountPerCall, kCountPerChunk };  // a counter advances by the call's / the chunk's frames

struct SurfacePlan {
    SurfaceNeeds need;
    int nonce = 0, nsource = 0, nafter = 0;
    PlanStep once[3];    // before the chunks: planes that reach neither a pass nor scratch
    bool chunked = false;  // chunks of what the scratch holds; otherwise the batch in one piece
    PlanStep source[3];  // per run: the source as planar LSB-aligned planes
    bool source_all_lines = true;  // ... in every line and one run per chunk; otherwise the lines each run's passes keep
    PlaneRef read[3], write[3];    // the passes' planes
    PlaneRef result[3];  // after the passes: where each plane's planar LSB-aligned result lies (write[], or read[] if not processed)
    PlanStep after[4];   // per chunk: the destination finished from result[]
    int8_t count_split = kCountNever, count_merged = kCountNever, count_copied = kCountNever;  // sn_surface_info
};

// luma_processed / chroma_processed: the passes work on that plane; all_lines: they read every line of their source.
// A call without a packed side sends planes that are not processed from source to destination once, before the chunks, and never
// through scratch.  With a packed side every plane goes through its planar form: the source is brought in every line as soon as a
// plane is not processed, and that plane leaves from where the source's planar form lies.
inline SurfacePlan surface_plan(const PlanSide& src, const PlanSide& dst, int planes, bool luma_processed, bool chroma_processed, bool all_lines)
{
    SurfacePlan P;
    const int ss = src.shift, ds = dst.shift;
    const bool lp = luma_processed, cp = chroma_processed, chroma = planes >= 3;
    const bool packed = src.packing || dst.packing, msb = ss != 0 || ds != 0;
    auto processed = [&](int p) { return p == 0 ? lp : chroma && cp; };
    // a plane has a planar form of its own in this call: the passes work on it, or the call has a packed side
    const bool y_planar = lp || packed, c_planar = chroma && (cp || packed);
    // ... which lies in scratch where the caller's plane is not it
    const bool y_in = y_planar && (src.packing || ss != 0), c_in = c_planar && (src.packing || src.semi || ss != 0);
    const bool y_out = dst.packing != 0, c_out = c_planar && (dst.packing || dst.semi);

    // before the chunks
    auto add = [](PlanStep* list, int& n, PlanOp op, int plane, bool uv_row = false) { list[n++] = PlanStep{(int8_t)op, (int8_t)plane, uv_row}; };
    if (chroma && !c_planar) {
        if (src.semi && dst.semi) add(P.once, P.nonce, msb ? kOpShift16 : kOpCopy, 1, true);  // (ss == ds: only the low bits go)
        else if (src.semi) add(P.once, P.nonce, kOpUvSplit, 1);
        else if (dst.semi) add(P.once, P.nonce, kOpUvMerge, 1);
        else add(P.once, P.nonce, kOpShift16, 1), add(P.once, P.nonce, kOpShift16, 2);  // planar on both sides, one of them MSB-aligned
    }
    if (!y_planar && msb) add(P.once, P.nonce, kOpShift16, 0);  // (otherwise the passes copy luma they do not process)

    // the source
    if (src.packing) {
        add(P.source, P.nsource, kOpUnpack, 0);
    } else {
        if (y_in) add(P.source, P.nsource, kOpShift16, 0);
        if (c_in && src.semi) add(P.source, P.nsource, kOpUvSplit, 1);
        else if (c_in) add(P.source, P.nsource, kOpShift16, 1), add(P.source, P.nsource, kOpShift16, 2);
    }
    P.source_all_lines = all_lines || (packed && !(lp && cp));

    // the passes.  Planes they leave alone: without a packed side the caller's plane 0 stands in, with one they point where
    // the plane would lie if it were processed
    for (int p = 0; p < 3; ++p) {
        const bool live = p == 0 ? lp || !(msb || packed) : processed(p);
        const bool in = p == 0 ? y_in : c_in, out = p == 0 ? y_out : c_out;
        const int8_t own = (int8_t)(p == 0 || c_planar ? p : 0);
        P.read[p] = in ? PlaneRef{(int8_t)(p == 0 ? kBufY : kBufIn), (int8_t)(p == 0 ? 0 : p - 1), live} : PlaneRef{kBufSrc, own, live};
        P.write[p] = out ? PlaneRef{(int8_t)(p == 0 ? kBufYo : kBufOut), (int8_t)(p == 0 ? 0 : p - 1), live} : PlaneRef{kBufDst, own, live};
        P.result[p] = processed(p) ? P.write[p] : P.read[p];
    }

    // the destination
    if (dst.packing) {
        add(P.after, P.nafter, kOpPack, 0);
    } else {
        if (c_out && !packed) add(P.after, P.nafter, kOpUvMerge, 1);
        for (int p = 0; p < planes && p < 3; ++p) {
            if (p > 0 && (dst.semi || !c_planar)) continue;  // the merge's, or gone before the chunks
            if (processed(p) ? ds != 0 : packed) add(P.after, P.nafter, processed(p) ? kOpShift16 : kOpCopyOrShift16, p);  // (shifted up in place)
        }
        if (c_out && packed) add(P.after, P.nafter, kOpUvMerge, 1);
    }

    // scratch is what the plan touches; without a packed side both chroma geometries, as ever
    P.need.y = y_in, P.need.yo = y_out;
    P.need.in = packed ? c_in : c_in || c_out;
    P.need.out = packed ? c_out : c_in || c_out;
    P.chunked = packed || P.need.in || P.need.y;

    if (c_in && (src.packing || src.semi)) P.count_split = kCountPerChunk;
    if (c_out) P.count_merged = kCountPerChunk;
    if (chroma && !cp) P.count_copied = packed ? kCountPerChunk : kCountPerCall;
    return P;
}

// The plan as one line of text (the check program's; nothing on the library's hot path calls it).
inline std::string surface_plan_text(const SurfacePlan& P)
{
    static const char* const ops[] = {"copy", "copy|shift16", "shift16", "uv_split", "uv_merge", "unpack", "pack"};
    static const char* const bufs[] = {"src", "dst", "in", "out", "y", "yo"};
    static const char* const counts[] = {"-", "call", "chunk"};
    auto steps = [&](const PlanStep* list, int n) {
        std::string s;
        for (int i = 0; i < n; ++i)
            s += std::string(i ? "," : "") + ops[list[i].op] + ":" + std::to_string(list[i].plane) + (list[i].uv_row ? "x2" : "");
        return s.empty() ? std::string("-") : s;
    };
    auto refs = [&](const PlaneRef* r, bool with_live) {
        std::string s;
        for (int p = 0; p < 3; ++p) {
            s += std::string(p ? "," : "") + bufs[r[p].buf];
            if (r[p].buf != kBufY && r[p].buf != kBufYo) s += std::to_string(r[p].idx);
            if (with_live && !r[p].live) s += "~";
        }
        return s;
    };
    std::string need;
    if (P.need.in) need += "in ";
    if (P.need.out) need += "out ";
    if (P.need.y) need += "y ";
    if (P.need.yo) need += "yo ";
    if (need.empty()) need = "- ";
    return "need " + need + "| once " + steps(P.once, P.nonce) + " | " + (P.chunked ? "chunks" : "whole") + " | source " + steps(P.source, P.nsource) +
           (P.nsource ? (P.source_all_lines ? " all" : " kept") : "") + " | read " + refs(P.read, true) + " | write " + refs(P.write, true) + " | after " +
           steps(P.after, P.nafter) + " from " + refs(P.result, false) + " | split " + counts[P.count_split] + " merged " + counts[P.count_merged] +
           " copied " + counts[P.count_copied];
}

}  // namespace sn
