// sangnom2_filter.hpp -- the SangNom2 filter object over the C ABI (include/sangnom_hip.h).
//
// Host-side mirror of the reference's class SangNom2 : GenericVideoFilter
// (/root/reference/src/SangNom2.h:40-67): same constructor arguments and defaults as
// Create_SangNom2 (src/SangNom2.cpp:399-435), same error text, GetFrame(n) with the same
// observable result (src/SangNom2.cpp:332-397).  All pixel work is done by libsangnom_hip.so:
// GetFrame hands the source planes to sn_process_host and receives the assembled output frame
// (kept field, border line, interpolated lines) in the destination planes.
//
// With Args::lookahead > 1 GetFrame(n) keeps frames n .. n+lookahead-1 in flight on the library's host ring
// (sn_submit_host / sn_collect_host): it requests the child's next frames ahead of the
// caller, so their transfers and sweeps overlap; a request out of sequence drains the ring and restarts there.
//
// The class is a template over a host-traits type so that the same code serves the real AviSynth+
// SDK (host/sangnom2_avs_plugin.cpp) and this repository's test host (host/sn_host_api.h).
#pragma once

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>

#include "sangnom_hip.h"

namespace sangnom {

struct Args {  // SangNom2(clip, order, aa, aac, threads, dh, luma, chroma, opt)
    int order = 1;
    int aa = 48;
    int aac = 0;
    int threads = 0;  // dummy in the reference too (README.md:40-41)
    bool dh = false;
    bool luma = true;
    bool chroma = true;
    int opt = -1;     // the reference's CPU code-path switch: 1 = its SSE2 arithmetic (SN_ARITH_SSE2), 0 and -1 = its C++ arithmetic
    int device = 0;   // HIP device ordinal (not a script argument)
    int lookahead = -1;  // frames in flight behind GetFrame; -1: $SANGNOM_LOOKAHEAD or 1 (synchronous)
    bool isolated = false;  // extension: every plane filtered as a Y clip of its own (sn_config.isolated_planes)
    bool fresh = false;     // extension: ... and every frame by a new instance (sn_config.fresh_pool)
    int reduce = 0;         // SangNomAA only, with dh: SN_AA_REDUCE_TENT / SN_AA_REDUCE_HALFBAND, the frame comes back at source size
    bool mask = false;      // SangNomAA only, at source size: the result is merged into the source through the source's Sobel edge mask
    int mask_lo = 8, mask_hi = 32, mask_expand = 1;  // ... sn_aa_mask.lo / hi / expand; starting values, not tuned on real footage
    bool mask_luma = false;  // ... chroma through the source luma plane's mask (sn_aa_mask_ex.chroma = SN_AA_MASK_CHROMA_LUMA), as the scripts do
    int sharpen = 0;         // SangNomAA only, at source size: contra-sharpening behind the last step, sn_aa_sharpen.amount (0 off, 1..255, 64 = unity)
    bool sharpen_chroma = false;  // ... of every processed plane, not of plane 0 alone (sn_aa_sharpen.chroma)
    bool both_fields = false;  // SangNomAA only, without dh: every pass interpolates both fields and averages (sn_aa_fields.mode = SN_AA_FIELDS_BOTH)
    int repair = 0;            // SangNomAA only, at source size: rank repair behind the sharpening, sn_aa_repair.rank (0 off, 1..4)
    bool repair_chroma = false;  // ... of every processed plane, not of plane 0 alone (sn_aa_repair.chroma)
    int column_parts = -1;  // sn_options.column_parts (16-bit / float planes wider than 3840 in column parts); -1: $SANGNOM_COLUMN_PARTS or 0
    sn_policy policy{};     // scheduling only (sangnom_hip.h); zeros = the defaults
};

// Args::column_parts, or the environment's word for it (read here, by the host adapter: the library reads no environment)
inline int column_parts_of(const Args& a)
{
    if (a.column_parts >= 0) return a.column_parts;
    const char* e = std::getenv("SANGNOM_COLUMN_PARTS");
    return e ? std::atoi(e) : 0;
}

template <class Host>
class Filter {
public:
    using Env = typename Host::Env;
    using ClipPtr = typename Host::ClipPtr;
    using FramePtr = typename Host::FramePtr;
    using Info = typename Host::Info;

    // Create_SangNom2's checks, in its order, with its text (src/SangNom2.cpp:407-422); `name`
    // is "SangNom2" or "SangNom" (the legacy wrapper reports under its own name, :446-459).
    Filter(ClipPtr child, const Args& a, Env* env, const char* name = "SangNom2") : child_(child), args_(a)
    {
        vi_ = Host::GetInfo(child);
        const std::string n(name);
        if (Host::IsRGB(vi_) || !Host::IsPlanar(vi_)) env->ThrowError("%s: clip must be in Y/YUV planar format.", name);
        if (Host::Height(vi_) % 2 != 0) env->ThrowError("%s: height must be even.", name);
        if (Host::Is420(vi_) && Host::Height(vi_) % 4) env->ThrowError("%s: height must be mod4.", name);
        if (a.order < 0 || a.order > 2) env->ThrowError("%s: order must be between 0..2.", name);
        if (a.aa < 0 || a.aa > 128) env->ThrowError("%s: aa must be between 0..128.", name);
        if (n != "SangNom" && (a.aac < 0 || a.aac > 128)) env->ThrowError("%s: aac must be between 0..128.", name);
        if (a.opt < -1 || a.opt > 1) env->ThrowError("%s: opt must be between -1..2.", name);  // sic

        sn_config c{};
        c.struct_size = (int32_t)sizeof c;
        c.width = Host::Width(vi_);
        c.height = Host::Height(vi_);
        c.bytes_per_sample = Host::ComponentSize(vi_);
        c.bits_per_sample = Host::BitsPerComponent(vi_);
        c.num_planes = std::min(Host::NumComponents(vi_), 3);
        c.sub_w = c.num_planes > 1 ? Host::SubW(vi_) : 0;
        c.sub_h = c.num_planes > 1 ? Host::SubH(vi_) : 0;
        c.order = a.order;
        c.aa = a.aa;
        c.aac = a.aac;
        c.dh = a.dh;
        c.luma = a.luma;
        c.chroma = a.chroma;
        c.device = a.device;
        c.max_batch = 1;
        c.mode = SN_MODE_AUTO;
        int la = a.lookahead;
        if (la < 0) {
            const char* e = std::getenv("SANGNOM_LOOKAHEAD");
            la = e ? std::atoi(e) : 1;
        }
        c.host_depth = std::max(1, std::min(la, 256));
        c.isolated_planes = a.isolated ? 1 : 0;
        c.fresh_pool = a.fresh ? 1 : 0;
        sn_policy pol = a.policy;
        pol.struct_size = (int32_t)sizeof pol;
        sn_options opts{};
        opts.struct_size = (int32_t)sizeof opts;
        opts.arithmetic = a.opt == 1 ? SN_ARITH_SSE2 : SN_ARITH_CXX;
        opts.column_parts = column_parts_of(a);
        const int rc = sn_create_ex(&c, &pol, &opts, &ctx_);
        if (rc != SN_OK) env->ThrowError("%s: %s", name, sn_last_error(nullptr));
        if (a.dh) Host::SetHeight(vi_, Host::Height(vi_) * 2);  // src/SangNom2.cpp:284-285
        planes_ = c.num_planes;
        alpha_ = Host::NumComponents(vi_) == 4;
        num_frames_ = Host::NumFrames(vi_);
        // look-ahead processes frames the caller may never ask for; where results depend on the order of
        // processing (history-carrying configurations) GetFrame therefore stays synchronous
        sn_info info{};
        info.struct_size = (int32_t)sizeof info;
        const bool ahead = c.host_depth > 1 && sn_get_info(ctx_, &info) == SN_OK && info.history_free;
        slots_ = ahead ? sn_host_slots(ctx_) : 1;
    }
    Filter(const Filter&) = delete;
    Filter& operator=(const Filter&) = delete;
    ~Filter()
    {
        inflight_.clear();  // frames still in the ring are dropped with the context
        sn_destroy(ctx_);
    }

    const Info& GetInfo() const { return vi_; }

    // SangNom2::GetFrame, src/SangNom2.cpp:332-397.
    FramePtr GetFrame(int n, Env* env)
    {
        if (slots_ > 1) return GetFrameAhead(n, env);
        FramePtr src = Host::GetFrame(child_, n, env);
        FramePtr dst = Host::NewFrame(env, vi_, src);
        const void* sp[3] = {nullptr, nullptr, nullptr};
        void* dp[3] = {nullptr, nullptr, nullptr};
        int32_t spitch[3] = {0, 0, 0}, dpitch[3] = {0, 0, 0};
        for (int p = 0; p < planes_; ++p) {
            sp[p] = Host::ReadPtr(src, p);
            dp[p] = Host::WritePtr(dst, p);
            spitch[p] = Host::Pitch(src, p);
            dpitch[p] = Host::Pitch(dst, p);
        }
        const int parity = args_.order == 0 ? (Host::GetParity(child_, n) ? 1 : 0) : 1;
        if (sn_process_host(ctx_, sp, spitch, dp, dpitch, parity) != SN_OK)
            env->ThrowError("SangNom2: %s", sn_last_error(ctx_));
        CopyAlpha(src, dst);
        return dst;
    }

    // One instance per host thread, like the reference (src/SangNom2.h:63-66): a context owns its
    // stream, device pool and staging buffers.
    static constexpr bool kMultiInstance = true;

private:
    struct Pending {
        int n;
        FramePtr src, dst;  // src is held until its planes have been staged (submit copies them at once)
        int32_t slot;
    };

    void Planes(const FramePtr& src, const FramePtr& dst, const void* sp[3], int32_t spitch[3], void* dp[3], int32_t dpitch[3])
    {
        for (int p = 0; p < planes_; ++p) {
            if (src) { sp[p] = Host::ReadPtr(src, p); spitch[p] = Host::Pitch(src, p); }
            if (dst) { dp[p] = Host::WritePtr(dst, p); dpitch[p] = Host::Pitch(dst, p); }
        }
    }

    // EXTENSION: the reference never writes a fourth plane (src/SangNom2.cpp:346-348 stops at
    // min(NumComponents, 3)), so the alpha of a YUVA clip comes out as whatever the new frame held.  Here it is passed
    // through: copied line by line, and with dh every source line fills two output lines.
    void CopyAlpha(const FramePtr& src, const FramePtr& dst) const
    {
        if (!alpha_) return;
        const uint8_t* s = Host::ReadPtr(src, 3);
        uint8_t* d = Host::WritePtr(dst, 3);
        const int sp = Host::Pitch(src, 3), dp = Host::Pitch(dst, 3);
        const size_t row = (size_t)Host::Width(vi_) * Host::ComponentSize(vi_);
        const int h_out = Host::Height(vi_);
        for (int y = 0; y < h_out; ++y) std::memcpy(d + (size_t)y * dp, s + (size_t)(args_.dh ? y / 2 : y) * sp, row);
    }

    FramePtr Collect(Env* env)
    {
        Pending p = inflight_.front();
        inflight_.pop_front();
        const void* sp[3] = {nullptr, nullptr, nullptr};
        void* dp[3] = {nullptr, nullptr, nullptr};
        int32_t spitch[3] = {0, 0, 0}, dpitch[3] = {0, 0, 0};
        Planes(FramePtr(), p.dst, sp, spitch, dp, dpitch);
        if (sn_collect_host(ctx_, p.slot, dp, dpitch) != SN_OK) env->ThrowError("SangNom2: %s", sn_last_error(ctx_));
        return p.dst;
    }

    FramePtr GetFrameAhead(int n, Env* env)
    {
        if (inflight_.empty() || inflight_.front().n != n) {  // not the frame at the head: start over at n
            while (!inflight_.empty()) Collect(env);
            next_ = n;
        }
        while ((int)inflight_.size() < slots_ && next_ < num_frames_) {
            Pending p;
            p.n = next_++;
            p.src = Host::GetFrame(child_, p.n, env);
            p.dst = Host::NewFrame(env, vi_, p.src);
            const void* sp[3] = {nullptr, nullptr, nullptr};
            void* dp[3] = {nullptr, nullptr, nullptr};
            int32_t spitch[3] = {0, 0, 0}, dpitch[3] = {0, 0, 0};
            Planes(p.src, FramePtr(), sp, spitch, dp, dpitch);
            const int parity = args_.order == 0 ? (Host::GetParity(child_, p.n) ? 1 : 0) : 1;
            if (sn_submit_host(ctx_, sp, spitch, parity, &p.slot) != SN_OK) env->ThrowError("SangNom2: %s", sn_last_error(ctx_));
            CopyAlpha(p.src, p.dst);
            // p.src stays referenced until the slot is collected: a source plane that lies in pinned memory is read by
            // the device straight from the host's frame, asynchronously (sn_submit_host, sangnom_hip.h)
            inflight_.push_back(p);
        }
        if (inflight_.empty()) env->ThrowError("SangNom2: frame %d is outside the clip", n);
        return Collect(env);
    }

    std::deque<Pending> inflight_;
    int next_ = 0;
    int num_frames_ = 0;
    int slots_ = 1;
    ClipPtr child_;
    Args args_;
    Info vi_{};
    sn_context* ctx_ = nullptr;
    int planes_ = 1;
    bool alpha_ = false;
};

// SangNomAA(clip, order, aa, aac): the anti-aliasing idiom TurnLeft().SangNom2(order, aa, aac).TurnRight().SangNom2(order,
// aa, aac) as one filter over sn_aa_process_host -- the frame crosses PCIe once each way instead of four times
// (README.md:3 of the reference: "mainly used in anti-aliasing scripts").  Same checks and messages
// as SangNom2 for the clip itself; the turned clip must pass them as well (e.g. an even WIDTH).
// Args::lookahead works as in Filter, over sn_aa_submit_host / sn_aa_collect_host, and only when BOTH passes are
// history-free (sn_aa_get_info); otherwise GetFrame stays synchronous, for the reason given in Filter's constructor.
// With Args::dh both passes run with dh=true: TurnLeft().SangNom2(dh=true).TurnRight().SangNom2(dh=true), enlargement by
// two in both directions.  The filter's clip is then twice as wide and twice as high, every plane is processed (luma /
// chroma are ignored, as in the reference), and the alpha of a YUVA clip fills a 2 x 2 block per source sample.
// With Args::reduce (1 tent, 2 half-band; needs dh) the library reduces the enlarged frame on the device, centred on the
// source samples (sangnom_hip.h, "Anti-aliasing at source size"): the filter's clip is the source's again -- a drop-in
// anti-aliaser --, a frame of source size comes down, and the alpha passes through 1:1.
// With Args::mask (the clip at source size: no dh, or dh with reduce) the library merges the result into the source through
// a Sobel edge mask of the source (sangnom_hip.h, "Edge mask"; mask_lo <= mask_hi in 0..255, mask_expand 0 or 1), which is
// what the anti-aliasing scripts do behind the filter: flat areas and texture keep the source's samples.  Args::mask_luma
// merges chroma through the luma plane's mask reduced to chroma's geometry instead of chroma's own (needs luma processed).
// With Args::sharpen (1..255, 64 = unity; the clip at source size) the library contra-sharpens the result behind the last
// step and before the mask (sangnom_hip.h, "Contra-sharpening"): plane 0, or with Args::sharpen_chroma every processed plane.
// With Args::both_fields (without dh) every pass runs for order 1 and for order 2 and the library averages the two results
// (sangnom_hip.h, "Both fields"), as daa and its relatives do: Args::order and the frames' parity then have no influence.
// With Args::repair (1..4; the clip at source size) the library clamps each sample of the result into the range of the
// repair-th smallest and repair-th largest of the nine source samples around it (sangnom_hip.h, "Rank repair"), behind the
// sharpening and before the mask: plane 0, or with Args::repair_chroma every processed plane.
template <class Host>
class AAFilter {
public:
    using Env = typename Host::Env;
    using ClipPtr = typename Host::ClipPtr;
    using FramePtr = typename Host::FramePtr;
    using Info = typename Host::Info;

    AAFilter(ClipPtr child, const Args& a, Env* env, const char* name = "SangNomAA") : child_(child), args_(a)
    {
        vi_ = Host::GetInfo(child);
        if (Host::IsRGB(vi_) || !Host::IsPlanar(vi_)) env->ThrowError("%s: clip must be in Y/YUV planar format.", name);
        if (Host::Height(vi_) % 2 != 0) env->ThrowError("%s: height must be even.", name);
        if (Host::Is420(vi_) && Host::Height(vi_) % 4) env->ThrowError("%s: height must be mod4.", name);
        if (a.order < 0 || a.order > 2) env->ThrowError("%s: order must be between 0..2.", name);
        if (a.aa < 0 || a.aa > 128) env->ThrowError("%s: aa must be between 0..128.", name);
        if (a.aac < 0 || a.aac > 128) env->ThrowError("%s: aac must be between 0..128.", name);
        if (a.reduce < 0 || a.reduce > 2) env->ThrowError("%s: reduce must be between 0..2.", name);
        if (a.reduce && !a.dh) env->ThrowError("%s: reduce needs dh=true", name);
        if (a.mask) {
            if (a.mask_lo < 0 || a.mask_lo > 255) env->ThrowError("%s: sn_aa_mask.lo must be 0..255", name);
            if (a.mask_hi < 0 || a.mask_hi > 255) env->ThrowError("%s: sn_aa_mask.hi must be 0..255", name);
            if (a.mask_lo > a.mask_hi) env->ThrowError("%s: sn_aa_mask.lo must not be above sn_aa_mask.hi", name);
            if (a.mask_expand < 0 || a.mask_expand > 1) env->ThrowError("%s: sn_aa_mask.expand must be 0 or 1", name);
            if (a.dh && !a.reduce) env->ThrowError("%s: mask needs the frame at source size (dh=false, or dh=true with reduce)", name);
            if (a.mask_luma && Host::NumComponents(vi_) >= 3 && !a.dh && !a.luma && a.chroma)
                env->ThrowError("%s: a luma-derived chroma mask needs luma processed (luma=true)", name);
        }
        if (a.sharpen < 0 || a.sharpen > 255) env->ThrowError("%s: sn_aa_sharpen.amount must be 0 (off) or 1..255", name);
        if (a.sharpen && a.dh && !a.reduce) env->ThrowError("%s: sharpen needs the frame at source size (dh=false, or dh=true with reduce)", name);
        if (a.both_fields && a.dh) env->ThrowError("%s: both fields needs dh=false", name);
        if (a.repair < 0 || a.repair > 4) env->ThrowError("%s: sn_aa_repair.rank must be 0 (off) or 1..4", name);
        if (a.repair && a.dh && !a.reduce) env->ThrowError("%s: repair needs the frame at source size (dh=false, or dh=true with reduce)", name);
        sn_config c{};
        c.struct_size = (int32_t)sizeof c;
        c.width = Host::Width(vi_);
        c.height = Host::Height(vi_);
        c.bytes_per_sample = Host::ComponentSize(vi_);
        c.bits_per_sample = Host::BitsPerComponent(vi_);
        c.num_planes = std::min(Host::NumComponents(vi_), 3);
        c.sub_w = c.num_planes > 1 ? Host::SubW(vi_) : 0;
        c.sub_h = c.num_planes > 1 ? Host::SubH(vi_) : 0;
        c.order = a.order;
        c.aa = a.aa;
        c.aac = a.aac;
        c.dh = a.dh;
        c.luma = a.luma;
        c.chroma = a.chroma;
        c.device = a.device;
        c.max_batch = 1;
        int la = a.lookahead;
        if (la < 0) {
            const char* e = std::getenv("SANGNOM_LOOKAHEAD");
            la = e ? std::atoi(e) : 1;
        }
        c.host_depth = std::max(1, std::min(la, 256));
        c.isolated_planes = a.isolated ? 1 : 0;
        c.fresh_pool = a.fresh ? 1 : 0;
        sn_policy pol = a.policy;
        pol.struct_size = (int32_t)sizeof pol;
        sn_options opts{};
        opts.struct_size = (int32_t)sizeof opts;
        opts.arithmetic = a.opt == 1 ? SN_ARITH_SSE2 : SN_ARITH_CXX;
        opts.column_parts = column_parts_of(a);
        sn_aa_options aopts{};
        aopts.struct_size = (int32_t)sizeof aopts;
        aopts.reduce = a.reduce;
        sn_aa_mask mask{};
        mask.struct_size = (int32_t)sizeof mask;
        mask.kind = a.mask ? SN_AA_MASK_SOBEL : SN_AA_MASK_NONE;
        mask.lo = a.mask_lo, mask.hi = a.mask_hi, mask.expand = a.mask_expand;
        sn_aa_mask_ex mask_ex{};
        mask_ex.struct_size = (int32_t)sizeof mask_ex;
        mask_ex.chroma = a.mask_luma ? SN_AA_MASK_CHROMA_LUMA : SN_AA_MASK_CHROMA_OWN;
        sn_aa_sharpen sharpen{};
        sharpen.struct_size = (int32_t)sizeof sharpen;
        sharpen.amount = a.sharpen, sharpen.chroma = a.sharpen_chroma ? 1 : 0;
        sn_aa_fields fields{};
        fields.struct_size = (int32_t)sizeof fields;
        fields.mode = a.both_fields ? SN_AA_FIELDS_BOTH : SN_AA_FIELDS_ONE;
        sn_aa_repair repair{};
        repair.struct_size = (int32_t)sizeof repair;
        repair.rank = a.repair, repair.chroma = a.repair_chroma ? 1 : 0;
        if (sn_aa_create_ex7(&c, &pol, &opts, &aopts, &mask, &mask_ex, &sharpen, &fields, &repair, &ctx_) != SN_OK)
            env->ThrowError("%s: %s", name, sn_aa_last_error(nullptr));
        enlarged_ = a.dh && !a.reduce;
        if (enlarged_) {  // each pass doubles the height of what it is given: the clip comes out twice as wide and twice as high
            Host::SetWidth(vi_, Host::Width(vi_) * 2);
            Host::SetHeight(vi_, Host::Height(vi_) * 2);
        }
        planes_ = c.num_planes;
        alpha_ = Host::NumComponents(vi_) == 4;
        num_frames_ = Host::NumFrames(vi_);
        sn_info i0{}, i1{};
        i0.struct_size = i1.struct_size = (int32_t)sizeof i0;
        const bool ahead = c.host_depth > 1 && sn_aa_get_info(ctx_, 0, &i0) == SN_OK && sn_aa_get_info(ctx_, 1, &i1) == SN_OK &&
                           i0.history_free && i1.history_free;
        slots_ = ahead ? sn_aa_host_slots(ctx_) : 1;
    }
    AAFilter(const AAFilter&) = delete;
    AAFilter& operator=(const AAFilter&) = delete;
    ~AAFilter()
    {
        inflight_.clear();  // frames still in the ring are dropped with the context
        sn_aa_destroy(ctx_);
    }

    const Info& GetInfo() const { return vi_; }

    FramePtr GetFrame(int n, Env* env)
    {
        if (slots_ > 1) return GetFrameAhead(n, env);
        FramePtr src = Host::GetFrame(child_, n, env);
        FramePtr dst = Host::NewFrame(env, vi_, src);
        const void* sp[3] = {nullptr, nullptr, nullptr};
        void* dp[3] = {nullptr, nullptr, nullptr};
        int32_t spitch[3] = {0, 0, 0}, dpitch[3] = {0, 0, 0};
        for (int p = 0; p < planes_; ++p) {
            sp[p] = Host::ReadPtr(src, p);
            dp[p] = Host::WritePtr(dst, p);
            spitch[p] = Host::Pitch(src, p);
            dpitch[p] = Host::Pitch(dst, p);
        }
        const int parity = args_.order == 0 ? (Host::GetParity(child_, n) ? 1 : 0) : 1;
        if (sn_aa_process_host(ctx_, sp, spitch, dp, dpitch, parity) != SN_OK) env->ThrowError("SangNomAA: %s", sn_aa_last_error(ctx_));
        CopyAlpha(src, dst);
        return dst;
    }

private:
    struct Pending {
        int n;
        FramePtr src, dst;  // src is held until the slot is collected (pinned planes are read by the device as they lie)
        int32_t slot;
    };

    void CopyAlpha(const FramePtr& src, const FramePtr& dst) const  // passed through (see Filter::CopyAlpha)
    {
        if (!alpha_) return;
        const size_t B = (size_t)Host::ComponentSize(vi_);
        const size_t row = (size_t)Host::Width(vi_) * B;
        if (!enlarged_) {
            for (int y = 0; y < Host::Height(vi_); ++y)
                std::memcpy(Host::WritePtr(dst, 3) + (size_t)y * Host::Pitch(dst, 3), Host::ReadPtr(src, 3) + (size_t)y * Host::Pitch(src, 3), row);
            return;
        }
        // dh: every source sample fills a 2 x 2 block (Filter::CopyAlpha repeats lines; here the samples of a line as well)
        const int w_out = Host::Width(vi_);
        for (int y = 0; y < Host::Height(vi_); y += 2) {
            const uint8_t* s = Host::ReadPtr(src, 3) + (size_t)(y / 2) * Host::Pitch(src, 3);
            uint8_t* d = Host::WritePtr(dst, 3) + (size_t)y * Host::Pitch(dst, 3);
            for (int x = 0; x < w_out; ++x) std::memcpy(d + (size_t)x * B, s + (size_t)(x / 2) * B, B);
            std::memcpy(d + Host::Pitch(dst, 3), d, row);
        }
    }

    FramePtr Collect(Env* env)
    {
        Pending p = inflight_.front();
        inflight_.pop_front();
        void* dp[3] = {nullptr, nullptr, nullptr};
        int32_t dpitch[3] = {0, 0, 0};
        for (int i = 0; i < planes_; ++i) {
            dp[i] = Host::WritePtr(p.dst, i);
            dpitch[i] = Host::Pitch(p.dst, i);
        }
        if (sn_aa_collect_host(ctx_, p.slot, dp, dpitch) != SN_OK) env->ThrowError("SangNomAA: %s", sn_aa_last_error(ctx_));
        return p.dst;
    }

    // Filter::GetFrameAhead over the anti-aliasing call's ring: a request out of sequence drains it and starts over
    FramePtr GetFrameAhead(int n, Env* env)
    {
        if (inflight_.empty() || inflight_.front().n != n) {
            while (!inflight_.empty()) Collect(env);
            next_ = n;
        }
        while ((int)inflight_.size() < slots_ && next_ < num_frames_) {
            Pending p;
            p.n = next_++;
            p.src = Host::GetFrame(child_, p.n, env);
            p.dst = Host::NewFrame(env, vi_, p.src);
            const void* sp[3] = {nullptr, nullptr, nullptr};
            int32_t spitch[3] = {0, 0, 0};
            for (int i = 0; i < planes_; ++i) {
                sp[i] = Host::ReadPtr(p.src, i);
                spitch[i] = Host::Pitch(p.src, i);
            }
            const int parity = args_.order == 0 ? (Host::GetParity(child_, p.n) ? 1 : 0) : 1;
            if (sn_aa_submit_host(ctx_, sp, spitch, parity, &p.slot) != SN_OK) env->ThrowError("SangNomAA: %s", sn_aa_last_error(ctx_));
            CopyAlpha(p.src, p.dst);
            inflight_.push_back(p);
        }
        if (inflight_.empty()) env->ThrowError("SangNomAA: frame %d is outside the clip", n);
        return Collect(env);
    }

    std::deque<Pending> inflight_;
    int next_ = 0;
    int num_frames_ = 0;
    int slots_ = 1;
    ClipPtr child_;
    Args args_;
    Info vi_{};
    sn_aa_context* ctx_ = nullptr;
    int planes_ = 1;
    bool alpha_ = false;
    bool enlarged_ = false;  // dh without reduce: the clip is twice as wide and twice as high
};

// Legacy SangNom(clip, order, aa, opt): order 0/1/2 = bottom/top/double-rate is remapped to
// SangNom2's 2/1/0 (src/SangNom2.cpp:441,463).  The reference additionally reads arguments its
// signature does not have (args[3] lands in aac, :443); that quirk is not reproduced: aac = 0.
inline Args legacy_args(int order, int aa, int opt)
{
    Args a;
    static const int ord[3] = {2, 1, 0};
    a.order = (order >= 0 && order <= 2) ? ord[order] : order;
    a.aa = aa;
    a.opt = opt;
    return a;
}

}  // namespace sangnom
