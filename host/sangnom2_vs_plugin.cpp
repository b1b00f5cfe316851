// sangnom2_vs_plugin.cpp -- a VapourSynth (API 4) front-end over libsangnom_hip.so.
//
// The reference is itself a port of the VapourSynth plugin (README.md:5 of the reference); this translation unit
// offers the same filter to VapourSynth scripts through the C ABI of include/sangnom_hip.h:
//     core.sangnomhip.SangNom(clip, order=1, dh=False, aa=48, aac=0, luma=True, chroma=True,
//                             isolated=False, fresh=False)
//     core.sangnomhip.SangNomAA(clip, order=1, aa=48, aac=0, luma=True, chroma=True, isolated=False, fresh=False, dh=False, reduce=0,
//                               mask=False, mlo=8, mhi=32, mexpand=1, mluma=False, sharp=0, sharpc=False, both=False,
//                               repair=0, repairc=False)
// SangNomAA is the anti-aliasing idiom (a quarter turn, SangNom, the turn back, SangNom) as one call of the library
// (sn_aa_process_host); with dh=True both passes double the height: the clip comes out twice as wide and twice as high;
// with reduce=1 (tent) or 2 (half-band) on top of dh the library reduces it on the device and the clip keeps its size.
// mask=True (at source size: no dh, or dh with reduce) merges the result into the source through a Sobel edge mask of the
// source (thresholds mlo <= mhi in 0..255, mexpand 0 | 1); the defaults are starting values, not tuned on real footage.
// mluma=True merges chroma through the luma plane's mask, reduced to chroma's geometry, instead of its own (needs luma=True).
// sharp=1..255 (at source size) contra-sharpens the result behind the last step and before the mask (strength sharp / 64, limited
// by what the filter changed); sharpc=True: every processed plane, not luma alone.  64 is a starting value, not tuned on real footage.
// both=True (without dh) interpolates both fields in every pass (order 1 and order 2) and averages the two on the device; order
// then has no influence.
// repair=1..4 (at source size) clamps each sample of the result into the range of the repair-th smallest and repair-th largest of
// the nine source samples around it, behind the sharpening and before the mask; repairc=True: every processed plane, not luma alone.
// It needs the VapourSynth SDK header VapourSynth4.h, a third-party file that is not part of this repository or
// of the build image: without it this file compiles to nothing, so it has NOT been compiled or run here
// (INTEGRATION.md says so).  With the SDK:  make -C host VS_INCLUDE_DIR=<dir of VapourSynth4.h>.
#if defined(__has_include)
#if __has_include(<VapourSynth4.h>)
#define SN_HAVE_VAPOURSYNTH 1
#endif
#endif

#ifdef SN_HAVE_VAPOURSYNTH
#include <VapourSynth4.h>

#include <mutex>
#include <string>

#include "sangnom_hip.h"

namespace {

struct SangNomData {
    VSNode* node = nullptr;
    VSVideoInfo vi{};
    sn_context* ctx = nullptr;
    sn_aa_context* aa = nullptr;  // SangNomAA: the anti-aliasing call instead of one filter instance
    int planes = 1;
    int order = 1;
    std::mutex mtx;  // one context == one filter instance: frames go through it one at a time, in request order
};

const VSFrame* VS_CC sangnomGetFrame(int n, int activationReason, void* instanceData, void**, VSFrameContext* frameCtx, VSCore* core,
                                     const VSAPI* vsapi)
{
    SangNomData* d = static_cast<SangNomData*>(instanceData);
    if (activationReason == arInitial) {
        vsapi->requestFrameFilter(n, d->node, frameCtx);
        return nullptr;
    }
    if (activationReason != arAllFramesReady) return nullptr;
    const VSFrame* src = vsapi->getFrameFilter(n, d->node, frameCtx);
    VSFrame* dst = vsapi->newVideoFrame(&d->vi.format, d->vi.width, d->vi.height, src, core);
    const void* sp[3] = {nullptr, nullptr, nullptr};
    void* dp[3] = {nullptr, nullptr, nullptr};
    int32_t spitch[3] = {0, 0, 0}, dpitch[3] = {0, 0, 0};
    for (int p = 0; p < d->planes; ++p) {
        sp[p] = vsapi->getReadPtr(src, p);
        dp[p] = vsapi->getWritePtr(dst, p);
        spitch[p] = (int32_t)vsapi->getStride(src, p);
        dpitch[p] = (int32_t)vsapi->getStride(dst, p);
    }
    int parity = 1;  // order == 0: the field to keep follows the frame's _Field / _FieldBased property (1 = top)
    if (d->order == 0) {
        int err = 0;
        const VSMap* props = vsapi->getFramePropertiesRO(src);
        int64_t field = vsapi->mapGetInt(props, "_Field", 0, &err);
        if (err) field = vsapi->mapGetInt(props, "_FieldBased", 0, &err) == 1 ? 0 : 1;
        parity = field ? 1 : 0;
    }
    int rc;
    {
        std::lock_guard<std::mutex> lk(d->mtx);
        rc = d->aa ? sn_aa_process_host(d->aa, sp, spitch, dp, dpitch, parity) : sn_process_host(d->ctx, sp, spitch, dp, dpitch, parity);
        if (rc != SN_OK)
            vsapi->setFilterError((std::string(d->aa ? "SangNomAA: " : "SangNom: ") + (d->aa ? sn_aa_last_error(d->aa) : sn_last_error(d->ctx))).c_str(),
                                  frameCtx);
    }
    vsapi->freeFrame(src);
    if (rc != SN_OK) {
        vsapi->freeFrame(dst);
        return nullptr;
    }
    return dst;
}

void VS_CC sangnomFree(void* instanceData, VSCore*, const VSAPI* vsapi)
{
    SangNomData* d = static_cast<SangNomData*>(instanceData);
    vsapi->freeNode(d->node);
    if (d->aa) sn_aa_destroy(d->aa);
    else sn_destroy(d->ctx);
    delete d;
}

void VS_CC sangnomCreate(const VSMap* in, VSMap* out, void* userData, VSCore* core, const VSAPI* vsapi)
{
    const bool aa = userData != nullptr;  // registered as SangNomAA
    const std::string name = aa ? "SangNomAA: " : "SangNom: ";
    SangNomData* d = new SangNomData;
    int err = 0;
    d->node = vsapi->mapGetNode(in, "clip", 0, &err);
    d->vi = *vsapi->getVideoInfo(d->node);
    auto geti = [&](const char* key, int def) {
        int e = 0;
        const int64_t v = vsapi->mapGetInt(in, key, 0, &e);
        return e ? def : (int)v;
    };
    auto fail = [&](const std::string& msg) {
        vsapi->mapSetError(out, (name + msg).c_str());
        vsapi->freeNode(d->node);
        delete d;
    };
    const VSVideoFormat& f = d->vi.format;
    if (f.colorFamily != cfGray && f.colorFamily != cfYUV) return fail("clip must be in Y/YUV planar format.");
    sn_config c{};
    c.struct_size = (int32_t)sizeof c;
    c.width = d->vi.width;
    c.height = d->vi.height;
    c.bytes_per_sample = f.bytesPerSample;
    c.bits_per_sample = f.bitsPerSample;
    c.num_planes = f.numPlanes < 3 ? 1 : 3;
    c.sub_w = c.num_planes > 1 ? f.subSamplingW : 0;
    c.sub_h = c.num_planes > 1 ? f.subSamplingH : 0;
    c.order = d->order = geti("order", 1);
    c.aa = geti("aa", 48);
    c.aac = geti("aac", 0);
    c.dh = geti("dh", 0) != 0;
    c.luma = geti("luma", 1) != 0;
    c.chroma = geti("chroma", 1) != 0;
    c.isolated_planes = geti("isolated", 0) != 0;
    c.fresh_pool = geti("fresh", 0) != 0;
    c.max_batch = 1;
    c.mode = SN_MODE_AUTO;
    auto bare = [](const char* m) { return std::string(m + (std::string(m).rfind("SangNom2: ", 0) == 0 ? 10 : 0)); };  // the reference's prefix
    char msg[256];
    if (sn_validate(&c, msg, sizeof msg) != SN_OK) return fail(bare(msg));
    // SangNomAA: the turned clip and, with dh, the clip twice as wide are validated by the creation itself
    sn_aa_options ao{};
    ao.struct_size = (int32_t)sizeof ao;
    ao.reduce = aa ? geti("reduce", 0) : 0;
    if (ao.reduce && !c.dh) return fail("reduce needs dh=true");
    sn_aa_mask mk{};
    mk.struct_size = (int32_t)sizeof mk;
    mk.kind = aa && geti("mask", 0) ? SN_AA_MASK_SOBEL : SN_AA_MASK_NONE;
    mk.lo = geti("mlo", 8), mk.hi = geti("mhi", 32), mk.expand = geti("mexpand", 1);
    sn_aa_mask_ex mx{};
    mx.struct_size = (int32_t)sizeof mx;
    mx.chroma = aa && geti("mluma", 0) ? SN_AA_MASK_CHROMA_LUMA : SN_AA_MASK_CHROMA_OWN;
    sn_aa_sharpen sh{};
    sh.struct_size = (int32_t)sizeof sh;
    sh.amount = aa ? geti("sharp", 0) : 0, sh.chroma = aa && geti("sharpc", 0) ? 1 : 0;
    sn_aa_fields fl{};
    fl.struct_size = (int32_t)sizeof fl;
    fl.mode = aa && geti("both", 0) ? SN_AA_FIELDS_BOTH : SN_AA_FIELDS_ONE;
    if (fl.mode == SN_AA_FIELDS_BOTH && c.dh) return fail("both fields needs dh=false");
    sn_aa_repair rp{};
    rp.struct_size = (int32_t)sizeof rp;
    rp.rank = aa ? geti("repair", 0) : 0, rp.chroma = aa && geti("repairc", 0) ? 1 : 0;
    if (aa ? sn_aa_create_ex7(&c, nullptr, nullptr, &ao, &mk, &mx, &sh, &fl, &rp, &d->aa) != SN_OK : sn_create(&c, &d->ctx) != SN_OK) return fail(bare(aa ? sn_aa_last_error(nullptr) : sn_last_error(nullptr)));
    d->planes = c.num_planes;
    if (c.dh && !ao.reduce) d->vi.height *= 2;
    if (c.dh && aa && !ao.reduce) d->vi.width *= 2;  // both passes double the height of what they are given
    // The context keeps the reference's per-instance state (scratch pool, frame order), so frames are served one at
    // a time in request order: fmFrameState.  With fresh=True every frame is independent, but the context is still
    // not re-entrant (one stream, one staging area), hence the mutex above rather than a parallel mode.
    VSFilterDependency deps[] = {{d->node, rpStrictSpatial}};
    vsapi->createVideoFilter(out, aa ? "SangNomAA" : "SangNom", &d->vi, sangnomGetFrame, sangnomFree, fmFrameState, deps, 1, d, core);
}

}  // namespace

VS_EXTERNAL_API(void) VapourSynthPluginInit2(VSPlugin* plugin, const VSPLUGINAPI* vspapi)
{
    vspapi->configPlugin("com.github.sangnom.hip", "sangnomhip", "SangNom2 edge-directed interpolation on AMD GPUs (libsangnom_hip)",
                         VS_MAKE_VERSION(1, 0), VAPOURSYNTH_API_VERSION, 0, plugin);
    vspapi->registerFunction("SangNom",
                             "clip:vnode;order:int:opt;dh:int:opt;aa:int:opt;aac:int:opt;luma:int:opt;chroma:int:opt;isolated:int:opt;fresh:int:opt;",
                             "clip:vnode;", sangnomCreate, nullptr, plugin);
    static int aa_tag = 1;
    vspapi->registerFunction("SangNomAA",
                             "clip:vnode;order:int:opt;aa:int:opt;aac:int:opt;luma:int:opt;chroma:int:opt;isolated:int:opt;fresh:int:opt;dh:int:opt;reduce:int:opt;mask:int:opt;mlo:int:opt;mhi:int:opt;mexpand:int:opt;mluma:int:opt;sharp:int:opt;sharpc:int:opt;both:int:opt;repair:int:opt;repairc:int:opt;",
                             "clip:vnode;", sangnomCreate, &aa_tag, plugin);
}
#endif  // SN_HAVE_VAPOURSYNTH
