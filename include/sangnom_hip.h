/*
 * sangnom_hip.h -- C ABI of libsangnom_hip.so, the MI355X (gfx950) implementation of the
 * SangNom2 edge-directed interpolation hot path.
 *
 * What this boundary replaces in the reference (Asd-g/AviSynth-SangNom2 v0.6.1):
 *   - the per-plane kernel entry   void (SangNom2::*process)(dstp, dstStride, w, h, offset, plane)
 *                                  src/SangNom2.h:58, called at src/SangNom2.cpp:393
 *   - its drivers                  SangNom2::sangnom_c  src/SangNom2.cpp:259-273
 *                                  SangNom2::sangnom_sse src/SangNom2_SSE2.cpp:1258-1272
 *   - the frame assembly around it SangNom2::GetFrame   src/SangNom2.cpp:346-394
 *   - instance state               ctor: thresholds, pool geometry  src/SangNom2.cpp:275-310
 *   - argument validation          Create_SangNom2      src/SangNom2.cpp:407-422
 *
 * The reference has no FFI of its own (it is one C++ plugin); the functions below are what a
 * plugin adapter (host/sangnom2_avs_plugin.cpp) binds instead of calling (this->*process)().
 * Plain C: pointers, sizes and integer return codes only; no exceptions cross this boundary and
 * no torch / HIP types appear in the signatures (a hipStream_t travels as void*).
 *
 * Results are bit-exact to the reference's opt=0 path for 8..16-bit integer formats and for
 * 32-bit float, under the conventions that make the reference's output defined
 * (zero-filled scratch pool, one context == one filter instance, frames in call order).
 * With sn_options.arithmetic = SN_ARITH_SSE2 (sn_create_ex) they are bit-exact to its opt=1 path
 * instead -- what its default opt=-1 computes on every x86-64 host.
 *
 * There is NO CPU fallback: every entry point that computes needs a HIP device and fails with
 * SN_ERR_NO_DEVICE / SN_ERR_HIP otherwise.
 */
#ifndef SANGNOM_HIP_H
#define SANGNOM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SN_ABI_VERSION 4

typedef struct sn_context sn_context;

/* Return codes. */
enum {
    SN_OK = 0,
    SN_ERR_INVALID_ARG = 1, /* null pointer, bad struct_size, bad pitch ...                   */
    SN_ERR_CONFIG = 2,      /* rejected by the reference's own checks; message = its text     */
    SN_ERR_HIP = 3,         /* a HIP runtime call failed; message names it                    */
    SN_ERR_NO_DEVICE = 4,   /* no usable HIP device                                           */
    SN_ERR_UNSUPPORTED = 5, /* geometry outside what the kernels handle (see sn_create)       */
    SN_ERR_BUSY = 6         /* sn_submit_host: every slot of the host ring holds a frame      */
};

/* Execution path selection (sn_config.mode). */
enum {
    SN_MODE_AUTO = 0,   /* fused tile kernel where eligible, else the pool path               */
    SN_MODE_POOL = 1,   /* always the three-kernel path over the HBM-resident pool            */
    SN_MODE_FUSED = 2   /* require the fused kernel; sn_create fails if not eligible          */
};

/* Clip format + the script arguments of SangNom2(clip, order, aa, aac, threads, dh, luma,
 * chroma, opt)  (src/SangNom2.cpp:399-435, README.md:20-57).  `threads` is a dummy in the
 * reference and `opt` selects its CPU code path; neither exists here. */
typedef struct sn_config {
    int32_t struct_size;      /* = sizeof(sn_config)                                         */
    int32_t width;            /* luma width, pixels                                          */
    int32_t height;           /* luma height of the INPUT clip (before dh doubles it)        */
    int32_t bytes_per_sample; /* 1, 2 or 4 (float)              vi.ComponentSize()           */
    int32_t bits_per_sample;  /* 8..16 or 32                    vi.BitsPerComponent()        */
    int32_t num_planes;       /* 1 (Y) or 3 (YUV); alpha is never touched (SangNom2.cpp:347) */
    int32_t sub_w;            /* log2 horizontal chroma subsampling                          */
    int32_t sub_h;            /* log2 vertical chroma subsampling                            */
    int32_t order;            /* 0 = field by parity, 1 = keep top, 2 = keep bottom          */
    int32_t aa;               /* luma anti-aliasing strength 0..128 (default 48)             */
    int32_t aac;              /* chroma anti-aliasing strength 0..128 (default 0)            */
    int32_t dh;               /* double the height                                           */
    int32_t luma;             /* process luma (default 1)                                    */
    int32_t chroma;           /* process chroma (default 1)                                  */
    int32_t device;           /* HIP device ordinal                                          */
    int32_t max_batch;        /* frames one sn_process_device_strided call may carry (>= 1)  */
    int32_t mode;             /* SN_MODE_*                                                   */
    int32_t host_depth;       /* frames sn_submit_host may keep in flight (0 = 4)            */
    int32_t isolated_planes;  /* EXTENSION, default 0.  1: every plane is filtered as a Y clip *
                               * of its own (own scratch geometry, nothing shared) -- what    *
                               * ExtractY/U/V -> SangNom2 -> CombinePlanes gives with the      *
                               * reference -- instead of the reference's luma-sized pool that *
                               * subsampled chroma shares with luma (SangNom2.cpp:287-310)    */
    int32_t fresh_pool;       /* EXTENSION, default 0.  1: every plane of every frame is      *
                               * filtered as by a newly created reference instance (scratch   *
                               * zero-filled, planes isolated).  Removes the dependence on     *
                               * earlier frames that the reference has when the width is not   *
                               * a multiple of 32, and with it the need to     *
                               * run such clips frame by frame                                 */
    void*   stream;           /* hipStream_t to run on; NULL = the context creates its own   */
} sn_config;

/* Scheduling policy of a context (sn_create_with_policy / sn_set_policy).  Nothing here changes a result -- every path
 * is exact -- only which kernels run and how much memory they may take.  A zero in any field means "the default".
 * (Rounds 1-2 read these from environment variables; the library reads none now.  A build with -DSN_TEST_HOOKS still
 * honours SN_PREFER_POOL, SN_CHAIN, SN_COPY_THREADS and SN_SCRATCH_BUDGET_MB as overrides, for bisecting in the field.) */
enum {
    SN_SMALL_AUTO = 0,   /* launches of a few frames (a synchronous GetFrame, a short look-ahead) are cut into row   *
                          * bands, or go to the pool kernels where the cost model says so        */
    SN_SMALL_SWEEP = 1   /* whole-plane sweeps whenever the configuration is eligible, whatever the launch size     */
};
typedef struct sn_policy {
    int32_t struct_size;        /* = sizeof(sn_policy)                                                             */
    int32_t small_launches;     /* SN_SMALL_*                                                                      */
    int32_t chain;              /* history-carrying clips as chains of passes: 0 = on, -1 = off;  *
                                 * 1, 2, 4, 8 = on, with at most that many workgroups (CUs) per cost buffer (0 picks *
                                 * 8; wide pool rows allow fewer; 1 is the single-workgroup chain of round 2)       */
    int32_t copy_threads;       /* host threads that stage / copy lines, the caller included; 0 = by core count,   *
                                 * at most 16.  Takes effect when the context first needs them                      */
    int32_t scratch_budget_mb;  /* device scratch per kind (pool slots; hand-off pools of the coupled sweeps; the    *
                                 * chain's ring takes an eighth); 0 = 24576.  Read at creation only                  */
    int32_t chroma_sweeps;      /* 8-bit 4:2:0 clips in the sweeps: 0 = U and V as ONE sweep where the geometry allows *
                                 * (sn_fused_u8_uv.hip: the U -> V hand-off stays in registers), 1 = one sweep per      *
                                 * chroma plane with a hand-off pool between them (rounds 1-3).  May change any time   */
    int32_t sse2_sweeps;        /* SN_ARITH_SSE2 contexts only (no effect otherwise): 0 = the kernels of the release   *
                                 * that introduced the arithmetic -- sweeps for 8-bit planes on their own, the pool    *
                                 * kernels for 9..16-bit clips and for 8-bit clips whose subsampled chroma shares the   *
                                 * luma pool; 1 = sweeps for every configuration that has them in SN_ARITH_CXX (same    *
                                 * pixels, several times faster).  Read at creation only (sn_set_policy ignores it).    *
                                 * Took the place of reserved[0]: a caller who zeroes the reserved words gets 0         */
    int32_t reserved[1];        /* zero                                                                            */
} sn_policy;

/* What a context computes (sn_create_ex), as opposed to how (sn_policy).  Fixed for the context's life.
 * The reference has two code paths that do not give the same pixels for integer samples: its C++ path (opt=0)
 * wraps modulo 2^(8 sizeof T) in two narrowing steps where its SSE2 path (opt=1, and opt=-1 on every x86-64 host)
 * saturates to the container's maximum MAXT (255; 65535 for every 9..16-bit depth):
 *   the SangNom value (4 p1 + 5 p2 - p3) >> 3    SSE2: MAXT if the sum is negative or the value exceeds MAXT
 *                                                (src/SangNom2_SSE2.cpp:446-516, used by stages 1 and 3)
 *   the box of stage 2, sum / 16                 SSE2: min(sum >> 4, MAXT)   (src/SangNom2_SSE2.cpp:748-761)
 * Everything else, and all of float, is the same.  SN_ARITH_CXX is this library's default and what sn_create /
 * sn_create_with_policy give.  Which kernels run in SN_ARITH_SSE2: every fused sweep has instances of this arithmetic
 * (8-bit, 8-bit U and V as one sweep, 9..16-bit; plain, padded, row bands and the pool-coupled sweeps of 4:2:0 / 4:2:2),
 * and sn_policy.sse2_sweeps says which a context uses.  With 0, the default, 8-bit planes on their own (Y8, 4:4:4,
 * isolated_planes, fresh_pool) are served by the sweeps as in the default arithmetic (sn_info.fused_eligible = 1,
 * SN_MODE_FUSED accepted), while 8-bit clips whose subsampled chroma shares the luma pool (4:2:0, 4:2:2) and every
 * 9..16-bit clip run on the pool path: sn_info.fused_eligible is 0 and SN_MODE_FUSED fails at creation.  With 1 every
 * configuration is served as in SN_ARITH_CXX.  Float clips run as ever.  Every processed plane
 * must be at least two SSE2 vectors wide -- 32 / 16 / 8 samples for 8-bit / 16-bit / float, where the reference's SSE2
 * path reads outside the row below that -- else SN_ERR_UNSUPPORTED. */
enum {
    SN_ARITH_CXX = 0,   /* the reference's opt=0                                              */
    SN_ARITH_SSE2 = 1   /* the reference's opt=1 (its default on x86-64)                      */
};
/* sn_options: what is fixed when the context is created (sn_policy holds what may change between launches, and has no
 * free word left).
 * column_parts = 1: 9..16-bit and float planes too wide for one workgroup of the fused sweeps (more than 3840 columns;
 * width a multiple of 32, at most 8192) are swept in 2..N column parts, one workgroup each, over windows that overlap
 * by a ghost margin; no workgroup waits for another.  Each frame is checked -- both windows around a seam must agree bit
 * for bit on the smoothed values of the 16 columns around it, which proves the parts exact -- and a frame that fails is
 * redone by the pool path, so the output is the same either way (sn_get_parts_info counts such frames).  It applies to
 * planes on their own (Y, 4:4:4, isolated_planes); then sn_info.fused_eligible is 1 and SN_MODE_FUSED is accepted.  A wide
 * 4:2:0 / 4:2:2 clip whose chroma shares the luma pool stays on the pool path.  8-bit contexts accept the option; it has
 * no effect there.  0, the default, changes nothing. */
typedef struct sn_options {
    int32_t struct_size;   /* = sizeof(sn_options)                                           */
    int32_t arithmetic;    /* SN_ARITH_*                                                     */
    int32_t column_parts;  /* 0 (default) or 1; took the place of reserved[0]                */
    int32_t reserved[5];   /* zero                                                           */
} sn_options;

/* The column parts of a live context (all zero without sn_options.column_parts). */
typedef struct sn_parts_info {
    int32_t struct_size;
    int32_t parts[3];        /* per plane; 0 = not in parts                                  */
    int32_t ghost_columns;   /* least overlap of a window beyond a seam, per side            */
    int64_t part_frames;     /* frames swept in parts                                        */
    int64_t part_fallbacks;  /* ... of which the check sent to the pool path                 */
} sn_parts_info;

/* Geometry and counters of a live context. */
typedef struct sn_info {
    int32_t struct_size;
    int32_t out_height;       /* luma output height                                          */
    int32_t pool_stride;      /* elements per pool row  = roundup(width, 32)                 */
    int32_t pool_rows;        /* bufferHeight + 1                                            */
    int32_t fused_eligible;   /* 1 if the fused kernel serves this configuration             */
    int32_t history_free;     /* 1 if a frame's result cannot depend on earlier frames       */
    int64_t frames;           /* frames processed so far                                     */
    int64_t fused_frames;     /* ... of which by the fused sweeps (a single 4:2:0 frame whose luma *
                               * ran in row bands and whose chroma ran on the pool kernels counts) */
    int32_t coupled_rows;     /* rows per buffer the fused 4:2:0 sweeps hand from plane to   *
                               * plane (0: this configuration has no such hand-off)          */
    int32_t uv_sweeps;        /* 1 once U and V of a 4:2:0 frame have run as ONE sweep on this *
                               * context (8-bit; sn_policy.chroma_sweeps), else 0              */
    double  threshold[3];     /* aaf[plane] after conversion to the sample type              */
    int64_t banded_frames;    /* ... of fused_frames, swept in row bands (small launches)    */
    int64_t band_fallbacks;   /* ... of which the check sent to the pool path (up to the     *
                               * last synchronisation)                                       */
    int64_t chained_frames;   /* frames of a history-carrying clip whose passes ran as one   *
                               * chain (several frames per launch, or one frame with two or  *
                               * three processed planes) instead of one pass at a time       */
    int64_t chain_redone;     /* launches of such chains over several workgroups per buffer  *
                               * in which a workgroup gave up waiting for its neighbour (it   *
                               * was not scheduled next to it in time) and which were redone  *
                               * on one workgroup per buffer before their frames were handed  *
                               * on (up to the last synchronisation); the frames are right    *
                               * either way                                                   */
} sn_info;

/* Create_SangNom2's argument checks, same order, same message text (src/SangNom2.cpp:407-422).
 * Returns SN_OK or SN_ERR_CONFIG (+ message). */
int sn_validate(const sn_config* cfg, char* msg, size_t msg_len);

/* Constructor of the filter instance (src/SangNom2.cpp:275-330): thresholds, pool geometry,
 * device pool (zero-filled), stream.  Runs sn_validate first. */
int sn_create(const sn_config* cfg, sn_context** out);
int sn_create_with_policy(const sn_config* cfg, const sn_policy* policy /* NULL = defaults */, sn_context** out);
/* ... with options (NULL, or arithmetic = SN_ARITH_CXX: exactly sn_create_with_policy). */
int sn_create_ex(const sn_config* cfg, const sn_policy* policy /* NULL = defaults */, const sn_options* options /* NULL = defaults */,
                 sn_context** out);
int sn_get_arithmetic(sn_context* ctx); /* SN_ARITH_* of a live context; -1 for NULL */
void sn_destroy(sn_context* ctx);

/* The policy in force / a new one (small_launches, chain, copy_threads and chroma_sweeps may change during a context's life; the
 * scratch budget is fixed at creation and ignored here). */
int sn_get_policy(sn_context* ctx, sn_policy* policy);
int sn_set_policy(sn_context* ctx, const sn_policy* policy);

/* Text of the last error on this context; with ctx == NULL, of the last failed sn_create /
 * sn_validate on the calling thread.  Never NULL. */
const char* sn_last_error(const sn_context* ctx);

/* One GetFrame (src/SangNom2.cpp:332-397) with HOST planes: H2D, kernels, D2H, synchronous.
 * src planes have the input geometry, dst planes the output geometry; pitches in bytes, any
 * value >= row size.  parity = child->GetParity(n), used only when order == 0.
 * Only the lines the filter reads (the kept field of a processed plane) are sent to the device, and only the
 * interpolated lines come back: the kept lines of the output -- copies of source lines, src/SangNom2.cpp:361-391 --
 * and planes that are merely copied are written from src to dst on the host meanwhile.  src and dst planes must
 * not overlap. */
int sn_process_host(sn_context* ctx, const void* const src[3], const int32_t src_pitch[3],
                    void* const dst[3], const int32_t dst_pitch[3], int32_t parity);

/* The same with DEVICE planes, asynchronous on the context's stream. */
int sn_process_device(sn_context* ctx, const void* const src[3], const int32_t src_pitch[3],
                      void* const dst[3], const int32_t dst_pitch[3], int32_t parity);

/* nframes (<= max_batch) device-resident frames in one call: frame f's plane p starts at
 * src[p] + f * src_frame_stride[p] bytes (likewise dst).  Equivalent to nframes calls of
 * sn_process_device in order; when the configuration is history-free the frames are processed
 * concurrently.  parity may be NULL (= all 1). */
int sn_process_device_strided(sn_context* ctx, int32_t nframes,
                              const void* const src[3], const int64_t src_frame_stride[3],
                              const int32_t src_pitch[3],
                              void* const dst[3], const int64_t dst_frame_stride[3],
                              const int32_t dst_pitch[3], const int32_t* parity);

/* Pipelined host path (what a plugin's GetFrame with look-ahead binds).  The context owns
 * sn_host_slots() frame slots (about cfg.host_depth; fewer if scratch is short), each with pinned staging and
 * device buffers for one source and one output frame.  sn_submit_host copies the source planes into the next
 * slot (planes in pinned memory are not copied: see "Pinned host frames" below) and queues its H2D without waiting; the slots form up to four groups, and when a group is full (or one
 * of its frames is collected early) one launch sweeps its frames on the group's stream, D2H behind it.
 * sn_collect_host waits for the slot's group and copies the output planes out.  Transfers and sweeps of
 * different groups overlap.  Slots are handed out round-robin, so collecting in submission order never blocks
 * on a later frame; SN_ERR_BUSY means the next slot has not been collected.  History-carrying configurations
 * (sn_info.history_free == 0) still sweep their frames in submission order.
 * Not thread-safe per context; do not interleave with the batch entry points without sn_synchronize. */
int sn_host_slots(sn_context* ctx);
int sn_submit_host(sn_context* ctx, const void* const src[3], const int32_t src_pitch[3], int32_t parity,
                   int32_t* slot);
int sn_collect_host(sn_context* ctx, int32_t slot, void* const dst[3], const int32_t dst_pitch[3]);

/* Pinned host frames (optional).  A host that owns its frame memory can pin it once (hipHostRegister under the
 * hood; the caller keeps the memory alive and unpins it before freeing it).  Planes that lie inside pinned memory move
 * over PCIe directly: sn_process_host and sn_submit_host skip the staging copy of the source, and sn_submit_host_to
 * -- sn_submit_host with the destination planes named at submission, as a plugin's GetFrame has them
 * (env->NewVideoFrame before the kernel runs, src/SangNom2.cpp:344) -- has the output written straight into them;
 * sn_collect_host (dst = NULL allowed then) only waits.  Unpinned planes take the staged route as before, plane by
 * plane.  When every destination plane of a submission is pinned, the kept lines of the output are copied from src
 * to dst on the host during sn_submit_host_to and only the interpolated lines cross PCIe afterwards: the caller must
 * leave the announced planes alone until the slot is collected (and src, dst must not overlap).  Process-wide
 * registry, thread-safe.
 * LIFETIME OF A PINNED SOURCE: sn_submit_host / sn_submit_host_to do not capture a source plane that lies in pinned
 * memory -- the transfer reads the caller's memory asynchronously -- so such a plane must stay valid and UNCHANGED
 * until its slot has been collected (a host that recycles frame buffers keeps the frame referenced until then, as
 * host/sangnom2_filter.hpp does).  Unpinned source planes are copied into the slot's staging before the call
 * returns, as ever.  sn_unpin_host_buffer waits for the outstanding work of every device this library has a context on
 * before it unregisters; when the runtime refuses to unregister, the range stays pinned and known (SN_ERR_HIP).
 * EXPERIMENTAL on ROCm 7.2 / gfx950: a process that has registered and later UNREGISTERED host memory was seen to abort,
 * about once in twenty young processes, inside a LATER asynchronous copy from or to PAGEABLE memory -- the runtime's
 * own pin-on-the-fly path, torch's transfers included; never inside this library, which stages every pageable plane
 * through its own pinned buffers (profiles/r3_page_fault.md, tools/repro_pageable_after_unpin.sh).  A host that uses
 * these two entry points should (a) pin its frame arenas once and unpin them only at shutdown, and (b) keep its other
 * device transfers on pinned memory as well.  Without them nothing is registered and the hazard does not arise. */
int sn_pin_host_buffer(void* ptr, size_t bytes);
int sn_unpin_host_buffer(void* ptr);
int sn_submit_host_to(sn_context* ctx, const void* const src[3], const int32_t src_pitch[3], void* const dst[3],
                      const int32_t dst_pitch[3], int32_t parity, int32_t* slot);

/* TurnRight (direction > 0, clockwise) / TurnLeft (direction < 0) of `nframes` device-resident planes of
 * width x height samples of the context's sample type, on the context's stream: dst is height wide and width
 * high.  For pipelines that keep frames on the GPU between the two SangNom2 passes of an anti-aliasing script
 * (TurnLeft().SangNom2().TurnRight().SangNom2()).  No counterpart in the reference. */
int sn_turn_device(sn_context* ctx, int32_t direction, int32_t nframes, const void* src, int64_t src_frame_stride,
                   int32_t src_pitch, int32_t width, int32_t height, void* dst, int64_t dst_frame_stride,
                   int32_t dst_pitch);

/* The reduction of the anti-aliasing call (below: "Anti-aliasing at source size", which defines the arithmetic) on its
 * own, for pipelines that keep frames on the device, like sn_turn_device: `nframes` planes of 2 width x 2 height samples
 * to width x height, centred on src[2y + oy][2x + ox], on the context's stream.  Sample type and bit depth (the clamp)
 * come from the context.  kernel: SN_AA_REDUCE_TENT or SN_AA_REDUCE_HALFBAND; ox, oy: 0 or 1; src_pitch >= 2 width
 * samples, dst_pitch >= width samples; pointers, pitches and frame strides multiples of the sample size (multiples of 16
 * on a side: 16 bytes per lane and access on that side).  Nothing beyond width samples of a destination row is written. */
int sn_reduce_device(sn_context* ctx, int32_t kernel, int32_t nframes, const void* src, int64_t src_frame_stride, int32_t src_pitch,
                     int32_t width, int32_t height /* of dst; src is 2 width x 2 height */, int32_t ox, int32_t oy, void* dst,
                     int64_t dst_frame_stride, int32_t dst_pitch);

/* The edge mask of the anti-aliasing call (below: "Edge mask", which defines the arithmetic).  kind SN_AA_MASK_SOBEL: lo <= hi
 * in 0..255 (8-bit scale, like aa), expand 0 or 1.  The defaults the plugins offer (lo 8, hi 32, expand 1) are a starting
 * point: nobody has tuned them on real footage. */
enum { SN_AA_MASK_NONE = 0, SN_AA_MASK_SOBEL = 1 };
typedef struct sn_aa_mask {
    int32_t struct_size; /* sizeof(sn_aa_mask) */
    int32_t kind;        /* SN_AA_MASK_*; with SN_AA_MASK_NONE the fields below are ignored */
    int32_t lo, hi;      /* e <= lo keeps the source, e >= hi takes the result */
    int32_t expand;      /* 1: the mask is its own maximum over 3 x 3 */
    int32_t reserved[3]; /* zero */
} sn_aa_mask;            /* 32 bytes */

/* The mask and the merge on their own, for pipelines that keep frames on the device and for tuning thresholds: `nframes`
 * planes of width x height samples on the context's stream; sample type and bit depth come from the context.  The mask is
 * built from src; dst = src where it is 0, aa where it is 256, the blend between (see "Edge mask").  aa == NULL: dst is the
 * mask itself, integers (m * (2^bits - 1) + 128) >> 8, float (float)m * 0.00390625f.  mask->kind must be SN_AA_MASK_SOBEL;
 * the struct is checked as sn_aa_create_ex3 checks it.  dst may be the very plane aa lies in (same base, pitch and frame
 * stride: each sample of aa is read by the thread that overwrites it); src must not overlap dst.  Pitches >= width samples;
 * pointers, pitches and frame strides multiples of the sample size (multiples of 16 on a side: 16 bytes per lane and access on
 * that side).  Nothing beyond width samples of a destination row is written.  A refused call queues nothing. */
int sn_mask_merge_device(sn_context* ctx, const sn_aa_mask* mask, int32_t nframes, const void* src, int64_t src_frame_stride, int32_t src_pitch,
                         const void* aa /* NULL: write the mask */, int64_t aa_frame_stride, int32_t aa_pitch, int32_t width, int32_t height,
                         void* dst, int64_t dst_frame_stride, int32_t dst_pitch);

/* Which mask merges chroma in the anti-aliasing call (below: "Edge mask", the paragraph on mc).  SN_AA_MASK_CHROMA_OWN: every
 * processed plane through the mask of its own source (the default, and what a context made without this struct does).
 * SN_AA_MASK_CHROMA_LUMA: planes 1 and 2 through the mask of the source LUMA plane, reduced to chroma's geometry. */
enum { SN_AA_MASK_CHROMA_OWN = 0, SN_AA_MASK_CHROMA_LUMA = 1 };
typedef struct sn_aa_mask_ex {
    int32_t struct_size; /* sizeof(sn_aa_mask_ex) */
    int32_t chroma;      /* SN_AA_MASK_CHROMA_* */
    int32_t reserved[6]; /* zero */
} sn_aa_mask_ex;         /* 32 bytes */

/* The luma-derived chroma merge on its own: `nframes` frames on the context's stream.  The mask m_L is built from `luma`,
 * (width << sub_w) x (height << sub_h) samples, reduced to mc (see "Edge mask") and merges aa[p] into src[p] for one or two
 * chroma planes of width x height samples in one launch: src[1] == NULL means one plane, and then dst[1] and aa[1] must be
 * NULL too.  aa == NULL or every entry of it NULL: dst[p] is the reduced mask itself, integers (mc * (2^bits - 1) + 128) >> 8,
 * float (float)mc * 0.00390625f; with two planes aa[0] and aa[1] are both given or both NULL.  sub_w, sub_h: 0..2.  mask is
 * checked as sn_mask_merge_device checks it; sample type and bit depth come from the context.  dst[p] may be the very plane
 * aa[p] lies in; luma and src must not overlap dst.  Pitches >= the row; pointers, pitches and frame strides multiples of the
 * sample size (multiples of 16 on a side -- luma, or src, aa or dst of one plane: 16 bytes per lane and access on that side).
 * Nothing beyond width samples of a destination row is written.  A refused call queues nothing. */
int sn_mask_merge_luma_device(sn_context* ctx, const sn_aa_mask* mask, int32_t nframes, const void* luma, int64_t luma_frame_stride,
                              int32_t luma_pitch, int32_t sub_w, int32_t sub_h, const void* const src[2], const int64_t src_frame_stride[2],
                              const int32_t src_pitch[2], const void* const aa[2] /* NULL, or both entries NULL: write the mask */,
                              const int64_t aa_frame_stride[2], const int32_t aa_pitch[2], int32_t width,
                              int32_t height /* of a chroma plane; luma is (width << sub_w) x (height << sub_h) */, void* const dst[2],
                              const int64_t dst_frame_stride[2], const int32_t dst_pitch[2]);

/* The contra-sharpening of the anti-aliasing call (below: "Contra-sharpening", which defines the arithmetic).  amount 0: off,
 * and the fields below it are ignored; 1..255 with 64 = unity.  The 64 the plugins document is a starting point: nobody has
 * tuned it on real footage. */
typedef struct sn_aa_sharpen {
    int32_t struct_size; /* sizeof(sn_aa_sharpen) */
    int32_t amount;      /* 0 = off (the fields below are ignored); 1..255, 64 = unity */
    int32_t chroma;      /* 0: plane 0 only; 1: every processed plane */
    int32_t reserved[5]; /* zero */
} sn_aa_sharpen;         /* 32 bytes */

/* The contra-sharpening on its own, for pipelines that keep frames on the device: `nframes` planes of width x height samples
 * on the context's stream; `aa` (the filtered plane R) is sharpened towards `src` (the plane S it was filtered from) and
 * written to dst (see "Contra-sharpening").  amount: 1..255; sample type and bit depth (the clamp) come from the context.
 * Pitches >= width samples; pointers, pitches and frame strides multiples of the sample size (multiples of 16 on a side: 16
 * bytes per lane and access on that side).  dst must overlap neither src nor aa, because the stencil reads neighbours of
 * both: the same base as aa or src is refused with SN_ERR_INVALID_ARG, wider overlap is the caller's contract.  Nothing
 * beyond width samples of a destination row is written.  A refused call queues nothing. */
int sn_contra_sharpen_device(sn_context* ctx, int32_t amount, int32_t nframes, const void* src, int64_t src_frame_stride, int32_t src_pitch,
                             const void* aa, int64_t aa_frame_stride, int32_t aa_pitch, int32_t width, int32_t height, void* dst,
                             int64_t dst_frame_stride, int32_t dst_pitch);

/* Which fields a pass of the anti-aliasing call interpolates (below: "Both fields", which defines the arithmetic).
 * SN_AA_FIELDS_ONE: the field cfg.order names, as a context made without this struct does.  SN_AA_FIELDS_BOTH: every pass
 * runs twice, order 1 and order 2, and the two results are averaged on the device. */
enum { SN_AA_FIELDS_ONE = 0, SN_AA_FIELDS_BOTH = 1 };
typedef struct sn_aa_fields {
    int32_t struct_size; /* sizeof(sn_aa_fields) */
    int32_t mode;        /* SN_AA_FIELDS_*; with SN_AA_FIELDS_ONE the fields below are ignored */
    int32_t reserved[6]; /* zero */
} sn_aa_fields;          /* 32 bytes */

/* The average of the both-fields call on its own (below: "Both fields" defines avg), for pipelines that keep frames on the
 * device: `nframes` planes of width x height samples on the context's stream, dst = avg(a, b) sample by sample; the sample
 * type comes from the context.  Pitches >= width samples; pointers, pitches and frame strides multiples of the sample size
 * (rows of all three planes that start on multiples of 16 bytes: 16 bytes per lane and access).  dst may be a or b exactly
 * (same pointer, pitch and frame stride: each sample is read by the thread that overwrites it); a dst whose bytes overlap a
 * or b in any other way is refused with SN_ERR_INVALID_ARG.  Nothing beyond width samples of a destination row is written.
 * A refused call queues nothing. */
int sn_merge_device(sn_context* ctx, int32_t nframes, const void* a, int64_t a_frame_stride, int32_t a_pitch, const void* b, int64_t b_frame_stride,
                    int32_t b_pitch, int32_t width, int32_t height, void* dst, int64_t dst_frame_stride, int32_t dst_pitch);
/* sn_turn_device of avg(a, b) in one kernel (the planes are read once and the average never reaches memory): a and b are
 * width x height, dst is height wide and width high; direction as for sn_turn_device.  dst must overlap neither a nor b. */
int sn_turn_merge_device(sn_context* ctx, int32_t direction, int32_t nframes, const void* a, int64_t a_frame_stride, int32_t a_pitch, const void* b,
                         int64_t b_frame_stride, int32_t b_pitch, int32_t width, int32_t height, void* dst, int64_t dst_frame_stride,
                         int32_t dst_pitch);

/* The rank repair of the anti-aliasing call (below: "Rank repair", which defines the arithmetic).  rank 0: off, and the
 * fields below it are ignored; 1..4 is the rank of the two order statistics of the source's 3 x 3 neighbourhood that bound
 * the result, as modes 1..4 of Repair in RemoveGrain / RgTools. */
typedef struct sn_aa_repair {
    int32_t struct_size; /* sizeof(sn_aa_repair) */
    int32_t rank;        /* 0 = off (the fields below are ignored); 1..4 */
    int32_t chroma;      /* 0: plane 0 only; 1: every processed plane */
    int32_t reserved[5]; /* zero */
} sn_aa_repair;          /* 32 bytes */

/* The rank repair on its own, for pipelines that keep frames on the device: `nframes` planes of width x height samples on
 * the context's stream; each sample of `aa` (the filtered plane R) is clamped into the rank range of the nine samples of
 * `src` (the plane S it was filtered from) around it and written to dst (see "Rank repair").  rank: 1..4; the sample type
 * comes from the context.  Pitches >= width samples; pointers, pitches and frame strides multiples of the sample size
 * (multiples of 16 on a side: 16 bytes per lane and access on that side).  dst must not overlap src, because the stencil
 * reads its neighbours.  dst may be aa exactly (same pointer, pitch and frame stride: each sample of R is read by the
 * thread that overwrites it); a dst whose bytes overlap src at all, or aa in any other way, is refused with
 * SN_ERR_INVALID_ARG ("... overlap ...").  Nothing beyond width samples of a destination row is written.  A refused call
 * queues nothing. */
int sn_repair_device(sn_context* ctx, int32_t rank, int32_t nframes, const void* src, int64_t src_frame_stride, int32_t src_pitch, const void* aa,
                     int64_t aa_frame_stride, int32_t aa_pitch, int32_t width, int32_t height, void* dst, int64_t dst_frame_stride,
                     int32_t dst_pitch);

/* The anti-aliasing idiom TurnLeft().SangNom2(order, aa, aac).TurnRight().SangNom2(order, aa, aac) as ONE call with
 * host planes (README.md:3 of the reference: "mainly used in anti-aliasing scripts"): the frame
 * crosses PCIe once each way and stays on the device between the two passes (two filter instances -- one for the
 * turned clip, one for the clip itself -- on one stream, sn_turn_device in between).  `cfg` describes the clip
 * (dh: see below; luma / chroma / isolated_planes / fresh_pool / device apply to both passes; max_batch >= 1: frames one
 * sn_aa_process_device_strided call may carry; host_depth: slots of the host ring, 0 = 4, allocated when
 * sn_aa_submit_host is first called; stream: the stream of the call's device work, NULL = one of its own; mode is
 * ignored: both passes run SN_MODE_AUTO); the turned clip must pass the reference's checks too (sn_aa_create reports the first
 * pass's message otherwise).  The result is what that script gives with the reference: two instances, so for widths
 * or heights that are not a multiple of 32 each pass carries its own pool history from frame to frame.  Not a
 * function of the reference; host/sangnom2_avs_plugin.cpp registers it as SangNomAA.
 *
 * With cfg.dh = 1 the call is TurnLeft().SangNom2(order, aa, aac, dh=true).TurnRight().SangNom2(order, aa, aac, dh=true):
 * enlargement by two in both directions, the SangNom counterpart of nnedi3_rpow2(2).  cfg.width / cfg.height and every
 * src plane, pitch and frame stride still describe the input clip; every dst plane is twice as wide and twice as high as
 * its source plane (dst pitch >= 2 * plane width * bytes_per_sample).  As in the reference, dh forces every plane through
 * both passes: luma and chroma are ignored.  The first instance filters the turned clip (height x width in, height x
 * 2 width out), the second one a clip of 2 width x height (sn_aa_get_info(ctx, 1): out_height = 2 height, pool_stride =
 * roundup(2 width, 32)); each is validated as SangNom2 validates it, the turned clip first (an odd width: "SangNom2:
 * height must be even."), and 2 width is held against the width limit.  The first pass carries history when height is
 * not a multiple of 32, the second when 2 width is not.  Both passes read every line of their source, so the turns are
 * whole turns, and the intermediates per processed plane and frame are the turned source, the first pass's output
 * (twice that) and the second pass's input (twice that again, up to pitch rounding): five plane sizes against three
 * without dh, counted against sn_policy.scratch_budget_mb in the same way.  On the host path a whole source frame goes
 * up and a frame four times its size comes down; nothing of it can be copied on the host.
 *
 * Anti-aliasing at source size (sn_aa_create_ex2 with sn_aa_options.reduce != 0; needs cfg.dh = 1, otherwise SN_ERR_CONFIG
 * "reduce needs dh"): both passes run exactly as above (sn_aa_get_info(ctx, 1) still reports the 2 width clip), their
 * 2W x 2H result E stays in an intermediate of the library (nine plane sizes with reduce, counted against
 * scratch_budget_mb like the others; a contra-sharpened plane adds one: four without dh, ten with reduce) and a reduction kernel writes the destination.  Every destination plane, pitch check
 * and frame stride of EVERY sn_aa_* entry point then describes the source geometry W_p x H_p (a packed or semi-planar dst
 * has rows for W), and on the host path a frame of the source's size comes down.  No counterpart in the reference (it has
 * no resampler); the arithmetic is defined here, exactly:
 *   `off` is the kept-field offset of the frame: 0 for order 1, 1 for order 2, parity ? 0 : 1 for order 0.  The source
 *   sample (x, y) reappears untouched at E[2y + oy][2x + ox] with oy = off and ox = 1 - off.  The reduction is a symmetric
 *   odd filter centred on that position, so the result has no sub-pixel shift; coordinates outside E are clamped to the edge.
 *     SN_AA_REDUCE_TENT = 1:     taps k = [1 2 1], shift s = 2 per direction.
 *     SN_AA_REDUCE_HALFBAND = 2: taps k = [-1 0 9 16 9 0 -1], shift s = 5 per direction (the sharper one).
 *   Let r be the radius (1 or 3), X = 2x + ox, Y = 2y + oy, cx(i) = clamp(i, 0, 2W-1) and cy(j) = clamp(j, 0, 2H-1).
 *   Integer samples (8..16 bit), all sums in signed 32-bit:
 *     h[j] = sum_i k[i] * E[cy(Y+j-r)][cx(X+i-r)]
 *     v    = sum_j k[j] * h[j]
 *     out  = clamp((v + (1 << (2s-1))) >> 2s, 0, 2^bits_per_sample - 1) with an arithmetic shift.
 *   |v| <= 36*36*65535 fits in 32 bits.  The clamp is to the clip's range, not the container's: a reduced 10-bit plane is
 *   always valid in an MSB or v210 destination.  For the tent kernel only the upper clamp can act, when E itself is out of range.
 *   Float samples: one rounding per written operation, in this order, with no contraction:
 *     tent:      h = (a[-1] + a[+1]) + (a[0] + a[0]);  v = (h[-1] + h[+1]) + (h[0] + h[0]);  out = v * 0.0625f
 *     half-band: h = ((a[-1] + a[+1]) * 9.0f + a[0] * 16.0f) - (a[-3] + a[+3]);  v is the same expression over h[-3..3];
 *                out = v * 0.0009765625f
 *   No clamp.
 *   The same reduction follows both arithmetics (sn_options.arithmetic); only E differs.  Every plane is reduced, because dh
 *   forces every plane through both passes.
 *
 * Edge mask (sn_aa_create_ex3 with mask->kind = SN_AA_MASK_SOBEL): what every anti-aliasing script built on SangNom does
 * behind the filter.  An edge mask is built from the SOURCE plane and the call's result is merged into the source through
 * it, in place on the destination behind the last step: flat areas and texture keep the source's samples untouched.  The
 * destination must have the source's size: dh = 0, or dh = 1 with a reduction; otherwise SN_ERR_CONFIG "SangNomAA: mask
 * needs the frame at source size (dh=false, or dh=true with reduce)", before a device is touched.  No scratch is added and
 * neither pass changes; source and destination must not overlap (already the rule).  The mask is computed per processed
 * plane from that plane's own source, with the same lo, hi, expand for every plane (subsampled chroma gets no luma-derived
 * mask).  Planes that are not processed are copied as without a mask.  Without dh the kept lines of the result are copies
 * of the source, so the merge leaves them as they are.  Neither the reference nor masktools defines these pixels; the
 * arithmetic is the library's own, exactly:
 *   S is the source plane (W x H), R the call's result for it, S(y, x) = S[clamp(y, 0, H-1)][clamp(x, 0, W-1)].
 *   Integer samples (8..16 bit), all in signed 32-bit:
 *     gx = (S(y-1,x+1) + 2 S(y,x+1) + S(y+1,x+1)) - (S(y-1,x-1) + 2 S(y,x-1) + S(y+1,x-1))
 *     gy = (S(y+1,x-1) + 2 S(y+1,x) + S(y+1,x+1)) - (S(y-1,x-1) + 2 S(y-1,x) + S(y-1,x+1))
 *     e  = (|gx| + |gy|) >> 2                  (a step of height d across a straight edge gives e = d)
 *     Tlo = lo << (bits_per_sample - 8),  Thi = hi << (bits_per_sample - 8)
 *     m0 = 0 if e <= Tlo;  256 else if e >= Thi;  else ((e - Tlo) * 256) / (Thi - Tlo)  (floor; the product is below 2^24)
 *     m  = m0 with expand = 0;  the maximum of m0 over the 3 x 3 neighbourhood (clamped coordinates) with expand = 1
 *     out = (S * (256 - m) + R * m + 128) >> 8
 *   m = 0 gives S exactly and m = 256 gives R exactly; no clamp is needed.
 *   Float samples: one rounding per written operation, no contraction:
 *     col(dx) = (S(y-1,x+dx) + S(y+1,x+dx)) + (S(y,x+dx) + S(y,x+dx));  row(dy) = (S(y+dy,x-1) + S(y+dy,x+1)) + (S(y+dy,x) + S(y+dy,x))
 *     gx = col(+1) - col(-1);  gy = row(+1) - row(-1);  e = (|gx| + |gy|) * 0.25f
 *     Tlo = (float)lo / 255.0f,  Thi = (float)hi / 255.0f,  k = 256.0f / (Thi - Tlo): single precision, computed on the host
 *       (k only when hi > lo)
 *     m0 = 0 if !(e > Tlo) (a NaN keeps the source);  256 else if e >= Thi;  else min(256, (int)((e - Tlo) * k)) (truncation)
 *     m as above
 *     out = S if m == 0;  R if m == 256;  else S + (R - S) * ((float)m * 0.00390625f)
 *   Chroma through the luma plane's mask (sn_aa_create_ex4 with sn_aa_mask_ex.chroma = SN_AA_MASK_CHROMA_LUMA; opt-in): what
 *   the scripts do that the mask was modelled on -- one mask from luma merges all three planes, chroma through the mask scaled
 *   to chroma's geometry.  Plane 0 is merged as above.  L is the SOURCE luma plane, Wl x Hl, and m_L the m above computed on
 *   L at luma resolution with the call's lo, hi, expand and the clip's bit depth (float: the float rules, NaN included).
 *   For a chroma plane of W x H samples with Wl = W << sw and Hl = H << sh (sw, sh in 0..2) and n = sw + sh:
 *     mc(y, x) = (sum_{j < 2^sh} sum_{i < 2^sw} m_L[(y << sh) + j][(x << sw) + i] + ((1 << n) >> 1)) >> n
 *   all in signed 32-bit (the sum is at most 16 * 256); for n = 0, mc = m_L.  A block of zeros gives 0 exactly and a block of
 *   256 gives 256 exactly, so "m = 0 gives S, m = 256 gives R" still holds.  out is the merge formula above (integer and
 *   float) with S = the chroma source, R = the chroma result and m = mc.  Where the mask itself is written
 *   (sn_mask_merge_luma_device with aa == NULL) it is mc through the rule of sn_mask_merge_device: integers
 *   (mc * (2^bits - 1) + 128) >> 8, float (float)mc * 0.00390625f.  The block mean places a chroma sample at the centre of its
 *   block of luma samples; for left-sited (MPEG-2) chroma that is a quarter of a luma pixel off horizontally.  No siting option
 *   is offered.  These pixels are the library's own too: neither the reference nor masktools defines them.
 *   Rules of the call: planes 1 and 2, where processed, are merged through mc; a Y clip accepts the option and it has no
 *   effect; chroma = 0 without dh copies chroma as without a mask; cfg.luma == 0 without dh and with chroma != 0 is refused
 *   before a device is touched, SN_ERR_CONFIG "SangNomAA: a luma-derived chroma mask needs luma processed (luma=true)" (the
 *   host routes never upload a plane that is not processed).  No scratch is added and neither pass changes.
 *
 * Contra-sharpening (sn_aa_create_ex5 with sharpen->amount != 0; opt-in): SangNom interpolates every second line from a
 * smoothed cost field, and the result is softer than the source.  The scripts answer with a sharpening that is allowed only
 * as far as the filter changed the picture and only in the direction of the source (daa, QTGMC's sharpening branch, the
 * ContraSharpening helper of the *AA collections).  The stage runs behind the last step (the second pass, or the reduction)
 * and before the edge mask, which then merges the SHARPENED result into the source (m = 0 still gives S exactly; the
 * mask's own arithmetic, chroma through the luma mask included, does not change).  Like the mask it needs the frame at source
 * size: amount != 0 with dh = 1 and no reduction is SN_ERR_CONFIG "SangNomAA: sharpen needs the frame at source size
 * (dh=false, or dh=true with reduce)", before a device is touched.  Only processed planes are sharpened -- plane 0 with
 * chroma = 0, every processed plane with chroma = 1 --; a plane that is merely copied stays a copy, and with chroma = 0
 * planes 1 and 2 are what they are without the stage.  The last step writes each sharpened plane into one more intermediate
 * of the library, of the destination's geometry: one plane size per sharpened plane and frame, counted against
 * scratch_budget_mb like the others (four plane sizes instead of three without dh, ten instead of nine with reduce); the
 * sharpening kernel writes the destination from it and the source.  Neither the reference nor any script defines these
 * pixels; the arithmetic is the library's own, exactly:
 *   S is the source plane (W x H), R the call's result for it, P(y, x) = P[clamp(y, 0, H-1)][clamp(x, 0, W-1)] for either
 *   plane; amount is 1..255 and 64 is unity.
 *   Integer samples (8..16 bit), all in signed 32-bit:
 *     h(y, x) = R(y, x-1) + 2 R(y, x) + R(y, x+1)
 *     B       = (h(y-1, x) + 2 h(y, x) + h(y+1, x) + 8) >> 4       ([1 2 1] x [1 2 1], rounded)
 *     d       = R(y, x) - B                                        (what an unsharp mask of strength 1 adds)
 *     d1      = sgn(d) * ((|d| * amount) >> 6)                      (|d| * 255 < 2^24)
 *     D(j, i) = S(j, i) - R(j, i)                                   (what the filter took away, per sample)
 *     mn      = min(0, min of D over the 3 x 3 neighbourhood),  mx = max(0, max of D over the same)  (clamped coordinates)
 *     c       = min(max(d1, mn), mx)
 *     out     = min(max(R(y, x) + c, 0), 2^bits_per_sample - 1)
 *   Because mn <= 0 <= mx, c never exceeds d1 in magnitude, never points away from every nearby S - R, and is 0 wherever
 *   the filter changed nothing in the neighbourhood: S == R over a 3 x 3 block gives out == R.  The clamp is to the clip's
 *   range, as in the reduction: a sharpened 10-bit plane is always valid in an MSB or v210 destination.  Only without reduce
 *   can R itself exceed that range (a container wider than the clip), and then it is clamped too.
 *   Float samples: one rounding per written operation, no contraction:
 *     h  = (R(y,x-1) + R(y,x+1)) + (R(y,x) + R(y,x));  v = (h(y-1) + h(y+1)) + (h(y) + h(y));  B = v * 0.0625f
 *     d  = R(y,x) - B;  d1 = d * k,  k = (float)amount * 0.015625f (exact)
 *     mn = mx = 0.0f;  for every (j, i) of the 3 x 3 neighbourhood: t = S(j,i) - R(j,i); if (t < mn) mn = t; if (t > mx) mx = t;
 *       (a NaN t is ignored)
 *     c  = d1; if (c < mn) c = mn; if (c > mx) c = mx;
 *     out = R(y,x) if d1 is NaN or c == 0 (either zero);  else R(y,x) + c.        No clamp.
 *   No NaN is generated into the output:
 *     an infinite or NaN R(y,x) makes B infinite or NaN, so d = R - B and with it d1 is NaN, and R(y,x) is copied;
 *     otherwise R(y,x) is finite, and c is d1, mn or mx, none of which is NaN here (mn and mx never take a NaN);
 *     a finite value plus a value that is no NaN is no NaN: every output sample is a copy of R or such a sum.
 *
 * Both fields (sn_aa_create_ex6 with fields->mode = SN_AA_FIELDS_BOTH; opt-in): a pass keeps one field and interpolates the
 * other, so half of the lines of each pass come out untouched.  The single-field scripts the contra-sharpening comes from
 * (daa and its relatives) interpolate BOTH fields and average: Merge(SangNom2(order=1), SangNom2(order=2)).  Every line is
 * then half source and half interpolation, and the result is symmetric in the two fields.  The definition is the library's own:
 *   For a clip c let A(c) = avg(SangNom2(c, order=1), SangNom2(c, order=2)), sample by sample.  The two SangNom2 are two
 *   separate filter instances, each with its own pool and history.
 *   The call computes A( A(c.TurnLeft()).TurnRight() ): four instances in all.  Each carries history exactly as a reference
 *   instance would: widths that are not a multiple of 32 carry state from frame to frame, and Y, U and V share the pool
 *   unless isolated_planes or fresh_pool is set.
 *   avg, per sample type:
 *     integer samples of any depth in 8- or 16-bit containers: (a + b + 1) >> 1, computed without overflow;
 *     float samples: (a + b) * 0.5f in single precision, in that order; any NaN result is written as the one pattern
 *     0x7FC00000 (x86 and gfx950 disagree on which NaN an add returns).
 * The four instances are created from the same configuration with only `order` replaced: cfg.order and the per-frame parity
 * have NO influence in this mode -- the twins always use orders 1 and 2, which take no parity.  Mask (own and luma-derived),
 * sharpening, luma / chroma, isolated_planes, fresh_pool, arithmetic, column_parts, policy and options apply unchanged; the
 * sharpening and the mask see the averaged result of the second pass.  mode = BOTH with cfg.dh is SN_ERR_CONFIG "SangNomAA: both
 * fields needs dh=false", before a device is touched: the two dh results place the source on different lines, and their
 * average is a half-line blur, not an anti-aliaser (reduce needs dh and falls with it).  A chunk runs: turn left (every line,
 * one launch), first pass order 1, first pass order 2, turn right of the average of the two (one kernel, sn_turn_merge_device),
 * second pass order 1 into the destination (or the sharpening's intermediate), second pass order 2 into one more intermediate,
 * the average in place (sn_merge_device), then sharpening and mask as ever.  A processed plane costs five plane sizes of
 * intermediates per frame instead of three (six instead of four where it is sharpened), counted against scratch_budget_mb.
 * sn_aa_get_info / sn_aa_get_parts_info take pass 2 and 3 for the order-2 twins of passes 0 and 1 (SN_ERR_INVALID_ARG in
 * one-field mode).  Measured on one MI355X the call takes 1.97 times the one-field call at 1080p 4:2:0 and 1.99 times at 2160p
 * Y8: the passes dominate and double.
 *
 * Rank repair (sn_aa_create_ex7 with repair->rank != 0; opt-in): where SangNom's cost ladder picks a wrong direction, an
 * interpolated sample is the mean of two samples up to three columns away on the neighbouring lines; it can lie outside
 * anything the source has nearby and shows as a bright or dark speck on or beside an edge.  The contra-sharpening only
 * limits its own correction, and the mask hands edges through.  The scripts answer with Repair(filtered, source, mode) of
 * RemoveGrain / RgTools, modes 1..4: each filtered sample is clamped into the range spanned by the rank-th smallest and
 * the rank-th largest of the nine source samples around it.  The stage runs behind the contra-sharpening (or behind the
 * last step where there is none) and before the edge mask, in place on the destination: a sample's result depends on R at
 * that sample only, so no workgroup reads what another writes.  It adds no intermediate and nothing to scratch_budget_mb.
 * Like the mask it needs the frame at source size: rank != 0 with dh = 1 and no reduction is SN_ERR_CONFIG "SangNomAA:
 * repair needs the frame at source size (dh=false, or dh=true with reduce)", before a device is touched.  It works with
 * both fields, either mask form and the sharpening, through every sn_aa_* entry point.  Only processed planes are repaired
 * -- plane 0 with chroma = 0, every processed plane with chroma = 1 --; a plane that is merely copied stays a copy.  The
 * arithmetic is the library's own, exactly:
 *   S is the source plane (W x H), R the call's result for it (sharpened, where the call sharpens);
 *   S(y, x) = S[clamp(y, 0, H-1)][clamp(x, 0, W-1)];
 *   a[1] <= ... <= a[9] are the nine samples S(y+j, x+i), j, i in {-1, 0, 1}, the centre included;
 *   lo = a[rank], hi = a[10 - rank].
 *   Integer samples (8..16 bit): out = min(max(R(y,x), lo), hi).  No range clamp: out is R, or a source sample.
 *   Float samples:
 *     if R(y,x) is a NaN, or any of the nine source samples is a NaN: out = R(y,x), bit for bit;
 *     otherwise the nine are ordered by <, with -0.0 and +0.0 equal;
 *     out = R(y,x), bit for bit, where lo <= R(y,x) <= hi; otherwise out is the bound that R crossed, and a bound that is a
 *     zero is written as +0.0 (by a select, not by an addition: which of two equal zeros a selection network delivers
 *     does not show).  Infinities are ordinary values.  No NaN is generated, and there is no float arithmetic at all.
 *   What the ranks mean for samples the filter did not touch: without dh the kept lines of R are copies of S.  Rank 1 leaves
 *   them alone, because the centre is one of the nine and so lies within [a[1], a[9]].  Ranks 2..4 also move a SOURCE sample
 *   that is one of the rank - 1 smallest or rank - 1 largest of its own neighbourhood -- an isolated bright or dark pixel
 *   of the source is pulled in --, exactly as Repair does in the scripts; the mask, which runs later, gives flat areas back
 *   to the source.  Modes 5 and up of Repair (line pairs, modes built on the centre) are not offered. */
enum { SN_AA_REDUCE_NONE = 0, SN_AA_REDUCE_TENT = 1, SN_AA_REDUCE_HALFBAND = 2 };
typedef struct sn_aa_options {
    int32_t struct_size; /* sizeof(sn_aa_options) */
    int32_t reduce;      /* SN_AA_REDUCE_* */
    int32_t reserved[6]; /* zero */
} sn_aa_options;         /* 32 bytes */
typedef struct sn_aa_context sn_aa_context;
int sn_aa_create(const sn_config* cfg, sn_aa_context** out);
int sn_aa_create_with_policy(const sn_config* cfg, const sn_policy* policy /* NULL = defaults; both passes */, sn_aa_context** out);
int sn_aa_create_ex(const sn_config* cfg, const sn_policy* policy, const sn_options* options /* both passes */, sn_aa_context** out);
/* sn_aa_create_ex is sn_aa_create_ex2 with aa_options = NULL (the defaults: no reduction).  A bad struct_size, a reduce
 * outside 0..2 or a non-zero reserved word: SN_ERR_INVALID_ARG, naming the field. */
int sn_aa_create_ex2(const sn_config* cfg, const sn_policy* policy, const sn_options* options, const sn_aa_options* aa_options /* NULL = defaults */,
                     sn_aa_context** out);
int sn_aa_get_reduce(sn_aa_context* ctx); /* SN_AA_REDUCE_* of a live context; -1 for NULL */
/* sn_aa_create_ex2 is sn_aa_create_ex3 with mask = NULL (no mask).  A bad struct_size, a kind outside 0..1, lo or hi outside
 * 0..255, lo > hi, an expand outside 0..1 or a non-zero reserved word: SN_ERR_INVALID_ARG, naming the field; with kind =
 * SN_AA_MASK_NONE only struct_size and kind are looked at. */
int sn_aa_create_ex3(const sn_config* cfg, const sn_policy* policy, const sn_options* options, const sn_aa_options* aa_options /* NULL = defaults */,
                     const sn_aa_mask* mask /* NULL = none */, sn_aa_context** out);
int sn_aa_get_mask(sn_aa_context* ctx, sn_aa_mask* out /* struct_size set by the caller */); /* kind 0 when there is none */
/* sn_aa_create_ex3 is sn_aa_create_ex4 with mask_ex = NULL (the defaults: every plane through its own mask).  A bad
 * struct_size, a chroma outside 0..1 or a non-zero reserved word: SN_ERR_INVALID_ARG, naming sn_aa_mask_ex.<field>; with
 * mask == NULL or kind = SN_AA_MASK_NONE only struct_size of mask_ex is looked at. */
int sn_aa_create_ex4(const sn_config* cfg, const sn_policy* policy, const sn_options* options, const sn_aa_options* aa_options /* NULL = defaults */,
                     const sn_aa_mask* mask /* NULL = none */, const sn_aa_mask_ex* mask_ex /* NULL = defaults */, sn_aa_context** out);
int sn_aa_get_mask_ex(sn_aa_context* ctx, sn_aa_mask_ex* out /* struct_size set by the caller */); /* chroma 0 when there is no mask */
/* sn_aa_create_ex4 is sn_aa_create_ex5 with sharpen = NULL (no contra-sharpening).  A bad struct_size, an amount outside
 * 0..255, a chroma outside 0..1 or a non-zero reserved word: SN_ERR_INVALID_ARG, naming sn_aa_sharpen.<field>; with amount = 0
 * only struct_size is looked at. */
int sn_aa_create_ex5(const sn_config* cfg, const sn_policy* policy, const sn_options* options, const sn_aa_options* aa_options /* NULL = defaults */,
                     const sn_aa_mask* mask /* NULL = none */, const sn_aa_mask_ex* mask_ex /* NULL = defaults */,
                     const sn_aa_sharpen* sharpen /* NULL = off */, sn_aa_context** out);
int sn_aa_get_sharpen(sn_aa_context* ctx, sn_aa_sharpen* out /* struct_size set by the caller */); /* amount 0 when off */
/* sn_aa_create_ex5 is sn_aa_create_ex6 with fields = NULL (one field per pass).  A bad struct_size, a mode outside 0..1 or a
 * non-zero reserved word: SN_ERR_INVALID_ARG, naming sn_aa_fields.<field>; with mode = SN_AA_FIELDS_ONE only struct_size is
 * looked at. */
int sn_aa_create_ex6(const sn_config* cfg, const sn_policy* policy, const sn_options* options, const sn_aa_options* aa_options /* NULL = defaults */,
                     const sn_aa_mask* mask /* NULL = none */, const sn_aa_mask_ex* mask_ex /* NULL = defaults */,
                     const sn_aa_sharpen* sharpen /* NULL = off */, const sn_aa_fields* fields /* NULL = one field */, sn_aa_context** out);
int sn_aa_get_fields(sn_aa_context* ctx, sn_aa_fields* out /* struct_size set by the caller */);
/* sn_aa_create_ex6 is sn_aa_create_ex7 with repair = NULL (no rank repair).  A bad struct_size, a rank outside 0..4, a chroma
 * outside 0..1 or a non-zero reserved word: SN_ERR_INVALID_ARG, naming sn_aa_repair.<field>; with rank = 0 only struct_size
 * is looked at. */
int sn_aa_create_ex7(const sn_config* cfg, const sn_policy* policy, const sn_options* options, const sn_aa_options* aa_options /* NULL = defaults */,
                     const sn_aa_mask* mask /* NULL = none */, const sn_aa_mask_ex* mask_ex /* NULL = defaults */,
                     const sn_aa_sharpen* sharpen /* NULL = off */, const sn_aa_fields* fields /* NULL = one field */,
                     const sn_aa_repair* repair /* NULL = off */, sn_aa_context** out);
int sn_aa_get_repair(sn_aa_context* ctx, sn_aa_repair* out /* struct_size set by the caller */); /* rank 0 when off */
int sn_aa_process_host(sn_aa_context* ctx, const void* const src[3], const int32_t src_pitch[3], void* const dst[3],
                       const int32_t dst_pitch[3], int32_t parity);
const char* sn_aa_last_error(const sn_aa_context* ctx); /* ctx == NULL: last failed sn_aa_create on this thread */
void sn_aa_destroy(sn_aa_context* ctx); /* waits for frames still in flight */

/* The same idiom on `nframes` (<= cfg.max_batch) device-resident frames, laid out as for sn_process_device_strided;
 * asynchronous on the call's stream.  Frame f of the result is what nframes calls of sn_aa_process_host give in order
 * (each pass sees its frames in order, so history-carrying clips are the script's).  The frames are walked in chunks:
 * turn, first pass, turn back, second pass; the intermediates are allocated at creation and count against
 * sn_policy.scratch_budget_mb, a batch beyond what fits takes more chunks.  A turn writes only the lines the following
 * pass keeps (with dh: every line); a plane that is not processed (luma / chroma = 0, never with dh) is copied from src
 * to dst once. */
int sn_aa_process_device_strided(sn_aa_context* ctx, int32_t nframes, const void* const src[3], const int64_t src_frame_stride[3],
                                 const int32_t src_pitch[3], void* const dst[3], const int64_t dst_frame_stride[3],
                                 const int32_t dst_pitch[3], const int32_t* parity /* NULL = all 1 */);
/* Waits for everything the context has queued (device batches and host frames in flight). */
int sn_aa_synchronize(sn_aa_context* ctx);
/* The hipStream_t of the call's device work (cfg.stream if one was given); NULL for a NULL context. */
void* sn_aa_get_stream(sn_aa_context* ctx);
/* sn_get_info of one of the filter instances: pass 0 is the turned clip's, pass 1 the clip's; with SN_AA_FIELDS_BOTH pass 2
 * and 3 are their order-2 twins (the instances of pass 0 and 1 then run order 1). */
int sn_aa_get_info(sn_aa_context* ctx, int32_t pass, sn_info* info);
int sn_aa_get_parts_info(sn_aa_context* ctx, int32_t pass, sn_parts_info* info);
/* The host ring of the anti-aliasing call, with the contract of sn_host_slots / sn_submit_host / sn_collect_host: slots
 * are taken round-robin, SN_ERR_BUSY when the next slot has not been collected, and collecting in submission order never
 * waits for a later frame.  Upload, device work and download of different frames overlap; the device work runs in
 * submission order.  Planes inside memory pinned with sn_pin_host_buffer are transferred as they lie (keep them until
 * the slot is collected), others are staged.  sn_aa_host_slots returns the number of slots (<= 0 on failure). */
int sn_aa_host_slots(sn_aa_context* ctx);
int sn_aa_submit_host(sn_aa_context* ctx, const void* const src[3], const int32_t src_pitch[3], int32_t parity, int32_t* slot);
int sn_aa_collect_host(sn_aa_context* ctx, int32_t slot, void* const dst[3], const int32_t dst_pitch[3]);

/* Decoder and encoder surfaces: device-resident frames whose chroma is ONE plane of U,V pairs (semi-planar) -- NV12
 * (8-bit 4:2:0), P010 / P016 (the same with 16-bit words), NV16 (4:2:2), NV24 (4:4:4) -- in and out of the two batch
 * calls, without the caller converting anything.  A surface description names its layout; source and destination are
 * independent (NV12 in and planar out, or the reverse, are fine).
 *   SN_LAYOUT_PLANAR      plane[0..2] = Y, U, V, as for sn_process_device_strided (a Y clip: plane[0] only)
 *   SN_LAYOUT_SEMIPLANAR  plane[0] = Y, plane[1] = the UV plane: row y of frame f is U0 V0 U1 V1 ... at plane[1] +
 *                         f * frame_stride[1] + y * pitch[1], 2 * chroma width samples long; plane[2] must be NULL and
 *                         pitch[2] / frame_stride[2] are ignored
 *   SN_LAYOUT_PLANAR_MSB, SN_LAYOUT_SEMIPLANAR_MSB
 *                         the same two, except that every sample is a 16-bit word whose bits_per_sample significant bits
 *                         are the HIGH bits (P010 on a 10-bit context, P012 on a 12-bit one; see below)
 * Pointers, pitches and frame strides need the alignment of the sample size only (a UV plane may start at an odd byte);
 * surfaces whose bases, pitches and frame strides are multiples of 16 bytes -- every decoder's -- move 16 bytes per
 * lane and access.  With both sides SN_LAYOUT_PLANAR the call IS sn_process_device_strided / sn_aa_process_device_strided
 * (same checks, same result, no scratch).  Otherwise the result for a semi-planar surface is, bit for bit, what the planar
 * call gives on the de-interleaved planes, re-interleaved, in every configuration the context accepts: the library splits
 * the lines the filter keeps of a semi-planar source into planar chroma scratch of its own (every line with dh and in the
 * anti-aliasing call), runs its passes there, and merges their output into the destination's UV plane; luma never goes
 * through scratch (but for an MSB-aligned source, below).  Chroma that is not processed (chroma = 0 without dh) never
 * reaches a pass: with the same layout on both sides the UV plane is copied once, with different layouts it is converted
 * straight from src to dst.
 * Scratch: two planes of the source's and two of the destination's chroma geometry per frame, pitches rounded up to 256
 * bytes, for min(max_batch, what fits) frames, where a SIXTEENTH of sn_policy.scratch_budget_mb is what may be taken
 * (1.5 GiB by default: 180 frames of 8-bit 2160p 4:2:0, 90 of 16-bit) and one frame is always held; a batch beyond that
 * is walked in chunks, in order, so history-carrying clips stay exact.  It is allocated by the first call that has a
 * semi-planar side with processed chroma, before anything of that call is queued, and freed with the context.
 * Both calls are asynchronous on the context's stream, like the planar calls; that first call allocates and may
 * synchronise the stream.
 * P010 / P012 keep the sample in the high bits of a 16-bit word.  There are two ways to take them, and they give different
 * pixels: the floor of stage 2 (sum / 16) does not commute with the shift, so low bits differ.
 *   - As a 16-bit clip: a context with bits_per_sample = 16 and SN_LAYOUT_SEMIPLANAR.  The result is what the reference
 *     gives on that 16-bit clip, low bits of the words included.
 *   - As the 10- / 12-bit clip it is: a context with bits_per_sample = 10 (12) and SN_LAYOUT_SEMIPLANAR_MSB.  The result is
 *     the reference's on the YUV420P10 (P12) clip, MSB-aligned again.
 * The _MSB layouts: the shift s = 16 - bits_per_sample is implied (6 for P010, 4 for P012, 0 on a 16-bit context, where the
 * _MSB layouts are the plain ones).  With ss and ds the shifts of the two sides (0 for a layout without _MSB) the destination
 * holds, bit for bit, what the call gives on src >> ss (logical, every plane and line), every sample shifted left by ds:
 * interpolated lines, kept lines, planes that are only copied and the copied border line alike.  Low bits of an MSB source
 * never reach the output (a plane copied between two MSB sides is masked), and the input is always in range for the context.
 * (The output need not be: like the reference the filter does not clamp to the clip's range, and an interpolated sample above
 * 2^bits - 1 loses its high bits when it is shifted up inside its 16-bit word.)
 * The two sides are independent: P010 in and planar YUV420P10 out is fine, as is every other pairing.  The passes see
 * LSB-aligned planes: the planes of an MSB source are shifted down into scratch (its UV plane inside the split; luma into a
 * luma plane of scratch, pitch rounded up to 256 bytes, which an MSB source with processed luma adds to the sum below), those
 * of an MSB destination are shifted up where the passes wrote them (its UV plane inside the merge).  A context that first
 * needs the luma scratch after the chroma scratch (or the reverse) gives back what it held and takes both under the same rule.
 * SN_ERR_INVALID_ARG names the field: struct_size, layout, reserved, plane[2] set with SN_LAYOUT_SEMIPLANAR, a NULL
 * plane, a pitch below the row (the UV plane's row is 2 * chroma width * bytes_per_sample; the anti-aliasing call with dh
 * writes planes twice as wide and twice as high: 2 * (2 * chroma width) * bytes_per_sample).  SN_ERR_UNSUPPORTED:
 * SN_LAYOUT_SEMIPLANAR on a context with num_planes == 1 or bytes_per_sample == 4 (no such surface exists); an _MSB
 * layout on a context with bytes_per_sample != 2 (the text names layout).  A refused call queues nothing and leaves the
 * context usable.
 *
 * Packed 4:2:2 -- what SDI / HDMI capture and uncompressed intermediates hand over: ONE plane that holds Y, U and V.
 *   SN_LAYOUT_PACKED_YUYV      Y0 U0 Y1 V0 ..., samples of the context's type (YUY2 on an 8-bit context, Y216 on a 16-bit one)
 *   SN_LAYOUT_PACKED_UYVY      U0 Y0 V0 Y1 ... (UYVY; v216 on a 16-bit context)
 *   SN_LAYOUT_PACKED_YUYV_MSB  as PACKED_YUYV, 16-bit words with the sample in the high bits (Y210 on a 10-bit context, Y212
 *                              on a 12-bit one); the shift is 16 - bits_per_sample as for the other _MSB layouts
 *   SN_LAYOUT_PACKED_UYVY_MSB  as PACKED_UYVY, MSB-aligned
 *   SN_LAYOUT_PACKED_V210      v210, 10-bit contexts only: blocks of 16 bytes, four little-endian 32-bit words for six pixels,
 *                              three 10-bit fields per word at bits 0-9, 10-19 and 20-29:
 *                                word 0 = U0 | Y0 << 10 | V0 << 20      word 1 = Y1 | U1 << 10 | Y2 << 20
 *                                word 2 = V1 | Y3 << 10 | U2 << 20      word 3 = Y4 | V2 << 10 | Y5 << 20
 *                              The width is even, so a partial last block holds 2 or 4 pixels.  On input bits 30-31 of every
 *                              word and the fields of pixels >= width are ignored; on output every field is sample & 0x3FF,
 *                              bits 30-31 are zero and the fields of pixels >= width are zero.  (The filter does not clamp: an
 *                              interpolated sample above 1023 loses its high bits, as in an MSB destination.)
 * (Values 4..7 are not layouts.)  plane[0] / pitch[0] / frame_stride[0] describe the surface; plane[1] and plane[2] must be
 * NULL (SN_ERR_INVALID_ARG names the field), their pitches and strides are ignored.  A row of luma width w -- the side's own:
 * the anti-aliasing call's dh destination is 2 w wide -- is 2 * w * bytes_per_sample bytes for YUYV / UYVY and 16 * ceil(w / 6)
 * for v210; pitch[0] below that is SN_ERR_INVALID_ARG naming pitch[0].  Base, pitch and frame stride are multiples of the sample
 * size, for v210 of 4 (the conventional v210 pitch, a multiple of 128, is accepted and not required); surfaces whose base,
 * pitch and frame stride are multiples of 16 move 16 bytes per access.  The context must be 4:2:2 with integer samples
 * (num_planes == 3, sub_w == 1, sub_h == 0, bytes_per_sample 1 or 2), with bytes_per_sample == 2 for the _MSB forms and
 * bits_per_sample == 10 for v210; anything else is SN_ERR_UNSUPPORTED with "layout" in the text.
 * One rule: the destination holds, bit for bit, what the planar call gives on the unpacked planes (MSB words shifted down,
 * v210 fields extracted), packed as the destination's layout says (MSB shift up, v210 mask) -- in every configuration the
 * context accepts and in both calls.  The two sides are independent: packed pairs with planar, semi-planar (NV16) and the
 * other packed layouts in either direction.  Bytes of a destination row beyond the row size, and everything between rows,
 * are never written; the source is never written.
 * A packed source is unpacked into planar scratch (the lines the passes keep; every line with dh, in the anti-aliasing call and
 * when a plane is only copied), the passes run there, and a packed destination is packed from planar scratch behind them, all
 * lines.  A plane that is not processed never reaches a pass: it goes from the unpacked source to the destination.  A packed
 * source frame counts once in split_frames, a packed destination frame once in merged_frames; copied_frames keeps its meaning.
 * Scratch per frame of a call with a packed side, pitches rounded up to 256 bytes (R(x) = x rounded up to 256; w, h the
 * source's luma geometry, W, H the destination's, B = bytes_per_sample):
 *     source packed, MSB-aligned or semi-planar:   2 * R(w / 2 * B) * h   (U and V in)
 *     source packed or MSB-aligned:                + R(w * B) * h         (Y in)
 *     destination packed or semi-planar:           2 * R(W / 2 * B) * H   (U and V out)
 *     destination packed:                          + R(W * B) * H         (Y out)
 * for min(max_batch, what a sixteenth of the budget holds, at least 1) frames, as above.  A context whose need grows gives
 * back what it holds and takes the union of what it held and what it needs now; the calls without a packed side ask for what
 * they always did. */
enum {
    SN_LAYOUT_PLANAR = 0, SN_LAYOUT_SEMIPLANAR = 1, SN_LAYOUT_PLANAR_MSB = 2, SN_LAYOUT_SEMIPLANAR_MSB = 3,
    SN_LAYOUT_PACKED_YUYV = 8, SN_LAYOUT_PACKED_UYVY = 9, SN_LAYOUT_PACKED_YUYV_MSB = 10, SN_LAYOUT_PACKED_UYVY_MSB = 11,
    SN_LAYOUT_PACKED_V210 = 12
};
typedef struct sn_surfaces {
    int32_t struct_size;      /* = sizeof(sn_surfaces)                                        */
    int32_t layout;           /* SN_LAYOUT_*                                                 */
    void*   plane[3];         /* SEMIPLANAR: plane[1] = the UV plane, plane[2] = NULL         */
    int32_t pitch[3];         /* bytes; SEMIPLANAR: pitch[1] >= 2 * chroma width * bytes_per_sample */
    int32_t reserved;         /* zero                                                        */
    int64_t frame_stride[3];  /* bytes, as for sn_process_device_strided                     */
} sn_surfaces;
int sn_process_device_surfaces(sn_context* ctx, int32_t nframes, const sn_surfaces* src, const sn_surfaces* dst,
                               const int32_t* parity /* NULL = all 1 */);
int sn_aa_process_device_surfaces(sn_aa_context* ctx, int32_t nframes, const sn_surfaces* src, const sn_surfaces* dst,
                                  const int32_t* parity /* NULL = all 1 */);
/* What the surface calls of a context have done so far (all zero while every call had planar surfaces on both sides). */
typedef struct sn_surface_info {
    int32_t struct_size, reserved;
    int64_t scratch_bytes;     /* planar scratch this context holds for the call: chroma plus luma (0 until first needed) */
    int64_t split_frames;      /* frames whose UV plane was split into U and V for the passes                  */
    int64_t merged_frames;     /* frames whose U and V were merged into a UV plane                             */
    int64_t copied_frames;     /* frames whose unprocessed chroma went from src to dst without a pass (copied or converted) */
} sn_surface_info;
int sn_get_surface_info(sn_context* ctx, sn_surface_info* info);
int sn_aa_get_surface_info(sn_aa_context* ctx, sn_surface_info* info);

int sn_synchronize(sn_context* ctx);
void* sn_get_stream(sn_context* ctx); /* the hipStream_t the context launches on */
int sn_get_info(sn_context* ctx, sn_info* info);
int sn_get_parts_info(sn_context* ctx, sn_parts_info* info); /* synchronises the stream */

/* Test hook: copy the device scratch pool of batch slot `slot` to host memory
 * (9 x pool_rows x pool_stride elements).  Synchronises the stream. */
int sn_debug_read_pool(sn_context* ctx, int32_t slot, void* host_dst, size_t bytes);

/* Test hook for the fused 4:2:0 sweeps: the smoothed rows one plane's sweep left for the next one
 * (which = 0: luma -> U, 1: U -> V) of batch slot 0, rearranged to 9 x coupled_rows x width samples --
 * what rows 0..coupled_rows-1 of the reference's shared pool (src/SangNom2.cpp:322-329) hold at that
 * point, row 0 unused.  Synchronises the stream. */
int sn_debug_read_coupled_rows(sn_context* ctx, int32_t which, void* host_dst, size_t bytes);

/* Test hook for the row-band sweeps that serve small launches in SN_MODE_AUTO (a frame is cut into bands of
 * rows that start `warm_rows` rows early from a guessed state and are verified; a frame that fails the check is
 * redone by the pool path): bands > 0 forces that many bands per frame, 0 restores the automatic choice, < 0
 * turns the bands off; warm_rows = 0 restores the default run-up.  A run-up of 1 makes nearly every frame fail. */
int sn_debug_set_bands(sn_context* ctx, int32_t bands, int32_t warm_rows);

/* Test hook for the column parts (sn_options.column_parts = 1; tests and the bench tool only): parts > 0 forces that
 * many parts for every 16-bit or float plane on its own that is wide enough to hold them, planes that fit one workgroup
 * included; 0 restores the automatic choice.  ghost_columns > 0 (a multiple of 8) moves every seam to that distance from
 * the end of the window left of it (windows keep their widths): 8 makes nearly every frame fail the check; 0 restores the
 * default.  SN_ERR_UNSUPPORTED without the option. */
int sn_debug_set_column_parts(sn_context* ctx, int32_t parts, int32_t ghost_columns);

/* Test hook for the chains over several workgroups per cost buffer (sn_policy.chain): the NEXT such launch starts with
 * its fault word up, as if a workgroup had given up waiting at once -- its waves then take rows before they are written,
 * as after a real time-out -- so that the guarded redo behind the launch has something to repair.  The frames must come
 * out right and sn_info.chain_redone must count the launch.  SN_ERR_UNSUPPORTED if the context has not run a chain yet. */
int sn_debug_raise_chain_fault(sn_context* ctx);

int sn_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
