"""The shortest and the narrowest planes through every route of the library (tests/test_small_planes_gpu.py runs them on the
device, tests/test_small_planes_cpu.py checks the table itself).  TEST INFRASTRUCTURE ONLY.

Which kernels serve a launch, and with what row counts, is decided on the host by a handful of rules over the planes' geometry.
Each of them has a boundary at the lower end of the geometry -- a plane with no interpolated row, a pool of one row, a chroma
plane too short for the one-sweep form -- and the tables below are derived from the rules so that every boundary has a case on
each side.  The rules live in csrc/sn_route.h and are restated ONCE here (test_small_planes_cpu.py puts every case of the tables
to the header on a host compiler, tests/c/route_check.cpp, and holds each restatement against its answer):

  nr = h_out / 2 - 1              rows a plane interpolates (plan_parts and chain_planes ask for nr >= 1)
  bh = (h_out + 1) >> 1           rows of the luma-sized pool, row 0 not counted (pool_stage2_for: bh <= 1 has no stage 2;
                                  chain_planes asks for bh >= 2)
  reach = min(nr_c + 2, bh - 1)   rows of the hand-off pool a coupled chroma sweep reaches (coupled_reach, clip_plan)
  nr_c >= 2 kSkew + 2             U and V as ONE sweep (fused_uv_ok; kSkew = 2, so nr_c >= 6)
  nb <= nr / kMinBandRows         row bands of at least kMinBandRows = 8 rows, at least two of them (band_count, band_geometry)

clip_plan, band_count_auto and prefer_pool below restate creation's plan, auto mode's own band count and its estimate of the
faster path for tests/config_space.py, whose CPU test holds them against the header for every launch of its table.

A case is a tuple; its frames differ in content (noise, sine, edges, ...) and in parity.  Expected frames come from the C oracle,
once per session; history-carrying clips (width not a multiple of 32) run against ONE oracle instance across their frames.
"""
import numpy as np

from avisynth_sangnom2_amd import ClipFormat, clip_format, synth
from oracle.oracle import Oracle
from tests.util import oracle_cfg

SEED = 311
PATTERNS = ("noise", "sine", "edges")
PARITIES = (1, 0, 1)

# ---- the rules, restated ---------------------------------------------------------------------------------------------------------
K_SKEW = 2                                 # sn_route.h uv::kSkew
MIN_BAND_ROWS = 8                          # sn_route.h kMinBandRows
BAND_WARM = {1: 32, 2: 40, 4: 48}          # sn_route.h band_warm_rows: the default run-up per sample size
MAX_SWEEP_WIDTH = {1: 7680, 2: 3840, 4: 3840}  # the widest whole-plane sweep (eight waves)
MAX_WIDTH = 8192
PARTS_GHOST = {2: 64, 4: 96}               # sn_route.h kPartsGhost16 / kPartsGhost32


def nr(h_out):
    return h_out // 2 - 1


def bh(h_out):
    return (h_out + 1) >> 1


def reach(nr_c, bh_):
    return min(nr_c + 2, bh_ - 1)


def uv_rows_ok(nr_c, bh_):
    """fused_uv_ok's row condition."""
    return 2 * K_SKEW + 2 <= nr_c <= bh_ - 1


def band_count(nr_, forced):
    """Bands per frame of a launch with sn_debug_set_bands(forced, ...): band_rows_available, band_count."""
    if nr_ < 2 * MIN_BAND_ROWS:
        return 0
    nb = min(forced, nr_ // MIN_BAND_ROWS)
    return nb if nb >= 2 else 0


def sweep_plane_ok(B, w):
    """A whole-plane sweep has an instance for this plane (fused_plane_eligible)."""
    return w % 32 == 0 and w <= MAX_SWEEP_WIDTH[B]


def parts_marked(B, w):
    """Creation marks the plane for column parts (fused_parts_plane_eligible): by width alone."""
    return B in (2, 4) and w % 32 == 0 and w <= MAX_WIDTH and not sweep_plane_ok(B, w)


def strips_for(nl):
    return 1 if nl <= 64 else 1 + (nl - 62 + 59) // 60


def pool_schedule(B, stride, bh_, frames):
    """sn_pool_dispatch.h pool_stage2_for, the schedule's name."""
    if bh_ <= 1:
        return "none"
    if stride >= 512 and strips_for(stride // 8) <= 16 and (B != 4 or frames <= 8):
        return "strips"
    if 256 <= stride <= 8192:
        return "x8"
    return "strided" if stride < 256 else "refused"


def pool_stride(w):
    return (w + 31) & ~31


def planes_of(clip, kw):
    """Per plane (width, h_out, processed) as the library sees them."""
    dh = bool(kw.get("dh"))
    out = []
    for p in range(clip.planes):
        w, h = clip.width >> (clip.subw if p else 0), clip.height >> (clip.subh if p else 0)
        on = dh or bool(kw.get("luma", True) if p == 0 else kw.get("chroma", True))
        out.append((w, 2 * h if dh else h, on))
    return out


def needs_pools(clip, kw):
    """fused_needs_pools: subsampled chroma that is processed -- its passes share the luma-sized pool with the luma pass."""
    return clip.planes == 3 and bool(kw.get("dh") or kw.get("chroma", True)) and (clip.subw != 0 or clip.subh != 0)


def history_free(clip, kw):
    """compute_history_free of a clip whose planes share one pool (not isolated_planes, not fresh_pool)."""
    if clip.width % 32 != 0:
        return False
    if clip.planes == 1 or not needs_pools(clip, kw):
        return True
    return bool(kw.get("dh") or kw.get("luma", True))


def chain_passes(clip, kw):
    """chain_planes: passes per frame of the chain a history-carrying clip's launches run as, 0 = no chain."""
    planes = planes_of(clip, kw)
    b = bh(planes[0][1])
    if history_free(clip, kw) or pool_stride(clip.width) < 64 or b < 2:
        return 0
    on = [(w, ho) for w, ho, o in planes if o]
    return len(on) if all(w % 8 == 0 and 1 <= nr(ho) < b for w, ho in on) else 0


def chain_ok(clip, kw):
    """chain_planes: the batch of a history-carrying clip runs as a chain of passes."""
    return chain_passes(clip, kw) > 0


def uv_geometry(clip, kw):
    """fused_uv_ok on the clip: the geometry allows U and V of an 8-bit frame as ONE sweep (at most eight strips: 3840 columns)."""
    if clip.bytes != 1 or not needs_pools(clip, kw):
        return False
    (w, ho, _), (wc, hc, _) = planes_of(clip, kw)[:2]
    return w % 32 == 0 and wc % 8 == 0 and 0 < wc < w and strips_for(w // 8) <= 8 and uv_rows_ok(nr(hc), bh(ho))


def clip_plan(clip, kw, ext="none", sse2=None, pool_mode=False, parts_on=False):
    """sn_route.h clip_plan, as far as the routes need it: per plane (fused, padded, marked for column parts) and the clip's
    flags.  ext: "none" | "isolated" | "fresh"; sse2: None (opt=0) or sn_policy.sse2_sweeps of an opt=1 context; pool_mode:
    mode="pool"; parts_on: column_parts=1.  info_eligible: what sn_info.fused_eligible says of the context."""
    B, planes, np_ = clip.bytes, planes_of(clip, kw), clip.planes
    fresh = ext == "fresh"
    isolated = fresh or (ext == "isolated" and np_ > 1)
    pools = needs_pools(clip, kw)
    sat = sse2 is not None and B < 4
    sat_sweeps = sse2 == 1 or (B == 1 and (isolated or not pools))
    cfg_eligible = sweep_plane_ok(B, clip.width) and (not pools or (bool(kw.get("dh") or kw.get("luma", True)) and planes[1][0] % 8 == 0))
    padded_ok = lambda pw: pw % 8 == 0 and sweep_plane_ok(B, pool_stride(pw))  # noqa: E731  (fused_padded_plane_eligible)
    fused, padded, marked = [False] * 3, [False] * 3, [False] * 3
    eligible, hf = cfg_eligible, history_free(clip, kw)
    if isolated:
        eligible = True
        hf = fresh or all(w % 32 == 0 for w, ho, on in planes if on)
        for p, (pw, ho, on) in enumerate(planes):
            if not on:
                continue
            fused[p] = sweep_plane_ok(B, pw)
            if not fused[p] and parts_on and not fresh and parts_marked(B, pw):
                fused[p] = marked[p] = True
            if fresh and not fused[p] and padded_ok(pw):
                fused[p] = padded[p] = True
            eligible = eligible and fused[p]
    elif not eligible and parts_on and not pools and parts_marked(B, clip.width):
        eligible = True
        marked = [on and pw == clip.width for pw, ho, on in planes] + [False] * (3 - np_)
    info_eligible = cfg_eligible
    if sat and not sat_sweeps:  # the pool kernels serve every plane in this arithmetic
        eligible, info_eligible = False, False
        fused, padded, marked = [False] * 3, [False] * 3, [False] * 3
    elif isolated:
        info_eligible = all(sweep_plane_ok(B, pw) or (fresh and padded_ok(pw)) for pw, ho, on in planes if on)
    use_fused = eligible and not pool_mode
    if pool_mode:  # the pool path serves every plane: nothing stays marked, and sn_info answers as for a clip without the option
        marked = [False] * 3
        if isolated:
            fused = [False] * 3
    if any(marked):
        info_eligible = eligible
    fused420 = use_fused and not isolated and pools
    return dict(clip=clip, kw=kw, planes=planes, fresh=fresh, isolated=isolated, pools=pools, fused=fused, padded=padded, marked=marked,
                use_fused=use_fused, fused420=fused420, uv=fused420 and uv_geometry(clip, kw), info_eligible=info_eligible, history_free=hf, sat=sat,
                pool_mode=pool_mode)


def sweeps_serve_all(plan):
    """band_rows_available's condition on the planes: every processed plane has a whole-plane sweep (not the padded one)."""
    if any(plan["marked"]) or plan["pool_mode"] or not plan["history_free"]:
        return False
    if plan["isolated"]:
        return all(plan["fused"][p] and not plan["padded"][p] for p, (w, ho, on) in enumerate(plan["planes"]) if on)
    return plan["use_fused"]


def nr_min(plan):
    return min(nr(ho) for w, ho, on in plan["planes"] if on)


def band_count_auto(plan, n):
    """band_count of an auto-mode launch of n frames without sn_debug_set_bands (its slots at hand): about 512 workgroups in
    all, bands of at least kMinBandRows rows and of at least a quarter of the run-up, at least three bands by count."""
    if not sweeps_serve_all(plan) or nr_min(plan) < 2 * MIN_BAND_ROWS:
        return 0
    nb = min(512 // n, nr_min(plan) // MIN_BAND_ROWS, 128)
    if nb < 3:
        return 0
    quarter = BAND_WARM[plan["clip"].bytes] // 4
    if nr_min(plan) // nb < quarter:
        nb = nr_min(plan) // quarter
    return nb if nb >= 2 else 0


# sn_route.h prefer_pool's fitted constants, per sample size: seconds per pool element and frame, per pool row, per sweep row
# (planes of more than 3840 columns: 8-bit only), per row of a coupled chroma sweep (8-bit: two sweeps; U and V as one: 1.9e-6)
POOL_PER_ELEM = {1: 12.9e-12, 2: 19.4e-12, 4: 32.6e-12}
POOL_PER_ROW = {1: 0.25e-6, 2: 0.22e-6, 4: 0.33e-6}
SWEEP_ROW = {1: 2.6e-6, 2: 2.8e-6, 4: 4.3e-6}
SWEEP_ROW_COUPLED = {1: 3.0e-6, 2: 3.15e-6, 4: 4.7e-6}


def prefer_pool(plan, n, chroma_sweeps=0):
    """prefer_pool for an auto-mode launch of n frames that is not cut into bands (policy SN_SMALL_AUTO, its slots at hand):
    the estimate says the pool path is faster than the sweeps."""
    if plan["pool_mode"] or not plan["history_free"]:
        return False
    B, planes = plan["clip"].bytes, plan["planes"]
    fused = pool = 0.0
    for p, (pw, ho, on) in enumerate(planes):
        if not on:
            continue
        own = plan["isolated"]
        stride = pool_stride(pw if own else planes[0][0])
        b = bh(ho if own else planes[0][1])
        rows = ho // 2
        t_row = (3.8e-6 if stride > 3840 else SWEEP_ROW[1]) if B == 1 else SWEEP_ROW[B]
        if plan["fused420"] and p > 0:
            t_row = 1.9e-6 if B == 1 and plan["uv"] and chroma_sweeps == 0 else SWEEP_ROW_COUPLED[B]
        fused += rows * t_row
        b_run = rows + 2 if not own and rows + 2 < b else b
        pool += b_run * (POOL_PER_ROW[B] + 0.036e-6 * ((stride + 1023) // 1024)) + 60e-6 + float(n) * stride * b_run * POOL_PER_ELEM[B]
    return pool < fused


# ---- the tables ------------------------------------------------------------------------------------------------------------------
Y = {1: "Y8", 2: "Y16", 4: "Y32"}
TYPES = ("Y8", "Y16", "Y32")

# Column parts (mode="fused", column_parts=1): (format, width, height, filter kwargs, context kwargs).  At height 2 a plane has no
# interpolated row (nr = 0): plan_parts refuses it, and the launch must take the pool path's assemble, not a whole-plane sweep
# that has no instance this wide.  Heights 4 and 6 (nr = 1, 2) are the other side: the parts run, and on one or two rows every
# seam converges inside the ghost (an error travels three columns per row), so no frame may fall back.
PARTS_WIDE = (("Y32", 6144), ("Y16", 3872), ("Y32", 8192))  # 6144x2: what the fuzz run ended on
PARTS = [(fmt, w, h, {}, {}) for h in (2, 4, 6) for fmt, w in PARTS_WIDE] + [
    ("Y16", 3872, 2, dict(dh=True), {}),                                # h_out 4: nr = 1, the parts run
    ("YUV444P16", 3872, 2, dict(aac=48), {}),                           # three planes, none with a row
    ("YUV420P16", 8192, 4, dict(aac=48), dict(isolated_planes=True)),   # luma in parts with one row, chroma 4096x2 with none
    ("YUV420PS", 8192, 4, dict(aac=48), dict(isolated_planes=True)),
]
PARTS_WAYS = ("host", "ring1", "ring4", "batch")
PARTS_FORCED = [(fmt, 512, 4, parts) for fmt in ("Y16", "Y32") for parts in (2, 3, 4)]

# Whole-plane sweeps at eight waves, heights 2 and 4.  tests/sweep_geometry_cases.py has these planes as host frames of noise
# (SEAM_WIDTHS x HEIGHTS), so here they run the other way: a device batch of three frames of different content, and with dh.
WIDE = [(t, MAX_SWEEP_WIDTH[b], h, kw) for b, t in Y.items() for h in (2, 4) for kw in ({}, dict(dh=True))]
# ... and the SSE2 arithmetic's instances (opt=1, sse2_sweeps=1) against tests/sse2_model.py
WIDE_SSE2 = [(t, 256, h) for t in ("Y8", "Y16") for h in (2, 4)]

# Coupled sweeps (hand-off pools).  4:2:0 heights 4, 8, 12: chroma nr_c = 0, 1, 2 and reach = 1, 3, 4 -- the bh - 1 arm of the
# minimum, both arms equal, the nr_c + 2 arm.  4:2:2 heights 2 and 4: reach = 0 (a hand-off pool of row 0 alone) and 1.
COUPLED = [(fmt, w, h) for fmt in ("YUV420P8", "YUV420P16", "YUV420PS") for h in (4, 8, 12) for w in (1024, 3840)] + \
          [("YUV420P8", 7680, 8)] + [(fmt, w, h) for fmt in ("YUV422P8", "YUV422P16") for h in (2, 4) for w in (1024, 3840)]
HANDOFF = [("YUV420P8", 1024, 8), ("YUV420P16", 1024, 12), ("YUV420PS", 1024, 4)]

# U and V as one sweep: both sides of nr_c >= 6.  (format, width, height, dh).  Without dh the heights give nr_c = 5 and 6.  With
# dh the chroma plane is h (4:2:0) or 2 h (4:2:2) lines high and the reference takes 4:2:0 heights that are a multiple of 4 and
# 4:2:2 heights that are even only, so nr_c = 6 cannot be had: the two heights next to the rule give nr_c = 5 and 7.
UV = [("YUV420P8", w, h, False) for h in (24, 28) for w in (256, 3840)] + [("YUV422P8", w, h, False) for h in (12, 14) for w in (256, 3840)] + \
     [("YUV420P8", 256, h, True) for h in (12, 16)] + [("YUV422P8", 256, h, True) for h in (6, 8)]

# Row bands, sn_debug_set_bands(bands, warm): (type, width, height, bands forced).  32 lines: nr = 15, below two bands of eight
# rows, so not cut even when forced.  34 lines: nr = 16, two bands of eight rows.  50 and 52 lines: nr = 24 and 25, three bands.
# The run-up: a band starts max(1, first own row - run-up) -- at these heights every default run-up (32 / 40 / 48 rows) is longer
# than the rows above the last band (8 at 34 lines, 16 / 18 at 50 / 52), so every band starts at row 1, where the zero state it
# starts from IS the state: the library is expected to sweep those rows again, pass every check and fall back on no frame.  With
# a run-up of one row the guess is wrong on ordinary content; the frame is then redone by the pool kernels, exact either way.
BANDS = [(t, 512, h, 2 if h < 50 else 3) for t in TYPES for h in (32, 34, 50, 52)]
BAND_WARMS = (0, 1)

# Pool path (mode="pool"): heights 2 and 4 (bh = 1: no stage 2 at all; bh = 2: one smoothed row) at every stage-2 schedule.
POOL_WIDTHS = (256, 512, 544, 7680, 8192, 100, 520)
POOL = [(t, w, h) for t in TYPES for w in POOL_WIDTHS for h in (2, 4)]
POOL_CONTENTS = [(t, w, h) for t in TYPES for w, h in ((520, 4), (100, 2))]

# Chains (history-carrying batches, ten frames a launch): (format, width, height, filter kwargs).  Height 2: bh = 1 and nr = 0,
# no chain.  Heights 4 and 6: chained.  YUV420P8 720x4: bh = 2 but the chroma planes have no row, no chain; 720x8: chained.
CHAIN_FRAMES = 10
CHAINS = [(t, w, h, {}) for t in ("Y8", "Y12", "Y32") for w in (40, 1000) for h in (2, 4, 6)] + \
         [("YUV420P8", 720, 4, dict(aac=48)), ("YUV420P8", 720, 8, dict(aac=48))]
CHAIN_POLICIES = (0, 2)

# Narrow planes: nothing in the device suite is narrower than 32 columns.  With fresh_pool, 8 and 24 columns take the padded sweep
# over the 32-column pool stride (a multiple of 8 and not of 32), every other width the pool path.
NARROW_WIDTHS = (1, 2, 7, 8, 9, 24, 31)
NARROW = [(t, w, h) for t in TYPES for h in (2, 4, 16) for w in NARROW_WIDTHS]
NARROW_CLIPS = [("YUV420P8", 4, 4), ("YUV420P8", 8, 4), ("YUV422P16", 2, 2), ("YUV444PS", 1, 2)]

# Surfaces: (format, width, height, source side, destination side).  Sides: "planar", "semi" (NV12 / P016 / NV16), "semi_msb"
# (P010), a packed layout of tests/packed_surface_cases.py.  Every layout with itself and with a planar other side.
def _both_ways(fmt, w, h, side):
    return [(fmt, w, h, side, side), (fmt, w, h, side, "planar"), (fmt, w, h, "planar", side)]


SURFACES = [c for fmt in ("YUV420P8", "YUV420P16") for w in (2, 6, 34) for c in _both_ways(fmt, w, 4, "semi")] + \
    _both_ways("YUV420P10", 34, 4, "semi_msb") + _both_ways("YUV422P8", 2, 2, "semi") + \
    [c for side in ("yuyv", "uyvy") for w in (2, 66) for c in _both_ways("YUV422P8", w, 2, side)] + \
    _both_ways("YUV422P10", 34, 2, "yuyv_msb") + [c for w in (2, 6, 50) for c in _both_ways("YUV422P10", w, 2, "v210")]

# The anti-aliasing call: (format, width, height, dh).  Turned chroma of the 4:2:0 clip is 4 wide.
AA = [(fmt, w, h, dh) for fmt, w, h in (("Y8", 64, 8), ("Y8", 8, 64), ("Y16", 64, 6), ("YUV420P8", 64, 8)) for dh in (False, True)]
# ... with dh and column_parts=1: the first pass enlarges the turned clip (2 wide) to 2 x 3872, the second pass's clip is 3872
# wide and 2 high with h_out = 4 -- nr = 1, the near side of plan_parts' nr >= 1: the second pass runs in parts.
AA_PARTS = ("Y16", 1936, 2)


# ---- frames and expected frames --------------------------------------------------------------------------------------------------
def frames_of(clip, n=3, seed0=SEED, patterns=PATTERNS):
    return [synth.frame(clip, patterns[i % len(patterns)], seed=seed0 + i) for i in range(n)]


def parities_of(n):
    return [PARITIES[i % len(PARITIES)] for i in range(n)]


def _frozen(frames):
    for fr in frames:
        for pl in fr:
            pl.setflags(write=False)
    return frames


def y_clip(clip, p):
    return ClipFormat(width=clip.width >> (clip.subw if p else 0), height=clip.height >> (clip.subh if p else 0), bytes=clip.bytes, bits=clip.bits)


def plane_kw(kw, p):
    k = {x: y for x, y in kw.items() if x != "aac"}
    k["aa"] = kw.get("aa", 48) if p == 0 else kw.get("aac", 0)
    return k


_cache = {}


def expected(fmt, w, h, kw=None, ckw=None, n=3, patterns=PATTERNS, seed0=SEED):
    """(clip, frames, parities, the oracle's frames), computed once per session and left unchanged.  One oracle instance across
    the frames; isolated_planes: one per plane, on the plane as a Y clip; fresh_pool: a new one per plane and frame."""
    kw, ckw = kw or {}, ckw or {}
    key = (fmt, w, h, tuple(sorted(kw.items())), tuple(sorted(ckw.items())), n, tuple(patterns), seed0)
    if key not in _cache:
        clip = clip_format(fmt, w, h)
        frames, par = frames_of(clip, n, seed0, patterns), parities_of(n)
        isolated, fresh = bool(ckw.get("isolated_planes")) and clip.planes > 1, bool(ckw.get("fresh_pool"))
        if isolated or fresh:
            keep, want = {}, []
            for fr, pa in zip(frames, par):
                planes = []
                for p in range(clip.planes):
                    if fresh or p not in keep:
                        keep[p] = Oracle(oracle_cfg(y_clip(clip, p), **plane_kw(kw, p)))
                    planes.append(keep[p].process([fr[p]], parity=pa)[0])
                want.append(planes)
        else:
            ora = Oracle(oracle_cfg(clip, **kw))
            want = [ora.process(fr, parity=pa) for fr, pa in zip(frames, par)]
        _cache[key] = (clip, _frozen(frames), par, _frozen(want))
    return _cache[key]


def expected_aa(fmt, w, h, dh, n=2, **kw):
    """(clip, frames, parities, the script's frames) of the anti-aliasing call (tests/aa_script.py, tests/aa_dh_script.py)."""
    key = ("aa", fmt, w, h, dh, n, tuple(sorted(kw.items())))
    if key not in _cache:
        from tests import aa_dh_script, aa_script
        clip = clip_format(fmt, w, h)
        frames, par = frames_of(clip, n, SEED + 40), parities_of(n)
        script = (aa_dh_script if dh else aa_script).Script(clip, **kw)
        _cache[key] = (clip, _frozen(frames), par, _frozen([script.frame(fr, parity=pa) for fr, pa in zip(frames, par)]))
    return _cache[key]


def to_torch(frames, clip, dev):
    from tests import column_parts_cases as cc
    return cc.to_torch(frames, clip, dev)


# ---- every clip of the table, for the checks on the CPU ------------------------------------------------------------------------------
def aa_pass_clips(fmt, w, h, dh):
    """The two filter instances of the anti-aliasing script: (clip, dh) of the turned clip's and of the clip's."""
    from tests.aa_dh_script import widened_clip
    from tests.aa_script import turned_clip
    clip = clip_format(fmt, w, h)
    return [(turned_clip(clip), dh), (widened_clip(clip) if dh else clip, dh)]


def every_clip():
    """Every distinct (ClipFormat, filter kwargs) an oracle instance of the table is made for.  Isolated planes: the planes as Y
    clips.  The SSE2 cases are tests/sse2_model.py's; their clips are listed for the default arithmetic all the same."""
    out, seen = [], set()

    def add(clip, kw):
        key = (clip.width, clip.height, clip.bytes, clip.bits, clip.planes, clip.subw, clip.subh, tuple(sorted(kw.items())))
        if key not in seen:
            seen.add(key)
            out.append((clip, dict(kw)))

    def add_fmt(fmt, w, h, kw=None, ckw=None):
        clip, kw = clip_format(fmt, w, h), kw or {}
        if (ckw or {}).get("isolated_planes") and clip.planes > 1:
            for p in range(clip.planes):
                add(y_clip(clip, p), plane_kw(kw, p))
        else:
            add(clip, kw)

    for fmt, w, h, kw, ckw in PARTS:
        add_fmt(fmt, w, h, kw, ckw)
    for fmt, w, h, _ in PARTS_FORCED:
        add_fmt(fmt, w, h)
    for fmt, w, h, kw in WIDE:
        add_fmt(fmt, w, h, kw)
    for fmt, w, h in WIDE_SSE2 + POOL + NARROW:
        add_fmt(fmt, w, h)
    for fmt, w, h in COUPLED + NARROW_CLIPS:
        add_fmt(fmt, w, h, dict(aac=48))
    for fmt, w, h, dh in UV:
        add_fmt(fmt, w, h, dict(aac=48, dh=True) if dh else dict(aac=48))
    for fmt, w, h, _ in BANDS:
        add_fmt(fmt, w, h)
    for fmt, w, h, kw in CHAINS:
        add_fmt(fmt, w, h, kw)
    for fmt, w, h, _, _ in SURFACES:
        add_fmt(fmt, w, h)
    for fmt, w, h, dh in AA + [AA_PARTS + (True,)]:
        for clip, d in aa_pass_clips(fmt, w, h, dh):
            add(clip, dict(aac=48, dh=True) if d else dict(aac=48))
    return out


def line_doubled(src, h_out, dh, offset=0):
    """A plane by plain line doubling: every missing line a copy of the kept line above it (offset 0: the even lines are kept)."""
    out = np.empty((h_out, src.shape[1]), dtype=src.dtype)
    kept = src if dh else src[offset::2]
    out[0::2], out[1::2] = kept, kept
    return out
