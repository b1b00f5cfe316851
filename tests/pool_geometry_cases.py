"""Pools, heights and launches that walk the geometry of the pool path's stage 2 and of its chains (tests/test_pool_geometry_gpu.py
runs them on the device, tests/test_pool_geometry_cpu.py checks the table itself).  TEST INFRASTRUCTURE ONLY.

Stage 2 of the pool path (csrc/sn_pool_kernels.hip) is about twenty hand-written kernels behind three schedules, and which one a
pool gets follows from its sample size, its row stride, its rows and the frames of the launch alone (csrc/sn_pool_dispatch.h).
The rules are restated ONCE here -- strips_for and the schedule's name are tests/small_plane_cases.py's -- and every table below
is derived from them; nothing is drawn at random:

  STRIPS   the narrowest and the widest stride of every strip count 1 .. 16 of the strips schedule (float: a launch of 3 frames)
  EDGE     every stride from 512 to 1472, so that the last real lane walks the second and third strip from end to end, and for each
           a plane 8 columns narrower: history-carrying, its last columns smoothed again with every frame
  ROWS     row loops that end at every phase of the strips' five-row refresh and of the x8 kernels' unroll by four
  X8       the x8 schedule below the strips (256 .. 480), above them (7712 .. 8192), and for float launches of nine frames at both
           ends of every wave count and on both sides of the 48 KiB LDS boundary
  STRIDED  pools narrower than 256 columns, and planes around the 256-thread blocks of stages 1 and 3
  SSE2     the saturating instances (opt=1, sse2_sweeps=0) against tests/sse2_model.py
  CHAIN    chains at every strip count a type's chain takes, over every number of workgroups the rule grants, in launches long
           enough that every set of waves carries two passes; the 8-bit instances by block size; the first strides refused

Every case is a Y clip with mode="pool", so pool 0 is the plane's pool.  A case's frames are `noise` (full-range costs: the box
wraps), `edges` (`noise01` with opt=1: the box saturates) and further noise where history matters; order = 1 unless stated.
"""
from collections import namedtuple

from avisynth_sangnom2_amd import clip_format, synth
from tests import small_plane_cases as sp

BYTES = {"Y8": 1, "Y16": 2, "Y32": 4}
TYPES = ("Y8", "Y16", "Y32")
SEED = 523
H = 24  # the height of every case that does not walk the rows

# ---- the rules, restated -------------------------------------------------------------------------------------------------------------
SMOOTH_THREADS = 1024     # sn_pool_dispatch.h kSmoothThreads
CHAIN8_THREADS = 1024     # sn_pool_dispatch.h kChain8Threads
CHAIN_MAX_GROUPS = 8      # sn_internal.h kChainMaxGroups
GH = 2                    # sn_sweep_args.h v3c::GH: ghost lanes on each side of a strip
K_REFRESH, X8_UNROLL = 5, 4  # v3c::K: rows between two refreshes of the ghost lanes; the x8 kernels' unroll

strips_for, pool_stride, bh = sp.strips_for, sp.pool_stride, sp.bh


def pool_stage2(B, stride, bh_, frames):
    """sn_pool_dispatch.h pool_stage2_for: (schedule, threads, dynamic LDS bytes, lds_attr)."""
    name = sp.pool_schedule(B, stride, bh_, frames)
    nl, lane_bytes = stride // 8, 16 if B == 1 else 32
    if name == "strips":
        nw = strips_for(nl)
        return name, 64 * nw, 2 * nw * 2 * GH * lane_bytes, False
    if name == "x8":
        lds = 2 * nl * lane_bytes
        return name, (nl + 63) // 64 * 64, lds, lds > 48 * 1024
    if name == "strided":
        return name, SMOOTH_THREADS, 2 * stride * 4, False
    return name, 0, 0, False


def chain_lanes(B, stride):
    """pool_chain_lanes: passes one workgroup keeps in flight, 0 = no chain for this pool."""
    if stride < 64:
        return 0
    nw = strips_for(stride // 8)
    if B == 1:
        return 2 * (CHAIN8_THREADS // 64 // nw) if nw <= CHAIN8_THREADS // 64 else 0
    return SMOOTH_THREADS // 64 // nw if nw <= SMOOTH_THREADS // 128 else 0


def chain_waves(B, groups):
    every = CHAIN8_THREADS // 64 if B == 1 else 2 * (SMOOTH_THREADS // 64)
    return min(every // groups, SMOOTH_THREADS // 64)


def chain_groups(B, stride, want):
    """pool_chain_groups: workgroups per buffer the chain runs over for `want`."""
    if want <= 1:
        return 1
    nw, g = strips_for(stride // 8), 1
    while g * 2 <= want and g * 2 <= CHAIN_MAX_GROUPS and chain_waves(B, g * 2) >= nw:
        g *= 2
    return g


def lanes_per_workgroup(B, stride, g):
    """launch_pool_chain: passes in flight in ONE workgroup of a chain over g workgroups per buffer."""
    if g <= 1:
        return chain_lanes(B, stride)
    return (2 if B == 1 else 1) * (chain_waves(B, g) // strips_for(stride // 8))


def chain_block(B, stride, g, npass):
    """launch_pool_chain: threads of a workgroup (a short chain on one workgroup leaves no idle waves at the barrier)."""
    lanes = lanes_per_workgroup(B, stride, g)
    if g <= 1 and npass < lanes:
        lanes = (npass + 1) & ~1 if B == 1 else npass
    return (lanes // 2 if B == 1 else lanes) * strips_for(stride // 8) * 64


def chain_instance(B, stride, g, npass, opt=0):
    """launch_pool_chain's dispatch: the kernel instance, by name."""
    if B == 4:
        return "f32-grouped" if g > 1 else "f32"
    a = "-sse2" if opt else ""
    if B == 2:
        return ("u16-grouped" if g > 1 else "u16") + a
    if g > 1:
        return "u8-grouped-512" + a
    return ("u8-512" if chain_block(B, stride, g, npass) <= CHAIN8_THREADS // 2 else "u8-1024") + a


def field_runs(order, parities):
    """run_batch: the launch as runs of equal field offset (sn_route.h field_offset, field_run)."""
    off = [{0: 0 if p else 1, 1: 0}.get(order, 1) for p in parities]
    runs, start = [], 0
    for i in range(1, len(off) + 1):
        if i == len(off) or off[i] != off[start]:
            runs.append(i - start)
            start = i
    return runs


def last_lane(stride):
    """(strip, lane of that strip) of the last lane that owns columns: strip 0 has no left ghosts, every later strip two."""
    gl = stride // 8 - 1
    if stride // 8 <= 64:
        return 0, gl
    return 1 + (gl - 62) // 60, GH + (gl - 62) % 60


def strip_bounds(strides):
    """{strip count: (narrowest, widest)} over the given strides."""
    out = {}
    for s in strides:
        lo, _ = out.get(strips_for(s // 8), (s, s))
        out[strips_for(s // 8)] = (lo, s)
    return out


STRIPS_STRIDES = tuple(s for s in range(512, 8193, 32) if strips_for(s // 8) <= 16)    # what the strips schedule takes: 512 .. 7680
STRIP_BOUNDS = strip_bounds(STRIPS_STRIDES)
ALL_BOUNDS = strip_bounds(range(64, 8193, 32))                                         # from 64 columns on, up to seventeen strips


def x8_wave_bounds():
    """{waves: (narrowest, widest stride)} of the x8 schedule, whose waves are 64 lanes each without ghosts."""
    out = {}
    for s in range(256, 8193, 32):
        n = (s // 8 + 63) // 64
        lo, _ = out.get(n, (s, s))
        out[n] = (lo, s)
    return out


X8_WAVE_BOUNDS = x8_wave_bounds()

# ---- a case --------------------------------------------------------------------------------------------------------------------------
# table, fmt, w, h: the Y clip.  launch: 0 = frames one by one through get_frame; n > 0: process_batch launches of n frames.
# patterns: per frame of ONE launch (launch = 0: of the case); launches: how often that launch is sent (new frames each time).
# chain: sn_policy.chain (None: the default).  parities: per frame of a launch.
Case = namedtuple("Case", "table fmt w h launch patterns launches order aa opt chain parities seed note")


def _case(table, fmt, w, h=H, launch=0, patterns=None, launches=1, order=1, aa=48, opt=0, chain=None, parities=None, seed=None, note=""):
    if patterns is None:
        second = "noise01" if opt else "edges"
        n = launch or (2 if w % 32 == 0 else 3)
        patterns = tuple(("noise", second)[i % 2] if i < 2 or launch else "noise" for i in range(n))
    n = len(patterns)
    if parities is None:
        parities = (1,) * n
    if seed is None:
        seed = SEED + 7 * w + 3 * h + BYTES[fmt]
    return Case(table, fmt, w, h, launch, tuple(patterns), launches, order, aa, opt, chain, tuple(parities), seed, note)


def case_id(c):
    s = f"{c.fmt}-{c.w}x{c.h}"
    if c.launch:
        s += f"-n{c.launch}"
    if c.chain is not None:
        s += f"-g{c.chain}"
    if c.order != 1:
        s += f"-order{c.order}"
    if c.opt:
        s += "-sse2"
    return s + (f"-{c.note}" if c.note else "")


def stride_of(c):
    return pool_stride(c.w)


def stage2_of(c):
    """The schedule a plane case's launches get: pool_stage2 of its pool and of the frames per launch."""
    return pool_stage2(BYTES[c.fmt], stride_of(c), bh(c.h), c.launch or 1)


# ---- the tables ----------------------------------------------------------------------------------------------------------------------
STRIPS = [_case("STRIPS", t, s, launch=3 if t == "Y32" else 0) for t in TYPES for n in sorted(STRIP_BOUNDS) for s in sorted(set(STRIP_BOUNDS[n]))]

EDGE_STRIDES = tuple(range(512, 1473, 32))
EDGE = [_case("EDGE", t, w) for t in TYPES for s in EDGE_STRIDES for w in (s, s - 8)]

# The reference (and creation) refuses an odd height ("SangNom2: height must be even."), so a plane's rows are walked through the
# even heights: bh = 2 .. 17, and bh - 1 = 1 .. 16 meets every residue mod 5 three times over and mod 4 four times.  Heights 42, 46
# and 66 add the pools of 21, 23 and 33 rows.
ROW_HEIGHTS = tuple(range(4, 35, 2)) + (42, 46, 66)
ODD_HEIGHTS_REFUSED = (21, 23, 33)
ROW_STRIDES = (544, 7680, 480, 8192)  # two strips, sixteen; x8 below the strips and above them
ROWS = [_case("ROWS", t, s, h) for t in TYPES for s in ROW_STRIDES for h in ROW_HEIGHTS]

X8_LOW, X8_HIGH = tuple(range(256, 481, 32)), tuple(range(7712, 8193, 32))
X8_FLOAT9_STRIDES = tuple(sorted({s for n in sorted(X8_WAVE_BOUNDS) for s in X8_WAVE_BOUNDS[n]} | {6144, 6176}))
X8 = [_case("X8", t, s) for t in TYPES for s in X8_LOW + X8_HIGH] + [_case("X8", "Y32", s, launch=9) for s in X8_FLOAT9_STRIDES]

STRIDED_STRIDES = tuple(range(32, 225, 32))
STRIDED_WIDTHS = (255, 256, 257, 513)  # around the 256-thread blocks of k_prepare / k_finalize, and an odd right edge
STRIDED = [_case("STRIDED", t, w) for t in TYPES for w in STRIDED_STRIDES + STRIDED_WIDTHS]

SSE2_STRIDES = tuple(sorted({STRIP_BOUNDS[n][0] for n in STRIP_BOUNDS} | {256, 480, 7712, 8192, 32, 224}))
SSE2 = [_case("SSE2", t, s, opt=1) for t in ("Y8", "Y16") for s in SSE2_STRIDES]

PLANE_TABLES = dict(STRIPS=STRIPS, EDGE=EDGE, ROWS=ROWS, X8=X8, STRIDED=STRIDED, SSE2=SSE2)


def chain_nws(B):
    """Strip counts the type's chain takes."""
    return tuple(range(1, (CHAIN8_THREADS // 64 if B == 1 else SMOOTH_THREADS // 128) + 1))


def chain_stride(nw):
    """The narrowest stride of nw strips the chain takes (a pool of 32 columns has no chain)."""
    return ALL_BOUNDS[nw][0]


def granted(B, stride):
    """Every distinct answer of pool_chain_groups over want = 1, 2, 4, 8."""
    return tuple(sorted({chain_groups(B, stride, want) for want in (1, 2, 4, 8)}))


def _chain_case(t, stride, g, k, opt=0, frames=None, note=""):
    """A chain case: planes 8 columns narrower than the stride, two launches of 2 x lanes per workgroup x g + 1 frames (so that
    every set of waves carries at least two passes, and the 8-bit pair has an idle half at the end), one frame of the other parity
    in the middle of a launch and -- every third case -- order = 0, where that frame splits the launch into two chains and a frame
    on its own."""
    B = BYTES[t]
    n = frames or 2 * max(lanes_per_workgroup(B, stride, g), 1) * g + 1
    parities = (1,) * (n // 2) + (0,) + (1,) * (n - n // 2 - 1)
    second = "noise01" if opt else "edges"
    patterns = tuple(second if i == 1 else "noise" for i in range(n))
    return _case("CHAIN", t, stride - 8, launch=n, patterns=patterns, launches=2, order=0 if k % 3 == 2 else 1, opt=opt, chain=g, parities=parities, note=note)


def _chains():
    out, k = [], 0
    for t in TYPES:
        B = BYTES[t]
        for nw in chain_nws(B):
            for g in granted(B, chain_stride(nw)):
                out.append(_chain_case(t, chain_stride(nw), g, k))
                k += 1
        # the first stride the type's chain refuses, with the launch of the widest it takes: frame by frame, chained_frames = 0
        top = chain_nws(B)[-1]
        out.append(_chain_case(t, chain_stride(top + 1), 1, 0, frames=2 * chain_lanes(B, chain_stride(top)) + 1, note="refused"))
        out.append(_chain_case(t, 32, 1, 0, frames=5, note="refused"))  # ... and the pool of 32 columns, below the chain
        if B != 4:  # opt=1 twins on one workgroup per buffer and on the most the rule grants; sse2_sweeps stays 0: the pool path serves them
            for nw in (1, 5, 8) + ((16,) if B == 1 else ()):
                for g in sorted({1, granted(B, chain_stride(nw))[-1]}):
                    out.append(_chain_case(t, chain_stride(nw), g, 0, opt=1))
    # the three 8-bit instances by block size, one strip, one workgroup per buffer: a short chain of 5 passes (3 sets of waves, 192
    # threads), 16 passes (8 sets: 512 threads, the instance bounded by kChain8Threads / 2) and 18 (9 sets, 576 threads: the other)
    for n in (5, 16, 18):
        out.append(_chain_case("Y8", 64, 1, 0, frames=n, note="block"))
    out.append(_chain_case("Y8", 64, 1, 0, opt=1, frames=5, note="block"))  # ... and the smaller instance in the saturating arithmetic
    return out


CHAIN = _chains()


def chained_frames(c):
    """sn_info.chained_frames after the case's launches: a run of one frame (one pass) is no chain."""
    if chain_lanes(BYTES[c.fmt], stride_of(c)) < 2:
        return 0
    return c.launches * sum(r for r in field_runs(c.order, c.parities) if r > 1)


def chain_launches_of(c):
    """(groups, passes, instance) of every chain launch of ONE launch of the case."""
    B, s = BYTES[c.fmt], stride_of(c)
    if chain_lanes(B, s) < 2:
        return []
    g = chain_groups(B, s, c.chain)
    return [(g, r, chain_instance(B, s, g, r, c.opt)) for r in field_runs(c.order, c.parities) if r > 1]


def every_case():
    return [c for table in PLANE_TABLES.values() for c in table] + CHAIN


# ---- frames and the reference ----------------------------------------------------------------------------------------------------------
def clip_of(c):
    return clip_format(c.fmt, c.w, c.h)


def frames_of(c):
    """Per launch the frames of the case (launch = 0: one "launch" of all its frames)."""
    clip, n = clip_of(c), len(c.patterns)
    return [[synth.frame(clip, c.patterns[i], seed=c.seed + launch * n + i) for i in range(n)] for launch in range(c.launches)]


def reference_of(c):
    """One reference instance fed the case's frames in order: the opt=0 oracle, or the numpy model of the SSE2 path for opt=1."""
    clip = clip_of(c)
    if c.opt:
        from tests.sse2_model import Sse2SangNom
        return Sse2SangNom(clip.width, clip.height, bytes=clip.bytes, bits=clip.bits, order=c.order, aa=c.aa)
    from oracle.oracle import Oracle
    from tests.util import oracle_cfg
    return Oracle(oracle_cfg(clip, order=c.order, aa=c.aa))


def reference_frame(ref, c, src, parity):
    """(output plane, copy of the pool after it) of the next frame."""
    if c.opt:
        out = ref.get_frame(src, parity=parity)[0]
        return out, ref.pool.astype(clip_of(c).dtype)
    out = ref.process(src, parity=parity)[0]
    return out, ref.pool().copy()
