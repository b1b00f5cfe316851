"""Every pair of configuration options through ONE covering table (tests/test_config_pairs_gpu.py runs its rows on the device,
tests/test_config_pairs_cpu.py checks the table itself).  TEST INFRASTRUCTURE ONLY.

The other case tables walk one dimension of the library each and hold the rest still (order=1, aa=48, no dh, every plane on,
the default arithmetic).  Here the dimensions are FACTORS, the rules that make a combination impossible are CONSTRAINTS, each
stated once as a predicate over a partial assignment, and ROWS is built at import, without random numbers, so that

  * every feasible pair of levels of any two factors occurs in at least one row, and
  * every feasible triple of levels of the factors that decide routing (ROUTING) occurs in at least one row.

A pair or a triple is infeasible only if NO complete assignment contains it; that is decided by search with backtracking
(complete()), never by the builder giving up.  The infeasible pairs are listed by family with their reasons (INFEASIBLE_PAIRS);
a triple over ROUTING is infeasible only where one of its pairs is (INFEASIBLE_TRIPLES is empty, and the CPU test proves it).

The generator (build_rows) works in parameter order with open slots: the rows start as every feasible combination of the three
routing factors with most levels (SPINE: 92 rows, and no table that covers the triples can be shorter); every other factor
then goes into every row at the level that closes most of what is still open among the levels that leave the row completable,
ties to the level declared first, and a slot that would close nothing stays open for a later combination; what a factor leaves
open goes into the first row whose open slots take it, or seeds a new row.  It reaches 113 rows for 1872 pairs and 1186 triples
(a crude greedy gives 55 rows for the pairs alone; the triples over SPINE alone need 92).  EXTRA holds the rows the algorithm
cannot express: a 12-bit row, rows for the routes the covering rows reach less than twice for certain, and every mismatch
this table finds (none so far: all rows were bit-exact and on their routes when the table was built).

expected(row) composes the reference as tools/fuzz.py does (which imports compose() from here); predicted(row) says what
sn_info / sn_parts_info / sn_surface_info must report after the row has run.  It decides every launch of the row as
decide_launch does, from the predictors of tests/small_plane_cases.py -- auto mode's band count and its estimate of the faster
path (prefer_pool) included, restated there and held against sn_route.h for every launch of every row by the CPU test.  More
than one count is allowed only where the content decides: after a band that failed its check, the unforced bands of later
launches may be paused.
"""
import itertools

import numpy as np

from avisynth_sangnom2_amd import ClipFormat, capi, synth
from oracle.oracle import Config, Oracle
from tests import msb_surface_cases as mc
from tests import small_plane_cases as sp
from tests import sse2_model as sm

# ---- factors ---------------------------------------------------------------------------------------------------------------------
FACTORS = (
    ("stype", ("u8", "u10", "u16", "f32")),
    ("chroma", ("y", "420", "422", "444")),
    ("width", (64, 72, 544, 1000, 3872)),
    ("height", (40, 8, 200)),
    ("order", (1, 0, 2)),
    ("aa", (48, 128, 0)),
    ("aac", (48, 128, 0)),
    ("dh", (0, 1)),
    ("planes", ("all", "luma_off", "chroma_off")),
    ("ext", ("none", "isolated", "fresh")),
    ("way", ("host", "ring", "batch", "surf", "semi_in", "semi_out")),
    ("align", ("lsb", "msb_in", "msb_out")),
    ("arith", ("cxx", "sse2_k0", "sse2_k1")),
    ("launch", ("sweep", "auto", "bands3", "bands6top", "pool")),
    ("chroma_sweeps", (0, 1)),
    ("chain", (0, -1, 2)),
    ("parts", (0, 1)),
    ("nframes", (3, 1, 9)),
    ("pattern", ("edges", "noise", "checker", "sine")),
)
NAMES = tuple(n for n, _ in FACTORS)
LEVELS = dict(FACTORS)
ROUTING = ("stype", "chroma", "width", "ext", "arith", "launch")
STYPE = {"u8": (1, 8), "u10": (2, 10), "u12": (2, 12), "u16": (2, 16), "f32": (4, 32)}  # (bytes, bits); u12: EXTRA only
SUBSAMPLING = {"y": (1, 0, 0), "420": (3, 1, 1), "422": (3, 1, 0), "444": (3, 0, 0)}   # (planes, sub_w, sub_h)
SURFACE_WAYS = ("surf", "semi_in", "semi_out")
SSE2_PATTERN = {"noise": "noise", "checker": "checker2", "edges": "noise01", "sine": "noise01"}  # tests/golden/SSE2_FIXTURES.md
RING_DEPTHS = (2, 8)  # host_depth of the ring rows, alternating: below and above three frames

# ---- constraints: a predicate over a PARTIAL assignment (g(name) is None where the factor is still open) -------------------------
_SUB = ("420", "422")


def _in(v, allowed):
    return v is None or v in allowed


CONSTRAINTS = (
    ("plane switches need three planes",
     "sn_route.h ClipPlan::process: luma / chroma name planes 0 and 1..2; tools/fuzz.py draws them for every clip, a Y clip has none to switch",
     lambda g: _in(g("planes"), ("all",)) or _in(g("chroma"), ("420", "422", "444"))),
    ("semi-planar needs three planes and is not float",
     "sangnom_hip.h SN_LAYOUT_SEMIPLANAR: a UV plane of 8- or 16-bit samples (tools/fuzz.py: clip.planes == 3 and clip.bytes < 4)",
     lambda g: _in(g("way"), ("host", "ring", "batch", "surf")) or (_in(g("chroma"), ("420", "422", "444")) and _in(g("stype"), ("u8", "u10", "u16")))),
    ("MSB needs 9 to 15 bits and a surface way",
     "sangnom_hip.h SN_LAYOUT_*_MSB: shift 16 - bits_per_sample, only sn_process_device_surfaces takes a layout",
     lambda g: _in(g("align"), ("lsb",)) or (_in(g("stype"), ("u10",)) and _in(g("way"), SURFACE_WAYS))),
    ("opt=1 is not float, and its narrowest plane is at least 32 / bytes columns",
     "sn_route.h clip_plan: SN_ARITH_SSE2 is refused below two vectors per row, float has one arithmetic (tools/fuzz.py skips both)",
     lambda g: _in(g("arith"), ("cxx",)) or (_in(g("stype"), ("u8", "u10", "u16")) and (g("width") is None or g("width") // 2 >= 32))),
    ("chroma_sweeps=1 is 8-bit 4:2:0 or 4:2:2",
     "sn_route.h clip_plan: uv_geometry needs bytes_per_sample == 1 and subsampled chroma; elsewhere the policy field is not read",
     lambda g: _in(g("chroma_sweeps"), (0,)) or (_in(g("stype"), ("u8",)) and _in(g("chroma"), _SUB))),
    ("column_parts=1 needs a width of 3872, 2 or 4 bytes, and a plane on its own",
     "sn_route.h fused_parts_plane_eligible / plan_parts: 16-bit or float, wider than 3840, not behind fused_needs_pools (Y, 4:4:4 or isolated)",
     lambda g: _in(g("parts"), (0,)) or (_in(g("width"), (3872,)) and _in(g("stype"), ("u10", "u16", "f32")) and
                                        (_in(g("chroma"), ("y", "444")) or _in(g("ext"), ("isolated",))))),
    ("band levels need height 200",
     "sn_route.h band_count: at least two bands of kMinBandRows rows in every processed plane (tests/small_plane_cases.band_count); the levels are auto mode's",
     lambda g: _in(g("launch"), ("sweep", "auto", "pool")) or _in(g("height"), (200,))),
    ("chain != 0 needs a history-carrying clip",
     "sn_route.h chain_planes (tests/small_plane_cases.chain_ok): not history-free, not isolated, every processed plane a multiple of 8 wide",
     lambda g: _in(g("chain"), (0,)) or (_in(g("width"), (72, 1000)) and _in(g("ext"), ("none",)) and
                                        (_in(g("chroma"), ("y", "444")) or _in(g("planes"), ("chroma_off",)) and _in(g("dh"), (0,))))),
    ("9 frames go through a device way only",
     "tools/fuzz.py: host frames and the ring take 1..4 frames, a device batch 2..10",
     lambda g: _in(g("nframes"), (1, 3)) or _in(g("way"), ("batch",) + SURFACE_WAYS)),
    ("the checkers do not go with dh",
     "no rule of the library's but of this table (no row tests nothing): with dh every line is kept, a line pair of checker / checker2 is identical or inverse, "
     "and smoothed over three rows the vertical cost is the least or the least is above the threshold -- the plain mean everywhere, whatever the seed",
     lambda g: _in(g("pattern"), ("edges", "noise", "sine")) or _in(g("dh"), (0,))),
    ("the checker needs a threshold of 128",
     "no rule of the library's but of this table (no row tests nothing): the kept lines of the three-line checker are identical or inverse in pairs and its least "
     "smoothed cost lies between the thresholds of 48 and 128 -- with 48 the plain mean wins on half the geometries, whatever the seed (opt=1 rows run checker2)",
     lambda g: not (g("pattern") == "checker" and g("arith") == "cxx" and (g("aa") == 48 or (g("aac") == 48 and g("chroma") in ("420", "422", "444"))))),
    ("the checker needs more than four lines in every plane",
     "no rule of the library's but of this table (no row tests nothing): the 4:2:0 chroma planes of an 8-line clip keep two lines of the same three-line "
     "block, and the one line between them is their mean (opt=1 rows run checker2, whose blocks are two lines high)",
     lambda g: not (g("pattern") == "checker" and g("arith") == "cxx" and g("height") == 8 and g("chroma") == "420")),
    ("3872 does not go with height 200",
     "cost only: nothing in the library forbids it, the largest row is 1000x200 or 3872x40",
     lambda g: _in(g("width"), (64, 72, 544, 1000)) or _in(g("height"), (8, 40))),
)


def adjust(chroma, w, h):
    """Subsampled widths and heights as tools/fuzz.py adjusts them (none of the table's levels moves: the CPU test asserts it)."""
    planes, subw, subh = SUBSAMPLING[chroma]
    if planes == 3:
        w -= w % (4 if subw else 1) or 0
        if subh:
            h += (-h) % 4
        if subw and (w // 2) % 2:
            w += 2
    return w, h


def consistent(r):
    return all(pred(r.get) for _, _, pred in CONSTRAINTS)


_complete_cache = {}


def complete(partial):
    """A complete assignment that contains `partial`, or None: depth-first over the open factors in declared order, every
    constraint asked as soon as the factors it names are set."""
    key = tuple(sorted(partial.items(), key=lambda kv: NAMES.index(kv[0])))
    if key not in _complete_cache:
        r = dict(partial)

        def go(i):
            if i == len(NAMES):
                return True
            n = NAMES[i]
            if n in partial:
                return go(i + 1)
            for v in LEVELS[n]:
                r[n] = v
                if consistent(r) and go(i + 1):
                    return True
            r.pop(n, None)
            return False
        _complete_cache[key] = dict(r) if consistent(r) and go(0) else None
    return _complete_cache[key]


def combos(names, k):
    """Every assignment of levels to k of the named factors, as a tuple of (factor, level) in declared order."""
    for fs in itertools.combinations(names, k):
        for vs in itertools.product(*(LEVELS[f] for f in fs)):
            yield tuple(zip(fs, vs))


def feasible_targets():
    """(the feasible pairs of any two factors, the feasible triples over ROUTING), in declared order."""
    pairs = [c for c in combos(NAMES, 2) if complete(dict(c)) is not None]
    triples = [c for c in combos(ROUTING, 3) if complete(dict(c)) is not None]
    return pairs, triples


# ---- the infeasible combinations, by family: {factor: levels} x {factor: levels}, and why -----------------------------------------
INFEASIBLE_PAIRS = (
    (dict(chroma=("y",)), dict(planes=("luma_off", "chroma_off")), "plane switches need three planes"),
    (dict(chroma=("y",)), dict(way=("semi_in", "semi_out")), "semi-planar needs three planes"),
    (dict(stype=("f32",)), dict(way=("semi_in", "semi_out")), "semi-planar is not float"),
    (dict(stype=("u8", "u16", "f32")), dict(align=("msb_in", "msb_out")), "MSB needs 9 to 15 bits"),
    (dict(way=("host", "ring", "batch")), dict(align=("msb_in", "msb_out")), "MSB needs a surface way"),
    (dict(stype=("f32",)), dict(arith=("sse2_k0", "sse2_k1")), "opt=1 is not float"),
    (dict(stype=("u10", "u16", "f32")), dict(chroma_sweeps=(1,)), "chroma_sweeps=1 is 8-bit"),
    (dict(chroma=("y", "444")), dict(chroma_sweeps=(1,)), "chroma_sweeps=1 is 4:2:0 or 4:2:2"),
    (dict(align=("msb_in", "msb_out")), dict(chroma_sweeps=(1,)), "MSB is 10-bit, chroma_sweeps=1 8-bit"),
    (dict(width=(64, 72, 544, 1000)), dict(parts=(1,)), "column_parts=1 needs a width of 3872"),
    (dict(stype=("u8",)), dict(parts=(1,)), "column_parts=1 needs 2 or 4 bytes"),
    (dict(chroma_sweeps=(1,)), dict(parts=(1,)), "chroma_sweeps=1 is 8-bit, column_parts=1 is not"),
    (dict(height=(200,)), dict(parts=(1,)), "column_parts=1 needs 3872, which does not go with height 200"),
    (dict(launch=("bands3", "bands6top")), dict(parts=(1,)), "band levels need height 200, column_parts=1 a width that excludes it"),
    (dict(chain=(-1, 2)), dict(parts=(1,)), "chain != 0 needs width 72 or 1000, column_parts=1 3872"),
    (dict(height=(8, 40)), dict(launch=("bands3", "bands6top")), "band levels need height 200"),
    (dict(width=(3872,)), dict(launch=("bands3", "bands6top")), "band levels need height 200, which 3872 does not go with"),
    (dict(width=(64, 544, 3872)), dict(chain=(-1, 2)), "chain != 0 needs a history-carrying clip: width 72 or 1000"),
    (dict(ext=("isolated", "fresh")), dict(chain=(-1, 2)), "chain != 0: chain_planes takes no isolated context"),
    (dict(nframes=(9,)), dict(way=("host", "ring")), "9 frames go through a device way only"),
    (dict(dh=(1,)), dict(pattern=("checker",)), "the checkers do not go with dh: the plain mean everywhere, the row would prove nothing"),
    (dict(width=(3872,)), dict(height=(200,)), "3872 does not go with height 200 (cost only)"),
)
INFEASIBLE_TRIPLES = ()  # over ROUTING: none beyond those that hold an infeasible pair


def listed_infeasible_pairs():
    out = {}
    for a, b, why in INFEASIBLE_PAIRS:
        (fa, la), (fb, lb) = list(a.items())[0], list(b.items())[0]
        for x in la:
            for y in lb:
                c = tuple(sorted(((fa, x), (fb, y)), key=lambda kv: NAMES.index(kv[0])))
                out[c] = why
    return out


# ---- the generator ---------------------------------------------------------------------------------------------------------------
def _key(kv):
    return NAMES.index(kv[0])


def _closed_by(r, new):
    """The pairs, and the triples over ROUTING, among what the partial row r holds that contain one of the factors `new`."""
    items = sorted(r.items(), key=_key)
    out = {c for c in itertools.combinations(items, 2) if c[0][0] in new or c[1][0] in new}
    rit = [kv for kv in items if kv[0] in ROUTING]
    if any(n in ROUTING for n in new):
        out |= {c for c in itertools.combinations(rit, 3) if any(kv[0] in new for kv in c)}
    return out


def _put(r, levels, open_):
    r.update(levels)
    open_ -= _closed_by(r, set(levels))


def _extend(r, n, open_, must):
    """Sets factor n of the partial row r to the level that closes most of what is open, among the levels that leave the row
    completable; ties go to the level declared first.  A level that closes nothing is not set unless `must`: the slot stays
    open for a combination that needs it later."""
    best, best_gain = None, 0 if not must else -1
    for v in LEVELS[n]:
        r[n] = v
        if complete(r) is not None:
            gain = len(_closed_by(r, {n}) & open_)
            if gain > best_gain:
                best, best_gain = v, gain
        del r[n]
    if best is not None:
        _put(r, {n: best}, open_)


SPINE = ("stype", "width", "launch")  # the three routing factors with most levels: their feasible product is the table's spine
ROUTING_REST = ("chroma", "ext", "arith")  # the order in which the other routing factors go in


def build_rows():
    """In parameter order, with open slots.  The rows start as every feasible combination of SPINE (no table that covers the
    triples can be shorter).  Every other factor, the routing factors first, then goes into all rows, row by row (_extend);
    each combination it leaves open among the factors handled so far goes into the first row whose open slots take it, or
    seeds a new row.  At the end every slot still open is filled the same greedy way."""
    pairs, triples = feasible_targets()
    targets = triples + pairs
    open_ = set(targets)
    rows = []
    for c in combos(SPINE, 3):
        if complete(dict(c)) is not None:
            rows.append({})
            _put(rows[-1], dict(c), open_)
    done = list(SPINE)
    for n in list(ROUTING_REST) + [m for m in NAMES if m not in ROUTING]:
        for r in rows:
            _extend(r, n, open_, False)
        done.append(n)
        for t in targets:
            if t not in open_ or not all(f in done for f, _ in t):
                continue
            for r in rows:
                if all(r.get(f, v) == v for f, v in t) and complete({**r, **dict(t)}) is not None:
                    break
            else:
                r = {}
                rows.append(r)
            _put(r, {f: v for f, v in t if f not in r}, open_)
    for r in rows:
        for n in NAMES:
            if n not in r:
                _extend(r, n, open_, True)
    assert not open_, sorted(open_)[:5]
    for r in rows:
        assert consistent(r) and set(r) == set(NAMES)
    return [{n: r[n] for n in NAMES} for r in rows]


class Row(dict):
    """A complete assignment, its position in the table (the seeds derive from it) and what is fixed by hand for EXTRA rows."""

    def __init__(self, levels, index, name=None):
        super().__init__(levels)
        self.index, self.name = index, name

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    @property
    def id(self):
        r = self
        tag = f"{r.stype}-{r.chroma}-{r.width}x{r.height}-o{r.order}-aa{r.aa}-aac{r.aac}-dh{r.dh}-{r.planes}-{r.ext}-{r.way}-{r.align}-{r.arith}-" \
              f"{r.launch}-cs{r.chroma_sweeps}-ch{r.chain}-cp{r.parts}-n{r.nframes}-{pattern_of(r)}"
        return tag if self.name is None else f"{self.name}-{tag}"


ROWS = [Row(r, i) for i, r in enumerate(build_rows())]

_PLAIN = dict(height=40, order=1, aa=48, aac=48, dh=0, planes="all", ext="none", align="lsb", arith="cxx", launch="sweep", chroma_sweeps=0, chain=0,
              parts=0, nframes=3, pattern="edges")

# Rows the algorithm cannot express.  The first: a 12-bit clip (P012 on the way in: shift 4), the one odd depth besides 10.
EXTRA = [
    Row(dict(stype="u12", chroma="420", width=544, height=40, order=0, aa=48, aac=128, dh=0, planes="all", ext="none", way="semi_in", align="msb_in",
             arith="cxx", launch="sweep", chroma_sweeps=0, chain=0, parts=0, nframes=3, pattern="edges"), 1000, "p012"),
    # routes the covering rows reach less than twice for certain (the spine has one row per sample type, width and launch level):
    # U and V as one sweep, 4:2:0 and 4:2:2; the coupled luma sweep with two chroma sweeps, by sample type and by policy; column parts;
    # the padded sweep at 1000 columns
    Row(dict(_PLAIN, stype="u8", chroma="420", width=544, way="host"), 1001, "uv"),
    Row(dict(_PLAIN, stype="u8", chroma="422", width=64, way="batch", nframes=9, order=0, dh=1), 1002, "uv"),
    Row(dict(_PLAIN, stype="u16", chroma="420", width=544, way="ring", order=2), 1003, "coupled"),
    Row(dict(_PLAIN, stype="u8", chroma="420", width=64, way="batch", chroma_sweeps=1, pattern="noise"), 1004, "coupled"),
    Row(dict(_PLAIN, stype="f32", chroma="y", width=3872, way="batch", parts=1, pattern="noise"), 1005, "parts"),
    Row(dict(_PLAIN, stype="u16", chroma="y", width=1000, way="host", ext="fresh", pattern="sine"), 1006, "padded"),
    # auto mode cutting bands by its own count (no covering row has a plane of 16 rows that the sweeps serve in auto mode): noise
    # never fails the check, edges may
    Row(dict(_PLAIN, stype="u8", chroma="y", width=544, height=200, way="host", launch="auto", pattern="noise"), 1007, "autobands"),
    Row(dict(_PLAIN, stype="f32", chroma="444", width=64, height=200, way="batch", launch="auto"), 1008, "autobands"),
]
ALL_ROWS = ROWS + EXTRA


# ---- a row as the library and the references see it -------------------------------------------------------------------------------
PARITIES = (1, 0, 0, 1, 1, 0, 1, 0, 1)
SEED_BUMP = {}  # row id -> added to the row's seeds: where the first seeds left a processed plane on the threshold arm alone


def pattern_of(row):
    """The row's pattern; rows with opt=1 draw from the three on which the two arithmetics differ (SSE2_PATTERN)."""
    return row["pattern"] if row["arith"] == "cxx" else SSE2_PATTERN[row["pattern"]]


def clip_of(row):
    (B, bits), (planes, subw, subh) = STYPE[row["stype"]], SUBSAMPLING[row["chroma"]]
    w, h = adjust(row["chroma"], row["width"], row["height"])
    return ClipFormat(width=w, height=h, bytes=B, bits=bits, planes=planes, subw=subw, subh=subh)


def kw_of(row):
    """The filter's arguments."""
    return dict(order=row["order"], aa=row["aa"], aac=row["aac"], dh=bool(row["dh"]), luma=row["planes"] != "luma_off", chroma=row["planes"] != "chroma_off")


def opt_of(row):
    return 0 if row["arith"] == "cxx" else 1


def isolated_context(row):
    """ClipPlan::isolated: fresh_pool, or isolated_planes on a clip of three planes."""
    return row["ext"] == "fresh" or (row["ext"] == "isolated" and clip_of(row).planes > 1)


def is_history_free(row):
    """sn_info.history_free (clip_plan)."""
    clip, kw = clip_of(row), kw_of(row)
    if row["ext"] == "fresh":
        return True
    if isolated_context(row):
        return all(w % 32 == 0 for w, ho, on in sp.planes_of(clip, kw) if on)
    return sp.history_free(clip, kw)


def calls_of(row):
    """Calls per row: a history-carrying clip runs its way twice on one context, so that pool state crosses a call boundary; so
    does a one-frame row with order=0, whose parities must include both 0 and 1."""
    return 2 if not is_history_free(row) or (row["nframes"] == 1 and row["order"] == 0) else 1


def ring_depth(row):
    ring_rows = [r.index for r in ALL_ROWS if r["way"] == "ring"]
    return RING_DEPTHS[ring_rows.index(row.index) % 2]


def context_kw(row):
    """Everything SangNom2(clip, **context_kw(row)) takes."""
    kw = kw_of(row)
    kw.update(isolated_planes=row["ext"] == "isolated", fresh_pool=row["ext"] == "fresh", opt=opt_of(row), chroma_sweeps=row["chroma_sweeps"],
              chain=row["chain"], column_parts=row["parts"], max_batch=row["nframes"])
    if row["arith"] != "cxx":
        kw["sse2_sweeps"] = 1 if row["arith"] == "sse2_k1" else 0
    if row["launch"] == "sweep":
        kw["small_launches"] = capi.SN_SMALL_SWEEP
    else:
        kw["small_launches"] = capi.SN_SMALL_AUTO
    if row["launch"] == "pool":
        kw["mode"] = "pool"
    if row["way"] == "ring":
        kw["host_depth"] = ring_depth(row)
    return kw


def bands_of(row):
    """set_bands' arguments, or None.  bands6top: a run-up of every row there is -- each band starts at row 1, where the zero state
    it starts from IS the state, so no input can fail its check."""
    if row["launch"] == "bands3":
        return (3, 0)
    if row["launch"] == "bands6top":
        return (6, 2 * clip_of(row).height)
    return None


def frames_of(row):
    """(frames, parities) of all calls of the row: synth.frame with seeds derived from the row's index."""
    clip, n = clip_of(row), row["nframes"] * calls_of(row)
    seed0 = 7919 * (row.index + 1) + SEED_BUMP.get(row.id, 0)
    frames = [synth.frame(clip, pattern_of(row), seed=seed0 + f) for f in range(n)]
    return frames, [PARITIES[f % len(PARITIES)] for f in range(n)]


# ---- expected values ---------------------------------------------------------------------------------------------------------------
def cfg_of(clip, **kw):
    return Config(width=clip.width, height=clip.height, bytes=clip.bytes, bits=clip.bits, planes=clip.planes, subw=clip.subw, subh=clip.subh, **kw)


def reference(clip, opt, **kw):
    """process(planes, parity) of one reference instance: the C oracle (opt=0) or the numpy model of the SSE2 path (opt=1)."""
    if opt == 1:
        m = sm.model_for(1, clip.width, clip.height, bytes=clip.bytes, bits=clip.bits, planes=clip.planes, subw=clip.subw, subh=clip.subh, **kw)
        return lambda planes, parity: m.get_frame(planes, parity=parity)
    o = Oracle(cfg_of(clip, **kw))
    return lambda planes, parity: o.process(planes, parity=parity)


def compose(clip, frames, parity, kw, ext, opt):
    """The reference's frames for one context: ext "none": one instance through the frames; "isolated": one Y-clip instance per
    plane; "fresh": a new instance per plane and frame.  kw: order, aa, aac, dh, luma, chroma."""
    if ext == "none":
        ora = reference(clip, opt, **kw)
        return [ora(frames[f], parity[f]) for f in range(len(frames))]
    per_plane = {}
    want = []
    for f in range(len(frames)):
        outs = []
        for p in range(clip.planes):
            pl = frames[f][p]
            yclip = ClipFormat(width=pl.shape[1], height=pl.shape[0], bytes=clip.bytes, bits=clip.bits)
            enabled = kw["luma"] if p == 0 else kw["chroma"]
            mk = lambda: reference(yclip, opt, order=kw["order"], aa=kw["aa"] if p == 0 else kw["aac"], dh=kw["dh"], luma=enabled)  # noqa: E731
            o = mk() if ext == "fresh" else per_plane.setdefault(p, mk())
            outs.append(o([pl], parity[f])[0])
        want.append(outs)
    return want


_cache = {}


def _frozen(frames):
    for fr in frames:
        for pl in fr:
            pl.setflags(write=False)
    return frames


def shift_of(row):
    return mc.shift_of(clip_of(row))


def reference_frames(row, opt=None):
    """(clip, frames, parities, the reference's LSB-aligned frames), once per session and left unchanged."""
    opt = opt_of(row) if opt is None else opt
    key = (row.id, opt)
    if key not in _cache:
        clip = clip_of(row)
        frames, par = frames_of(row)
        want = [[np.asarray(pl).astype(clip.dtype) for pl in fr] for fr in compose(clip, frames, par, kw_of(row), row["ext"], opt)]
        _cache[key] = (clip, _frozen(frames), par, _frozen(want))
    return _cache[key]


def expected(row):
    """(clip, frames, parities, what the destination must hold): the reference's frames, shifted left inside their 16-bit word
    where the destination is MSB-aligned."""
    clip, frames, par, want = reference_frames(row)
    if row["align"] == "msb_out":
        want = _frozen(mc.up(want, shift_of(row)))
    return clip, frames, par, want


def source_words(row):
    """The frames as the source surface holds them: MSB-aligned with random non-zero low bits where the row says so."""
    clip, frames, par, _ = reference_frames(row)
    return mc.msb_source(frames, shift_of(row), seed=row.index) if row["align"] == "msb_in" else frames


# ---- route prediction --------------------------------------------------------------------------------------------------------------
def route_plan(row):
    """clip_plan of the row (tests/small_plane_cases.clip_plan)."""
    return sp.clip_plan(clip_of(row), kw_of(row), ext=row["ext"], sse2={"cxx": None, "sse2_k0": 0, "sse2_k1": 1}[row["arith"]],
                        pool_mode=row["launch"] == "pool", parts_on=row["parts"] == 1)


def ring_launches(depth, nframes, calls):
    """Frames per launch of the host ring, per call: ensure_ring's groups (up to four, depth / groups slots each), a group is
    launched when its last slot is staged or when one of its staged slots is collected.  The test submits until every slot is
    in flight, collects the oldest, and collects the rest at the end of the call."""
    groups = min(depth, 4)
    per = depth // groups
    depth = groups * per
    lo, hi = [0] * groups, [0] * groups
    nxt, out = 0, []
    for _ in range(calls):
        launches, inflight = [], []

        def launch(g):
            if hi[g] > lo[g]:
                launches.append(hi[g] - lo[g])
                lo[g] = hi[g]

        def collect(slot):
            launch(slot // per)

        for _f in range(nframes):
            if len(inflight) == depth:
                collect(inflight.pop(0))
            g, k = nxt // per, nxt % per
            if k == 0:
                lo[g] = hi[g] = 0
            hi[g] = k + 1
            inflight.append(nxt)
            nxt = (nxt + 1) % depth
            if hi[g] == per:
                launch(g)
        while inflight:
            collect(inflight.pop(0))
        out.append(launches)
    return out


def launches_of(row):
    """Per call, the frames of each run_batch the row's way makes."""
    n, calls = row["nframes"], calls_of(row)
    if row["way"] == "host":
        return [[1] * n for _ in range(calls)]
    if row["way"] == "ring":
        return ring_launches(ring_depth(row), n, calls)
    return [[n] for _ in range(calls)]


def field_offset(order, parity):
    return (0 if parity else 1) if order == 0 else 0 if order == 1 else 1


def chained_frames(row):
    """run_batch on a history-carrying clip: the launch is cut into runs of one field offset (one frame each where there is no
    chain); a run of L frames with pn passes per frame is a chain when L * pn > 1."""
    if is_history_free(row) or isolated_context(row) or row["chain"] < 0:
        return 0
    pn = sp.chain_passes(clip_of(row), kw_of(row))
    if pn == 0:
        return 0
    _, par = frames_of(row)
    f, total = 0, 0
    for call in launches_of(row):
        for n in call:
            offs = [field_offset(row["order"], p) for p in par[f:f + n]]
            for _, run in itertools.groupby(offs):
                L = len(list(run))
                if L * pn > 1:
                    total += L
            f += n
    return total


def group_runs(row):
    """The frames of every run_group a history-free row makes: each launch of its way, cut into runs of one field offset."""
    _, par = frames_of(row)
    f, runs = 0, []
    for call in launches_of(row):
        for n in call:
            offs = [field_offset(row["order"], p) for p in par[f:f + n]]
            runs += [len(list(run)) for _, run in itertools.groupby(offs)]
            f += n
    return runs


def predicted(row):
    """What the info structs must report after every call of the row: counter -> the set of allowed values, and "routes": the
    routes the row reaches for certain (the CPU test counts them).  Every launch is decided as decide_launch decides it
    (tests/small_plane_cases.py restates band_count and prefer_pool; the CPU test holds both against the header for every launch
    of every row).  More than one value is allowed only where the content decides: a band that fails its check is counted in
    band_fallbacks, and the unforced bands of later launches are then paused (FallbackPause) as soon as the host has seen the
    count, so each later launch may go either way.  Noise with the default run-up and the run-up from the top never fail."""
    P = route_plan(row)
    clip, planes = P["clip"], P["planes"]
    B, T = clip.bytes, row["nframes"] * calls_of(row)
    hf, launch = P["history_free"], row["launch"]
    on = [o for _, _, o in planes] + [False] * (3 - clip.planes)
    swept = [on[p] and (P["fused"][p] if P["isolated"] else P["use_fused"]) for p in range(3)]
    # plan_parts: the planes a launch cuts; in auto mode a launch small enough for row bands (512 / n >= 3) sends them to the pool path
    cut = [swept[p] and P["marked"][p] and B >= 2 and not P["fresh"] and sp.nr(planes[p][1]) >= 1 and
           (not P["padded"][p] if P["isolated"] else not P["pools"]) for p in range(3)]
    if launch != "sweep":
        swept = [swept[p] and not P["marked"][p] for p in range(3)]
        cut = [False] * 3
    chained = chained_frames(row)
    rest = T - chained
    any_swept = any(swept)
    forced = bands_of(row)[0] if bands_of(row) else 0
    one_sweep = P["fused420"] and P["uv"] and row["chroma_sweeps"] == 0
    # every launch: (frames, bands, the estimate prefers the pool path)
    estimate = hf and launch in ("auto", "bands3", "bands6top")
    decided = []
    for n in (group_runs(row) if hf else [1] * rest):
        nb = 0
        if forced:
            nb = sp.band_count(sp.nr_min(P), forced) if sp.sweeps_serve_all(P) else 0
        elif launch == "auto":
            nb = sp.band_count_auto(P, n)
        decided.append((n, nb, estimate and sp.prefer_pool(P, n, row["chroma_sweeps"])))
    fallback_free = launch == "bands6top" or pattern_of(row) == "noise"
    # the ways the row can go: after a failed band every later UNFORCED band launch may be paused and left to the estimate
    ways = set()
    unforced = [k for k, (n, nb, pool) in enumerate(decided) if nb and not forced]
    later = unforced[1:] if not fallback_free else []
    for paused in itertools.chain.from_iterable(itertools.combinations(later, m) for m in range(len(later) + 1)):
        fused = banded = uv = 0
        for k, (n, nb, pool) in enumerate(decided):
            if nb and k not in paused:
                fused, banded = fused + (n if any_swept else 0), banded + n
            elif any_swept and not pool:
                fused, uv = fused + n, uv or int(one_sweep)
        ways.add((fused, banded, uv))
    certain = len(ways) == 1
    banded_any = any(w[1] for w in ways)
    out, routes = {}, set()
    out["history_free"], out["fused_eligible"] = {int(hf)}, {int(P["info_eligible"])}
    out["chained_frames"] = {chained}
    out["fused_frames"], out["banded_frames"], out["uv_sweeps"] = ({w[k] for w in ways} for k in range(3))
    out["band_fallbacks"] = {0} if fallback_free or not banded_any else set(range(max(w[1] for w in ways) + 1))
    fused_n, banded_n, uv_n = next(iter(ways))
    out["part_frames"] = {rest if any(cut) else 0}
    chroma_planar = clip.planes == 3 and on[1]
    out["split_frames"] = {T if row["way"] == "semi_in" and chroma_planar else 0}
    out["merged_frames"] = {T if row["way"] == "semi_out" and chroma_planar else 0}
    # the routes reached for certain
    if certain and fused_n:
        if banded_n:
            routes.add("bands")
        if fused_n > banded_n:  # launches on the whole-plane sweeps
            if P["fused420"]:
                routes.add("uv" if one_sweep else "coupled2")
            else:
                if any(cut):
                    routes.add("parts")
                if any(swept[p] and P["padded"][p] for p in range(3)):
                    routes.add("padded")
                if any(swept[p] and not P["padded"][p] and not cut[p] for p in range(3)):
                    routes.add({1: "sweep8", 2: "sweep16", 4: "sweep32"}[B])
    if certain and rest and (fused_n < rest or not all(swept[p] for p in range(3) if on[p])):
        routes.add("pool_request" if launch == "pool" else "pool_routed")
    if chained:
        routes.add("chain")
        if row["chain"] == 2:
            routes.add("chain_groups")
    if out["split_frames"] != {0}:
        routes.add("split")
    if out["merged_frames"] != {0}:
        routes.add("merge")
    if row["align"] != "lsb":
        routes.add("msb")
    out["routes"] = routes
    return out
