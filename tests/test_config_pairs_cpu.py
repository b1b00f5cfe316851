"""The covering table of tests/config_space.py, checked without a GPU: the coverage it promises is recomputed from the factors
and the constraints and found in the rows themselves; the constraints and the lists of infeasible combinations are audited by
exhaustive search; no row is one whose result any route would get right; the routes the table means to reach are predicted for
at least two rows each; and every prediction a row makes is held against csrc/sn_route.h on a host compiler.
"""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from avisynth_sangnom2_amd import clip_format
from oracle.oracle import validate
from tests import config_space as cs
from tests import small_plane_cases as sp
from tests.test_small_planes_cpu import MODES, ROOT, _compile, _plane, _route_answers
from tests.test_small_planes_cpu import _route_query as _small_query
from tests.util import same


# ---- 1. coverage, from the table alone ---------------------------------------------------------------------------------------------

def _search(partial):
    """Exhaustive: every assignment of the open factors, pruned only where a constraint already fails."""
    names = [n for n in cs.NAMES if n not in partial]
    r = dict(partial)

    def go(i):
        if not cs.consistent(r):
            return False
        if i == len(names):
            return True
        for v in cs.LEVELS[names[i]]:
            r[names[i]] = v
            if go(i + 1):
                return True
            del r[names[i]]
        return False
    return go(0)


@pytest.fixture(scope="module")
def feasible():
    pairs = {c for c in cs.combos(cs.NAMES, 2) if _search(dict(c))}
    triples = {c for c in cs.combos(cs.ROUTING, 3) if _search(dict(c))}
    return pairs, triples


def test_every_feasible_pair_and_every_feasible_routing_triple_is_in_a_row(feasible):
    pairs, triples = feasible
    have = set()
    for r in cs.ROWS:
        items = tuple((n, r[n]) for n in cs.NAMES)
        have |= set(itertools.combinations(items, 2))
        have |= set(itertools.combinations(tuple(kv for kv in items if kv[0] in cs.ROUTING), 3))
    assert not pairs - have, sorted(pairs - have, key=str)[:8]
    assert not triples - have, sorted(triples - have, key=str)[:8]
    assert len(pairs) > 1800 and len(triples) > 1100
    # every level of every factor is there at all, and the docstring's count is the table's
    for n, levels in cs.FACTORS:
        assert {r[n] for r in cs.ROWS} == set(levels), n
    assert f"reaches {len(cs.ROWS)} rows for {len(pairs)} pairs and {len(triples)} triples" in cs.__doc__
    assert len(cs.ROWS) <= 115  # about twice what a crude greedy needs for the pairs alone; 92 is the floor (SPINE)


def test_the_table_is_deterministic_and_its_ids_are_unique():
    again = cs.build_rows()
    assert [dict(r) for r in cs.ROWS] == again
    ids = [r.id for r in cs.ALL_ROWS]
    assert len(set(ids)) == len(ids)
    src = open(cs.__file__).read()
    assert "import random" not in src and "import time" not in src and "os.environ" not in src


# ---- 2. the constraints ------------------------------------------------------------------------------------------------------------

def test_no_row_violates_a_constraint_and_the_reference_accepts_every_row():
    for r in cs.ALL_ROWS:
        if r.name is None:
            assert set(r) == set(cs.NAMES) and all(r[n] in cs.LEVELS[n] for n in cs.NAMES), r.id
        broken = [name for name, _, pred in cs.CONSTRAINTS if not pred(dict(r, stype="u10" if r["stype"] == "u12" else r["stype"]).get)]
        assert not broken, (r.id, broken)
        clip, kw = cs.clip_of(r), cs.kw_of(r)
        assert (clip.width, clip.height) == (r["width"], r["height"])  # tools/fuzz.py's adjustment moves none of the levels
        assert validate(cs.cfg_of(clip, **kw)) == "", (r.id, validate(cs.cfg_of(clip, **kw)))
        if r["order"] == 0:
            assert set(cs.frames_of(r)[1]) == {0, 1}, r.id
        if r["chain"] != 0:
            assert sp.chain_ok(clip, kw) and not cs.isolated_context(r), r.id
        if r["arith"] != "cxx":  # two vectors per row in the narrowest processed plane
            assert min(w for w, ho, on in sp.planes_of(clip, kw) if on) >= 32 // clip.bytes, r.id
    for name, reason, _ in cs.CONSTRAINTS:
        assert any(h in reason for h in ("sn_route.h", "sangnom_hip.h", "tools/fuzz.py", "cost only", "no row tests nothing")), name


def test_the_listed_infeasible_combinations_are_exactly_the_infeasible_ones(feasible):
    pairs, triples = feasible
    listed = cs.listed_infeasible_pairs()
    infeasible = set(cs.combos(cs.NAMES, 2)) - pairs
    assert not set(listed) - infeasible, sorted(set(listed) - infeasible, key=str)[:8]   # every listed one is truly infeasible
    assert not infeasible - set(listed), sorted(infeasible - set(listed), key=str)[:8]   # and no infeasible one is missing
    assert all(why for why in listed.values())
    # triples over the routing factors: infeasible only where one of their pairs is
    genuine = [t for t in set(cs.combos(cs.ROUTING, 3)) - triples if not any(p in infeasible for p in itertools.combinations(t, 2))]
    assert sorted(genuine) == sorted(cs.INFEASIBLE_TRIPLES)
    # the backtracking search of the module agrees with the exhaustive one
    assert {c for c in cs.combos(cs.NAMES, 2) if cs.complete(dict(c)) is not None} == pairs
    assert cs.complete(dict(way="host", launch="bands3")) is not None  # (what a greedy builder had given up on)


def test_ring_depths_stand_on_both_sides_of_the_frame_count():
    sides = {(cs.ring_depth(r) > r["nframes"]) for r in cs.ROWS if r["way"] == "ring" and r["nframes"] == 3}
    assert sides == {True, False}
    assert {cs.ring_depth(r) for r in cs.ROWS if r["way"] == "ring"} == set(cs.RING_DEPTHS)
    # the ring's launches as the test drives it: groups of one slot, groups of two with a straggler launched at its collect
    assert cs.ring_launches(2, 3, 2) == [[1, 1, 1], [1, 1, 1]] and cs.ring_launches(8, 3, 2) == [[2, 1], [1, 2]] and cs.ring_launches(8, 1, 2) == [[1], [1]]


# ---- 3. no row tests nothing -------------------------------------------------------------------------------------------------------

def _plain_mean(a, b, clip):
    if clip.bytes == 4:
        return (a + b) * np.float32(0.5)
    return ((a.astype(np.int64) + b.astype(np.int64) + 1) >> 1).astype(clip.dtype)


def _leaves_the_threshold_arm(row):
    """Per processed plane with a threshold: do the reference's interpolated lines differ anywhere from the mean of the lines
    above and below?"""
    clip, frames, par, want = cs.reference_frames(row)
    kw = cs.kw_of(row)
    out = {}
    for p, (pw, ho, on) in enumerate(sp.planes_of(clip, kw)):
        if not on or (row["aa"] if p == 0 else row["aac"]) == 0:
            continue
        differs = False
        for f, fr in enumerate(want):
            off = cs.field_offset(row["order"], par[f])
            kept = frames[f][p] if kw["dh"] else frames[f][p][off::2]
            lines = fr[p][off + 1::2][:sp.nr(ho)]
            differs = differs or not same(np.ascontiguousarray(lines), _plain_mean(kept[:-1], kept[1:], clip)[:sp.nr(ho)])
        out[p] = differs
    return out


def test_every_row_leaves_the_threshold_arm_in_every_processed_plane():
    checked = 0
    for r in cs.ALL_ROWS:
        got = _leaves_the_threshold_arm(r)
        assert all(got.values()), (r.id, got)
        checked += len(got)
    assert checked > 150


def test_the_two_arithmetics_differ_on_at_least_half_of_the_sse2_rows():
    rows = [r for r in cs.ALL_ROWS if r["arith"] != "cxx"]
    differ = 0
    for r in rows:
        _, _, _, a = cs.reference_frames(r)
        _, _, _, b = cs.reference_frames(r, opt=0)
        differ += any(not same(x, y) for fa, fb in zip(a, b) for x, y in zip(fa, fb))
    assert len(rows) >= 20 and 2 * differ >= len(rows), (differ, len(rows))


# ---- 4. the routes are reached -----------------------------------------------------------------------------------------------------

ROUTES = ("sweep8", "sweep16", "sweep32", "padded", "coupled2", "uv", "bands", "pool_request", "pool_routed", "chain", "chain_groups", "parts",
          "split", "merge", "msb")


def test_every_route_is_predicted_for_at_least_two_rows():
    count = {k: 0 for k in ROUTES}
    for r in cs.ALL_ROWS:
        for k in cs.predicted(r)["routes"]:
            if k in count:
                count[k] += 1
    assert all(v >= 2 for v in count.values()), count
    padded = [r for r in cs.ALL_ROWS if "padded" in cs.predicted(r)["routes"]]
    assert len([r for r in padded if r["ext"] == "fresh" and r["width"] in (72, 1000)]) >= 2
    # ... and the predictions are sets of one value wherever the launch level fixes the route
    for r in cs.ALL_ROWS:
        P = cs.predicted(r)
        if r["launch"] != "auto" or cs.pattern_of(r) == "noise" or not cs.is_history_free(r):
            assert all(len(P[k]) == 1 for k in ("fused_frames", "banded_frames", "chained_frames", "part_frames", "uv_sweeps")), r.id
        if r["launch"] == "bands6top":
            assert P["band_fallbacks"] == {0}, r.id


# ---- 5. the predictions are the header's ------------------------------------------------------------------------------------------

def _query(row, n):
    clip, kw = cs.clip_of(row), cs.kw_of(row)
    bands = cs.bands_of(row) or (0, 0)
    mode = "pool" if row["launch"] == "pool" else "auto"
    return [clip.bytes, clip.bits, clip.planes, clip.subw, clip.subh, clip.width, clip.height, int(kw["dh"]), int(kw["luma"]), int(kw["chroma"]), MODES[mode],
            int(row["ext"] == "isolated"), int(row["ext"] == "fresh"), cs.opt_of(row), row["parts"], int(row["arith"] == "sse2_k1"),
            n, 0, max(n, 4), max(n, 4), 1, int(row["launch"] == "sweep"), bands[0], bands[1], 0, 0, row["chroma_sweeps"],
            2 if sp.pool_stride(clip.width) >= 64 else 0, 0, 0]


def test_predictions_agree_with_the_route_header(tmp_path):
    """Every row is put to tests/c/route_check.cpp as the device test creates and launches it -- once for every size of launch the
    row makes, on slot 0 -- and the restated clip_plan, band counts and estimate (tests/small_plane_cases.py) and the counters
    predicted from them are held against clip_plan / decide_launch."""
    exe = _compile(tmp_path, os.path.join(ROOT, "tests", "c", "route_check.cpp"), "route_check")
    asked = []
    for r in cs.ALL_ROWS:
        sizes = sorted(set(cs.group_runs(r))) if cs.is_history_free(r) else [1]
        asked += [(r, n) for n in sizes]
    answers = _route_answers(exe, [_query(r, n) for r, n in asked])
    per_row, both = {}, {"bands": set(), "pool": set()}
    for (r, n), a in zip(asked, answers):
        P = cs.route_plan(r)
        clip = P["clip"]
        assert a["refusal"] == 0, (r.id, a)
        assert (a["history_free"], a["isolated"], a["fresh"]) == (int(P["history_free"]), int(P["isolated"]), int(P["fresh"])), (r.id, a)
        assert (a["use_fused"], a["fused420"], a["uv_geometry"]) == (int(P["use_fused"]), int(P["fused420"]), int(P["uv"])), (r.id, a)
        for p, (pw, ho, on) in enumerate(P["planes"]):
            pl = _plane(a, p)
            assert (pl["w"], pl["h_out"], pl["on"]) == (pw, ho, int(on)), (r.id, p, pl)
            if P["isolated"] and on:
                assert (pl["fused"], pl["padded"]) == (int(P["fused"][p]), int(P["padded"][p])), (r.id, p, pl)
            assert pl["parts"] == int(P["marked"][p]), (r.id, p, pl)
        if any(P["marked"]):
            assert a["parts_eligible"] == int(P["info_eligible"]), r.id
        # chains: the header's count of passes (sn_policy.chain < 0 switches them off in sn_api.hip)
        pn = 0 if P["history_free"] or P["isolated"] else sp.chain_passes(clip, P["kw"])
        assert a["chain"] == pn, (r.id, a["chain"], pn)
        assert (cs.chained_frames(r) > 0) <= (pn > 0 and r["chain"] >= 0), r.id
        # the launch: bands, then the estimate
        forced = cs.bands_of(r)[0] if cs.bands_of(r) else 0
        nb = (sp.band_count(sp.nr_min(P), forced) if sp.sweeps_serve_all(P) else 0) if forced else sp.band_count_auto(P, n) if r["launch"] == "auto" else 0
        assert a["nbands"] == nb, (r.id, n, a["nbands"], nb)
        if r["launch"] in ("auto", "bands3", "bands6top"):
            assert a["prefer_pool"] == int(sp.prefer_pool(P, n, r["chroma_sweeps"])), (r.id, n, a["prefer_pool"])
            both["pool"].add(bool(a["prefer_pool"]))
            if r["launch"] == "auto":
                both["bands"].add(nb > 0)
        else:
            assert a["prefer_pool"] == 0, (r.id, n)
        per_row.setdefault(r.id, []).append((n, a))
    assert both == {"bands": {True, False}, "pool": {True, False}}, both
    # the unforced band count on both sides of each of its limits: three bands by count (512 / n), eight rows a band, a quarter of the run-up
    extra = [(fmt, 512, h, n) for fmt in ("Y8", "Y16", "Y32") for h in (32, 34, 50, 52, 200, 400) for n in (1, 3, 170, 171)]
    counts = set()
    for (fmt, w, h, n), a in zip(extra, _route_answers(exe, [_small_query(fmt, w, h, n=n, slots=256) for fmt, w, h, n in extra])):
        clip = clip_format(fmt, w, h)
        assert a["nbands"] == sp.band_count_auto(sp.clip_plan(clip, {}), n), (fmt, h, n, a["nbands"])
        counts.add(a["nbands"])
    assert {0, 2, 3, 12, 16, 24} <= counts, counts
    # the counters, from the header's decisions for the row's launches (no band failing its check)
    for r in cs.ALL_ROWS:
        want, P = cs.predicted(r), cs.route_plan(r)
        T = r["nframes"] * cs.calls_of(r)
        rest = T - cs.chained_frames(r)
        by_n = dict(per_row[r.id])
        runs = cs.group_runs(r) if cs.is_history_free(r) else [1] * rest
        fused = sum(n for n in runs if sum(by_n[n]["fused"]) > 0)
        banded = sum(n for n in runs if by_n[n]["nbands"] > 0)
        cut = sum(n for n in runs if by_n[n]["parts_cut"])
        assert fused in want["fused_frames"] and banded in want["banded_frames"], (r.id, fused, banded, want)
        assert want["part_frames"] == {cut}, (r.id, cut, want["part_frames"])
        if len(want["fused_frames"]) == 1:
            assert want["fused_frames"] == {fused} and want["banded_frames"] == {banded}, r.id
        if rest == 0:
            assert want["fused_frames"] == {0} and want["chained_frames"] == {T}, r.id
        coupled = any(by_n[n]["route"] == "coupled" and sum(by_n[n]["fused"]) for n in runs)
        assert (1 in want["uv_sweeps"]) == (coupled and P["uv"] and r["chroma_sweeps"] == 0), (r.id, want["uv_sweeps"])
        if "pool_routed" in want["routes"] or "pool_request" in want["routes"]:
            assert any(not all(by_n[n]["fused"][p] for p, (pw, ho, on) in enumerate(P["planes"]) if on) for n in runs), r.id
    # only a band that may fail its check leaves a choice
    loose = [r for r in cs.ALL_ROWS if len(cs.predicted(r)["fused_frames"]) > 1 or len(cs.predicted(r)["banded_frames"]) > 1]
    assert all(r["launch"] == "auto" and cs.pattern_of(r) != "noise" for r in loose), [r.id for r in loose]
    # the restated constants this table leans on, on both sides: widths the sweeps take, widths marked for parts, history
    assert {bool(a["use_fused"]) for a in answers} == {True, False} and {bool(a["history_free"]) for a in answers} == {True, False}
    assert any(_plane(a, 0)["parts"] for a in answers) and any(_plane(a, 0)["padded"] for a in answers)


# ---- 6. tools/fuzz.py shares the composition ---------------------------------------------------------------------------------------

def test_the_fuzz_tool_imports_and_composes_its_reference_here():
    code = "import sys; sys.argv=['fuzz']; import tools.fuzz as f; from tests import config_space as cs; " \
           "assert f.compose is cs.compose and f.reference is cs.reference and f.cfg_of is cs.cfg_of; print('ok')"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout[-1000:], r.stderr[-1000:])
