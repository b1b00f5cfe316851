"""The table of tests/pool_geometry_cases.py, checked without a GPU: its restated rules are the header's (csrc/sn_pool_dispatch.h on a
host compiler, plain and under AddressSanitizer / UBSan), its cases reach every strip count, lane, row phase, wave count, chain
instance and workgroup count they are meant to reach -- recomputed here, not copied -- and the reference alone shows that every
case has something to say: a pool that changes from frame to frame, that is not zero where only the next frame looks, and, for the
saturating arithmetic, a box that does saturate.
"""
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

from avisynth_sangnom2_amd import clip_format
from oracle.oracle import validate
from tests import pool_geometry_cases as gc
from tests.util import oracle_cfg, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avisynth_sangnom2_amd", "csrc")
TYPES, BYTES = gc.TYPES, gc.BYTES


# ---- counts ----------------------------------------------------------------------------------------------------------------------------
def test_case_counts():
    """A silently dropped row fails here.  STRIPS: one stride at one strip (512 alone) and two at each of 2 .. 16, per type.  EDGE:
    31 strides, each with its narrower twin.  ROWS: 19 heights at 4 strides.  X8: 8 + 16 strides per type and 32 float launches of
    nine frames.  STRIDED: 7 strides and 4 widths.  SSE2: 22 strides, two types.  CHAIN: per (type, strip count, workgroups granted)
    33 + 27 + 27, 3 x 2 refused, 7 + 6 + 1 saturating twins, 3 by block size."""
    counts = Counter(c.table for c in gc.every_case())
    assert counts == dict(STRIPS=93, EDGE=186, ROWS=228, X8=104, STRIDED=33, SSE2=44, CHAIN=109)
    ids = [c.table + "-" + gc.case_id(c) for c in gc.every_case()]
    assert len(set(ids)) == len(ids) == 797
    assert all(c.fmt in TYPES and c.h % 2 == 0 for c in gc.every_case())


def test_odd_heights_cannot_be_cases():
    """The reference refuses them, and so does creation (tests/test_gpu_parity.py holds its texts against the reference's): the
    rows are walked through the even heights, whose pools have 2 .. 17 rows and 21, 23 and 33."""
    for h in gc.ODD_HEIGHTS_REFUSED:
        assert validate(oracle_cfg(clip_format("Y8", 544, h))) == "SangNom2: height must be even."
    assert sorted({gc.bh(h) for h in gc.ROW_HEIGHTS}) == list(range(2, 18)) + [21, 23, 33]


# ---- the rules on a host compiler --------------------------------------------------------------------------------------------------
def _compile(tmp_path, sanitized):
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else []
    exe = str(tmp_path / ("pool_dispatch_check" + ("_san" if sanitized else "")))
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, *extra, os.path.join(ROOT, "tests", "c", "pool_dispatch_check.cpp"), "-o", exe])
    return exe


def _restated(q):
    B, stride, bh_, frames, want = q
    name, threads, lds, attr = gc.pool_stage2(B, stride, bh_, frames)
    g = gc.chain_groups(B, stride, want)
    return f"{name} {threads} {lds} {int(attr)} {gc.chain_lanes(B, stride)} {g} {gc.chain_waves(B, g)}"


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
def test_restated_rules_agree_with_the_dispatch_header(tmp_path, sanitized):
    """tests/c/pool_dispatch_check.cpp: its own checks (stage 2's rule and the chain's three, against values written out by hand)
    pass, and its answers to every case of the table -- and to every stride a context can have, at one frame and at nine, for every
    workgroup count a policy can ask for -- are the restatement's."""
    exe = _compile(tmp_path, sanitized)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-3000:], r.stderr[-2000:])
    queries = [(BYTES[c.fmt], gc.stride_of(c), gc.bh(c.h), c.launch or 1, c.chain or 1) for c in gc.every_case()]
    queries += [(B, s, 12, n, want) for B in (1, 2, 4) for s in range(32, 8193, 32) for n in (1, 9) for want in (1, 2, 4, 8)]
    queries += [(B, 544, bh_, 1, 0) for B in (1, 2, 4) for bh_ in (1, 2)]
    text = "".join(" ".join(str(v) for v in q) + "\n" for q in queries)
    r = subprocess.run([exe, "query"], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(queries)
    for q, line in zip(queries, lines):
        assert line == _restated(q), (q, line, _restated(q))
    assert {line.split()[0] for line in lines} == {"none", "strided", "x8", "strips"}


# ---- coverage, recomputed ------------------------------------------------------------------------------------------------------------
def _strips_by_hand(nl):
    """One strip up to 64 lanes, else 62 real lanes in the first and 60 in every later one."""
    if nl <= 64:
        return 1
    n, covered = 1, 62
    while covered < nl:
        covered, n = covered + 60, n + 1
    return n


def _last_lane_by_hand(nl):
    """(strip, lane) of the last lane that owns columns, by laying the strips out: two ghost lanes left of every strip but the first."""
    if nl <= 64:
        return 0, nl - 1
    strip, first = 0, 0  # first: the first owned lane of the strip
    while first + (62 if strip == 0 else 60) < nl:
        first += 62 if strip == 0 else 60
        strip += 1
    return strip, (0 if strip == 0 else 2) + nl - 1 - first


def _schedule_by_hand(B, stride, frames):
    if stride < 256:
        return "strided"
    if stride >= 512 and _strips_by_hand(stride // 8) <= 16 and not (B == 4 and frames > 8):
        return "strips"
    return "x8"


@pytest.mark.parametrize("t", TYPES)
def test_strips_cover_every_strip_count_at_both_ends(t):
    B = BYTES[t]
    ends = {}
    for s in range(32, 8193, 32):
        if _schedule_by_hand(B, s, 3) == "strips":
            n = _strips_by_hand(s // 8)
            ends[n] = (min(ends.get(n, (s, s))[0], s), s)
    assert sorted(ends) == list(range(1, 17)) and ends[1] == (512, 512) and ends[2] == (544, 960) and ends[16] == (7232, 7680)
    cases = [c for c in gc.STRIPS if c.fmt == t]
    assert sorted(c.w for c in cases) == sorted({s for n in ends for s in ends[n]})
    for c in cases:
        name, threads, lds, attr = gc.stage2_of(c)
        assert name == "strips" and threads == 64 * _strips_by_hand(c.w // 8) and not attr
        assert c.launch == (3 if t == "Y32" else 0) and c.w % 32 == 0 and c.h == 24 and c.opt == 0


def test_edge_covers_every_last_lane_of_the_second_and_third_strip():
    want = {(1, lane) for lane in range(7, 60, 4)} | {(2, lane) for lane in range(3, 60, 4)}  # (a second strip begins with 65 lanes + 3: lane 7)
    for t in TYPES:
        cases = [c for c in gc.EDGE if c.fmt == t]
        full = [c for c in cases if c.w % 32 == 0]
        assert [c.w for c in full] == list(range(512, 1473, 32))
        got = {_last_lane_by_hand(c.w // 8) for c in full}
        assert got == want | {(0, 63), (3, 3)}
        assert {gc.last_lane(c.w) for c in full} == got
        narrow = [c for c in cases if c.w % 32 != 0]
        assert [c.w for c in narrow] == [s - 8 for s in range(512, 1473, 32)]
        for c in narrow:  # history-carrying, the same pool, three frames one by one
            assert c.w % 8 == 0 and gc.stride_of(c) == c.w + 8 and len(c.patterns) == 3 and c.launch == 0
        assert all(gc.stage2_of(c)[0] == "strips" for c in cases)


def test_rows_end_the_row_loops_at_every_phase():
    for t in TYPES:
        for s, name, nw in ((544, "strips", 2), (7680, "strips", 16), (480, "x8", 1), (8192, "x8", 16)):
            cases = [c for c in gc.ROWS if c.fmt == t and c.w == s]
            assert len(cases) == 19
            assert all(gc.stage2_of(c)[0] == name and gc.stage2_of(c)[1] == 64 * nw for c in cases)
            last = [(c.h + 1) // 2 - 1 for c in cases]  # bh - 1: the last row stage 2 smooths
            assert Counter(v % 5 for v in last).keys() == set(range(5)) and min(Counter(v % 5 for v in last).values()) >= 2
            assert Counter(v % 4 for v in last).keys() == set(range(4)) and min(Counter(v % 4 for v in last).values()) >= 2
            assert set(range(1, 17)) <= set(last)  # every count from one smoothed row to three refreshes and a row


def test_x8_covers_every_wave_count_both_lds_sides_and_idle_last_waves():
    for t in TYPES:
        plain = [c for c in gc.X8 if c.fmt == t and c.launch == 0]
        assert [c.w for c in plain] == list(range(256, 481, 32)) + list(range(7712, 8193, 32))
        assert all(_schedule_by_hand(BYTES[t], c.w, 1) == "x8" == gc.stage2_of(c)[0] for c in plain)
        idle = {c.w // 8 % 64 for c in plain} - {0}
        assert idle == set(range(4, 61, 4)), idle  # lanes of a partly idle last wave
        assert {gc.stage2_of(c)[3] for c in plain if c.w >= 7712} == {BYTES[t] != 1}  # 16-bit and float: above 48 KiB up there
    nine = [c for c in gc.X8 if c.launch == 9]
    assert all(c.fmt == "Y32" and c.w % 32 == 0 and _schedule_by_hand(4, c.w, 9) == "x8" == gc.stage2_of(c)[0] for c in nine)
    waves = {}
    for c in nine:
        waves.setdefault((c.w // 8 + 63) // 64, []).append(c.w)
    assert sorted(waves) == list(range(1, 17))
    for n, ws in waves.items():  # the narrowest: 4 lanes in the last wave (the first wave: 256 columns); the widest: a full one
        lo, hi = (256 if n == 1 else 512 * (n - 1) + 32), 512 * n
        assert lo in ws and hi in ws and gc.stage2_of(next(c for c in nine if c.w == lo))[1] == 64 * n
    attr = {c.w: gc.stage2_of(c)[3] for c in nine}
    assert attr[6144] is False and attr[6176] is True and gc.stage2_of(next(c for c in nine if c.w == 6144))[2] == 48 * 1024
    assert sum(1 for c in nine if _schedule_by_hand(4, c.w, 8) == "strips") >= 28  # what the rule sends to x8 for the ninth frame alone


def test_strided_and_sse2_tables():
    for t in TYPES:
        cases = [c for c in gc.STRIDED if c.fmt == t]
        assert [c.w for c in cases] == list(range(32, 225, 32)) + [255, 256, 257, 513]
        assert all(gc.stage2_of(c)[0] == "strided" for c in cases if c.w <= 224)
        assert [gc.stage2_of(c)[0] for c in cases if c.w > 224] == ["x8", "x8", "x8", "strips"]
    for t in ("Y8", "Y16"):
        cases = [c for c in gc.SSE2 if c.fmt == t]
        assert all(c.opt == 1 and c.patterns == ("noise", "noise01") for c in cases)
        ws = [c.w for c in cases]
        narrowest = [min(s for s in range(512, 7681, 32) if _strips_by_hand(s // 8) == n) for n in range(1, 17)]
        assert sorted(ws) == sorted(narrowest + [256, 480, 7712, 8192, 32, 224])
        assert Counter(gc.stage2_of(c)[0] for c in cases) == dict(strips=16, x8=4, strided=2)
    assert not [c for c in gc.SSE2 if c.fmt == "Y32"]


# The kernels of stage 2 as launch_pool_plane_t and launch_pool_chain pick them: (schedule or chain form, sample type, arithmetic)
PLANE_INSTANCES = {(s, t, a) for s in ("strided", "x8", "strips") for t in TYPES for a in (0, 1) if not (t == "Y32" and a)}
CHAIN_INSTANCES = {"f32", "f32-grouped", "u16", "u16-grouped", "u16-sse2", "u16-grouped-sse2", "u8-512", "u8-1024", "u8-grouped-512",
                   "u8-512-sse2", "u8-1024-sse2", "u8-grouped-512-sse2"}


def test_the_table_launches_every_instance():
    plane = {(gc.stage2_of(c)[0], c.fmt, c.opt) for table in gc.PLANE_TABLES.values() for c in table}
    assert plane == PLANE_INSTANCES and len(plane) == 15
    chain = {inst for c in gc.CHAIN for _, _, inst in gc.chain_launches_of(c)}
    assert chain == CHAIN_INSTANCES and len(chain) == 12


def test_chain_covers_every_strip_count_workgroup_count_and_instance():
    for t in TYPES:
        B = BYTES[t]
        top = 16 if B == 1 else 8
        derived = [c for c in gc.CHAIN if c.fmt == t and not c.note and not c.opt]
        seen = set()
        for c in derived:
            s = gc.stride_of(c)
            nw = _strips_by_hand(s // 8)
            assert c.w == s - 8 and c.w % 8 == 0 and c.launches == 2 and c.h == 24
            assert s == min(x for x in range(64, 8193, 32) if _strips_by_hand(x // 8) == nw)  # the narrowest stride the chain takes
            # an explicit policy is taken as it is: the workgroups are what the rule grants for it, here the value itself
            assert gc.chain_groups(B, s, c.chain) == c.chain
            waves = (16 if B == 1 else 32) // c.chain
            per_wg = (2 if B == 1 else 1) * (min(waves, 16) // nw)  # passes in flight in a workgroup
            assert per_wg >= 1 and c.launch == 2 * per_wg * c.chain + 1 == len(c.parities)
            assert sum(1 for p in c.parities if p == 0) == 1 and c.parities[c.launch // 2] == 0
            seen.add((nw, c.chain))
        want = {(nw, g) for nw in range(1, top + 1) for g in (1, 2, 4, 8) if g == 1 or min((16 if B == 1 else 32) // g, 16) >= nw}
        assert seen == want and len(derived) == len(want)
        assert Counter(c.order for c in derived)[0] in (len(derived) // 3, len(derived) // 3 + 1)
        # a 2160-wide plane, the turned pass of the anti-aliasing call on a 2160p clip, is five strips
        assert _strips_by_hand(2176 // 8) == 5 and any(nw == 5 for nw, g in seen)
        refused = [c for c in gc.CHAIN if c.fmt == t and c.note == "refused"]
        assert sorted(_strips_by_hand(gc.stride_of(c) // 8) for c in refused) == [1, top + 1] and sorted(gc.stride_of(c) for c in refused)[0] == 32
        assert all(gc.chained_frames(c) == 0 and gc.chain_launches_of(c) == [] for c in refused)
        twins = [c for c in gc.CHAIN if c.fmt == t and c.opt and not c.note]
        assert {_strips_by_hand(gc.stride_of(c) // 8) for c in twins} == ({1, 5, 8, 16} if B == 1 else {1, 5, 8} if B == 2 else set())
        assert all(c.patterns[1] == "noise01" for c in twins)
    block = [c for c in gc.CHAIN if c.note == "block"]
    assert [(c.launch, c.opt, gc.chain_block(1, 64, 1, c.launch)) for c in block] == [(5, 0, 192), (16, 0, 512), (18, 0, 576), (5, 1, 192)]
    assert [gc.chain_launches_of(c)[0][2] for c in block] == ["u8-512", "u8-512", "u8-1024", "u8-512-sse2"]
    for c in gc.CHAIN:  # chained_frames: every frame of a launch but a run of one
        if c.note != "refused":
            assert gc.chained_frames(c) == 2 * (c.launch - (1 if c.order == 0 else 0)), gc.case_id(c)


# ---- every case tests something: the reference alone -----------------------------------------------------------------------------------
def _tail(c):
    """The columns only the next frame sees, as far as a case's frames can fill them: the last 8 of the stride -- or, where the
    plane ends more than 8 columns before its stride (the odd widths of STRIDED), the three next to it, which stage 2 fills from
    the plane's last columns with the first frame; the box reaches no further in one frame."""
    s = gc.stride_of(c)
    return slice(s - 8, s) if s - c.w <= 8 else slice(c.w, c.w + 3)


def _reference_run(c, edges_tail=None):
    """Runs the reference alone over the case's frames and asserts what the issue asks of every case."""
    ref, prev, b = gc.reference_of(c), None, gc.bh(c.h)
    for launch in gc.frames_of(c):
        for i, src in enumerate(launch):
            out, pool = gc.reference_frame(ref, c, src, c.parities[i] if c.launch else 1)
            assert pool.shape == (9, b + 1, gc.stride_of(c))
            assert prev is None or not same(prev, pool), f"{gc.case_id(c)}: the pool does not change with frame {i}"
            assert pool[:, 1:b, _tail(c)].any(), f"{gc.case_id(c)}: nothing in the last columns of the stride, frame {i}"
            assert all(pool[:, r, :].any() for r in range(1, b)), f"{gc.case_id(c)}: an empty pool row, frame {i}"
            prev = pool
            if edges_tail is not None and c.patterns[i] == "edges" and c.order == 1:
                rows = c.h // 2 - 1  # interpolated lines 1, 3, ...: the plain mean of their neighbours, or another arm
                wt = np.float32 if out.dtype == np.float32 else np.int64
                a, n = out[0:2 * rows:2, -8:].astype(wt), out[2:2 * rows + 2:2, -8:].astype(wt)
                mean = (a + n) * np.float32(0.5) if wt is np.float32 else (a + n + 1) >> 1
                edges_tail.append(int((out[1:2 * rows:2, -8:].astype(wt) != mean).sum()))
    if c.opt:
        assert ref.events["box_above"] > 0, f"{gc.case_id(c)}: the box never saturates"


@pytest.mark.parametrize("table", list(gc.PLANE_TABLES) + ["CHAIN"])
def test_every_case_tests_something(table):
    for c in gc.PLANE_TABLES.get(table, gc.CHAIN):
        _reference_run(c)


def test_edges_frames_leave_the_plain_mean_arm_at_the_right_edge():
    """In the last 8 columns of at least one case per schedule (and of a chain) the `edges` frame takes an arm of the ladder other
    than the plain mean, so those columns' costs decide pixels."""
    found = {}
    for c in gc.every_case():
        key = "chain" if c.table == "CHAIN" else gc.stage2_of(c)[0]
        if key in found or "edges" not in c.patterns or c.order != 1 or c.launches * len(c.patterns) > 40:
            continue
        tail = []
        _reference_run(c, tail)
        if sum(tail) > 0:
            found[key] = (gc.case_id(c), sum(tail))
    assert set(found) == {"strided", "x8", "strips", "chain"}, found
