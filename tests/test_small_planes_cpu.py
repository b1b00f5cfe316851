"""The table of tests/small_plane_cases.py, checked without a GPU: every dispatch rule it is derived from has a case on each
side, the restated rules are the library's (held against the answers of the headers on a host compiler), the two CPU
references agree bit for bit on every clip of the table, and the inputs can tell interpolation from line
doubling.
"""
import os
import subprocess

import numpy as np
import pytest

from avisynth_sangnom2_amd import clip_format
from oracle.oracle import Oracle
from oracle.sangnom_numpy import NumpySangNom
from tests import small_plane_cases as sp
from tests.util import oracle_cfg, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avisynth_sangnom2_amd", "csrc")
BYTES = {"Y8": 1, "Y12": 2, "Y16": 2, "Y32": 4}


def _compile(tmp_path, source, name):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, source, "-o", exe])
    return exe


# ---- 1. both sides of every rule ---------------------------------------------------------------------------------------------------

def _luma_and_chroma(fmt, w, h, dh=False):
    planes = sp.planes_of(clip_format(fmt, w, h), dict(dh=dh))
    return planes[0], planes[1]


def test_column_parts_cases_stand_on_both_sides_of_the_row_rule():
    """plan_parts: nr >= 1.  Every plane of the table that creation marks for parts, by the side it lands on."""
    sides = {}
    for fmt, w, h, kw, ckw in sp.PARTS:
        clip = clip_format(fmt, w, h)
        for p, (pw, ho, on) in enumerate(sp.planes_of(clip, kw)):
            if on and sp.parts_marked(clip.bytes, pw) and (ckw.get("isolated_planes") or pw == clip.width):
                sides.setdefault(sp.nr(ho) >= 1, []).append((fmt, w, h, p))
    assert set(sides) == {True, False}
    assert ("Y32", 6144, 2, 0) in sides[False] and ("Y16", 3872, 2, 0) in sides[False] and ("Y32", 8192, 2, 0) in sides[False]
    # the same widths with one and two rows, dh on the two-line clip, and the isolated 4:2:0 clips on both sides at once
    for fmt, w in sp.PARTS_WIDE:
        assert (fmt, w, 4, 0) in sides[True] and (fmt, w, 6, 0) in sides[True]
    assert ("Y16", 3872, 2, 0) in sides[True]  # (dh=True: h_out = 4)
    for fmt in ("YUV420P16", "YUV420PS"):
        assert (fmt, 8192, 4, 0) in sides[True] and (fmt, 8192, 4, 1) in sides[False] and (fmt, 8192, 4, 2) in sides[False]
    assert {p for f, w, h, p in sides[False] if f == "YUV444P16"} == {0, 1, 2}
    for fmt, w, h, parts in sp.PARTS_FORCED:  # forced parts: not marked, one row, wide enough for that many parts
        assert not sp.parts_marked(clip_format(fmt, w, h).bytes, w) and sp.nr(h) == 1 and w // parts >= 32
    assert sp.nr(2 * sp.AA_PARTS[2]) == 1 and sp.parts_marked(2, 2 * sp.AA_PARTS[1])  # the enlargement's second pass: near side


def test_coupled_cases_take_both_arms_of_the_reach():
    """reach = min(nr_c + 2, bh - 1), and a chroma plane with no row, one row, two rows."""
    got = set()
    for fmt, w, h in sp.COUPLED:
        (_, ho, _), (_, ho_c, _) = _luma_and_chroma(fmt, w, h)
        nr_c, b = sp.nr(ho_c), sp.bh(ho)
        got.add((fmt[:6], nr_c, sp.reach(nr_c, b), "rows" if nr_c + 2 < b - 1 else "pool" if nr_c + 2 > b - 1 else "equal"))
        assert not sp.uv_rows_ok(nr_c, b)  # none of them short of the one-sweep form by anything but its rows
    assert {g[1:] for g in got if g[0] == "YUV420"} == {(0, 1, "pool"), (1, 3, "equal"), (2, 4, "rows")}
    assert {g[1:] for g in got if g[0] == "YUV422"} == {(0, 0, "pool"), (1, 1, "pool")}
    for fmt, w, h in sp.HANDOFF:
        assert (fmt, w, h) in sp.COUPLED
    assert {clip_format(f, 32, 8).bytes for f, _, _ in sp.HANDOFF} == {1, 2, 4}
    assert {sp.reach(sp.nr(h // 2), sp.bh(h)) for _, _, h in sp.HANDOFF} == {1, 3, 4}


def test_one_sweep_cases_stand_on_both_sides_of_the_row_rule():
    """fused_uv_ok: nr_c >= 2 kSkew + 2, per format and with dh."""
    sides = {}
    for fmt, w, h, dh in sp.UV:
        (_, ho, _), (_, ho_c, _) = _luma_and_chroma(fmt, w, h, dh)
        nr_c = sp.nr(ho_c)
        # the two row counts next to the rule; with dh the nearest height the reference accepts on the near side gives one more
        assert nr_c in ((2 * sp.K_SKEW + 1, 2 * sp.K_SKEW + 3) if dh else (2 * sp.K_SKEW + 1, 2 * sp.K_SKEW + 2))
        sides.setdefault((fmt, dh), set()).add(sp.uv_rows_ok(nr_c, sp.bh(ho)))
    assert len(sides) == 4 and all(s == {True, False} for s in sides.values())
    assert {w for _, w, _, _ in sp.UV} == {256, 3840}


def test_band_cases_stand_on_both_sides_of_the_band_count():
    """nb <= nr / kMinBandRows."""
    for t in sp.TYPES:
        counts = {h: sp.band_count(sp.nr(h), forced) for tt, w, h, forced in sp.BANDS if tt == t}
        assert counts == {32: 0, 34: 2, 50: 3, 52: 3}
        assert sp.nr(32) == 2 * sp.MIN_BAND_ROWS - 1 and sp.nr(34) == 2 * sp.MIN_BAND_ROWS and sp.nr(50) == 3 * sp.MIN_BAND_ROWS
        # the comment on the run-up: every default run-up reaches above row 1 from the last band's first row
        for h, nb in counts.items():
            if nb:
                rows = -(-sp.nr(h) // nb)
                assert 1 + (nb - 1) * rows - sp.BAND_WARM[BYTES[t]] <= 1


def test_pool_cases_stand_on_both_sides_of_the_one_row_pool():
    """bh < 2: no stage 2.  Every schedule of sn_pool_dispatch.h at bh = 2, per sample type."""
    for t in sp.TYPES:
        B = BYTES[t]
        got = {(w, h): sp.pool_schedule(B, sp.pool_stride(w), sp.bh(h), 1) for tt, w, h in sp.POOL if tt == t}
        assert {s for (w, h), s in got.items() if h == 2} == {"none"}
        assert {w: s for (w, h), s in got.items() if h == 4} == {256: "x8", 512: "strips", 544: "strips", 7680: "strips", 8192: "x8",
                                                                  100: "strided", 520: "strips"}
    assert {sp.bh(h) for _, _, h in sp.POOL} == {1, 2}
    assert {sp.bh(h) for _, _, h in sp.POOL_CONTENTS} == {1, 2} and {t for t, _, _ in sp.POOL_CONTENTS} == set(sp.TYPES)


def test_chain_cases_stand_on_both_sides_of_both_conditions():
    """chain_planes: bh >= 2, and nr >= 1 for every processed plane."""
    got = {(fmt, w, h): sp.chain_ok(clip_format(fmt, w, h), kw) for fmt, w, h, kw in sp.CHAINS}
    for t in ("Y8", "Y12", "Y32"):
        for w in (40, 1000):
            assert [got[(t, w, h)] for h in (2, 4, 6)] == [False, True, True]
    assert sp.bh(2) == 1 and sp.bh(4) == 2  # bh >= 2 on both sides
    # bh = 2 and luma with a row, chroma with none: the rows alone decide
    assert got[("YUV420P8", 720, 4)] is False and sp.bh(4) >= 2 and sp.nr(4) == 1 and sp.nr(2) == 0
    assert got[("YUV420P8", 720, 8)] is True


def test_narrow_and_surface_tables_hold_what_they_promise():
    assert {w for _, w, _ in sp.NARROW} == {1, 2, 7, 8, 9, 24, 31} and {h for _, _, h in sp.NARROW} == {2, 4, 16}
    assert all(w < 32 for _, w, _ in sp.NARROW) and len(sp.NARROW) == 63
    padded = {w for w in sp.NARROW_WIDTHS if w % 8 == 0 and w % 32 != 0}
    assert padded == {8, 24}
    sides = {(fmt, w, h, s if s != "planar" else d) for fmt, w, h, s, d in sp.SURFACES}
    assert {(f, w, h) for f, w, h, s in sides if s == "semi"} == {(f, w, 4) for f in ("YUV420P8", "YUV420P16") for w in (2, 6, 34)} | {("YUV422P8", 2, 2)}
    assert {(w, h) for f, w, h, s in sides if s == "v210"} == {(2, 2), (6, 2), (50, 2)}
    assert {(w, h, s) for f, w, h, s in sides if s in ("yuyv", "uyvy")} == {(w, 2, s) for w in (2, 66) for s in ("yuyv", "uyvy")}
    assert ("YUV420P10", 34, 4, "semi_msb") in sides and ("YUV422P10", 34, 2, "yuyv_msb") in sides
    for fmt, w, h, s, d in sp.SURFACES:  # every layout with itself and with a planar other side, both directions
        other = s if s != "planar" else d
        assert {(a, b) for f, ww, hh, a, b in sp.SURFACES if (f, ww, hh) == (fmt, w, h) and other in (a, b)} == \
            {(other, other), (other, "planar"), ("planar", other)}
    assert max(w * h for c, kw in sp.every_clip() for w, h in [(c.width, c.height)] if c.height <= 6) == 8192 * 6


# ---- 2. the restated rules are the library's ----------------------------------------------------------------------------------------

def test_restated_widths_agree_with_build_sweep(tmp_path):
    """csrc/sn_sweep_args.h on a host compiler: the widest planes of the table are eight waves, the planes marked for column
    parts have NO whole-plane instance -- which is why a marked plane without a plan must not reach one."""
    exe = _compile(tmp_path, os.path.join(ROOT, "tests", "c", "sweep_args_check.cpp"), "sweep_args_check")
    for B in (1, 2, 4):
        widths = sorted({w for t, w, h, kw in sp.WIDE if BYTES[t] == B} | {w for t, w, h in sp.POOL + sp.WIDE_SSE2 if BYTES[t] == B and w % 32 == 0} |
                        {sp.MAX_SWEEP_WIDTH[B] + 32} | ({3872, 4096, 6144, 8192} if B != 1 else set()))
        r = subprocess.run([exe, str(B)] + [str(w) for w in widths], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(widths)
        for w, line in zip(widths, lines):
            if sp.sweep_plane_ok(B, w):
                strips = sp.strips_for(w // 8)
                assert line == f"{strips} {(strips + 1) // 2 if B == 1 else strips}", (B, w, line)
            else:
                assert line == "refused", (B, w, line)
                assert B == 1 or sp.parts_marked(B, w)
        assert lines[widths.index(sp.MAX_SWEEP_WIDTH[B])].split()[1] == "8"


POOL_QUERY = r"""
#include <stdio.h>
#include <stdlib.h>
#include "sn_pool_dispatch.h"
int main(int argc, char** argv)
{
    static const char* const names[] = {"none", "strided", "x8", "strips", "refused"};
    for (int i = 1; i + 3 < argc; i += 4)
        printf("%s\n", names[(int)sn::pool_stage2_for(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3])).schedule]);
    return 0;
}
"""


def test_restated_pool_schedule_agrees_with_the_dispatch_header(tmp_path):
    """csrc/sn_pool_dispatch.h on a host compiler: its own check (boundaries written out by hand) passes, and the restated rule
    names the schedule the header picks for every pool of the table, at one frame and at ten."""
    own = _compile(tmp_path, os.path.join(ROOT, "tests", "c", "pool_dispatch_check.cpp"), "pool_dispatch_check")
    r = subprocess.run([own], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout[-2000:], r.stderr[-2000:])
    src = tmp_path / "pool_query.cpp"
    src.write_text(POOL_QUERY)
    exe = _compile(tmp_path, str(src), "pool_query")
    queries = [(BYTES[t], sp.pool_stride(w), sp.bh(h), n) for t, w, h in sp.POOL + sp.NARROW for n in (1, 10)]
    queries += [(BYTES[t], sp.pool_stride(w), sp.bh(h), sp.CHAIN_FRAMES) for t, w, h, kw in sp.CHAINS if t in BYTES]
    r = subprocess.run([exe] + [str(v) for q in queries for v in q], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(queries)
    for q, line in zip(queries, lines):
        assert line == sp.pool_schedule(*q), (q, line)
    assert set(lines) == {"none", "strided", "x8", "strips"}


MODES = {"auto": 0, "pool": 1, "fused": 2}  # SN_MODE_*


def _route_query(fmt, w, h, kw=None, ckw=None, mode="auto", column_parts=0, **launch):
    """One query of tests/c/route_check.cpp: the clip as SangNom2(clip, mode=..., column_parts=..., **kw, **ckw) describes it, and
    a launch of n frames on slot 0 of a context with room for it (four pool slots, a seam record of four slots, the chain
    kernels where sn_pool_kernels.hip has them: pools of 64 columns and more)."""
    kw, ckw, clip = kw or {}, ckw or {}, clip_format(fmt, w, h)
    la = dict(n=1, slot0=0, slots=4, parts_slots=4, seam_record=1, sweeps_always=0, band_force=0, band_warm=0, parts_force=0, ghost_force=0,
              chroma_sweeps=0, chain_lanes=2 if sp.pool_stride(w) >= 64 else 0, bands_paused=0, parts_paused=0)
    assert set(launch) <= set(la), launch
    la.update(launch)
    return [clip.bytes, clip.bits, clip.planes, clip.subw, clip.subh, w, h, int(bool(kw.get("dh"))), int(kw.get("luma", True)), int(kw.get("chroma", True)),
            MODES[mode], int(bool(ckw.get("isolated_planes"))), int(bool(ckw.get("fresh_pool"))), 0, column_parts, 0] + list(la.values())


def _route_answers(exe, queries):
    r = subprocess.run([exe] + [str(v) for q in queries for v in q], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(queries)
    out = []
    for line in lines:
        head, _, text = line.partition(" text=")
        a = {}
        for k, v in (t.split("=") for t in head.split()):
            if k == "route":
                a[k] = v
            elif "," in v:  # a list; of a parts plan, the windows as [first column, seam]
                a[k] = [[int(x) for x in f.split(":")] if ":" in f else int(f) for f in v.split(",")]
            else:
                a[k] = int(v)
        a["text"] = text
        out.append(a)
    return out


PLANE = ("w", "h_out", "on", "fused", "padded", "parts", "sweep_ok", "pool_stride", "pool_bh")


def _plane(a, p):
    return dict(zip(PLANE, a[f"plane{p}"]))


def test_restated_rules_agree_with_the_route_header(tmp_path):
    """csrc/sn_route.h on a host compiler: every case of the tables is put to tests/c/route_check.cpp as the device test creates
    and launches it, and every rule restated in small_plane_cases.py is held against the header's answer -- on both sides of its
    boundary, which the tests of part 1 show the tables to stand on."""
    exe = _compile(tmp_path, os.path.join(ROOT, "tests", "c", "route_check.cpp"), "route_check")
    Q, checks = [], []

    def ask(check, *a, **k):
        Q.append(_route_query(*a, **k))
        checks.append(check)

    seen = {k: set() for k in ("nr", "bh", "reach", "uv", "bands", "warm", "sweep_ok", "marked", "chain", "ghost", "width")}

    def common(a, fmt, w, h, kw):
        """bh, nr-independent geometry and sweep_plane_ok / parts_marked's width half of every plane"""
        clip, planes = clip_format(fmt, w, h), sp.planes_of(clip_format(fmt, w, h), kw)
        assert a["refusal"] == 0 and a["bh"] == sp.bh(planes[0][1]) and a["stride_e"] == sp.pool_stride(w), (fmt, w, h, a)
        seen["bh"].add(a["bh"] >= 2)
        for p, (pw, ho, on) in enumerate(planes):
            pl = _plane(a, p)
            assert (pl["w"], pl["h_out"], pl["on"]) == (pw, ho, int(on)) and pl["sweep_ok"] == int(sp.sweep_plane_ok(clip.bytes, pw)), (fmt, w, h, p, pl)
            seen["sweep_ok"].add(bool(pl["sweep_ok"]))
        return clip, planes

    def ghosts(a, p, B, ghost):
        n, _, win_w, *parts = a[f"parts{p}"]
        assert len(parts) == n >= 2
        for k in range(1, n):  # the seam lies that far inside the window left of it and the window right of it
            (x_l, _), (x_r, seam) = parts[k - 1], parts[k]
            assert x_l + win_w - seam >= ghost and seam - x_r >= ghost, (p, k, parts, win_w)
            seen["ghost"].add(min(x_l + win_w - seam, seam - x_r) == ghost)

    def parts_case(fmt, w, h, kw, ckw):
        def check(a):
            clip, planes = common(a, fmt, w, h, kw)
            iso = bool(ckw.get("isolated_planes"))
            assert a["isolated"] == int(iso and clip.planes > 1) and a["parts_eligible"] == 1 and a["route"] == "planes" and a["nbands"] == 0
            for p, (pw, ho, on) in enumerate(planes):
                marked = on and sp.parts_marked(clip.bytes, pw) and (iso or pw == clip.width)
                cut = marked and sp.nr(ho) >= 1
                assert _plane(a, p)["parts"] == int(marked), (fmt, w, h, p)
                assert (a[f"parts{p}"][0] >= 2, a[f"parts{p}"][1] >= 2) == (cut, cut), (fmt, w, h, p, a[f"parts{p}"])
                assert a["fused"][p] == int(on and (cut or sp.sweep_plane_ok(clip.bytes, pw))), (fmt, w, h, p)
                if on:
                    seen["marked"].add(bool(marked))
                if marked:
                    seen["nr"].add(sp.nr(ho) >= 1)
                if cut:
                    ghosts(a, p, clip.bytes, sp.PARTS_GHOST[clip.bytes])
            assert a["parts_cut"] == int(any(a[f"parts{p}"][0] for p in range(clip.planes)))
        return check

    for fmt, w, h, kw, ckw in sp.PARTS:
        ask(parts_case(fmt, w, h, kw, ckw), fmt, w, h, kw, ckw, mode="fused", column_parts=1, n=3)

    def forced_case(fmt, w, h, parts):
        def check(a):
            clip, _ = common(a, fmt, w, h, {})
            assert _plane(a, 0)["parts"] == 0 and a["parts0"][:2] == [parts, parts] and a["fused"][0] == 1 and a["route"] == "planes", a
            ghosts(a, 0, clip.bytes, sp.PARTS_GHOST[clip.bytes])
            seen["marked"].add(bool(_plane(a, 0)["parts"]))  # the far side of parts_marked: a plane the whole-plane sweep takes
        return check

    for fmt, w, h, parts in sp.PARTS_FORCED:
        ask(forced_case(fmt, w, h, parts), fmt, w, h, mode="fused", column_parts=1, n=3, parts_force=parts)
        ask(lambda a: a["parts0"][:2] == [0, 0] or pytest.fail(str(a)), fmt, w, h, mode="fused", column_parts=1, n=3)

    def wide_case(fmt, w, h, kw):
        def check(a):
            clip, planes = common(a, fmt, w, h, kw)
            assert _plane(a, 0)["sweep_ok"] == 1 and a["use_fused"] == 1 and a["fused"][0] == 1 and (a["route"], a["nbands"]) == ("planes", 0), a
            assert a["stop"][0] == planes[0][1] // 2
        return check

    for fmt, w, h, kw in sp.WIDE:
        ask(wide_case(fmt, w, h, kw), fmt, w, h, kw, mode="fused", n=3)
    for B, fmt in sp.Y.items():  # the other side: one column strip more
        ask(lambda a, B=B: (_plane(a, 0)["sweep_ok"], a["use_fused"], _plane(a, 0)["parts"]) == (0, 0, 0) or pytest.fail(str(a)),
            fmt, sp.MAX_SWEEP_WIDTH[B] + 32, 4)

    def coupled_case(fmt, w, h, dh, table):
        def check(a):
            kw = dict(aac=48, dh=True) if dh else dict(aac=48)
            clip, planes = common(a, fmt, w, h, kw)
            nr_c, b = sp.nr(planes[1][1]), sp.bh(planes[0][1])
            assert a["fused420"] == 1 and a["fpool_rows"] == sp.reach(nr_c, b) + 1 and a["reach"] == sp.reach(nr_c, b), (fmt, w, h, a)
            assert a["route"] == "coupled" and a["fused"] == [1, 1, 1] and a["nbands"] == 0
            assert a["uv_geometry"] == int(clip.bytes == 1 and sp.uv_rows_ok(nr_c, b)), (fmt, w, h, dh, a)
            if table == "coupled":
                seen["reach"].add("rows" if nr_c + 2 < b - 1 else "pool" if nr_c + 2 > b - 1 else "equal")
            else:
                seen["uv"].add(bool(a["uv_geometry"]))
        return check

    for fmt, w, h in sp.COUPLED:
        ask(coupled_case(fmt, w, h, False, "coupled"), fmt, w, h, dict(aac=48), mode="fused", n=3)
    for fmt, w, h, dh in sp.UV:
        for cs in (0, 1):
            ask(coupled_case(fmt, w, h, dh, "uv"), fmt, w, h, dict(aac=48, dh=True) if dh else dict(aac=48), mode="fused", chroma_sweeps=cs)

    def bands_case(fmt, w, h, forced, warm):
        def check(a):
            clip, _ = common(a, fmt, w, h, {})
            nb = sp.band_count(sp.nr(h), forced)
            assert a["nbands"] == nb and a["route"] == ("banded_planes" if nb else "planes") and a["band_rows"] == (sp.nr(h) if nb else 0), (fmt, h, a)
            assert a["warm"] == (warm or sp.BAND_WARM[clip.bytes])
            seen["bands"].add(nb)
            seen["warm"].add(warm)
        return check

    for fmt, w, h, forced in sp.BANDS:
        for warm in sp.BAND_WARMS:
            ask(bands_case(fmt, w, h, forced, warm), fmt, w, h, band_force=forced, band_warm=warm)

    def chain_case(fmt, w, h, kw):
        def check(a):
            clip, planes = common(a, fmt, w, h, kw)
            ok = sp.chain_ok(clip, kw)
            assert a["history_free"] == 0 and (a["chain"] > 0) == ok and (not ok or a["chain"] == sum(on for _, _, on in planes)), (fmt, w, h, a)
            assert a["use_fused"] == 0 and a["fused"] == [0, 0, 0] and a["stop"] == [0, 0, 0]
            seen["chain"].add(ok)
        return check

    for fmt, w, h, kw in sp.CHAINS:
        ask(chain_case(fmt, w, h, kw), fmt, w, h, kw, n=sp.CHAIN_FRAMES)

    def pool_case(fmt, w, h):
        def check(a):
            common(a, fmt, w, h, {})
            assert a["history_free"] == int(w % 32 == 0) and a["use_fused"] == 0 and a["fused"] == [0, 0, 0] and a["route"] == "planes"
            assert a["stop"] == [0, 0, 0] and a["nbands"] == 0 and a["prefer_pool"] == 0  # the full emulation, pool contents included
        return check

    for fmt, w, h in sp.POOL:
        ask(pool_case(fmt, w, h), fmt, w, h, mode="pool")

    def narrow_case(fmt, w, h, fresh):
        def check(a):
            common(a, fmt, w, h, {})
            padded = fresh and w % 8 == 0
            pl = _plane(a, 0)
            assert (a["history_free"], a["fresh"], a["isolated"], a["use_fused"]) == (int(fresh), int(fresh), int(fresh), int(padded)), (fmt, w, h, fresh, a)
            assert (pl["padded"], pl["fused"], a["fused"][0]) == (int(padded), int(padded), int(padded)) and a["route"] == "planes" and a["nbands"] == 0
            assert a["stride_e"] == 32 and (not fresh or (pl["pool_stride"], pl["pool_bh"]) == (32, sp.bh(h)))
        return check

    for fmt, w, h in sp.NARROW:
        for fresh in (False, True):
            ask(narrow_case(fmt, w, h, fresh), fmt, w, h, {}, dict(fresh_pool=True) if fresh else {}, sweeps_always=1)

    def narrow_clip_case(fmt, w, h):
        def check(a):
            common(a, fmt, w, h, dict(aac=48))
            assert a["use_fused"] == 0 and a["fused"] == [0, 0, 0] and a["route"] == "planes" and a["nbands"] == 0 and a["chain"] == 0, (fmt, w, h, a)
        return check

    for fmt, w, h in sp.NARROW_CLIPS:
        ask(narrow_clip_case(fmt, w, h), fmt, w, h, dict(aac=48), sweeps_always=1)

    def width_case(w):
        def check(a):
            assert (a["refusal"] == 0) == (w <= sp.MAX_WIDTH) and (w <= sp.MAX_WIDTH or a["text"] == f"width {w} exceeds the supported maximum of 8192"), a
            seen["width"].add(w <= sp.MAX_WIDTH)
        return check

    for w in (sp.MAX_WIDTH, sp.MAX_WIDTH + 32):
        ask(width_case(w), "Y8", w, 4)

    answers = _route_answers(exe, Q)
    for check, a in zip(checks, answers):
        check(a)
    assert len(Q) > 300
    # every restated rule was asked on both sides of its boundary
    for rule in ("nr", "bh", "uv", "sweep_ok", "marked", "chain", "ghost", "width"):
        assert seen[rule] == {True, False}, (rule, seen[rule])
    assert seen["reach"] == {"rows", "pool", "equal"} and seen["bands"] == {0, 2, 3} and seen["warm"] == {0, 1}


# ---- 3. the references agree --------------------------------------------------------------------------------------------------------

CLIPS = sp.every_clip()


def _clip_id(c):
    clip, kw = c
    return f"{clip.planes}x{clip.bytes}B{clip.bits}-{clip.width}x{clip.height}-s{clip.subw}{clip.subh}" + "".join(f"-{k}{int(v)}" for k, v in sorted(kw.items()))


def test_the_table_is_not_empty_and_has_no_duplicates():
    assert len(CLIPS) > 200 and len({_clip_id(c) for c in CLIPS}) == len(CLIPS)


def test_the_reference_accepts_every_clip_of_the_table():
    """Create_SangNom2's checks (even heights, 4:2:0 heights a multiple of 4, ...): a case the reference refuses is a mistake of
    the table, not a finding."""
    from oracle.oracle import validate
    for clip, kw in CLIPS:
        assert validate(oracle_cfg(clip, **kw)) == "", (_clip_id((clip, kw)), validate(oracle_cfg(clip, **kw)))


@pytest.mark.parametrize("bytes_", [1, 2, 4])
def test_the_c_oracle_and_the_numpy_model_agree_on_every_clip_of_the_table(bytes_):
    """Two frames, both parities, one instance of each reference per clip: bit for bit, the pool included.  So the reference is
    defined on every shape of the table, and none of them is left out of the GPU run."""
    done = 0
    for clip, kw in CLIPS:
        if clip.bytes != bytes_:
            continue
        ora = Oracle(oracle_cfg(clip, **kw))
        model = NumpySangNom(clip.width, clip.height, bytes=clip.bytes, bits=clip.bits, planes=clip.planes, subw=clip.subw, subh=clip.subh, **kw)
        for f, src in enumerate(sp.frames_of(clip, 2)):
            a, b = ora.process(src, parity=f & 1), model.get_frame(src, parity=f & 1)
            for p in range(clip.planes):
                assert same(a[p], np.asarray(b[p]).astype(clip.dtype)), (_clip_id((clip, kw)), f, p)
        done += 1
    assert done >= 60


# ---- 4. the inputs discriminate ------------------------------------------------------------------------------------------------------

def _doubling_differs(fmt, w, h, kw=None, ckw=None, n=3):
    """Per plane with a row to interpolate: does any frame of the case differ from plain line doubling?"""
    kw = kw or {}
    clip, frames, par, want = sp.expected(fmt, w, h, kw, ckw, n=n)
    assert kw.get("order", 1) == 1  # the even lines are kept whatever the parity
    out = {}
    for p, (pw, ho, on) in enumerate(sp.planes_of(clip, kw)):
        if on and sp.nr(ho) >= 1:
            out[p] = any(not same(want[f][p], sp.line_doubled(frames[f][p], ho, bool(kw.get("dh")))) for f in range(n))
    return out


def test_outputs_differ_from_line_doubling_wherever_a_plane_has_a_row_to_interpolate():
    """A case whose result any route would get right proves nothing.  Exempt: planes with nr = 0 -- heights 2 (and 4:2:0
    chroma at height 4) -- whose output IS the kept line twice; they are in the table for the routing, not for the arithmetic."""
    table = [(f, w, h, kw, ckw) for f, w, h, kw, ckw in sp.PARTS] + [(f, w, h, {}, {}) for f, w, h, _ in sp.PARTS_FORCED + sp.BANDS] + \
            [(f, w, h, kw, {}) for f, w, h, kw in sp.WIDE + sp.CHAINS] + [(f, w, h, dict(aac=48), {}) for f, w, h in sp.COUPLED + sp.NARROW_CLIPS] + \
            [(f, w, h, dict(aac=48, dh=True) if dh else dict(aac=48), {}) for f, w, h, dh in sp.UV] + [(f, w, h, {}, {}) for f, w, h in sp.POOL + sp.NARROW] + \
            [(f, w, h, {}, {}) for f, w, h, _, _ in sp.SURFACES]
    checked = exempt = 0
    for fmt, w, h, kw, ckw in table:
        got = _doubling_differs(fmt, w, h, kw, ckw)
        if not got:
            assert sp.nr(2 * h if kw.get("dh") else h) == 0, (fmt, w, h)
            exempt += 1
            continue
        assert all(got.values()), (fmt, w, h, kw, got)
        checked += 1
    assert checked + exempt == len(table) and checked > 150 and exempt > 50
