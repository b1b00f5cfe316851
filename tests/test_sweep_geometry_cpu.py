"""The table of tests/sweep_geometry_cases.py, checked without a GPU: its strips_for is the header's, its widths reach every
wave count and every right-edge lane they are meant to reach, and its inputs can tell a wrong right-hand clamp from a right one.
"""
import os
import subprocess

import numpy as np
import pytest

from avisynth_sangnom2_amd import clip_format, synth
from oracle.oracle import Oracle
from tests import sweep_geometry_cases as gc
from tests.util import oracle_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ("Y8", "Y16", "Y32")


def test_strip_bounds_are_the_ones_worked_out_by_hand():
    b16 = {1: (32, 512), 2: (544, 960), 3: (992, 1440), 4: (1472, 1920), 5: (1952, 2400), 6: (2432, 2880), 7: (2912, 3360), 8: (3392, 3840)}
    b8 = dict(b16)
    b8.update({9: (3872, 4320), 10: (4352, 4800), 11: (4832, 5280), 12: (5312, 5760), 13: (5792, 6240), 14: (6272, 6720),
               15: (6752, 7200), 16: (7232, 7680)})
    assert gc.STRIP_BOUNDS == {"Y8": b8, "Y16": b16, "Y32": b16}
    assert [len(gc.WAVE_WIDTHS[t]) for t in TYPES] == [32, 16, 16]
    assert gc.EDGE_WIDTHS == tuple(range(32, 993, 32))
    assert gc.HEIGHTS == (2, 4, 6, 8, 10, 12, 14)
    assert [len(gc.PADDED[t]) for t in TYPES] == [22, 16, 16]


def test_restated_strips_for_agrees_with_the_header(tmp_path):
    """build_sweep (csrc/sn_sweep_args.h) on a host compiler gives the strips and waves the table expects: for every width of the
    table, every multiple of 32 the type's sweeps take, the first width they refuse, and every padded pair."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "sweep_args_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "avisynth_sangnom2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "sweep_args_check.cpp"), "-o", exe])
    for t in TYPES:
        B, top = gc.BYTES[t], gc.MAX_WIDTH[t]
        table = set(gc.WAVE_WIDTHS[t]) | set(gc.SEAM_WIDTHS[t]) | {c[1] for c in gc.GROUPS if c[0] == t}
        if B != 1:
            table |= set(gc.EDGE_WIDTHS) | {c[1] for c in gc.COUPLED16 if clip_format(c[0], 32, 8).bytes == B}
        else:
            table |= {c[1] for c in gc.COUPLED8 + gc.UV_ONE_SWEEP}
        plain = sorted(table | set(range(32, top + 1, 32)))
        padded = list(gc.PADDED[t]) + [(w, gc.pool_stride(w)) for c in gc.GROUPS_PADDED if c[0] == t for w in (c[1],)]
        args = [str(w) for w in plain] + [f"{w}:{s}" for w, s in padded] + [str(top + 32)]
        r = subprocess.run([exe, str(B)] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(args)
        for w, line in zip(plain, lines):
            assert line == f"{gc.strips_for(w // 8)} {gc.waves(B, w)}", (t, w, line)
        for (w, s), line in zip(padded, lines[len(plain):]):
            assert s == gc.pool_stride(w) and w % 8 == 0 and w % 32 != 0, (w, s)
            assert line == f"{gc.strips_for(s // 8)} {gc.waves(B, s)}", (t, w, s, line)
        assert lines[-1] == "refused" and gc.waves(B, top + 32) == 9
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)  # without arguments: the checks it always had
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-3000:], r.stderr[-2000:])


def _lines_end_before_the_last_strip(w, stride):
    return gc.last_lane(w)[0] < gc.last_lane(stride)[0]


@pytest.mark.parametrize("t", TYPES)
def test_the_table_reaches_every_instance(t):
    B = gc.BYTES[t]
    every = set(range(1, 9))
    strips = set(range(1, 17 if B == 1 else 9))
    # planes on their own: both ends of every strip count, so every wave count -- 8-bit: with a dead high half and without
    assert {gc.strips_for(w // 8) for w in gc.NARROWEST[t]} == strips and {gc.strips_for(w // 8) for w in gc.WIDEST[t]} == strips
    assert sorted(gc.WAVE_WIDTHS[t]) == sorted(gc.NARROWEST[t] + gc.WIDEST[t]) and len(set(gc.WAVE_WIDTHS[t])) == 2 * len(strips)
    assert {gc.waves(B, w) for w in gc.NARROWEST[t]} == every and {gc.waves(B, w) for w in gc.WIDEST[t]} == every
    for w in gc.WAVE_WIDTHS[t]:  # an end of a strip count: 32 columns fewer or more are another one (or none)
        s = gc.strips_for(w // 8)
        assert w == 32 or w == gc.MAX_WIDTH[t] or gc.strips_for((w - 32) // 8) != s or gc.strips_for((w + 32) // 8) != s
    # padded sweeps: the strides the table has -- one strip, two, and the strides that start a strip of two lanes, in which the
    # lines end 1, 2 and 3 lanes before the sweep does; at 2 and 3 lanes short of the latter the lines end in the strip before
    # the last, which then holds nothing but padding
    strides = sorted({s for _, s in gc.PADDED[t]})
    assert strides == [64, 512, 544, 992, 1472, 3392] + ([3872, 7232] if B == 1 else [])
    assert {gc.waves(B, s) for s in strides} == ({1, 2, 4, 5, 8} if B == 1 else {1, 2, 3, 4, 8})
    for s in strides:
        short = sorted(s - w for w, s2 in gc.PADDED[t] if s2 == s)
        assert short == ([24] if s == 64 else [8, 16, 24]), (s, short)
        crossing = sorted(s - w for w, s2 in gc.PADDED[t] if s2 == s and _lines_end_before_the_last_strip(w, s))
        assert crossing == ([16, 24] if s in (992, 1472, 3392, 3872, 7232) else []), (s, crossing)
        if crossing:
            assert gc.last_lane(s) == (gc.strips_for(s // 8) - 1, 3)  # the last strip: its two ghosts and two lanes
    # the coupled sweeps: the wave counts no other file launches
    if B == 1:
        new = {gc.waves(1, w) for _, w, _ in gc.COUPLED8}
        assert new == {5, 6, 7} and all(gc.strips_for(w // 8) % 2 == 1 for _, w, _ in gc.COUPLED8)
        assert {gc.strips_for(w // 8) for _, w, _ in gc.UV_ONE_SWEEP} == {5, 6, 7}  # one strip to a wave in that kernel
    else:
        fmts = {2: ("YUV420P16", "YUV422P16"), 4: ("YUV420PS",)}[B]
        for fmt in fmts:
            new = {gc.waves(B, w) for f, w, _ in gc.COUPLED16 if f == fmt}
            assert new == {5, 6}, fmt
    assert new | gc.COUPLED_ELSEWHERE[B] == every
    # frames per workgroup: a one-wave and a two-wave plane, plain and (16-bit, float) padded
    assert sorted(gc.waves(B, c[1]) for c in gc.GROUPS if c[0] == t) == [1, 2]
    if B != 1:
        assert sorted(gc.waves(B, gc.pool_stride(c[1])) for c in gc.GROUPS_PADDED if c[0] == t) == [1, 2]
    # the seam rows: two waves (8-bit: three strips) and eight
    assert [gc.waves(B, w) for w in gc.SEAM_WIDTHS[t]] == [2, 8]


def test_edge_widths_put_the_last_column_on_every_lane_it_can_take():
    got = {gc.last_lane(w) for w in gc.EDGE_WIDTHS}
    want = {(0, lane) for lane in range(3, 64, 4)} | {(1, lane) for lane in range(7, 60, 4)} | {(2, 3)}
    assert got == want and len(gc.EDGE_WIDTHS) == len(want)
    # (a second strip begins with 65 lanes, so its lane 3 is never the last one; its lanes 62 and 63 are ghosts or dead)
    assert gc.last_lane(512) == (0, 63) and gc.last_lane(544) == (1, 7) and gc.last_lane(960) == (1, 59) and gc.last_lane(992) == (2, 3)


def _extended(planes, extra, seed):
    """The planes with `extra` columns of other noise on their right."""
    out = []
    for k, p in enumerate(planes):
        more = synth.plane(p.shape[0], extra, p.dtype.itemsize, 8 * p.dtype.itemsize, "noise", seed * 3 + k)
        out.append(np.ascontiguousarray(np.concatenate([p, more.astype(p.dtype)], axis=1)))
    return out


def _differing_at_the_right_edge(t, w, wider, h=24, nframes=2):
    """Per frame the number of samples in the plane's last eight columns on which the oracle of the w-wide plane and the oracle
    of a plane `wider` columns wide, equal to it in its first w columns, disagree."""
    narrow, wide = clip_format(t, w, h), clip_format(t, wider, h)
    out = []
    for f, src in enumerate(gc.frames(narrow, "noise", nframes)):
        a = Oracle(oracle_cfg(narrow, order=1, aa=48)).process(src, parity=f & 1)[0]
        b = Oracle(oracle_cfg(wide, order=1, aa=48)).process(_extended(src, wider - w, 900 + f), parity=f & 1)[0]
        assert a.shape == (h, w) and b.shape == (h, wider)
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        out.append(int((a[:, w - 8:] != b[:, w - 8:w]).sum()))
    return out


@pytest.mark.parametrize("t", TYPES)
def test_the_noise_frames_can_see_a_wrong_right_clamp(t):
    """A sweep that read real pixels where the reference clamps at column w - 1 -- its own dead lanes' registers, a
    neighbouring frame's plane -- would give what a wider plane gives.  On the frames the GPU tests use, that differs from the
    right answer in the last eight columns of every width: on the first frame everywhere (1 .. 21 samples; the second frame, whose
    other parity keeps other lines, shows nothing at one float width)."""
    for w in sorted(set(gc.EDGE_WIDTHS) | set(gc.WAVE_WIDTHS[t])):
        n = _differing_at_the_right_edge(t, w, w + 32)
        assert n[0] >= 1, (t, w, n)


@pytest.mark.parametrize("t", TYPES)
def test_the_noise_frames_can_see_a_padded_sweep_that_misses_the_end_of_its_lines(t):
    """The same for the padded sweeps, against a plane as wide as the pool stride the sweep covers: 8 .. 30 samples of every frame."""
    for w, stride in gc.PADDED[t]:
        n = _differing_at_the_right_edge(t, w, stride)
        assert min(n) >= 1, (t, w, stride, n)
