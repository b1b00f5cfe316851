"""The plain 8-bit sweep with stage 1 and the vertical sum as two byte SADs on vertical pixel pairs (sn_fused_u8_parts.h:
PairLine), byte for byte against the references: opt=0 against oracle.oracle.Oracle, opt=1 against tests/sse2_model.py.
No tolerances.  tests/test_sad_pairs_cpu.py has the byte order on paper.

Widths: 32 (one strip, the high half dead), 544 (both halves of one wave), 992 (two waves, the last high half dead), 3392
(four waves).  Heights: 4 (one smoothed row, first and last at once), 6, 12, 14, 24, 26 -- whole and partial five-row
blocks; 26 at the two narrow widths.  Patterns: noise; the 0/255 two-pixel checker (the largest S per half, 765: a carry
between the halves or a wrong wrap shows); lines of one value each in an irregular sequence (every row has its own cost:
a pair with its bytes in the wrong order shows); two diagonal ramps f(x + y) and f(x - y) with a non-linear f (the +k /
-k operands swapped shows).  Also four frames in one workgroup (width 32) and a 4:4:4 clip, three plain planes.
"""
import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2, clip_format, synth
from oracle.oracle import Oracle
from tests import ladder_cases as lc
from tests import sse2_model as sm
from tests.util import describe_diff, oracle_cfg, same, to_host

pytestmark = pytest.mark.gpu

PATTERNS = ("noise", "checker2", "lines", "ramp+", "ramp-")
WIDTHS = (32, 544, 992, 3392)
HEIGHTS = (4, 6, 12, 14, 24, 26)
SHAPES = tuple((w, h) for w in WIDTHS for h in HEIGHTS if h != 26 or w <= 544)
_LINE_VALUES = np.array([0, 200, 10, 255, 30, 128, 7, 250, 90, 1, 64, 254, 33, 180, 5, 220], dtype=np.int64)


def _f(t):
    return (7 * t * t + 3 * t + 11) & 255  # non-linear, so f(x + y) and f(x - y) have no cost in common


def plane(w, h, pattern, seed):
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    if pattern == "noise":
        return synth.plane(h, w, 1, 8, "noise", seed)
    if pattern == "checker2":
        return synth.plane(h, w, 1, 8, "checker2", seed)
    if pattern == "lines":
        v = _LINE_VALUES[(y * 5 + seed) % len(_LINE_VALUES)]
    elif pattern == "ramp+":
        v = _f(x + y + seed)
    elif pattern == "ramp-":
        v = _f(x - y + seed)
    else:
        raise ValueError(pattern)
    return np.ascontiguousarray(v.astype(np.uint8))


def reference(clip, kw, opt):
    if opt == 0:
        ora = Oracle(oracle_cfg(clip, **kw))
        return lambda src, parity: ora.process(src, parity=parity)
    m = sm.Sse2SangNom(clip.width, clip.height, bytes=clip.bytes, bits=clip.bits, planes=clip.planes, subw=clip.subw, subh=clip.subh,
                       order=kw.get("order", 1), aa=kw.get("aa", 48), aac=kw.get("aac", 0))
    return lambda src, parity: m.get_frame(src, parity=parity)


@pytest.mark.parametrize("opt", (0, 1))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_y8_plane_matches_reference(hip_lib, shape, opt):
    w, h = shape
    clip = clip_format("Y8", w, h)
    for aa in lc.AA:
        kw = dict(order=1, aa=aa)
        want_of = reference(clip, kw, opt)
        with SangNom2(clip, mode="fused", opt=opt, **kw) as flt:
            n = 0
            for pattern in PATTERNS:
                for parity in (0, 1):
                    src = [plane(w, h, pattern, 31 + parity)]
                    want = want_of(src, parity)
                    got = flt.get_frame(src, parity=parity)
                    assert same(want[0], got[0]), f"Y8 {w}x{h} aa={aa} opt={opt} {pattern} parity {parity}: " + describe_diff(want[0], got[0])
                    n += 1
            assert flt.info().fused_frames == n


@pytest.mark.parametrize("opt", (0, 1))
def test_four_frames_share_a_workgroup(hip_lib, opt):
    import torch
    w, h = 32, 14
    clip = clip_format("Y8", w, h)
    kw = dict(order=1, aa=48)
    want_of = reference(clip, kw, opt)
    frames = [plane(w, h, p, 41 + i) for i, p in enumerate(("noise", "checker2", "lines", "ramp-"))]
    parity = [0, 1, 1, 0]
    dev = torch.device("cuda:0")
    with SangNom2(clip, mode="fused", opt=opt, max_batch=4, **kw) as flt:
        src = [torch.from_numpy(np.stack(frames)).pin_memory().to(dev)]
        dst = [torch.zeros_like(src[0])]
        torch.cuda.synchronize()
        flt.process_batch(src, dst, parity)
        flt.synchronize()
        assert flt.info().fused_frames == 4
        got = to_host(dst[0])
    for f in range(4):
        want = want_of([frames[f]], parity[f])
        assert same(want[0], got[f]), f"frame {f} opt={opt}: " + describe_diff(want[0], got[f])


def test_yuv444p8_three_plain_planes(hip_lib):
    w, h = 544, 14
    clip = clip_format("YUV444P8", w, h)
    kw = dict(order=1, aa=48, aac=48)
    want_of = reference(clip, kw, 0)
    with SangNom2(clip, mode="fused", **kw) as flt:
        for parity in (0, 1):
            src = [plane(w, h, p, 51 + parity) for p in ("ramp+", "noise", "lines")]
            want = want_of(src, parity)
            got = flt.get_frame(src, parity=parity)
            for p in range(3):
                assert same(want[p], got[p]), f"YUV444P8 parity {parity} plane {p}: " + describe_diff(want[p], got[p])
        assert flt.info().fused_frames == 2
