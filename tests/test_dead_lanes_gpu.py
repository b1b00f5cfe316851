"""The 8-bit sweeps' right-hand clamp at every place the last column can take in the last strip, bit-exact against the
CPU oracle.

The box reads the right neighbour of column w-1 like every other right-hand tap and adds the clamp on top, so it relies on
S being zero in every half that is not live (sn_fused_u8_parts.h, box7): the lines, the previous pass's rows and the
keys of such a half must all come out zero.  Every fused width is a multiple of 32, so column w-1 is the last pixel of a
lane that is 3 mod 4 in its strip; the widths below walk it through every such lane of the first strip (32 .. 512) and of
the second one (544 .. 992, where the first strip's right ghosts lie inside the plane).  8-bit 4:2:0 adds the coupled
luma sweep, the two chroma sweeps of the pool coupling and the one-sweep chroma kernel.  Flat and near-flat inputs give
keys below 0x400 and many ties, which the ladder decides by rank.
"""
import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2, clip_format, synth
from oracle.oracle import Oracle
from tests.util import describe_diff, oracle_cfg, same

pytestmark = pytest.mark.gpu

WIDTHS = tuple(range(32, 513, 32)) + tuple(range(544, 993, 32))
PATTERNS = ("noise", "flat", "near-flat")


def _frames(clip, pattern, n, seed0):
    frames = []
    for i in range(n):
        planes = synth.frame(clip, "noise", seed=seed0 + i)
        if pattern == "flat":
            planes = [np.full_like(p, 117 + 3 * i) for p in planes]
        elif pattern == "near-flat":  # costs of 0 .. 2: keys far below 0x400
            planes = [(96 + p % 3).astype(p.dtype) for p in planes]
        frames.append(planes)
    return frames


def _check(fmt, w, h, kw, pattern, nframes=2, bands=None, **policy):
    clip = clip_format(fmt, w, h)
    ora = Oracle(oracle_cfg(clip, **kw))
    with SangNom2(clip, mode="fused" if bands is None else "auto", **policy, **kw) as flt:
        if bands is not None:
            flt.set_bands(*bands)
        for f, src in enumerate(_frames(clip, pattern, nframes, seed0=71)):
            want = ora.process(src, parity=f & 1)
            got = flt.get_frame(src, parity=f & 1)
            for p in range(len(want)):
                assert same(want[p], got[p]), f"{fmt} {w}x{h} {kw} {pattern} frame {f} plane {p}: " + describe_diff(want[p], got[p])
        info = flt.info()
        if bands is None:
            assert info.fused_frames == nframes
        else:  # (the bands' check may send flat material to the pool kernels; noise passes it)
            assert info.banded_frames == nframes and (info.band_fallbacks == 0 or pattern != "noise")
    return info


@pytest.mark.parametrize("w", WIDTHS)
def test_y8_last_column_matches_oracle(hip_lib, w):
    for pattern in PATTERNS:
        _check("Y8", w, 24, dict(order=1, aa=48), pattern)


@pytest.mark.parametrize("w", WIDTHS)
def test_yuv420p8_last_column_matches_oracle(hip_lib, w):
    """Default policy: the one-sweep chroma kernel where the geometry allows it; chroma_sweeps = 1: the luma sweep hands
    off through its pool and U and V run as sweeps of their own."""
    for pattern in PATTERNS:
        _check("YUV420P8", w, 40, dict(order=1, aa=48, aac=48), pattern)
        info = _check("YUV420P8", w, 40, dict(order=1, aa=48, aac=48), pattern, chroma_sweeps=1)
        assert info.uv_sweeps == 0


@pytest.mark.parametrize("w", (96, 480, 992))
@pytest.mark.parametrize("pattern", PATTERNS)
def test_y8_band_last_column_matches_oracle(hip_lib, w, pattern):
    _check("Y8", w, 200, dict(order=1, aa=48), pattern, bands=(6, 0))
