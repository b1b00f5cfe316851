"""The ladder of the 9..16-bit sweep (sn_fused_u16_v3.hip) on the tie-heavy inputs of the 8-bit ladder tests, bit-exact
against the CPU oracle.

The sweep forms 20-bit keys (smoothed cost << 4) | rank and starts their minimum from the threshold key (thr + 1) << 4, with
thr = aa * 21 / 16 scaled by 1 << (bits - 8).  The inputs of tests/ladder_cases.py, scaled to the clip's depth, put every
cost at zero (flat: the rank alone decides), at 0 .. 2 (near-flat), near the top of the range (two-pixel checker of 0 and the
maximum) and on ties between the diagonal buffers (ramp, wrapping at the depth's modulus); aa = 0 makes the threshold key the
smallest there is, aa = 128 the largest.  Depths 9, 14 and 15 exercise the threshold's scale where no other test does, and
one case fills a 10-bit clip's 16-bit container: the reference wraps modulo 65536 whatever the depth.

Shapes: one wave, a second wave that is nearly empty, several waves; 4:2:0 (the coupled luma sweep and the chroma sweeps);
row bands with the default run-up and with a run-up from the top of the plane, which no pattern can fail.
"""
import pytest

from avisynth_sangnom2_amd import ClipFormat, SangNom2, clip_format
from oracle.oracle import Oracle
from tests import ladder_cases as lc
from tests.util import describe_diff, oracle_cfg, same

pytestmark = pytest.mark.gpu


def _check(clip, kw, pattern, mode="fused", bands=None):
    ora = Oracle(oracle_cfg(clip, **kw))
    with SangNom2(clip, mode="auto" if bands else mode, **kw) as flt:
        if bands:
            flt.set_bands(*bands)
        for f, src in enumerate(lc.frames(clip, pattern)):
            want = ora.process(src, parity=f & 1)
            got = flt.get_frame(src, parity=f & 1)
            for p in range(len(want)):
                assert same(want[p], got[p]), f"{clip} {kw} {pattern} {mode} bands={bands} frame {f} plane {p}: " + describe_diff(want[p], got[p])
        info = flt.info()
        if bands:
            # with the default run-up the bands' check may send flat or periodic material to the pool kernels (noise passes
            # it); with a run-up from the top of the plane every band is exact and no frame may fall back
            assert info.banded_frames == lc.NFRAMES
            assert info.band_fallbacks == 0 or (bands[1] == 0 and pattern != "noise"), (pattern, info.band_fallbacks)
        elif mode == "fused":
            assert info.fused_eligible == 1 and info.fused_frames == lc.NFRAMES and info.banded_frames == 0
        else:
            assert info.fused_frames == 0 and info.banded_frames == 0


@pytest.mark.parametrize("aa", lc.AA)
@pytest.mark.parametrize("shape", lc.Y16_SHAPES, ids=lambda s: f"{s[1]}x{s[2]}" + (f"-bands{s[3][1]}" if s[3] else ""))
def test_y16_ladder_matches_oracle(hip_lib, shape, aa):
    fmt, w, h, bands = shape
    for pattern in lc.U16_PATTERNS:
        _check(clip_format(fmt, w, h), dict(order=1, aa=aa), pattern, bands=bands)


@pytest.mark.parametrize("aa", lc.AA)
@pytest.mark.parametrize("shape", lc.YUV16_SHAPES, ids=lambda s: f"{s[1]}x{s[2]}")
def test_yuv420p16_ladder_matches_oracle(hip_lib, shape, aa):
    fmt, w, h, _ = shape
    for pattern in lc.U16_PATTERNS:
        _check(clip_format(fmt, w, h), dict(order=1, aa=aa, aac=aa), pattern)


@pytest.mark.parametrize("aa", lc.AA)
@pytest.mark.parametrize("bits", lc.ODD_DEPTHS)
def test_ladder_at_depths_between_the_usual_ones(hip_lib, bits, aa):
    """Y9, Y14, Y15: the threshold's scale 1 << (bits - 8) at every depth the usual formats skip."""
    for w, h in lc.ODD_DEPTH_SHAPES:
        clip = ClipFormat(width=w, height=h, bytes=2, bits=bits)
        for pattern in lc.U16_PATTERNS:
            _check(clip, dict(order=1, aa=aa), pattern)


@pytest.mark.parametrize("mode", ("fused", "pool"))
def test_samples_above_the_depths_maximum_wrap_like_the_reference(hip_lib, mode):
    """A 10-bit clip whose container holds 0 .. 65535: the reference narrows to uint16 whatever the depth, and so must the
    sweep (20-bit keys, 16-bit costs) and the pool kernels."""
    for w, h in lc.ODD_DEPTH_SHAPES:
        for aa in lc.AA:
            _check(clip_format("Y10", w, h), dict(order=1, aa=aa), "noise16", mode=mode)
