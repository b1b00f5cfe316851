"""The ladder's key minimum of the 8-bit sweeps, bit-exact against the CPU oracle on inputs that live where a float minimum
of integer keys could go wrong.

The sweeps fold the keys (smoothed cost << 4) | rank two at a time with v_pk_minimum3_f16 (sn_fused_v3_common.h,
pk_min3_keys).  That is the integer minimum only if the hardware hands denormal patterns on untouched (keys below 0x0400:
flat and near-flat inputs never leave that range, and there the rank nibble alone decides) and orders the patterns up to
0x0ff0 (the two-pixel checker) like integers.  The threshold key, which starts the minimum, is 0x0010, 0x0400 or 0x0a90:
a denormal pattern, the smallest normal, the top of the range.  test_ladder_min3_cpu.py shows that these inputs reach every
arm of the ladder, both key ranges, and ties inside the folded pairs in both rank orders.

Shapes (tests/ladder_cases.py): one wave, two strips, the five-wave workgroup; 4:2:0 under the default policy (coupled
luma sweep + one-sweep chroma kernel) and with chroma_sweeps=1 (the two chroma sweeps); row bands, once with the default
run-up and once with a run-up from the top of the plane, which no pattern can fail (so no frame is redone elsewhere).  opt=0 is checked
against oracle.oracle.Oracle; opt=1 (planes on their own are what has sweeps in that arithmetic) against the model of the
SSE2 arithmetic, tests/sse2_model.py, the reference of the existing SSE2 tests -- the C oracle has no such mode.
"""
import pytest

from avisynth_sangnom2_amd import SangNom2, clip_format
from oracle.oracle import Oracle
from tests import ladder_cases as lc
from tests import sse2_model as sm
from tests.util import describe_diff, oracle_cfg, same

pytestmark = pytest.mark.gpu


def _reference(clip, kw, opt):
    if opt == 0:
        ora = Oracle(oracle_cfg(clip, **kw))
        return lambda src, parity: ora.process(src, parity=parity)
    m = sm.Sse2SangNom(clip.width, clip.height, bytes=clip.bytes, bits=clip.bits, planes=clip.planes, subw=clip.subw, subh=clip.subh,
                       order=kw.get("order", 1), aa=kw.get("aa", 48), aac=kw.get("aac", 0))
    return lambda src, parity: m.get_frame(src, parity=parity)


def _check(fmt, w, h, kw, pattern, opt=0, bands=None, **policy):
    clip = clip_format(fmt, w, h)
    want_of = _reference(clip, kw, opt)
    with SangNom2(clip, mode="fused" if bands is None else "auto", opt=opt, **policy, **kw) as flt:
        if bands is not None:
            flt.set_bands(*bands)
        for f, src in enumerate(lc.frames(clip, pattern)):
            want = want_of(src, f & 1)
            got = flt.get_frame(src, parity=f & 1)
            for p in range(len(want)):
                assert same(want[p], got[p]), f"{fmt} {w}x{h} {kw} opt={opt} {pattern} frame {f} plane {p}: " + describe_diff(want[p], got[p])
        info = flt.info()
        if bands is None:
            assert info.fused_frames == lc.NFRAMES
        else:
            # with the default run-up the bands' check may send flat or periodic material to the pool kernels (noise passes
            # it); with a run-up from the top of the plane every band is exact and no frame may fall back
            assert info.banded_frames == lc.NFRAMES
            assert info.band_fallbacks == 0 or (bands[1] == 0 and pattern != "noise"), (pattern, info.band_fallbacks)
    return info


@pytest.mark.parametrize("opt", (0, 1))
@pytest.mark.parametrize("aa", lc.AA)
@pytest.mark.parametrize("shape", lc.Y8_SHAPES, ids=lambda s: f"{s[1]}x{s[2]}" + (f"-bands{s[3][1]}" if s[3] else ""))
def test_y8_ladder_matches_reference(hip_lib, shape, aa, opt):
    fmt, w, h, bands = shape
    for pattern in lc.PATTERNS:
        _check(fmt, w, h, dict(order=1, aa=aa), pattern, opt=opt, bands=bands)


@pytest.mark.parametrize("aa", lc.AA)
@pytest.mark.parametrize("shape", lc.YUV_SHAPES, ids=lambda s: f"{s[1]}x{s[2]}")
def test_yuv420p8_ladder_matches_oracle(hip_lib, shape, aa):
    """Default policy: the coupled luma sweep and the one-sweep chroma kernel; chroma_sweeps = 1: U and V as sweeps of their own."""
    fmt, w, h, _ = shape
    for pattern in lc.PATTERNS:
        info = _check(fmt, w, h, dict(order=1, aa=aa, aac=aa), pattern)
        assert info.uv_sweeps == 1
        info = _check(fmt, w, h, dict(order=1, aa=aa, aac=aa), pattern, chroma_sweeps=1)
        assert info.uv_sweeps == 0
