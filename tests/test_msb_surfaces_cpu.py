"""MSB-aligned surfaces without a GPU: the two new layout constants in the header and in the mirror, the ABI unchanged, and
the case table of tests/test_msb_surfaces_gpu.py held against what a caller gets today -- a 16-bit context on the same words
gives other pixels, so every GPU case can tell the two apart -- and against the rule's consequence that an MSB destination has
zero low bits."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from avisynth_sangnom2_amd import capi
from tests import msb_surface_cases as mc
from tests import sse2_sweep_cases as ssc
from tests.util import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r"""
#include <stdio.h>
#include "sangnom_hip.h"
int main(void)
{
    printf("%d %d %d %d %d %d\n", SN_LAYOUT_PLANAR, SN_LAYOUT_SEMIPLANAR, SN_LAYOUT_PLANAR_MSB, SN_LAYOUT_SEMIPLANAR_MSB, (int)sizeof(sn_surfaces),
           SN_ABI_VERSION);
    return 0;
}
"""


def test_the_constants_in_the_header_and_in_the_mirror(tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()
    assert [int(x) for x in out] == [0, 1, 2, 3, 72, 4]
    assert (capi.SN_LAYOUT_PLANAR, capi.SN_LAYOUT_SEMIPLANAR, capi.SN_LAYOUT_PLANAR_MSB, capi.SN_LAYOUT_SEMIPLANAR_MSB) == (0, 1, 2, 3)
    assert ctypes.sizeof(capi.SnSurfaces) == 72


def test_the_abi_version_stays(hip_lib):
    assert hip_lib.sn_abi_version() == 4


def test_surfaces_helper_takes_the_new_layouts():
    s = capi.surfaces(capi.SN_LAYOUT_SEMIPLANAR_MSB, [16, 32], [64, 128], [1024, 2048])
    assert (s.layout, s.plane[0], s.plane[1], s.plane[2], s.pitch[1], s.frame_stride[1], s.reserved) == (3, 16, 32, None, 128, 2048, 0)
    assert capi.surfaces(capi.SN_LAYOUT_PLANAR_MSB, [16], [64], [1024]).layout == 2


def test_the_source_helper():
    """Shifted down an MSB source is the frame again, every sample has a non-zero low part, and the low parts are not constant."""
    case = mc.PARITY[0]
    clip, frames, _, _ = mc.expected(case)
    s = mc.shift_of(clip)
    assert s == 6 and mc.shift_of(mc.expected(mc.PARITY[1])[0]) == 4 and mc.shift_of(mc.expected(mc.SIXTEEN)[0]) == 0
    src = mc.msb_source(frames, s)
    for fr, ws in zip(frames, src):
        for pl, w in zip(fr, ws):
            assert w.dtype == np.uint16 and same(w >> np.uint16(s), pl)
            low = w & np.uint16(63)
            assert low.min() >= 1 and low.max() == 63 and len(np.unique(low)) == 63
    assert mc.low_bits((4, 4), 0, 1).max() == 0
    assert len({c.id for c in mc.EVERY}) == len(mc.EVERY)


@pytest.mark.parametrize("case", mc.EVERY, ids=[c.id for c in mc.EVERY])
def test_a_sixteen_bit_context_gives_other_pixels(case):
    """What a caller gets today: a 16-bit context on the MSB-aligned words.  That differs from the clip's own result shifted up
    -- on the source words as the GPU tests upload them (low bits set) and on clean words (low bits zero), where only the
    interpolation can differ -- and the expected MSB frames have zero low bits."""
    clip, frames, par, want = mc.expected(case)
    s = mc.shift_of(clip)
    assert s > 0
    want_msb = mc.up(want, s)
    for fr in want_msb:
        for pl in fr:
            assert not np.any(pl & np.uint16((1 << s) - 1))
    # (the filter does not clamp to the clip's range -- the reference does not either --, so a 10-bit result may exceed 1023 on
    # hard input; shifted up in its 16-bit word such a sample loses its high bits, in the library as in numpy)
    assert ssc.differs(want_msb, mc.sixteen_bit_result(case, mc.msb_source(frames, s))), "a 16-bit context gives the same on these words"
    assert ssc.differs(want_msb, mc.sixteen_bit_result(case, mc.up(frames, s))), "a 16-bit context interpolates the same on clean words"


@pytest.mark.parametrize("fmt,dh", mc.AA, ids=[f"{f}-dh{int(d)}" for f, d in mc.AA])
def test_a_sixteen_bit_anti_aliasing_context_gives_other_pixels(fmt, dh):
    clip, frames, want = mc.expected_aa(fmt, dh)
    s = mc.shift_of(clip)
    want_msb = mc.up(want, s)
    assert not any(np.any(pl & np.uint16((1 << s) - 1)) for fr in want_msb for pl in fr)
    assert ssc.differs(want_msb, mc.sixteen_bit_result_aa(fmt, dh, mc.msb_source(frames, s)))
    assert ssc.differs(want_msb, mc.sixteen_bit_result_aa(fmt, dh, mc.up(frames, s)))


def test_the_scratch_formula():
    """The documented sum: chroma as before, plus a luma plane for an MSB source with processed luma."""
    clip = mc.expected(mc.CHUNKED)[0]
    assert mc.scratch_frame_bytes(clip, True, True, True) == 2 * (256 * 20 + 256 * 20) + 256 * 40
    assert mc.scratch_frame_bytes(clip, True, False, True) == 2 * (256 * 20 + 256 * 20)  # no MSB source: what it always was
    assert mc.scratch_frame_bytes(clip, False, False, False) == 0
    assert mc.scratch_frame_bytes(clip, False, False, True) == 2 * (256 * 20 + 256 * 20)
    assert mc.scratch_frame_bytes(clip, True, True, True, luma=False) == 2 * (256 * 20 + 256 * 20)
    assert mc.scratch_frame_bytes(clip, True, True, True, chroma=False) == 256 * 40
    assert mc.scratch_frames(mc.scratch_frame_bytes(clip, True, True, True), mc.CHUNKED.n, 1) == 2, "four frames must take two chunks under 1 MiB"
    y = mc.expected(mc.LUMA_ONLY[0])[0]
    assert mc.scratch_frame_bytes(y, False, True, False) == 256 * 32
