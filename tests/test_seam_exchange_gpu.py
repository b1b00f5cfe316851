"""The 8-bit sweep's seam exchange and its blocks of five rows, bit-exact against the CPU oracle.

Every seam lane publishes its registers whole and each ghost lane picks the half it needs; at the wrap seam (strip NW-1 |
strip NW) that is the other half of the published word.  The widths below give planes of 1, 2, 4 and 8 waves, and planes
with an odd number of strips, whose last wave has a dead high half.  The heights end in a partial block of rows, so the
rows after the last full block run on their own; the band launches start their own rows off the block grid.  8-bit 4:2:0
with two chroma sweeps takes the pool-coupled modes, which share the mailbox.
"""
import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2, clip_format
from oracle.oracle import Oracle
from tests.util import describe_diff, make_frames, oracle_cfg, same, to_host

pytestmark = pytest.mark.gpu

# 960 / 1920 / 3840 / 7680: 1 / 2 / 4 / 8 waves; 1440: 3 strips, 2912: 7 strips (the last wave's high half is dead)
WIDTHS = (960, 1440, 1920, 2912, 3840, 7680)
# kept lines 13, 19, 23: the row loop ends 2, 3 and 2 rows into a block
HEIGHTS = (26, 38, 46)


def _check(fmt, w, h, kw, nframes=2, **policy):
    clip = clip_format(fmt, w, h)
    ora = Oracle(oracle_cfg(clip, **kw))
    with SangNom2(clip, mode="fused", **policy, **kw) as flt:
        for f, src in enumerate(make_frames(clip, "noise", nframes, seed0=57)):
            want = ora.process(src, parity=f & 1)
            got = flt.get_frame(src, parity=f & 1)
            for p in range(len(want)):
                assert same(want[p], got[p]), f"{fmt} {w}x{h} {kw} frame {f} plane {p}: " + describe_diff(want[p], got[p])
        assert flt.info().fused_frames == nframes
        return flt.info()


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("order", [0, 1, 2])
def test_y8_seams_match_oracle(hip_lib, w, order):
    for h in HEIGHTS:
        _check("Y8", w, h, dict(order=order, aa=48))


@pytest.mark.parametrize("w", (960, 1408, 1920, 3328, 3840))
@pytest.mark.parametrize("order", [0, 1, 2])
def test_yuv420p8_two_chroma_sweeps_match_oracle(hip_lib, w, order):
    """chroma_sweeps = 1: the luma sweep hands off through its pool, U and V run as sweeps of their own (1408 and 3328
    columns: 3 and 7 strips, with chroma planes the sweeps take)."""
    info = _check("YUV420P8", w, 52, dict(order=order, aa=48, aac=48), chroma_sweeps=1)
    assert info.uv_sweeps == 0


@pytest.mark.parametrize("w,bands", [(960, 7), (1440, 6), (3840, 6), (2912, 9)])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_y8_band_launch_off_the_block_grid_matches_oracle(hip_lib, monkeypatch, w, bands, order):
    """Two frames cut into row bands whose first rows are not 1 + a multiple of five."""
    import torch
    from avisynth_sangnom2_amd import capi as _capi
    monkeypatch.setitem(_capi.POLICY_DEFAULTS, "small_launches", _capi.SN_SMALL_AUTO)
    kw = dict(order=order, aa=48)
    clip = clip_format("Y8", w, 300)
    frames = make_frames(clip, "noise", 2, seed0=61)
    parity = [0, 1]
    ora = Oracle(oracle_cfg(clip, **kw))
    want = [ora.process(frames[f], parity=parity[f]) for f in range(2)]
    dev = torch.device("cuda:0")
    with SangNom2(clip, max_batch=2, **kw) as flt:
        flt.set_bands(bands, 0)
        src = [torch.from_numpy(np.stack([frames[f][p] for f in range(2)])).pin_memory().to(dev) for p in range(clip.planes)]
        dst = [torch.zeros((2,) + flt.plane_shape_out(p), dtype=torch.uint8, device=dev) for p in range(clip.planes)]
        torch.cuda.synchronize()
        flt.process_batch(src, dst, parity=parity)
        flt.synchronize()
        assert flt.info().banded_frames == 2
        for f in range(2):
            for p in range(clip.planes):
                got = to_host(dst[p][f]).view(clip.dtype)
                assert same(want[f][p], got), f"frame {f} plane {p}: " + describe_diff(want[f][p], got)
