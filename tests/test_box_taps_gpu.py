"""The 8-bit sweeps' box filter and line unpack at the plane's edges, bit-exact against the CPU oracle.

The box's left clamp lives in lane 0 of the first strip and its right clamp in whichever lane, strip and wave holds
column w-1; the widths below put column w-1 at the end of a wave, inside one, in the second half of a register (the
other strip), and on either side of the eight-wave limit.  8-bit 4:2:0 adds the one-sweep chroma kernel and the coupled
luma sweep, whose line form packs F | B << 8.
"""
import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2, clip_format
from oracle.oracle import Oracle
from tests.util import describe_diff, make_frames, oracle_cfg, same

pytestmark = pytest.mark.gpu

WIDTHS = (32, 64, 480, 512, 960, 992, 1920, 3808, 3840, 4096, 7680)


def _check(fmt, w, h, kw, pattern, nframes=2, bands=None):
    clip = clip_format(fmt, w, h)
    ora = Oracle(oracle_cfg(clip, **kw))
    with SangNom2(clip, mode="fused" if bands is None else "auto", **kw) as flt:
        if bands is not None:
            flt.set_bands(*bands)
        for f, src in enumerate(make_frames(clip, pattern, nframes, seed0=31)):
            want = ora.process(src, parity=f & 1)
            got = flt.get_frame(src, parity=f & 1)
            for p in range(len(want)):
                assert same(want[p], got[p]), f"{fmt} {w}x{h} {kw} {pattern} frame {f} plane {p}: " + describe_diff(want[p], got[p])
        info = flt.info()
        if bands is None:
            assert info.fused_frames == nframes
        else:  # a run-up of one row fails the bands' check and sends the frame to the pool kernels
            assert info.banded_frames == nframes and (info.band_fallbacks == nframes) == (bands[1] == 1)
    return info


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("order", [0, 1, 2])
def test_y8_edges_match_oracle(hip_lib, w, order):
    for pattern in ("noise", "edges"):
        _check("Y8", w, 22, dict(order=order, aa=48), pattern)


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("order", [0, 1, 2])
def test_yuv420p8_edges_match_oracle(hip_lib, w, order):
    # narrow planes take the two-sweep chroma modes, wider ones the one-sweep chroma kernel: both are meant here
    _check("YUV420P8", w, 24, dict(order=order, aa=48, aac=48), "noise")


@pytest.mark.parametrize("fmt,w", [("Y8", 512), ("Y8", 992), ("Y8", 3840), ("YUV420P8", 960), ("YUV420P8", 3808)])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_two_frame_band_launch_matches_oracle(hip_lib, monkeypatch, fmt, w, order):
    """One device batch of two frames cut into row bands (frames x bands workgroups of the banded sweep)."""
    import torch
    from avisynth_sangnom2_amd import capi as _capi
    from tests.util import to_host
    monkeypatch.setitem(_capi.POLICY_DEFAULTS, "small_launches", _capi.SN_SMALL_AUTO)
    kw = dict(order=order, aa=48, aac=48) if fmt == "YUV420P8" else dict(order=order, aa=48)
    clip = clip_format(fmt, w, 320)
    frames = make_frames(clip, "noise", 2, seed0=43)
    parity = [0, 1]
    ora = Oracle(oracle_cfg(clip, **kw))
    want = [ora.process(frames[f], parity=parity[f]) for f in range(2)]
    dev = torch.device("cuda:0")
    with SangNom2(clip, max_batch=2, **kw) as flt:
        flt.set_bands(6, 0)
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
