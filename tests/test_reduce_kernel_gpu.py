"""sn_reduce_device (csrc/sn_reduce.hip) against the numpy statement of its contract (tests/reduce_model.py), bit for bit:
both kernels, all four (ox, oy), every sample type, the shapes at which the tile indexing can go wrong, aligned surfaces
(16 bytes per lane and access) and surfaces misaligned by one sample on either side (sample-wide accesses).  The frames of
one launch are the input patterns; their frame strides are larger than the plane, and the destination is pre-filled with
0x5C: every byte outside the W x H planes must be unchanged afterwards."""
import os
import re

import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2, capi, clip_format
from tests.reduce_model import KERNEL_ID, reduce_plane
from tests.util import describe_diff, same, to_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VT = {1: np.uint8, 2: np.int16, 4: np.float32}  # torch has no uint16: same bits


def _tile():
    text = open(os.path.join(ROOT, "avisynth_sangnom2_amd", "csrc", "sn_reduce.hip")).read()
    m = re.search(r"kReduceTileBytes = (\d+), kReduceTileH = (\d+);", text)
    return int(m.group(1)), int(m.group(2))


TILE_BYTES, TH = _tile()  # the kernel's output tile: 256 bytes of a row (256 / 128 / 64 samples) x 16 rows


def _shapes(B):
    """(W, H) of the destination: E narrower than the half-band's reach (every tap clamped); one less than the tile, the tile
    and one more in each direction; three tiles each way with ragged edges."""
    TW = TILE_BYTES // B
    return [(1, 1), (2, 3), (3, 2), (TW - 1, TH), (TW, TH), (TW + 1, TH), (TW, TH - 1), (TW, TH + 1), (2 * TW + 22, 2 * TH + 5)]


CONTEXTS = ["Y8", "Y10", "Y16", "Y32"]
LAYOUTS = ["aligned", "src_base", "dst_base", "pitches"]


def _inputs(clip, W, H, seed):
    """The frames of one launch: E planes [2H, 2W] of the clip's dtype."""
    rng = np.random.default_rng(seed)
    shape = (2 * H, 2 * W)
    cols = (np.arange(2 * W) & 1)[None, :] * np.ones((2 * H, 1), np.int64)
    rows = (np.arange(2 * H) & 1)[:, None] * np.ones((1, 2 * W), np.int64)
    if clip.bytes == 4:
        f = np.float32
        return [rng.random(shape, dtype=f), np.ones(shape, f), np.zeros(shape, f), cols.astype(f), rows.astype(f), (1 - cols).astype(f),
                (rng.random(shape, dtype=f) * f(2) - f(1)).astype(f)]
    mx = (1 << clip.bits) - 1
    dt = clip.dtype
    out = [rng.integers(0, mx + 1, shape).astype(dt), np.full(shape, mx, dt), np.zeros(shape, dt), (cols * mx).astype(dt), (rows * mx).astype(dt),
           ((1 - cols) * mx).astype(dt), ((cols ^ rows) * mx).astype(dt)]
    if clip.bits < 8 * clip.bytes:  # a plane beyond the clip's range: the upper clamp of either kernel
        out.append(rng.integers(0, 1 << (8 * clip.bytes), shape).astype(dt))
    return out


def _surface(planes, fill, base_off, odd_pitch, W, H, B):
    """[N, H + 2, pitch] of fill bytes with the planes at [:, :H, base_off:base_off + W]; pitch * B a multiple of 16 unless odd_pitch."""
    pitch = (W + 3 + 15) // 16 * 16 + (1 if odd_pitch else 0)
    big = np.full((len(planes), H + 2, pitch * B), fill, np.uint8).view(planes[0].dtype) if planes else None
    for f, pl in enumerate(planes):
        big[f, :H, base_off:base_off + W] = pl
    return big


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kernel", ["tent", "halfband"])
@pytest.mark.parametrize("fmt", CONTEXTS)
def test_reduce_device_matches_the_model(hip_lib, fmt, kernel, layout):
    import torch
    dev = torch.device("cuda:0")
    clip = clip_format(fmt, 64, 32)  # the context gives the sample type and the bit depth; its own size plays no part
    B = clip.bytes
    with SangNom2(clip, device=0) as flt:
        for si, (W, H) in enumerate(_shapes(B)):
            frames = _inputs(clip, W, H, seed=1000 + si)
            N = len(frames)
            s_off = 1 if layout == "src_base" else 0
            d_off = 1 if layout == "dst_base" else 0
            odd = layout == "pitches"
            src_h = _surface(frames, 0x11, s_off, odd, 2 * W, 2 * H, B)
            dst_h = _surface([np.zeros((H, W), clip.dtype)] * N, 0x5C, d_off, odd, W, H, B)
            dst_h.view(np.uint8)[...] = 0x5C
            src = torch.from_numpy(src_h.view(VT[B])).pin_memory().to(dev)
            for ox in (0, 1):
                for oy in (0, 1):
                    dst = torch.from_numpy(dst_h.view(VT[B]).copy()).pin_memory().to(dev)
                    s_view, d_view = src[:, :2 * H, s_off:s_off + 2 * W], dst[:, :H, d_off:d_off + W]
                    if layout == "aligned":
                        assert all(v % 16 == 0 for t in (s_view, d_view) for v in (t.data_ptr(), t.stride(0) * B, t.stride(1) * B))
                    else:
                        assert any(v % 16 for t in (s_view, d_view) for v in (t.data_ptr(), t.stride(0) * B, t.stride(1) * B))
                    torch.cuda.synchronize()
                    flt.reduce(s_view, d_view, kernel, ox, oy)
                    flt.synchronize()
                    got = to_host(dst).view(clip.dtype)
                    for f in range(N):
                        want = reduce_plane(frames[f], kernel, ox, oy, clip.bits)
                        g = got[f, :H, d_off:d_off + W]
                        assert same(want, g), f"{W}x{H} ox={ox} oy={oy} frame {f}: " + describe_diff(want, g)
                    outside = np.ones(got.shape, bool)
                    outside[:, :H, d_off:d_off + W] = False
                    assert np.array_equal(got.view(np.uint8).reshape(got.shape + (-1,))[outside], dst_h.view(np.uint8).reshape(got.shape + (-1,))[outside]), \
                        f"{W}x{H} ox={ox} oy={oy}: bytes outside the planes were written"


def test_bad_arguments_are_refused_and_nothing_is_queued(hip_lib):
    import torch
    dev = torch.device("cuda:0")
    W, H = 40, 20
    src = torch.zeros((1, 2 * H, 2 * W), dtype=torch.uint8, device=dev)
    dst = torch.full((1, H, W), 0x5C, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    L = capi.load()
    with SangNom2(clip_format("Y8", 64, 32), device=0) as flt:
        def call(kernel=1, ox=0, oy=0, sp=2 * W, dp=W, s=src.data_ptr(), d=dst.data_ptr()):
            return L.sn_reduce_device(flt._h, kernel, 1, s, 4 * W * H, sp, W, H, ox, oy, d, W * H, dp)
        for kw in (dict(ox=2), dict(oy=2), dict(ox=-1), dict(kernel=0), dict(kernel=3), dict(sp=2 * W - 1), dict(dp=W - 1), dict(s=None), dict(d=None)):
            assert call(**kw) == capi.SN_ERR_INVALID_ARG, kw
            assert b"sn_reduce_device" in L.sn_last_error(flt._h)
        flt.synchronize()
        assert np.all(to_host(dst) == 0x5C), "a refused call wrote the destination"
        assert call() == capi.SN_OK
        flt.synchronize()
        assert np.all(to_host(dst) == 0)
    with SangNom2(clip_format("Y16", 64, 32), device=0) as flt:  # pointers and pitches in whole samples
        assert L.sn_reduce_device(flt._h, 1, 1, src.data_ptr() + 1, 4 * W * H, 2 * W, W // 2, H, 0, 0, dst.data_ptr(), W * H, W) == capi.SN_ERR_INVALID_ARG
        assert L.sn_reduce_device(flt._h, 1, 1, src.data_ptr(), 4 * W * H, 2 * W, W // 2, H, 0, 0, dst.data_ptr(), W * H, W - 1) == capi.SN_ERR_INVALID_ARG
