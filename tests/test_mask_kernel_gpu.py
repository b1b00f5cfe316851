"""sn_mask_merge_device (csrc/sn_mask.hip) against the numpy statement of its contract (tests/mask_model.py), bit for bit:
every sample type, with and without the expansion, the shapes at which the tile indexing can go wrong, aligned surfaces (16
bytes per lane and access), each of src, aa and dst misaligned by one sample, odd pitches, and dst in place on aa.  The frames
of one launch are the input patterns; their frame strides are larger than the plane, and the destination is pre-filled with
0x5C: every byte outside the W x H planes must be unchanged afterwards.  aa = NULL writes the mask itself."""
import ctypes
import os
import re

import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2, capi, clip_format, synth
from tests.mask_model import edge_mask, mask_plane, merge_plane
from tests.util import describe_diff, same, to_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VT = {1: np.uint8, 2: np.int16, 4: np.float32}  # torch has no uint16: same bits
LO, HI = 16, 96


def _tile():
    text = open(os.path.join(ROOT, "avisynth_sangnom2_amd", "csrc", "sn_mask.hip")).read()
    m = re.search(r"kMaskTileBytes = (\d+), kMaskTileH = (\d+);", text)
    return int(m.group(1)), int(m.group(2))


TILE_BYTES, TH = _tile()  # the kernel's output tile: 256 bytes of a row (256 / 128 / 64 samples) x 16 rows


def _shapes(B):
    """(W, H): planes narrower than the window (every tap clamped); one less than the tile, the tile and one more in each
    direction; three tiles each way with ragged edges."""
    TW = TILE_BYTES // B
    return [(1, 1), (2, 3), (3, 2), (TW - 1, TH), (TW, TH), (TW + 1, TH), (TW, TH - 1), (TW, TH + 1), (2 * TW + 22, 2 * TH + 5)]


CONTEXTS = ["Y8", "Y10", "Y16", "Y32"]
LAYOUTS = ["aligned", "src_base", "aa_base", "dst_base", "pitches", "in_place"]


def _inputs(clip, W, H, seed):
    """The source frames of one launch [H, W]: edges (all three classes of the mask), constant, a one-pixel checker, full-range
    noise, and for float a constant plane with NaN and infinities in it, alone, side by side and on the plane's edges: there
    every sample of the result is a copy of S or of R, whatever a NaN's payload would do in the blend."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    if clip.bytes == 4:
        f = np.float32
        out = [synth.plane(H, W, 4, 32, "edges", seed), np.full((H, W), 0.3, f), ((x + y) & 1).astype(f),
               (rng.random((H, W), dtype=f) * f(2) - f(1)).astype(f)]
        sp = np.full((H, W), 0.5, f)
        for k, v in enumerate([np.nan, np.inf, -np.inf, np.nan, np.inf, np.inf]):
            sp[(k * 7) % H, (k * 29 + (k > 3)) % W] = v
        sp[H - 1, W - 1] = np.inf
        sp[0, W // 2] = np.nan
        out.append(sp)
        return out
    mx = (1 << clip.bits) - 1
    return [synth.plane(H, W, clip.bytes, clip.bits, "edges", seed), np.full((H, W), mx // 3, clip.dtype), (((x + y) & 1) * mx).astype(clip.dtype),
            rng.integers(0, mx + 1, (H, W)).astype(clip.dtype)]


def _results(clip, W, H, N, seed):
    rng = np.random.default_rng(seed)
    if clip.bytes == 4:
        return [rng.random((H, W), dtype=np.float32) for _ in range(N)]
    return [rng.integers(0, 1 << clip.bits, (H, W)).astype(clip.dtype) for _ in range(N)]


def _surface(planes, fill, base_off, odd_pitch, W, H, B):
    """[N, H + 2, pitch] of fill bytes with the planes at [:, :H, base_off:base_off + W]; pitch * B a multiple of 16 unless odd_pitch."""
    pitch = (W + 3 + 15) // 16 * 16 + (1 if odd_pitch else 0)
    big = np.full((len(planes), H + 2, pitch * B), fill, np.uint8).view(planes[0].dtype)
    for f, pl in enumerate(planes):
        big[f, :H, base_off:base_off + W] = pl
    return big


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("expand", [0, 1])
@pytest.mark.parametrize("fmt", CONTEXTS)
def test_mask_merge_device_matches_the_model(hip_lib, fmt, expand, layout):
    import torch
    dev = torch.device("cuda:0")
    clip = clip_format(fmt, 64, 32)  # the context gives the sample type and the bit depth; its own size plays no part
    B = clip.bytes
    with SangNom2(clip, device=0) as flt:
        for si, (W, H) in enumerate(_shapes(B)):
            S = _inputs(clip, W, H, seed=2000 + si)
            N = len(S)
            R = _results(clip, W, H, N, seed=3000 + si)
            s_off, a_off, d_off = (1 if layout == k else 0 for k in ("src_base", "aa_base", "dst_base"))
            odd = layout == "pitches"
            src_h = _surface(S, 0x11, s_off, odd, W, H, B)
            aa_h = _surface(R, 0x5C, a_off, odd, W, H, B)
            dst_h = _surface([np.zeros((H, W), clip.dtype)] * N, 0x5C, d_off, odd, W, H, B)
            dst_h.view(np.uint8)[...] = 0x5C
            src = torch.from_numpy(src_h.view(VT[B])).pin_memory().to(dev)
            aa = torch.from_numpy(aa_h.view(VT[B])).pin_memory().to(dev)
            dst = aa if layout == "in_place" else torch.from_numpy(dst_h.view(VT[B])).pin_memory().to(dev)
            before = aa_h if layout == "in_place" else dst_h
            views = [src[:, :H, s_off:s_off + W], aa[:, :H, a_off:a_off + W], dst[:, :H, d_off:d_off + W]]
            aligned = [all(v % 16 == 0 for v in (t.data_ptr(), t.stride(0) * B, t.stride(1) * B)) for t in views]
            assert aligned == [layout not in ("src_base", "pitches"), layout not in ("aa_base", "pitches"), layout not in ("dst_base", "pitches")]
            torch.cuda.synchronize()
            flt.mask_merge(views[0], views[1], views[2], LO, HI, expand)
            flt.synchronize()
            got = to_host(dst).view(clip.dtype)
            for f in range(N):
                want = merge_plane(S[f], R[f], LO, HI, expand, clip.bits)
                g = got[f, :H, d_off:d_off + W]
                assert same(want, g), f"{W}x{H} frame {f}: " + describe_diff(want, g)
            if W > 8 and H > 8:  # the launch is no trivial one: frame 0 holds samples of all three classes
                m = edge_mask(S[0], LO, HI, expand, clip.bits)
                assert (m == 0).any() and (m == 256).any() and ((m > 0) & (m < 256)).any()
            outside = np.ones(got.shape, bool)
            outside[:, :H, d_off:d_off + W] = False
            assert np.array_equal(got.view(np.uint8).reshape(got.shape + (-1,))[outside], before.view(np.uint8).reshape(got.shape + (-1,))[outside]), \
                f"{W}x{H}: bytes outside the planes were written"
            assert np.array_equal(to_host(src).view(np.uint8), src_h.view(np.uint8)), "the source was written"


@pytest.mark.parametrize("expand", [0, 1])
@pytest.mark.parametrize("fmt", CONTEXTS)
def test_without_a_result_the_mask_itself_is_written(hip_lib, fmt, expand):
    import torch
    dev = torch.device("cuda:0")
    clip = clip_format(fmt, 64, 32)
    B = clip.bytes
    with SangNom2(clip, device=0) as flt:
        for si, (W, H) in enumerate(_shapes(B)):
            S = _inputs(clip, W, H, seed=2100 + si)
            N = len(S)
            dst_h = _surface([np.zeros((H, W), clip.dtype)] * N, 0x5C, 0, False, W, H, B)
            dst_h.view(np.uint8)[...] = 0x5C
            src = torch.from_numpy(_surface(S, 0x11, 0, False, W, H, B).view(VT[B])).pin_memory().to(dev)
            dst = torch.from_numpy(dst_h.view(VT[B])).pin_memory().to(dev)
            torch.cuda.synchronize()
            flt.mask_merge(src[:, :H, :W], None, dst[:, :H, :W], LO, HI, expand)
            flt.synchronize()
            got = to_host(dst).view(clip.dtype)
            for f in range(N):
                want = mask_plane(S[f], LO, HI, expand, clip.bits)
                assert same(want, got[f, :H, :W]), f"{W}x{H} frame {f}: " + describe_diff(want, got[f, :H, :W])
            outside = np.ones(got.shape, bool)
            outside[:, :H, :W] = False
            assert np.all(got.view(np.uint8).reshape(got.shape + (-1,))[outside] == 0x5C), f"{W}x{H}: bytes outside the planes were written"


def test_equal_and_extreme_thresholds(hip_lib):
    """lo = hi (no ramp; the kernel's ramp divisor is never used), (0, 0), (255, 255) and (0, 255) on 8-bit, 16-bit and float."""
    import torch
    dev = torch.device("cuda:0")
    for fmt in ("Y8", "Y16", "Y32"):
        clip = clip_format(fmt, 64, 32)
        W, H = 150, 37
        S = synth.plane(H, W, clip.bytes, clip.bits, "edges", 77)
        R = _results(clip, W, H, 1, 9)[0]
        src = torch.from_numpy(S[None].view(VT[clip.bytes])).pin_memory().to(dev)
        aa = torch.from_numpy(R[None].view(VT[clip.bytes])).pin_memory().to(dev)
        with SangNom2(clip, device=0) as flt:
            for lo, hi in ((40, 40), (0, 0), (255, 255), (0, 255), (39, 40)):
                for expand in (0, 1):
                    dst = torch.zeros_like(aa)
                    torch.cuda.synchronize()
                    flt.mask_merge(src, aa, dst, lo, hi, expand)
                    flt.synchronize()
                    want = merge_plane(S, R, lo, hi, expand, clip.bits)
                    got = to_host(dst).view(clip.dtype)[0]
                    assert same(want, got), f"{fmt} lo {lo} hi {hi} expand {expand}: " + describe_diff(want, got)


def test_bad_arguments_are_refused_and_nothing_is_queued(hip_lib):
    import torch
    dev = torch.device("cuda:0")
    W, H = 40, 20
    src = torch.zeros((1, H, W), dtype=torch.uint8, device=dev)
    aa = torch.full((1, H, W), 9, dtype=torch.uint8, device=dev)
    dst = torch.full((1, H, W), 0x5C, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    L = capi.load()
    size = ctypes.sizeof(capi.SnAAMask)
    with SangNom2(clip_format("Y8", 64, 32), device=0) as flt:
        def call(mask=None, sp=W, ap=W, dp=W, s=src.data_ptr(), a=aa.data_ptr(), d=dst.data_ptr(), w=W, h=H, **mkw):
            m = capi.SnAAMask(**dict(dict(struct_size=size, kind=1, lo=16, hi=96, expand=1), **mkw))
            return L.sn_mask_merge_device(flt._h, ctypes.byref(m), 1, s, W * H, sp, a, W * H, ap, w, h, d, W * H, dp)
        for kw in (dict(lo=-1), dict(hi=256), dict(lo=97), dict(expand=2), dict(kind=0), dict(kind=2), dict(struct_size=size - 4), dict(sp=W - 1),
                   dict(ap=W - 1), dict(dp=W - 1), dict(s=None), dict(d=None), dict(w=0), dict(h=0)):
            assert call(**kw) == capi.SN_ERR_INVALID_ARG, kw
            assert b"sn_mask_merge_device" in L.sn_last_error(flt._h)
        bad = capi.SnAAMask(struct_size=size, kind=1, lo=16, hi=96, expand=1)
        bad.reserved[2] = 1
        assert L.sn_mask_merge_device(flt._h, ctypes.byref(bad), 1, src.data_ptr(), W * H, W, aa.data_ptr(), W * H, W, W, H, dst.data_ptr(), W * H, W) \
            == capi.SN_ERR_INVALID_ARG
        assert L.sn_mask_merge_device(flt._h, None, 1, src.data_ptr(), W * H, W, aa.data_ptr(), W * H, W, W, H, dst.data_ptr(), W * H, W) == capi.SN_ERR_INVALID_ARG
        flt.synchronize()
        assert np.all(to_host(dst) == 0x5C), "a refused call wrote the destination"
        assert call() == capi.SN_OK  # a constant source: the mask is empty and dst is the source
        flt.synchronize()
        assert np.all(to_host(dst) == 0)
    with SangNom2(clip_format("Y16", 64, 32), device=0) as flt:  # pointers and pitches in whole samples
        m = capi.SnAAMask(struct_size=size, kind=1, lo=16, hi=96, expand=1)
        for s_off, a_off, dp in ((1, 0, W), (0, 1, W), (0, 0, W - 1)):
            assert L.sn_mask_merge_device(flt._h, ctypes.byref(m), 1, src.data_ptr() + s_off, W * H, W, aa.data_ptr() + a_off, W * H, W, W // 2, H,
                                          dst.data_ptr(), W * H, dp) == capi.SN_ERR_INVALID_ARG
