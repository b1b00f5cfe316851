"""sn_contra_sharpen_device (csrc/sn_sharpen.hip) against the numpy statement of its contract (tests/sharpen_model.py), bit for
bit (floats on bit patterns): every sample type, amount 1, 64 and 255, the shapes at which the tile indexing can go wrong,
aligned surfaces (16 bytes per lane and access), each of src, aa and dst misaligned by one sample, and odd pitches.  The frames
of one launch are the input patterns; their frame strides are larger than the plane, and the destination is pre-filled with
0x5C: every byte outside the W x H planes must be unchanged afterwards."""
import os
import re

import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2, capi, clip_format, synth
from tests.sharpen_model import sharpen_plane, sharpen_terms
from tests.util import describe_diff, same, to_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VT = {1: np.uint8, 2: np.int16, 4: np.float32}  # torch has no uint16: same bits


def _tile():
    text = open(os.path.join(ROOT, "avisynth_sangnom2_amd", "csrc", "sn_sharpen.hip")).read()
    m = re.search(r"kSharpenTileBytes = (\d+), kSharpenTileH = (\d+);", text)
    return int(m.group(1)), int(m.group(2))


TILE_BYTES, TH = _tile()  # the kernel's output tile: 256 bytes of a row (256 / 128 / 64 samples) x 16 rows


def _shapes(B):
    """(W, H): planes narrower than the window (every tap clamped); one less than the tile, the tile and one more in each
    direction; three tiles each way with ragged edges."""
    TW = TILE_BYTES // B
    return [(1, 1), (2, 3), (3, 2), (TW - 1, TH), (TW, TH), (TW + 1, TH), (TW, TH - 1), (TW, TH + 1), (2 * TW + 22, 2 * TH + 5)]


CONTEXTS = ["Y8", "Y10", "Y16", "Y32"]
AMOUNTS = [1, 64, 255]
LAYOUTS = ["aligned", "src_base", "aa_base", "dst_base", "pitches"]


def _special(W, H):
    """0.5 with NaN (one with a payload), infinities of both signs and -0.0 in it, alone, side by side and on the plane's edges."""
    sp = np.full((H, W), 0.5, np.float32)
    for k, v in enumerate([np.nan, np.inf, -np.inf, -0.0, np.inf, np.inf, -np.inf]):
        sp[(k * 7) % H, (k * 29 + (k > 4)) % W] = v
    sp[H - 1, W - 1] = np.inf
    sp[0, W // 2] = np.nan
    sp.view(np.uint32)[H // 2, 0] = 0x7FC01234
    return sp


def _patterns(clip, W, H, seed):
    """(S, R) per frame of one launch [H, W]: edges against edges with noise on top, the left quarter of S a little above R
    everywhere (there every negative d1 is cut to 0: the limit acts in every class), a constant result, a one-pixel checker
    at full range against its inverse (at 16 bit the products |d| * amount reach their bound), full-range noise in both, and
    for float the NaN / infinity plane as R and as S in turn."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    if clip.bytes == 4:
        f = np.float32
        noise = lambda: (rng.random((H, W), dtype=f) * f(2) - f(1)).astype(f)
        edges = synth.plane(H, W, 4, 32, "edges", seed)
        chk = ((x + y) & 1).astype(f)
        soft = (edges + noise() * f(0.125)).astype(f)
        above = np.where(x < W // 4, (soft + f(0.01)).astype(f), edges)
        return [(above, soft), (noise(), np.full((H, W), 0.3, f)), ((f(1) - chk).astype(f), chk), (noise(), noise()), (noise(), _special(W, H)),
                (_special(W, H), noise())]
    mx = (1 << clip.bits) - 1
    noise = lambda: rng.integers(0, mx + 1, (H, W)).astype(clip.dtype)
    edges = synth.plane(H, W, clip.bytes, clip.bits, "edges", seed)
    soft = np.clip(edges.astype(np.int64) + rng.integers(-(mx >> 3), (mx >> 3) + 1, (H, W)), 0, mx).astype(clip.dtype)
    chk = (((x + y) & 1) * mx).astype(clip.dtype)
    above = np.where(x < W // 4, np.minimum(soft.astype(np.int64) + max(mx >> 6, 1), mx).astype(clip.dtype), edges)
    return [(above, soft), (noise(), np.full((H, W), mx // 3, clip.dtype)), ((mx - chk).astype(clip.dtype), chk), (noise(), noise())]


def _surface(planes, fill, base_off, odd_pitch, W, H, B):
    """[N, H + 2, pitch] of fill bytes with the planes at [:, :H, base_off:base_off + W]; pitch * B a multiple of 16 unless odd_pitch."""
    pitch = (W + 3 + 15) // 16 * 16 + (1 if odd_pitch else 0)
    big = np.full((len(planes), H + 2, pitch * B), fill, np.uint8).view(planes[0].dtype)
    for f, pl in enumerate(planes):
        big[f, :H, base_off:base_off + W] = pl
    return big


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("amount", AMOUNTS)
@pytest.mark.parametrize("fmt", CONTEXTS)
def test_contra_sharpen_device_matches_the_model(hip_lib, fmt, amount, layout):
    import torch
    dev = torch.device("cuda:0")
    clip = clip_format(fmt, 64, 32)  # the context gives the sample type and the bit depth; its own size plays no part
    B = clip.bytes
    with SangNom2(clip, device=0) as flt:
        for si, (W, H) in enumerate(_shapes(B)):
            pats = _patterns(clip, W, H, seed=4000 + si)
            S, R = [p[0] for p in pats], [p[1] for p in pats]
            N = len(S)
            s_off, a_off, d_off = (1 if layout == k else 0 for k in ("src_base", "aa_base", "dst_base"))
            odd = layout == "pitches"
            src_h = _surface(S, 0x11, s_off, odd, W, H, B)
            aa_h = _surface(R, 0x22, a_off, odd, W, H, B)
            dst_h = _surface([np.zeros((H, W), clip.dtype)] * N, 0x5C, d_off, odd, W, H, B)
            dst_h.view(np.uint8)[...] = 0x5C
            src = torch.from_numpy(src_h.view(VT[B])).pin_memory().to(dev)
            aa = torch.from_numpy(aa_h.view(VT[B])).pin_memory().to(dev)
            dst = torch.from_numpy(dst_h.view(VT[B])).pin_memory().to(dev)
            views = [src[:, :H, s_off:s_off + W], aa[:, :H, a_off:a_off + W], dst[:, :H, d_off:d_off + W]]
            aligned = [all(v % 16 == 0 for v in (t.data_ptr(), t.stride(0) * B, t.stride(1) * B)) for t in views]
            assert aligned == [layout not in ("src_base", "pitches"), layout not in ("aa_base", "pitches"), layout not in ("dst_base", "pitches")]
            torch.cuda.synchronize()
            flt.contra_sharpen(views[0], views[1], views[2], amount)
            flt.synchronize()
            got = to_host(dst).view(clip.dtype)
            for f in range(N):
                want = sharpen_plane(S[f], R[f], amount, clip.bits)
                g = got[f, :H, d_off:d_off + W]
                assert same(want, g), f"{W}x{H} frame {f}: " + describe_diff(want, g)
            if W > 8 and H > 8 and amount >= 64:  # the launch is no trivial one: frame 0 holds samples of every class of the limit
                d1, mn, mx, c = sharpen_terms(S[0], R[0], amount, clip.bits)
                assert ((c == d1) & (c != 0)).any() and ((c != d1) & (c != 0)).any() and ((c == 0) & (d1 != 0)).any()
            outside = np.ones(got.shape, bool)
            outside[:, :H, d_off:d_off + W] = False
            assert np.array_equal(got.view(np.uint8).reshape(got.shape + (-1,))[outside], dst_h.view(np.uint8).reshape(got.shape + (-1,))[outside]), \
                f"{W}x{H}: bytes outside the planes were written"
            assert np.array_equal(to_host(src).view(np.uint8), src_h.view(np.uint8)), "the source was written"
            assert np.array_equal(to_host(aa).view(np.uint8), aa_h.view(np.uint8)), "the filtered plane was written"


def test_bad_arguments_are_refused_and_nothing_is_queued(hip_lib):
    import torch
    dev = torch.device("cuda:0")
    W, H = 40, 20
    src = torch.zeros((1, H, W), dtype=torch.uint8, device=dev)
    aa = torch.full((1, H, W), 9, dtype=torch.uint8, device=dev)
    dst = torch.full((1, H, W), 0x5C, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    L = capi.load()
    with SangNom2(clip_format("Y8", 64, 32), device=0) as flt:
        def call(amount=64, sp=W, ap=W, dp=W, s=src.data_ptr(), a=aa.data_ptr(), d=dst.data_ptr(), w=W, h=H, n=1):
            return L.sn_contra_sharpen_device(flt._h, amount, n, s, W * H, sp, a, W * H, ap, w, h, d, W * H, dp)
        for kw in (dict(amount=0), dict(amount=256), dict(amount=-1), dict(sp=W - 1), dict(ap=W - 1), dict(dp=W - 1), dict(s=None), dict(a=None),
                   dict(d=None), dict(w=0), dict(h=0), dict(n=-1)):
            assert call(**kw) == capi.SN_ERR_INVALID_ARG, kw
            assert b"sn_contra_sharpen_device" in L.sn_last_error(flt._h)
        flt.synchronize()
        assert np.all(to_host(dst) == 0x5C), "a refused call wrote the destination"
        # dst with the base of aa or of src: refused, and neither plane is written
        assert call(d=aa.data_ptr()) == capi.SN_ERR_INVALID_ARG and b"overlap" in L.sn_last_error(flt._h)
        assert call(d=src.data_ptr()) == capi.SN_ERR_INVALID_ARG and b"overlap" in L.sn_last_error(flt._h)
        flt.synchronize()
        assert np.all(to_host(aa) == 9) and np.all(to_host(src) == 0)
        assert call() == capi.SN_OK  # a constant result comes back as it is
        flt.synchronize()
        assert np.all(to_host(dst) == 9)
    with SangNom2(clip_format("Y16", 64, 32), device=0) as flt:  # pointers and pitches in whole samples
        for s_off, a_off, dp in ((1, 0, W), (0, 1, W), (0, 0, W - 1)):
            assert L.sn_contra_sharpen_device(flt._h, 64, 1, src.data_ptr() + s_off, W * H, W, aa.data_ptr() + a_off, W * H, W, W // 2, H,
                                              dst.data_ptr(), W * H, dp) == capi.SN_ERR_INVALID_ARG
