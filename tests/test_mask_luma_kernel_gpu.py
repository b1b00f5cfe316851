"""sn_mask_merge_luma_device (csrc/sn_mask.hip) against the numpy statement of its contract (tests/mask_luma_model.py), bit for
bit: every sample type, with and without the expansion, one chroma plane and two, the chroma shapes at which the tile
indexing can go wrong, all nine subsamplings, aligned surfaces (16 bytes per lane and access), each of luma, src, aa and dst
misaligned by one sample, odd pitches, U and V with different pitches, and dst in place on aa.  The frames of one launch are
the input patterns; their frame strides are larger than the plane, and the destinations are pre-filled with 0x5C: every byte
outside the W x H planes must be unchanged afterwards, and so must luma and the sources.  aa = NULL writes the reduced mask."""
import ctypes
import os
import re

import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2, capi, clip_format, synth
from tests.mask_luma_model import chroma_mask, mask_plane_luma, merge_plane_luma
from tests.util import describe_diff, same, to_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VT = {1: np.uint8, 2: np.int16, 4: np.float32}  # torch has no uint16: same bits
LO, HI = 40, 96
SEED = 3 * 307  # the plane seed of tests/mask_luma_cases.py's first luma plane: stripes of slope 1


def _tile():
    text = open(os.path.join(ROOT, "avisynth_sangnom2_amd", "csrc", "sn_mask.hip")).read()
    m = re.search(r"kMaskTileBytes = (\d+), kMaskTileH = (\d+);", text)
    return int(m.group(1)), int(m.group(2))


TILE_BYTES, TH = _tile()  # the kernel's LUMA tile: 256 bytes of a row (256 / 128 / 64 samples) x 16 rows

CONTEXTS = ["Y8", "Y10", "Y16", "Y32"]
SUBS = [(sw, sh) for sw in range(3) for sh in range(3)]
LAYOUTS = ["aligned", "luma_base", "src_base", "aa_base", "dst_base", "pitches", "in_place", "uv_pitches"]


def _shapes(B, sw=1, sh=1):
    """Chroma (W, H): planes narrower than a block row; one less than the chroma tile, the tile and one more in each direction;
    two tiles each way plus a ragged rest."""
    TW, T_H = (TILE_BYTES // B) >> sw, TH >> sh
    return [(1, 1), (2, 3), (3, 2), (TW - 1, T_H), (TW, T_H), (TW + 1, T_H), (TW, T_H - 1), (TW, T_H + 1), (2 * TW + 11, 2 * T_H + 3)]


def _luma_inputs(clip, W, H):
    """The luma frames of one launch [H, W]: edges (mc = 0 and the ramp; mc = 256 where the blocks are small), full-range noise
    (m_L is 256 on most samples, but without the expansion only about one block of eight samples in a hundred is 256
    throughout), vertical stripes two samples wide (0 0 max max: |gx| = 4 max in every column but the plane's first and, where the
    clamp repeats its neighbour, last, so m_L = mc = 256 nearly everywhere, whatever the block), a constant, the one-pixel checker, and for float a constant plane with NaN and infinities in it,
    alone, side by side and on the plane's edges."""
    rng = np.random.default_rng(SEED + W * 7 + H)
    y, x = np.mgrid[0:H, 0:W]
    two = (x >> 1) & 1
    if clip.bytes == 4:
        f = np.float32
        out = [synth.plane(H, W, 4, 32, "edges", SEED), (rng.random((H, W), dtype=f) * f(2) - f(1)).astype(f), two.astype(f), np.full((H, W), 0.3, f),
               ((x + y) & 1).astype(f)]
        sp = np.full((H, W), 0.5, f)
        for k, v in enumerate([np.nan, np.inf, -np.inf, np.nan, np.inf, np.inf]):
            sp[(k * 7) % H, (k * 29 + (k > 3)) % W] = v
        sp[H - 1, W - 1] = np.inf
        sp[0, W // 2] = np.nan
        out.append(sp)
        return out
    mx = (1 << clip.bits) - 1
    return [synth.plane(H, W, clip.bytes, clip.bits, "edges", SEED), rng.integers(0, mx + 1, (H, W)).astype(clip.dtype), (two * mx).astype(clip.dtype),
            np.full((H, W), mx // 3, clip.dtype), (((x + y) & 1) * mx).astype(clip.dtype)]


def _random(clip, W, H, N, seed):
    rng = np.random.default_rng(seed)
    if clip.bytes == 4:
        return [rng.random((H, W), dtype=np.float32) for _ in range(N)]
    return [rng.integers(0, 1 << clip.bits, (H, W)).astype(clip.dtype) for _ in range(N)]


def _surface(planes, fill, base_off, extra_pitch, W, H, B):
    """[N, H + 2, pitch] of fill bytes with the planes at [:, :H, base_off:base_off + W]; pitch * B a multiple of 16 plus extra_pitch samples."""
    pitch = (W + 3 + 15) // 16 * 16 + extra_pitch
    big = np.full((len(planes), H + 2, pitch * B), fill, np.uint8).view(planes[0].dtype)
    for f, pl in enumerate(planes):
        big[f, :H, base_off:base_off + W] = pl
    return big


def _dev(a, B):
    import torch
    return torch.from_numpy(a.view(VT[B])).pin_memory().to(torch.device("cuda:0"))


def _assert_classes(clip, L, expand, sw, sh, what):
    """Over the frames of a launch, each class of mc reaches 5 % in at least one frame."""
    best = [0.0, 0.0, 0.0]
    for Lf in L:
        mc = chroma_mask(Lf, LO, HI, expand, clip.bits, sw, sh)
        for k, c in enumerate(((mc == 0).mean(), ((mc > 0) & (mc < 256)).mean(), (mc == 256).mean())):
            best[k] = max(best[k], float(c))
    assert min(best) >= 0.05, f"{what}: the launch's best shares of mc = 0 / ramp / 256 are {best}"


def _launch(flt, clip, W, H, sw, sh, expand, planes, layout, seed, merge=True):
    """One launch on every input pattern; asserts the result, the bytes outside the planes, and that no input was written."""
    B = clip.bytes
    Wl, Hl = W << sw, H << sh
    L = _luma_inputs(clip, Wl, Hl)
    N = len(L)
    S = [_random(clip, W, H, N, seed + 10 * p) for p in range(planes)]
    R = [_random(clip, W, H, N, seed + 10 * p + 5) for p in range(planes)]
    off = {k: (1 if layout == k else 0) for k in ("luma_base", "src_base", "aa_base", "dst_base")}
    extra = [1, 1] if layout == "pitches" else [0, 16 // B] if layout == "uv_pitches" else [0, 0]
    luma_h = _surface(L, 0x22, off["luma_base"], extra[0], Wl, Hl, B)
    luma = _dev(luma_h, B)
    src_h = [_surface(S[p], 0x11, off["src_base"], extra[p], W, H, B) for p in range(planes)]
    aa_h = [_surface(R[p], 0x5C, off["aa_base"], extra[p], W, H, B) for p in range(planes)]
    dst_h = []
    for p in range(planes):
        d = _surface([np.zeros((H, W), clip.dtype)] * N, 0x5C, off["dst_base"], extra[p], W, H, B)
        d.view(np.uint8)[...] = 0x5C
        dst_h.append(d)
    src = [_dev(a, B) for a in src_h]
    aa = [_dev(a, B) for a in aa_h]
    in_place = layout == "in_place" and merge
    dst = aa if in_place else [_dev(a, B) for a in dst_h]
    before = aa_h if in_place else dst_h
    d_off = off["aa_base"] if in_place else off["dst_base"]
    lv = luma[:, :Hl, off["luma_base"]:off["luma_base"] + Wl]
    sv = [t[:, :H, off["src_base"]:off["src_base"] + W] for t in src]
    av = [t[:, :H, off["aa_base"]:off["aa_base"] + W] for t in aa]
    dv = [t[:, :H, d_off:d_off + W] for t in dst]
    if layout in ("aligned", "in_place", "uv_pitches"):
        assert all(v % 16 == 0 for t in [lv] + sv + av + dv for v in (t.data_ptr(), t.stride(0) * B, t.stride(1) * B))
    if layout == "uv_pitches":
        assert sv[0].stride(1) != sv[1].stride(1) and dv[0].stride(1) != dv[1].stride(1)
    import torch
    torch.cuda.synchronize()
    one = planes == 1
    flt.mask_merge_luma(lv, sv[0] if one else sv, (av[0] if one else av) if merge else None, dv[0] if one else dv, LO, HI, expand, sw, sh)
    flt.synchronize()
    what = f"{W}x{H} sub ({sw}, {sh}) {layout}"
    for p in range(planes):
        got = to_host(dst[p]).view(clip.dtype)
        for f in range(N):
            want = merge_plane_luma(L[f], S[p][f], R[p][f], LO, HI, expand, clip.bits, sw, sh) if merge else \
                mask_plane_luma(L[f], LO, HI, expand, clip.bits, sw, sh)
            g = got[f, :H, d_off:d_off + W]
            assert same(want, g), f"{what} plane {p} frame {f}: " + describe_diff(want, g)
        outside = np.ones(got.shape, bool)
        outside[:, :H, d_off:d_off + W] = False
        assert np.array_equal(got.view(np.uint8).reshape(got.shape + (-1,))[outside], before[p].view(np.uint8).reshape(got.shape + (-1,))[outside]), \
            f"{what} plane {p}: bytes outside the planes were written"
        assert np.array_equal(to_host(src[p]).view(np.uint8), src_h[p].view(np.uint8)), "a source was written"
        if not in_place:
            assert np.array_equal(to_host(aa[p]).view(np.uint8), aa_h[p].view(np.uint8)), "a result plane was written"
    assert np.array_equal(to_host(luma).view(np.uint8), luma_h.view(np.uint8)), "luma was written"
    return L


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("expand", [0, 1])
@pytest.mark.parametrize("fmt", CONTEXTS)
def test_the_shapes_at_420(hip_lib, fmt, expand, planes):
    clip = clip_format(fmt, 64, 32)  # the context gives the sample type and the bit depth; its own size plays no part
    with SangNom2(clip, device=0) as flt:
        for si, (W, H) in enumerate(_shapes(clip.bytes)):
            L = _launch(flt, clip, W, H, 1, 1, expand, planes, "aligned", 4000 + si)
            if W > 8 and H > 8:
                _assert_classes(clip, L, expand, 1, 1, f"{W}x{H}")


@pytest.mark.parametrize("sub", SUBS, ids=[f"sub{sw}{sh}" for sw, sh in SUBS])
@pytest.mark.parametrize("expand", [0, 1])
@pytest.mark.parametrize("fmt", CONTEXTS)
def test_all_nine_subsamplings(hip_lib, fmt, expand, sub):
    """Two planes; chroma 70 x 37 and 257 x 17 (8-bit: one and two luma tiles across without subsampling, two and five at
    sub_w = 2), and the chroma tile of this subsampling plus one each way."""
    sw, sh = sub
    clip = clip_format(fmt, 64, 32)
    TW, T_H = (TILE_BYTES // clip.bytes) >> sw, TH >> sh
    with SangNom2(clip, device=0) as flt:
        for si, (W, H) in enumerate([(70, 37), (257, 17), (TW + 1, T_H + 1)]):
            L = _launch(flt, clip, W, H, sw, sh, expand, 2, "aligned", 5000 + si)
            _assert_classes(clip, L, expand, sw, sh, f"{W}x{H} sub ({sw}, {sh})")


@pytest.mark.parametrize("layout", LAYOUTS[1:])
@pytest.mark.parametrize("expand", [0, 1])
@pytest.mark.parametrize("fmt", CONTEXTS)
def test_the_layouts_at_420(hip_lib, fmt, expand, layout):
    clip = clip_format(fmt, 64, 32)
    TW, T_H = (TILE_BYTES // clip.bytes) >> 1, TH >> 1
    with SangNom2(clip, device=0) as flt:
        for si, (W, H) in enumerate([(3, 2), (TW + 1, T_H + 1), (2 * TW + 11, 2 * T_H + 3)]):
            L = _launch(flt, clip, W, H, 1, 1, expand, 2, layout, 6000 + si)
            if W > 8:
                _assert_classes(clip, L, expand, 1, 1, f"{W}x{H} {layout}")


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("expand", [0, 1])
@pytest.mark.parametrize("fmt", CONTEXTS)
def test_without_a_result_the_reduced_mask_is_written(hip_lib, fmt, expand, planes):
    clip = clip_format(fmt, 64, 32)
    with SangNom2(clip, device=0) as flt:
        for si, (W, H) in enumerate(_shapes(clip.bytes)[2:]):
            _launch(flt, clip, W, H, 1, 1, expand, planes, "aligned", 7000 + si, merge=False)
        _launch(flt, clip, 70, 37, 2, 0, expand, planes, "dst_base", 7100, merge=False)


def test_equal_and_extreme_thresholds(hip_lib):
    """lo = hi (no ramp in m_L; the block mean still gives values between), (0, 0), (255, 255) and (0, 255) on 8-bit, 16-bit and float."""
    import torch
    dev = torch.device("cuda:0")
    for fmt in ("Y8", "Y16", "Y32"):
        clip = clip_format(fmt, 64, 32)
        W, H = 150, 37
        L = synth.plane(2 * H, 2 * W, clip.bytes, clip.bits, "edges", SEED)
        S, R = _random(clip, W, H, 1, 77)[0], _random(clip, W, H, 1, 9)[0]
        luma, src, aa = (torch.from_numpy(a[None].view(VT[clip.bytes])).pin_memory().to(dev) for a in (L, S, R))
        with SangNom2(clip, device=0) as flt:
            for lo, hi in ((40, 40), (0, 0), (255, 255), (0, 255), (39, 40)):
                for expand in (0, 1):
                    dst = torch.zeros_like(aa)
                    torch.cuda.synchronize()
                    flt.mask_merge_luma(luma, src, aa, dst, lo, hi, expand)
                    flt.synchronize()
                    want = merge_plane_luma(L, S, R, lo, hi, expand, clip.bits, 1, 1)
                    got = to_host(dst).view(clip.dtype)[0]
                    assert same(want, got), f"{fmt} lo {lo} hi {hi} expand {expand}: " + describe_diff(want, got)


def test_bad_arguments_are_refused_and_nothing_is_queued(hip_lib):
    import torch
    dev = torch.device("cuda:0")
    W, H = 40, 20
    luma = torch.zeros((1, 2 * H, 2 * W), dtype=torch.uint8, device=dev)
    src = [torch.zeros((1, H, W), dtype=torch.uint8, device=dev) for _ in range(2)]
    aa = [torch.full((1, H, W), 9, dtype=torch.uint8, device=dev) for _ in range(2)]
    dst = [torch.full((1, H, W), 0x5C, dtype=torch.uint8, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    Lb = capi.load()
    size = ctypes.sizeof(capi.SnAAMask)
    P, I64, I32 = ctypes.c_void_p * 2, ctypes.c_int64 * 2, ctypes.c_int32 * 2
    ptrs = lambda ts: [t.data_ptr() for t in ts]
    with SangNom2(clip_format("Y8", 64, 32), device=0) as flt:
        def call(lp=2 * W, sub_w=1, sub_h=1, l=luma.data_ptr(), s=ptrs(src), a=ptrs(aa), d=ptrs(dst), sp=(W, W), ap=(W, W), dp=(W, W), w=W, h=H,
                 no_aa=False, **mkw):
            m = capi.SnAAMask(**dict(dict(struct_size=size, kind=1, lo=16, hi=96, expand=1), **mkw))
            fs = I64(W * H, W * H)
            return Lb.sn_mask_merge_luma_device(flt._h, ctypes.byref(m), 1, l, 4 * W * H, lp, sub_w, sub_h, P(*s), fs, I32(*sp),
                                                None if no_aa else P(*a), fs, I32(*ap), w, h, P(*d), fs, I32(*dp))
        bad = (dict(lo=-1), dict(hi=256), dict(lo=97), dict(expand=2), dict(kind=0), dict(kind=2), dict(struct_size=size - 4), dict(lp=2 * W - 1),
               dict(sp=(W - 1, W)), dict(sp=(W, W - 1)), dict(ap=(W, W - 1)), dict(dp=(W - 1, W)), dict(l=None), dict(s=[None, src[1].data_ptr()]),
               dict(d=[None, dst[1].data_ptr()]), dict(w=0), dict(h=0), dict(sub_w=3), dict(sub_w=-1), dict(sub_h=3), dict(sub_h=-1),
               dict(s=[src[0].data_ptr(), None]),                        # one plane: dst[1] and aa[1] must be NULL too
               dict(s=[src[0].data_ptr(), None], d=[dst[0].data_ptr(), None]),
               dict(d=[dst[0].data_ptr(), None]),                        # two planes need dst[1]
               dict(a=[aa[0].data_ptr(), None]), dict(a=[None, aa[1].data_ptr()]))  # aa: all planes or none
        for kw in bad:
            assert call(**kw) == capi.SN_ERR_INVALID_ARG, kw
            assert b"sn_mask_merge_luma_device" in Lb.sn_last_error(flt._h), kw
        m = capi.SnAAMask(struct_size=size, kind=1, lo=16, hi=96, expand=1)
        m.reserved[2] = 1
        fs = I64(W * H, W * H)
        assert Lb.sn_mask_merge_luma_device(flt._h, ctypes.byref(m), 1, luma.data_ptr(), 4 * W * H, 2 * W, 1, 1, P(*ptrs(src)), fs, I32(W, W),
                                            P(*ptrs(aa)), fs, I32(W, W), W, H, P(*ptrs(dst)), fs, I32(W, W)) == capi.SN_ERR_INVALID_ARG
        flt.synchronize()
        assert all(np.all(to_host(t) == 0x5C) for t in dst), "a refused call wrote a destination"
        assert call() == capi.SN_OK  # a constant luma plane: the mask is empty and dst is the source
        assert call(s=[src[0].data_ptr(), None], a=[aa[0].data_ptr(), None], d=[dst[0].data_ptr(), None]) == capi.SN_OK  # one plane
        flt.synchronize()
        assert all(np.all(to_host(t) == 0) for t in dst)
        assert call(no_aa=True) == capi.SN_OK and call(a=[None, None]) == capi.SN_OK  # the mask of a constant plane
        flt.synchronize()
        assert all(np.all(to_host(t) == 0) for t in dst)
    with SangNom2(clip_format("Y16", 64, 32), device=0) as flt:  # pointers and pitches in whole samples
        m = capi.SnAAMask(struct_size=size, kind=1, lo=16, hi=96, expand=1)
        fs = I64(W * H, W * H)
        for l_off, s_off, dp in ((1, 0, W), (0, 1, W), (0, 0, W - 1)):
            assert Lb.sn_mask_merge_luma_device(flt._h, ctypes.byref(m), 1, luma.data_ptr() + l_off, 4 * W * H, 2 * W, 1, 1,
                                                P(src[0].data_ptr() + s_off, src[1].data_ptr()), fs, I32(W, W), P(*ptrs(aa)), fs, I32(W, W), W // 2, H,
                                                P(*ptrs(dst)), fs, I32(W, dp)) == capi.SN_ERR_INVALID_ARG
