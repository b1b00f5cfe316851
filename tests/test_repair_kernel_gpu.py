"""sn_repair_device (csrc/sn_repair.hip) against the numpy statement of its contract (tests/repair_model.py), bit for bit (floats
on bit patterns): every sample type, ranks 1..4, the shapes at which the tile indexing can go wrong, aligned surfaces (16 bytes
per lane and access), each of src, aa and dst misaligned by one sample, odd pitches, and in place (dst == aa).  The frames of
one launch are the input patterns of tests/repair_cases.py; their frame strides are larger than the plane, and the destination
is pre-filled with 0x5C: every byte outside the W x H planes must be unchanged afterwards."""
import os
import re

import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2, capi, clip_format
from tests import repair_cases as rc
from tests.repair_model import repair_plane
from tests.util import describe_diff, same, to_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VT = {1: np.uint8, 2: np.int16, 4: np.float32}  # torch has no uint16: same bits


def _tile():
    text = open(os.path.join(ROOT, "avisynth_sangnom2_amd", "csrc", "sn_repair.hip")).read()
    m = re.search(r"kRepairTileBytes = (\d+), kRepairTileH = (\d+);", text)
    return int(m.group(1)), int(m.group(2))


TILE_BYTES, TH = _tile()  # the kernel's output tile: 256 bytes of a row (256 / 128 / 64 samples) x 16 rows

CONTEXTS = ["Y8", "Y10", "Y16", "Y32"]
RANKS = [1, 2, 3, 4]
LAYOUTS = ["aligned", "src_base", "aa_base", "dst_base", "pitches", "inplace"]

_WANT = {}  # (fmt, shape index, rank) -> the model's planes: computed once, shared by the layouts, left unchanged


def _case(clip, fmt, si, W, H, rank):
    key = (fmt, si, rank)
    if key not in _WANT:
        pats = rc.kernel_patterns(clip, W, H, seed=5000 + si)
        _WANT[key] = (pats, [repair_plane(S, R, rank, clip.bits) for S, R in pats])
    return _WANT[key]


def _surface(planes, fill, base_off, odd_pitch, W, H, B):
    """[N, H + 2, pitch] of fill bytes with the planes at [:, :H, base_off:base_off + W]; pitch * B a multiple of 16 unless odd_pitch."""
    pitch = (W + 3 + 15) // 16 * 16 + (1 if odd_pitch else 0)
    big = np.full((len(planes), H + 2, pitch * B), fill, np.uint8).view(planes[0].dtype)
    for f, pl in enumerate(planes):
        big[f, :H, base_off:base_off + W] = pl
    return big


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("fmt", CONTEXTS)
def test_repair_device_matches_the_model(hip_lib, fmt, rank, layout):
    import torch
    dev = torch.device("cuda:0")
    clip = clip_format(fmt, 64, 32)  # the context gives the sample type; its own size plays no part
    B = clip.bytes
    with SangNom2(clip, device=0) as flt:
        for si, (W, H) in enumerate(rc.kernel_shapes(B, TILE_BYTES, TH)):
            pats, want = _case(clip, fmt, si, W, H, rank)
            S, R = [p[0] for p in pats], [p[1] for p in pats]
            N = len(S)
            inplace = layout == "inplace"
            s_off, a_off, d_off = (1 if layout == k else 0 for k in ("src_base", "aa_base", "dst_base"))
            odd = layout == "pitches"
            src_h = _surface(S, 0x11, s_off, odd, W, H, B)
            aa_h = _surface(R, 0x5C if inplace else 0x22, a_off, odd, W, H, B)
            dst_h = _surface([np.zeros((H, W), R[0].dtype)] * N, 0x5C, d_off, odd, W, H, B)
            dst_h.view(np.uint8)[...] = 0x5C
            src = torch.from_numpy(src_h.view(VT[B])).pin_memory().to(dev)
            aa = torch.from_numpy(aa_h.view(VT[B])).pin_memory().to(dev)
            dst = aa if inplace else torch.from_numpy(dst_h.view(VT[B])).pin_memory().to(dev)
            views = [src[:, :H, s_off:s_off + W], aa[:, :H, a_off:a_off + W], dst[:, :H, d_off:d_off + W]]
            aligned = [all(v % 16 == 0 for v in (t.data_ptr(), t.stride(0) * B, t.stride(1) * B)) for t in views]
            assert aligned == [layout not in ("src_base", "pitches"), layout not in ("aa_base", "pitches"), layout not in ("dst_base", "pitches")]
            torch.cuda.synchronize()
            flt.repair(views[0], views[1], views[2], rank)
            flt.synchronize()
            got = to_host(dst).view(R[0].dtype)
            for f in range(N):
                g = got[f, :H, d_off:d_off + W]
                assert same(want[f], g), f"{W}x{H} frame {f}: " + describe_diff(want[f], g)
            if W > 8 and H > 8:  # the launch is no trivial one: frame 0 holds samples below, above and within the bounds
                below, above, inside = rc.classes(S[0], R[0], rank)
                assert below > 0 and above > 0 and inside > 0
                assert not same(want[0], R[0])
            outside = np.ones(got.shape, bool)
            outside[:, :H, d_off:d_off + W] = False
            before = aa_h if inplace else dst_h
            assert np.array_equal(got.view(np.uint8).reshape(got.shape + (-1,))[outside], before.view(np.uint8).reshape(got.shape + (-1,))[outside]), \
                f"{W}x{H}: bytes outside the planes were written"
            assert np.array_equal(to_host(src).view(np.uint8), src_h.view(np.uint8)), "the source was written"
            if not inplace:
                assert np.array_equal(to_host(aa).view(np.uint8), aa_h.view(np.uint8)), "the filtered plane was written"


def test_bad_arguments_are_refused_and_nothing_is_queued(hip_lib):
    import torch
    dev = torch.device("cuda:0")
    W, H = 40, 20
    src = torch.full((2, H, W), 9, dtype=torch.uint8, device=dev)
    aa = torch.full((2, H, W), 9, dtype=torch.uint8, device=dev)
    dst = torch.full((2, H, W), 0x5C, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    L = capi.load()
    with SangNom2(clip_format("Y8", 64, 32), device=0) as flt:
        def call(rank=2, sp=W, ap=W, dp=W, s=src.data_ptr(), a=aa.data_ptr(), d=dst.data_ptr(), w=W, h=H, n=1, afs=W * H, dfs=W * H):
            return L.sn_repair_device(flt._h, rank, n, s, W * H, sp, a, afs, ap, w, h, d, dfs, dp)
        for kw in (dict(rank=0), dict(rank=5), dict(rank=-1), dict(sp=W - 1), dict(ap=W - 1), dict(dp=W - 1), dict(s=None), dict(a=None),
                   dict(d=None), dict(w=0), dict(h=0), dict(n=-1)):
            assert call(**kw) == capi.SN_ERR_INVALID_ARG, kw
            assert b"sn_repair_device" in L.sn_last_error(flt._h)
        # dst on src, dst partly on src, dst partly on aa (one row down; one frame on), dst on aa with another pitch or frame stride
        for kw in (dict(d=src.data_ptr()), dict(d=src.data_ptr() + W), dict(d=aa.data_ptr() + W), dict(d=aa.data_ptr() + 1, w=W - 1),
                   dict(d=aa.data_ptr() + W * H, n=2), dict(d=aa.data_ptr(), dp=2 * W, h=H // 2), dict(d=aa.data_ptr(), n=2, dfs=W * H // 2, h=H // 2, afs=W * H)):
            assert call(**kw) == capi.SN_ERR_INVALID_ARG, kw
            assert b"overlap" in L.sn_last_error(flt._h), (kw, L.sn_last_error(flt._h))
        flt.synchronize()
        assert np.all(to_host(dst) == 0x5C) and np.all(to_host(aa) == 9) and np.all(to_host(src) == 9), "a refused call wrote a plane"
        assert call() == capi.SN_OK  # a constant result equal to the source comes back as it is
        assert call(d=aa.data_ptr()) == capi.SN_OK  # ... and in place
        assert call(n=0) == capi.SN_OK
        flt.synchronize()
        assert np.all(to_host(dst[0]) == 9) and np.all(to_host(dst[1]) == 0x5C) and np.all(to_host(aa) == 9)
    with SangNom2(clip_format("Y16", 64, 32), device=0) as flt:  # pointers and pitches in whole samples
        for s_off, a_off, dp in ((1, 0, W), (0, 1, W), (0, 0, W - 1)):
            assert L.sn_repair_device(flt._h, 1, 1, src.data_ptr() + s_off, W * H, W, aa.data_ptr() + a_off, W * H, W, W // 2, H,
                                      dst.data_ptr(), W * H, dp) == capi.SN_ERR_INVALID_ARG
