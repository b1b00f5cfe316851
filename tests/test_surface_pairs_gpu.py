"""Every ordered pair of surface side classes through sn_process_device_surfaces on one small 4:2:2 10-bit clip: planar,
planar-MSB, NV16-like semi-planar and its MSB form, YUYV in LSB 16-bit words, Y210 and v210 -- 49 calls per context, on a
context that processes every plane, one with chroma=False and one with luma=False.

100 x 16: a row of 100 is three 32-pixel vectors and a ragged tail, and 100 mod 6 = 4 leaves v210 a partial group.  Three frames
with order=0 and parities (0, 1, 0): two runs of equal field offset.  Every source carries junk where it must be ignored
(tests/msb_surface_cases.py, tests/packed_surface_cases.py); every destination row is followed by guard bytes that must stay.
A width of 100 is no multiple of 32, so the clip carries history from frame to frame: the context serves its 49 calls one after
the other and ONE oracle instance is fed the same three frames 49 times -- call k has to give the oracle's frames 3 k .. 3 k + 2,
whichever route the frames before them took.  The numpy models of those modules lay them out; tolerance zero.

The three sn_surface_info counters (per call) and scratch_bytes (after the call; a context keeps the union of what its calls
needed, so the order of the pairs matters) are compared with RECORDED: a run of the library that still had one hand-written
walk for calls with a packed side and one for calls without, taken down as it came and not derived from the code under test.
A change there is a change of the launch sequence.  All 147 calls passed on that library too."""
import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2
from oracle.oracle import Oracle
from tests import msb_surface_cases as mc
from tests import packed_surface_cases as pc
from tests import surface_cases as sc
from tests import test_surfaces_gpu as sg  # its device helpers
from tests.util import describe_diff, oracle_cfg, same, to_host

pytestmark = pytest.mark.gpu

SIDES = ("planar", "planar_msb", "nv16", "nv16_msb", "yuyv", "yuyv_msb", "v210")
PAIRS = [(s, d) for s in SIDES for d in SIDES]
C = sc.Case
CONTEXTS = {
    "all": C("YUV422P10", 100, 16, dict(order=0), parities=(0, 1, 0)),
    "chroma_off": C("YUV422P10", 100, 16, dict(order=0, chroma=False), parities=(0, 1, 0)),
    "luma_off": C("YUV422P10", 100, 16, dict(order=0, luma=False, aac=30), parities=(0, 1, 0)),
}
GUARD = 0x5C
GUARD_BYTES = 16  # after every destination row

# per context, in the order of PAIRS: (split_frames, merged_frames, copied_frames) the call added, scratch_bytes after it
RECORDED = {
    "all": [
        ((0, 0, 0), 0), ((0, 0, 0), 0), ((0, 3, 0), 49152), ((0, 3, 0), 49152), ((0, 3, 0), 61440), ((0, 3, 0), 61440), ((0, 3, 0), 61440),  # from planar
        ((0, 0, 0), 73728), ((0, 0, 0), 73728), ((0, 3, 0), 73728), ((0, 3, 0), 73728), ((0, 3, 0), 73728), ((0, 3, 0), 73728), ((0, 3, 0), 73728),  # from planar_msb
        ((3, 0, 0), 73728), ((3, 0, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728),  # from nv16
        ((3, 0, 0), 73728), ((3, 0, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728),  # from nv16_msb
        ((3, 0, 0), 73728), ((3, 0, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728),  # from yuyv
        ((3, 0, 0), 73728), ((3, 0, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728),  # from yuyv_msb
        ((3, 0, 0), 73728), ((3, 0, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728),  # from v210
    ],
    "chroma_off": [
        ((0, 0, 0), 0), ((0, 0, 3), 0), ((0, 0, 3), 0), ((0, 0, 3), 0), ((0, 3, 3), 36864), ((0, 3, 3), 36864), ((0, 3, 3), 36864),  # from planar
        ((0, 0, 3), 49152), ((0, 0, 3), 49152), ((0, 0, 3), 49152), ((0, 0, 3), 49152), ((0, 3, 3), 73728), ((0, 3, 3), 73728), ((0, 3, 3), 73728),  # from planar_msb
        ((0, 0, 3), 73728), ((0, 0, 3), 73728), ((0, 0, 3), 73728), ((0, 0, 3), 73728), ((3, 3, 3), 73728), ((3, 3, 3), 73728), ((3, 3, 3), 73728),  # from nv16
        ((0, 0, 3), 73728), ((0, 0, 3), 73728), ((0, 0, 3), 73728), ((0, 0, 3), 73728), ((3, 3, 3), 73728), ((3, 3, 3), 73728), ((3, 3, 3), 73728),  # from nv16_msb
        ((3, 0, 3), 73728), ((3, 0, 3), 73728), ((3, 3, 3), 73728), ((3, 3, 3), 73728), ((3, 3, 3), 73728), ((3, 3, 3), 73728), ((3, 3, 3), 73728),  # from yuyv
        ((3, 0, 3), 73728), ((3, 0, 3), 73728), ((3, 3, 3), 73728), ((3, 3, 3), 73728), ((3, 3, 3), 73728), ((3, 3, 3), 73728), ((3, 3, 3), 73728),  # from yuyv_msb
        ((3, 0, 3), 73728), ((3, 0, 3), 73728), ((3, 3, 3), 73728), ((3, 3, 3), 73728), ((3, 3, 3), 73728), ((3, 3, 3), 73728), ((3, 3, 3), 73728),  # from v210
    ],
    "luma_off": [
        ((0, 0, 0), 0), ((0, 0, 0), 0), ((0, 3, 0), 49152), ((0, 3, 0), 49152), ((0, 3, 0), 61440), ((0, 3, 0), 61440), ((0, 3, 0), 61440),  # from planar
        ((0, 0, 0), 61440), ((0, 0, 0), 61440), ((0, 3, 0), 61440), ((0, 3, 0), 61440), ((0, 3, 0), 73728), ((0, 3, 0), 73728), ((0, 3, 0), 73728),  # from planar_msb
        ((3, 0, 0), 73728), ((3, 0, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728),  # from nv16
        ((3, 0, 0), 73728), ((3, 0, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728),  # from nv16_msb
        ((3, 0, 0), 73728), ((3, 0, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728),  # from yuyv
        ((3, 0, 0), 73728), ((3, 0, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728),  # from yuyv_msb
        ((3, 0, 0), 73728), ((3, 0, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728), ((3, 3, 0), 73728),  # from v210
    ],
}


def _packed(side):
    return side in pc.LAYOUTS


def _rows(clip, frames, side, source):
    """LSB-aligned planar frames laid out as that side: per tensor of the surface one array [N, H, samples or words per row]."""
    if _packed(side):
        return [np.stack(pc.pack_frames(side, clip, frames, source=source))]
    s = mc.shift_of(clip) if side.endswith("_msb") else 0
    words = (mc.msb_source(frames, s) if source else mc.up(frames, s)) if s else frames
    if side.startswith("nv"):  # nv16, nv16_msb; nv12
        return [np.stack([fr[0] for fr in words]), np.stack([sc.uv_rows(fr[1], fr[2]) for fr in words])]
    return [np.stack([fr[p] for fr in words]) for p in range(3)]


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view({1: np.uint8, 2: np.int16, 4: np.int32}[a.dtype.itemsize])).pin_memory().to(sg._dev())


def _tensors(side, rows):
    """Device tensors over `rows` as process_surfaces takes that side: the UV plane of a semi-planar side as [N, H, Wc, 2]."""
    if side.startswith("nv"):
        return [rows[0], rows[1].unflatten(2, (rows[1].shape[2] // 2, 2))]
    return rows[0] if _packed(side) else rows


def _guarded(want):
    """Per expected array a device allocation with GUARD_BYTES behind every row, all GUARD, and the view of the rows themselves."""
    import torch
    full, views = [], []
    for a in want:
        n, h, r = a.shape
        t = torch.empty((n, h, r + GUARD_BYTES // a.dtype.itemsize), dtype={1: torch.uint8, 2: torch.int16, 4: torch.int32}[a.dtype.itemsize], device=sg._dev())
        t.view(torch.uint8).fill_(GUARD)
        full.append(t)
        views.append(t[:, :, :r])
    return full, views


def _keywords(side):
    return dict(msb=side.endswith("_msb"), packed=pc.order_of(side) if _packed(side) else None)


def walk(name):
    """The 49 calls of one context, each checked byte for byte; yields (src, dst, counters the call added, scratch_bytes)."""
    import torch
    case = CONTEXTS[name]
    clip, frames = sc.frames_of(case)
    par = case.par
    assert sorted(set(par)) == [0, 1] and clip.width % 32 and clip.width % 6 == 4
    sources = {side: _tensors(side, [_up(a) for a in _rows(clip, frames, side, True)]) for side in SIDES}
    ora = Oracle(oracle_cfg(clip, **case.kw))
    with SangNom2(clip, max_batch=case.n, **case.kw) as flt:
        before = (0, 0, 0)
        for src, dst in PAIRS:
            expect = _rows(clip, [ora.process(fr, parity=q) for fr, q in zip(frames, par)], dst, False)
            full, views = _guarded(expect)
            s, d = _keywords(src), _keywords(dst)
            torch.cuda.synchronize()
            flt.process_surfaces(sources[src], _tensors(dst, views), par, src_msb=s["msb"], dst_msb=d["msb"], src_packed=s["packed"],
                                 dst_packed=d["packed"])
            flt.synchronize()
            for k, (a, t) in enumerate(zip(expect, full)):
                got = to_host(t).view(a.dtype)
                r = a.shape[2]
                assert same(a, got[:, :, :r]), f"{name} {src} -> {dst} tensor {k}: " + describe_diff(a, np.ascontiguousarray(got[:, :, :r]))
                assert np.all(np.ascontiguousarray(got[:, :, r:]).view(np.uint8) == GUARD), f"{name} {src} -> {dst} tensor {k}: bytes between rows written"
            i = flt.surface_info()
            now = (i.split_frames, i.merged_frames, i.copied_frames)
            yield src, dst, tuple(b - a for a, b in zip(before, now)), i.scratch_bytes
            before = now
        assert flt.info().frames == len(PAIRS) * case.n


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_every_pair_of_side_classes(hip_lib, name):
    done = list(walk(name))
    assert [(s, d) for s, d, _, _ in done] == PAIRS
    for (src, dst, counters, scratch), recorded in zip(done, RECORDED[name]):
        print(f"{name} {src} -> {dst}: {counters} {scratch}")
        assert (counters, scratch) == recorded, f"{name} {src} -> {dst}: {(counters, scratch)}, recorded {recorded}"
    assert len(RECORDED[name]) == len(PAIRS)
