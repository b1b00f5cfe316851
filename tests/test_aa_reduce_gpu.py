"""The anti-aliasing call with dh and a reduction (sn_aa_options.reduce): the frame comes back at source size.  Every entry
point against reduce_model(Script(...).frame(...)) -- the dh script of tests/aa_dh_script.py followed by the numpy statement
of the reduction (tests/reduce_model.py) -- bit for bit: device batches, strides, chunks, the host call and ring, pinned
destinations, and semi-planar and packed destinations with rows for W."""
import ctypes

import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNomAA, SangNomAAHost, SangNomError, capi, clip_format, synth
from avisynth_sangnom2_amd.filter import pin_host_array, unpin_host_array
from tests import packed_surface_cases as pc
from tests.aa_dh_script import Script
from tests.reduce_model import reduce_model, reduce_unclamped
from tests.util import describe_diff, same, to_host

pytestmark = pytest.mark.gpu

VT = {1: np.uint8, 2: np.int16, 4: np.float32}  # torch has no uint16: same bits
KERNELS = ["tent", "halfband"]


def _assert_frame(want, got, what):
    for p, (a, b) in enumerate(zip(want, got)):
        assert a.shape == b.shape, f"{what} plane {p}: shape {b.shape}, expected {a.shape}"
        assert same(a, b), f"{what} plane {p}: " + describe_diff(a, b)


def _to_dev(clip, frames):
    import torch
    dev = torch.device("cuda:0")
    return [torch.from_numpy(np.stack([fr[p] for fr in frames]).view(VT[clip.bytes])).pin_memory().to(dev) for p in range(clip.planes)]


def _batch(aa, clip, frames, parity=None):
    import torch
    src = _to_dev(clip, frames)
    dst = [torch.zeros((len(frames),) + aa.plane_shape_out(p), dtype=src[p].dtype, device=src[p].device) for p in range(clip.planes)]
    torch.cuda.synchronize()
    aa.process_batch(src, dst, parity)
    aa.synchronize()
    return [[to_host(dst[p][f]).view(clip.dtype) for p in range(clip.planes)] for f in range(len(frames))]


# (format, width, height, filter kwargs, context kwargs, script kwargs, pattern, parities of the first call)
BATCH = [
    ("Y8", 128, 64, {}, {}, {}, "noise", None),
    ("Y8", 96, 80, {}, {}, {}, "noise", None),                      # history in the turned pass
    ("Y8", 40, 96, {}, {}, {}, "noise", None),                      # history in the second pass
    ("Y8", 200, 136, {}, {}, {}, "noise", None),                    # ragged turn and reduce tiles
    ("Y32", 132, 66, {}, {}, {}, "noise", None),
    ("Y16", 96, 64, dict(order=2), {}, {}, "noise", None),
    ("Y10", 64, 48, {}, {}, {}, "checker", None),                   # the half-band kernel clamps at 1023
    ("YUV420P8", 128, 64, dict(aac=48), {}, {}, "noise", None),
    ("YUV422P8", 128, 64, dict(aac=48), {}, {}, "noise", None),
    ("YUV444PS", 64, 32, {}, {}, {}, "noise", None),
    ("Y8", 128, 64, dict(order=0), {}, {}, "noise", [1, 0, 0, 1, 1]),
    ("Y8", 128, 64, {}, dict(opt=1), dict(opt=1), "noise01", None),
    ("YUV420P8", 128, 64, dict(aac=48), dict(opt=1), dict(opt=1), "noise01", None),
    ("YUV420P8", 128, 64, dict(luma=False, aac=48), {}, {}, "noise", None),  # planes are forced
]

_E = {}     # case index -> (frames, parities, the dh script's frames): computed once, left unchanged
_WANT = {}  # (case index, kernel) -> the reduced frames


def _expected(i, kernel):
    if i not in _E:
        fmt, w, h, kw, ckw, skw, pattern, par = BATCH[i]
        clip = clip_format(fmt, w, h)
        frames = [synth.frame(clip, pattern, seed=300 + f) for f in range(8)]
        parities = (par or [1] * 5) + [1, 1, 1]
        script = Script(clip, **kw, **skw)
        _E[i] = (frames, parities, [script.frame(fr, parity=parities[f]) for f, fr in enumerate(frames)])
    if (i, kernel) not in _WANT:
        fmt, w, h, kw = BATCH[i][:4]
        clip = clip_format(fmt, w, h)
        frames, parities, E = _E[i]
        _WANT[(i, kernel)] = [reduce_model(E[f], kernel, order=kw.get("order", 1), parity=parities[f], bits=clip.bits) for f in range(8)]
    return _E[i][0], _E[i][1], _WANT[(i, kernel)]


@pytest.mark.parametrize("small", ["sweep", "auto"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("i", range(len(BATCH)), ids=[f"{c[0]}-{c[1]}x{c[2]}-{i}" for i, c in enumerate(BATCH)])
def test_batches_match_the_reduced_script(hip_lib, i, kernel, small):
    """Five frames in one call, then three more on the same context."""
    fmt, w, h, kw, ckw, skw, pattern, par = BATCH[i]
    clip = clip_format(fmt, w, h)
    frames, parities, want = _expected(i, kernel)
    if fmt == "Y10" and kernel == "halfband":
        E = _E[i][2][0][0]
        assert ((reduce_unclamped(E, "halfband", 1, 0) + 512) >> 10).max() > 1023, "the case does not reach the clamp"
    sl = capi.SN_SMALL_SWEEP if small == "sweep" else capi.SN_SMALL_AUTO
    with SangNomAA(clip, max_batch=5, small_launches=sl, dh=True, reduce=kernel, **kw, **ckw) as aa:
        assert capi.load().sn_aa_get_reduce(aa._h) == capi.REDUCE_KERNELS[kernel]
        assert all(aa.plane_shape_out(p) == aa.plane_shape(p) for p in range(clip.planes))
        assert aa.info(1).pool_stride >= 2 * w  # the second pass still runs on the 2W clip
        got = _batch(aa, clip, frames[:5], parities[:5] if par else None) + _batch(aa, clip, frames[5:])
    for f in range(8):
        _assert_frame(want[f], got[f], f"frame {f}")


@pytest.mark.parametrize("kernel", KERNELS)
def test_strides_and_pitches(hip_lib, kernel):
    """Pitches larger than the row, frame strides larger than the plane, destination pre-filled: nothing outside the W x H planes
    is written; a destination pitch below W * B is refused; a 2W-sized destination tensor is refused by the Python shape check."""
    import torch
    clip = clip_format("YUV420P8", 128, 64)
    N = 4
    frames = [synth.frame(clip, "noise", seed=520 + i) for i in range(N)]
    script = Script(clip, aac=48)
    want = [reduce_model(script.frame(fr), kernel) for fr in frames]
    dev = torch.device("cuda:0")
    src, dst, before = [], [], []
    for p in range(3):
        hp, wp = frames[0][p].shape
        big = np.full((N, hp + 3, wp + 40), 0x11, np.uint8)
        for f in range(N):
            big[f, :hp, :wp] = frames[f][p]
        src.append(torch.from_numpy(big).pin_memory().to(dev)[:, :hp, :wp])
        fill = np.full((N, hp + 5, wp + 23), 0x5C, np.uint8)
        before.append(fill)
        dst.append(torch.from_numpy(fill.copy()).pin_memory().to(dev))
    torch.cuda.synchronize()
    with SangNomAA(clip, max_batch=N, aac=48, dh=True, reduce=kernel) as aa:
        aa.process_batch(src, [d[:, :s.shape[1], :s.shape[2]] for d, s in zip(dst, src)])
        aa.synchronize()
        L = capi.load()
        sp, dp = (ctypes.c_void_p * 3)(), (ctypes.c_void_p * 3)()
        spi, dpi = (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 3)()
        sfs, dfs = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
        for p in range(3):
            sp[p], dp[p] = src[p].data_ptr(), dst[p].data_ptr()
            spi[p], sfs[p] = src[p].stride(1), src[p].stride(0)
            dpi[p], dfs[p] = src[p].shape[2] - 1, dst[p].stride(0)
        assert L.sn_aa_process_device_strided(aa._h, N, sp, sfs, spi, dp, dfs, dpi, None) == capi.SN_ERR_INVALID_ARG
        aa.synchronize()
        with pytest.raises(ValueError):
            aa.process_batch(src, [torch.zeros((N, 2 * s.shape[1], 2 * s.shape[2]), dtype=torch.uint8, device=dev) for s in src])
    for p in range(3):
        hp, wp = frames[0][p].shape
        got = to_host(dst[p])
        for f in range(N):
            assert same(want[f][p], got[f, :hp, :wp]), f"frame {f} plane {p}: " + describe_diff(want[f][p], got[f, :hp, :wp])
        outside = np.ones(got.shape, bool)
        outside[:, :hp, :wp] = False
        assert np.array_equal(got[outside], before[p][outside]), f"plane {p}: bytes outside the plane were written"


def test_a_tiny_scratch_budget_walks_a_batch_in_chunks(hip_lib):
    """Y8 512x256 with dh and reduce: 131 072 + 2 x 262 144 + 524 288 = 1 179 648 bytes of intermediates per frame (the last
    term is E), so a budget of 2 MB holds one frame and a batch of five takes five chunks."""
    clip = clip_format("Y8", 512, 256)
    frames = [synth.frame(clip, "noise", seed=700 + i) for i in range(5)]
    with SangNomAA(clip, max_batch=5, dh=True, reduce="halfband") as aa:
        one = _batch(aa, clip, frames)
    with SangNomAA(clip, max_batch=5, scratch_budget_mb=2, dh=True, reduce="halfband") as aa:
        chunked = _batch(aa, clip, frames)
    script = Script(clip)
    for f in range(5):
        _assert_frame(one[f], chunked[f], f"frame {f} (chunked against one chunk)")
        if f < 2:
            _assert_frame(reduce_model(script.frame(frames[f]), "halfband"), chunked[f], f"frame {f} (script)")


HOST = [("Y8", 128, 64, {}), ("YUV420P8", 128, 64, dict(aac=48)), ("Y16", 96, 64, {})]
_HOST_WANT = {}


def _host_expected(i, kernel):
    if (i, kernel) not in _HOST_WANT:
        fmt, w, h, kw = HOST[i]
        clip = clip_format(fmt, w, h)
        if i not in _HOST_WANT:
            frames = [synth.frame(clip, "noise", seed=40 + f) for f in range(7)]
            script = Script(clip, **kw)
            _HOST_WANT[i] = (frames, [script.frame(fr) for fr in frames])
        frames, E = _HOST_WANT[i]
        _HOST_WANT[(i, kernel)] = (frames, [reduce_model(e, kernel, bits=clip.bits) for e in E])
    return _HOST_WANT[(i, kernel)]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("i", range(len(HOST)), ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in HOST])
def test_the_host_call_and_the_ring(hip_lib, i, kernel):
    """get_frame, then the ring: submit and collect, depth 4, 7 frames; frames of source size come down."""
    fmt, w, h, kw = HOST[i]
    clip = clip_format(fmt, w, h)
    frames, want = _host_expected(i, kernel)
    with SangNomAAHost(clip, host_depth=4, dh=True, reduce=kernel, **kw) as ring, SangNomAAHost(clip, dh=True, reduce=kernel, **kw) as sync:
        for k in range(2):
            _assert_frame(want[k], sync.get_frame(frames[k]), f"get_frame {k}")
        n = ring.slots()
        assert 1 <= n <= 4
        got, pending, f = [], [], 0
        while len(got) < len(frames):
            while f < len(frames) and len(pending) < n:
                pending.append(ring.submit(frames[f]))
                f += 1
            got.append(ring.collect(pending.pop(0)))
        for k in range(len(frames)):
            _assert_frame(want[k], got[k], f"ring frame {k}")
        # the destination is the source's size: a 2W x 2H one is refused by the shape check, a pitch below W * B by the library
        with pytest.raises(ValueError):
            sync.get_frame(frames[0], dst=[np.zeros((2 * a.shape[0], 2 * a.shape[1]), a.dtype) for a in frames[0]])
    if i == 0:
        with SangNomAAHost(clip, dh=True, reduce=kernel) as aa:
            dst = np.zeros((h, w - 1), np.uint8)
            ptr, pitch = (ctypes.c_void_p * 3)(frames[0][0].ctypes.data), (ctypes.c_int32 * 3)(w)
            dp, dpi = (ctypes.c_void_p * 3)(dst.ctypes.data), (ctypes.c_int32 * 3)(w - 1)
            assert capi.load().sn_aa_process_host(aa._h, ptr, pitch, dp, dpi, 1) == capi.SN_ERR_INVALID_ARG


# ---- surfaces ------------------------------------------------------------------------------------------------------------------

def _semi(clip, frames):
    import torch
    dev = torch.device("cuda:0")
    return [torch.from_numpy(np.stack([fr[0] for fr in frames]).view(VT[clip.bytes])).pin_memory().to(dev),
            torch.from_numpy(np.stack([np.stack([fr[1], fr[2]], axis=-1) for fr in frames]).view(VT[clip.bytes])).pin_memory().to(dev)]


@pytest.mark.parametrize("kernel", KERNELS)
def test_nv12_in_nv12_out_at_source_size(hip_lib, kernel):
    import torch
    clip = clip_format("YUV420P8", 128, 64)
    frames = [synth.frame(clip, "noise", seed=900 + f) for f in range(3)]
    script = Script(clip, aac=48)
    want = [reduce_model(script.frame(fr), kernel) for fr in frames]
    with SangNomAA(clip, max_batch=3, aac=48, dh=True, reduce=kernel) as aa:
        src = _semi(clip, frames)
        dst = [torch.full_like(t, 0x5C) for t in src]
        torch.cuda.synchronize()
        aa.process_surfaces(src, dst)
        aa.synchronize()
        i = aa.surface_info()
        assert (i.split_frames, i.merged_frames, i.copied_frames) == (3, 3, 0)
        with pytest.raises(ValueError):  # rows for 2W are refused
            aa.process_surfaces(src, [torch.zeros((3, 128, 256), dtype=torch.uint8, device=src[0].device),
                                      torch.zeros((3, 64, 128, 2), dtype=torch.uint8, device=src[0].device)])
    y, uv = to_host(dst[0]), to_host(dst[1])
    for f in range(3):
        _assert_frame(want[f], [y[f], uv[f][..., 0], uv[f][..., 1]], f"NV12 frame {f}")


@pytest.mark.parametrize("kernel", KERNELS)
def test_planar_422_in_yuy2_out(hip_lib, kernel):
    import torch
    clip = clip_format("YUV422P8", 128, 64)
    frames = [synth.frame(clip, "noise", seed=910 + f) for f in range(3)]
    script = Script(clip, aac=48)
    want = [reduce_model(script.frame(fr), kernel) for fr in frames]
    with SangNomAA(clip, max_batch=3, aac=48, dh=True, reduce=kernel) as aa:
        src = _to_dev(clip, frames)
        dst = torch.full((3, 64, 256), 0x5C, dtype=torch.uint8, device=src[0].device)
        torch.cuda.synchronize()
        aa.process_surfaces(src, dst, dst_packed="yuyv")
        aa.synchronize()
    got = to_host(dst)
    for f in range(3):
        a = pc.pack_yuyv(want[f][0], want[f][1], want[f][2], "yuyv")
        assert same(a, got[f]), f"YUY2 frame {f}: " + describe_diff(a, got[f])


def test_planar_422_ten_bit_in_v210_out_on_checker(hip_lib):
    """The half-band kernel overshoots 1023 on these frames; the clamp to the clip's range keeps every v210 field valid."""
    import torch
    clip = clip_format("YUV422P10", 96, 48)
    frames = [synth.frame(clip, "checker", seed=920 + f) for f in range(2)]
    script = Script(clip, aac=48)
    E = [script.frame(fr) for fr in frames]
    assert max(((reduce_unclamped(pl, "halfband", 1, 0) + 512) >> 10).max() for e in E for pl in e) > 1023, "the case does not reach the clamp"
    want = [reduce_model(e, "halfband", bits=10) for e in E]
    with SangNomAA(clip, max_batch=2, aac=48, dh=True, reduce="halfband") as aa:
        src = _to_dev(clip, frames)
        dst = torch.full((2, 48, 4 * pc.v210_blocks(96)), 0x5C5C5C5C, dtype=torch.int32, device=src[0].device)
        torch.cuda.synchronize()
        aa.process_surfaces(src, dst, dst_packed="v210")
        aa.synchronize()
    got = to_host(dst).view(np.uint32)
    for f in range(2):
        assert all(pl.max() <= 1023 for pl in want[f])
        a = pc.pack_v210(want[f][0], want[f][1], want[f][2])
        assert same(a, got[f]), f"v210 frame {f}: " + describe_diff(a, got[f])


# ---- unchanged paths -----------------------------------------------------------------------------------------------------------

def test_reduce_zero_is_the_dh_call(hip_lib):
    clip = clip_format("YUV420P8", 128, 64)
    frames = [synth.frame(clip, "noise", seed=60 + i) for i in range(3)]
    script = Script(clip, aac=48)
    with SangNomAA(clip, max_batch=3, aac=48, dh=True, reduce=0) as aa:
        assert capi.load().sn_aa_get_reduce(aa._h) == 0
        assert aa.plane_shape_out(0) == (128, 256)
        got = _batch(aa, clip, frames)
    for f, fr in enumerate(frames):
        _assert_frame(script.frame(fr), got[f], f"frame {f}")
    with pytest.raises(SangNomError) as e:
        SangNomAA(clip, reduce="tent")
    assert e.value.code == capi.SN_ERR_CONFIG and "reduce needs dh" in str(e.value)


def test_pinned_and_pageable_destinations(hip_lib):
    """Destination planes of source size inside memory pinned with sn_pin_host_buffer are written from the device; pageable ones
    through the staging.  Last in the file: it registers and unregisters host memory."""
    clip = clip_format("YUV420P8", 128, 64)
    frames = [synth.frame(clip, "noise", seed=80 + i) for i in range(3)]
    script = Script(clip, aac=48)
    want = [reduce_model(script.frame(fr), "tent") for fr in frames]
    per = 64 * 128 * 3 // 2
    arena_in = np.zeros(3 * per, np.uint8)
    arena_out = np.zeros(3 * per, np.uint8)
    pin_host_array(arena_in)
    pin_host_array(arena_out)
    try:
        def planes(arena, f):
            base = arena[f * per:(f + 1) * per]
            return [base[:8192].reshape(64, 128), base[8192:10240].reshape(32, 64), base[10240:].reshape(32, 64)]
        with SangNomAAHost(clip, aac=48, dh=True, reduce="tent") as aa:
            for f, fr in enumerate(frames):
                src = planes(arena_in, f)
                for p in range(3):
                    src[p][...] = fr[p]
                dst = planes(arena_out, f)
                aa.get_frame(src, dst=dst)
                _assert_frame(want[f], dst, f"pinned frame {f}")
                _assert_frame(want[f], aa.get_frame(fr), f"pageable frame {f}")
    finally:
        unpin_host_array(arena_out)
        unpin_host_array(arena_in)
