"""The anti-aliasing call with dh -- TurnLeft().SangNom2(dh=true).TurnRight().SangNom2(dh=true), enlargement by two in
both directions -- on device batches, the synchronous host call and the host ring, against the script built from the
reference's semantics (tests/aa_dh_script.py).  Bit-exact, tolerance zero.  The library fills its intermediate planes
with 0xA5 and a dh pass reads every line of its source, so a turn that left a line out would show up here."""
import ctypes

import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNomAA, SangNomAAHost, SangNomError, capi, clip_format, synth
from avisynth_sangnom2_amd.filter import pin_host_array, unpin_host_array
from tests import aa_script
from tests.aa_dh_script import Script, kept_offset
from tests.util import describe_diff, same, to_host

pytestmark = pytest.mark.gpu

VT = {1: np.uint8, 2: np.int16, 4: np.float32}  # torch has no uint16: same bits


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
    ("Y8", 128, 64, {}, {}, {}, "noise", None),                     # both passes history-free and fused
    ("Y8", 96, 80, {}, {}, {}, "noise", None),                      # the turned pass is 80 wide: a dh chain carrying history
    ("Y8", 40, 96, {}, {}, {}, "noise", None),                      # the second pass is 80 wide and carries history
    ("Y8", 200, 136, {}, {}, {}, "noise", None),                    # ragged turn tiles in both turns, both passes carry history
    ("Y8", 512, 64, {}, {}, {}, "noise", None),                     # second pass 1024 wide: three strips; U1 is 64 x 1024
    ("Y8", 1920, 32, {}, {}, {}, "noise", None),                    # second pass 3840 wide: the eight-strip sweep
    ("Y32", 132, 66, {}, {}, {}, "noise", None),
    ("Y16", 96, 64, dict(order=2), {}, {}, "noise", None),
    ("Y10", 64, 48, {}, {}, {}, "noise", None),
    ("YUV420P8", 128, 64, dict(aac=48), {}, {}, "noise", None),
    ("YUV422P8", 128, 64, dict(aac=48), {}, {}, "noise", None),     # the turned clip is 4:4:0
    ("YUV420P16", 96, 64, dict(aac=48), {}, {}, "noise", None),
    ("YUV444PS", 64, 32, dict(aac=20), {}, {}, "noise", None),
    ("YUV420P8", 128, 64, dict(luma=False, aac=48), {}, {}, "noise", None),  # planes are forced
    ("Y8", 96, 80, {}, dict(fresh_pool=True), dict(fresh=True), "noise", None),
    ("YUV420P8", 128, 64, {}, dict(isolated_planes=True), dict(isolated=True), "noise", None),
    ("Y8", 128, 64, dict(order=0), {}, {}, "noise", [1, 0, 0, 1, 1]),
    ("Y8", 128, 64, {}, dict(opt=1), dict(opt=1), "noise01", None),
    ("YUV420P8", 128, 64, dict(aac=48), dict(opt=1), dict(opt=1), "noise01", None),
    ("Y16", 96, 64, {}, dict(opt=1), dict(opt=1), "noise01", None),
]

_WANT = {}  # case index -> (frames, parities, the script's frames): computed once, shared by both launch policies, left unchanged


def _expected(i):
    if i not in _WANT:
        fmt, w, h, kw, ckw, skw, pattern, par = BATCH[i]
        clip = clip_format(fmt, w, h)
        frames = [synth.frame(clip, pattern, seed=300 + f) for f in range(8)]
        parities = (par or [1] * 5) + [1, 1, 1]
        script = Script(clip, **kw, **skw)
        want = [script.frame(fr, parity=parities[f]) for f, fr in enumerate(frames)]
        if skw.get("opt") == 1:
            other = Script(clip, **kw)
            assert any(not same(a, b) for f, fr in enumerate(frames[:3]) for a, b in zip(want[f], other.frame(fr, parity=parities[f]))), \
                "opt=1 and opt=0 agree on these frames: the case shows nothing"
        _WANT[i] = (frames, parities, want)
    return _WANT[i]


@pytest.mark.parametrize("small", ["sweep", "auto"])
@pytest.mark.parametrize("i", range(len(BATCH)), ids=[f"{c[0]}-{c[1]}x{c[2]}-{i}" for i, c in enumerate(BATCH)])
def test_batches_match_the_script(hip_lib, i, small):
    """Five frames in one call, then three more on the same context: frame f is what the script gives, state carried on."""
    fmt, w, h, kw, ckw, skw, pattern, par = BATCH[i]
    clip = clip_format(fmt, w, h)
    frames, parities, want = _expected(i)
    sl = capi.SN_SMALL_SWEEP if small == "sweep" else capi.SN_SMALL_AUTO
    with SangNomAA(clip, max_batch=5, small_launches=sl, dh=True, **kw, **ckw) as aa:
        got = _batch(aa, clip, frames[:5], parities[:5] if par else None) + _batch(aa, clip, frames[5:])
    for f in range(8):
        _assert_frame(want[f], got[f], f"frame {f}")
        if fmt in ("Y8", "YUV420P8"):  # the source samples reappear untouched
            off = kept_offset(kw.get("order", 1), parities[f])
            for p in range(clip.planes):
                assert np.array_equal(got[f][p][off::2, (1 - off)::2], frames[f][p]), f"frame {f} plane {p}: the source samples are not kept"


def test_strides_and_pitches(hip_lib):
    """Pitches larger than the row, frame strides larger than the plane, destination pre-filled: the planes are the
    script's and every byte outside the 2W x 2H planes stays as it was; a destination pitch below the doubled row is refused."""
    import torch
    clip = clip_format("YUV420P8", 128, 64)
    N = 4
    frames = [synth.frame(clip, "noise", seed=520 + i) for i in range(N)]
    script = Script(clip, aac=48)
    want = [script.frame(fr) for fr in frames]
    dev = torch.device("cuda:0")
    src, dst, before = [], [], []
    for p in range(3):
        hp, wp = frames[0][p].shape
        big = np.full((N, hp + 3, wp + 40), 0x11, np.uint8)
        for f in range(N):
            big[f, :hp, :wp] = frames[f][p]
        src.append(torch.from_numpy(big).pin_memory().to(dev)[:, :hp, :wp])
        fill = np.full((N, 2 * hp + 5, 2 * wp + 24), 0x5C, np.uint8)
        before.append(fill)
        dst.append(torch.from_numpy(fill.copy()).pin_memory().to(dev))
    torch.cuda.synchronize()
    with SangNomAA(clip, max_batch=N, aac=48, dh=True) as aa:
        aa.process_batch(src, [d[:, :2 * s.shape[1], :2 * s.shape[2]] for d, s in zip(dst, src)])
        aa.synchronize()
        # a destination whose pitch holds the source's row but not the doubled one: refused by the library itself
        L = capi.load()
        sp, dp = (ctypes.c_void_p * 3)(), (ctypes.c_void_p * 3)()
        spi, dpi = (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 3)()
        sfs, dfs = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
        for p in range(3):
            sp[p], dp[p] = src[p].data_ptr(), dst[p].data_ptr()
            spi[p], sfs[p] = src[p].stride(1), src[p].stride(0)
            dpi[p], dfs[p] = 2 * src[p].shape[2] - 1, dst[p].stride(0)
        assert L.sn_aa_process_device_strided(aa._h, N, sp, sfs, spi, dp, dfs, dpi, None) == capi.SN_ERR_INVALID_ARG
        aa.synchronize()
    for p in range(3):
        hp, wp = frames[0][p].shape
        got = to_host(dst[p])
        for f in range(N):
            assert same(want[f][p], got[f, :2 * hp, :2 * wp]), f"frame {f} plane {p}: " + describe_diff(want[f][p], got[f, :2 * hp, :2 * wp])
        outside = np.ones(got.shape, bool)
        outside[:, :2 * hp, :2 * wp] = False
        assert np.array_equal(got[outside], before[p][outside]), f"plane {p}: bytes outside the plane were written"


def test_a_batch_beyond_the_scratch_budget_is_walked_in_chunks(hip_lib):
    """Y8 512x256 with dh: 131 072 + 2 x 262 144 = 655 360 bytes of intermediates per frame (pitches rounded to 256), so a
    budget of 2 MB holds three frames and a 12-frame batch takes four chunks; the result is what one chunk gives (and
    the script's for the frames checked against it)."""
    clip = clip_format("Y8", 512, 256)
    frames = [synth.frame(clip, "noise", seed=700 + i) for i in range(12)]
    with SangNomAA(clip, max_batch=12, dh=True) as aa:
        one = _batch(aa, clip, frames)
    with SangNomAA(clip, max_batch=12, scratch_budget_mb=2, dh=True) as aa:
        chunked = _batch(aa, clip, frames)
    script = Script(clip)
    for f in range(12):
        _assert_frame(one[f], chunked[f], f"frame {f} (chunked against one chunk)")
        if f < 3:
            _assert_frame(script.frame(frames[f]), chunked[f], f"frame {f} (script)")


RING = [("Y8", 128, 64, {}), ("YUV420P8", 128, 64, dict(aac=48)), ("Y16", 96, 64, {}), ("Y8", 96, 80, {})]  # 96x80: history-carrying
_RING_WANT = {}


def _ring_expected(i):
    if i not in _RING_WANT:
        fmt, w, h, kw = RING[i]
        clip = clip_format(fmt, w, h)
        frames = [synth.frame(clip, "noise", seed=40 + f) for f in range(10)]
        script = Script(clip, **kw)
        _RING_WANT[i] = (frames, [script.frame(fr) for fr in frames])
    return _RING_WANT[i]


@pytest.mark.parametrize("depth", [1, 3, 8])
@pytest.mark.parametrize("i", range(len(RING)), ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in RING])
def test_the_host_ring(hip_lib, i, depth):
    fmt, w, h, kw = RING[i]
    clip = clip_format(fmt, w, h)
    frames, want = _ring_expected(i)
    with SangNomAAHost(clip, host_depth=depth, dh=True, **kw) as ring, SangNomAAHost(clip, dh=True, **kw) as sync:
        n = ring.slots()
        assert 1 <= n <= depth
        got, pending, f = [], [], 0
        while len(got) < len(frames):
            while f < len(frames) and len(pending) < n:  # as many in flight as the ring holds
                pending.append(ring.submit(frames[f]))
                f += 1
            if f < len(frames):  # the next slot has not been collected
                with pytest.raises(SangNomError) as e:
                    ring.submit(frames[f])
                assert e.value.code == capi.SN_ERR_BUSY
            got.append(ring.collect(pending.pop(0)))
        for k, fr in enumerate(frames):
            _assert_frame(want[k], got[k], f"ring frame {k}")
            _assert_frame(sync.get_frame(fr), got[k], f"ring frame {k} against get_frame")


def test_host_pitches_are_checked_against_the_doubled_row(hip_lib):
    clip = clip_format("Y8", 128, 64)
    fr = synth.frame(clip, "noise", seed=3)
    with SangNomAAHost(clip, dh=True) as aa:
        dst = np.zeros((128, 255), np.uint8)
        ptr, pitch = (ctypes.c_void_p * 3)(fr[0].ctypes.data), (ctypes.c_int32 * 3)(128)
        dp, dpi = (ctypes.c_void_p * 3)(dst.ctypes.data), (ctypes.c_int32 * 3)(255)
        assert capi.load().sn_aa_process_host(aa._h, ptr, pitch, dp, dpi, 1) == capi.SN_ERR_INVALID_ARG
        with pytest.raises(ValueError):
            aa.get_frame(fr, dst=[np.zeros((64, 128), np.uint8)])


def test_info_and_limits(hip_lib):
    with SangNomAA(clip_format("Y8", 96, 80), max_batch=4, dh=True) as aa:  # the turned clip is 80 wide; the second pass 192
        assert aa.info(0).history_free == 0 and aa.info(1).history_free == 1
        assert aa.info(0).out_height == 2 * 96
        assert aa.info(1).out_height == 2 * 80 and aa.info(1).pool_stride == 192
        assert aa.plane_shape_out(0) == (160, 192)
    with SangNomAA(clip_format("Y8", 40, 96), dh=True) as aa:  # the second pass is 80 wide
        assert aa.info(0).history_free == 1 and aa.info(1).history_free == 0
        assert aa.info(1).out_height == 192 and aa.info(1).pool_stride == 96
    with pytest.raises(SangNomError) as e:
        SangNomAA(clip_format("Y8", 4128, 64), dh=True)  # 2W = 8256
    assert e.value.code == capi.SN_ERR_UNSUPPORTED and "8192" in str(e.value)
    with SangNomAA(clip_format("Y8", 4128, 64)) as aa:  # without dh the same clip is served
        assert aa.info(1).out_height == 64


def test_without_dh_the_call_is_what_it_was(hip_lib):
    """dh=False through the new keyword: the anti-aliasing script's frames, the destination in the clip's geometry."""
    clip = clip_format("YUV420P8", 128, 64)
    frames = [synth.frame(clip, "noise", seed=60 + i) for i in range(3)]
    script = aa_script.Script(clip, chroma=False)
    with SangNomAA(clip, max_batch=3, chroma=False, dh=False) as aa:
        assert aa.plane_shape_out(1) == aa.plane_shape(1)
        got = _batch(aa, clip, frames)
    for f, fr in enumerate(frames):
        _assert_frame(script.frame(fr), got[f], f"frame {f}")


def test_destroying_a_context_with_frames_in_flight(hip_lib):
    clip = clip_format("Y8", 128, 64)
    frames = [synth.frame(clip, "noise", seed=5 + i) for i in range(3)]
    aa = SangNomAAHost(clip, host_depth=4, dh=True)
    for fr in frames:
        aa.submit(fr)
    aa.close()  # neither hangs nor faults
    with SangNomAAHost(clip, dh=True) as again:
        _assert_frame(Script(clip).frame(frames[0]), again.get_frame(frames[0]), "a new context afterwards")


def test_pinned_source_and_destination(hip_lib):
    """Source and destination planes inside memory pinned with sn_pin_host_buffer: transferred as they lie, the
    destination written from the device in its doubled geometry.  Last in the file: it registers and unregisters host memory."""
    clip = clip_format("YUV420P8", 128, 64)
    frames = [synth.frame(clip, "noise", seed=80 + i) for i in range(3)]
    script = Script(clip, aac=48)
    want = [script.frame(fr) for fr in frames]
    arena_in = np.zeros(3 * (64 * 128 + 2 * 32 * 64), np.uint8)
    arena_out = np.zeros(4 * arena_in.size, np.uint8)
    pin_host_array(arena_in)
    pin_host_array(arena_out)
    try:
        def planes(arena, f, scale):
            hs, ws = 64 * scale, 128 * scale
            per = hs * ws * 3 // 2
            base = arena[f * per:(f + 1) * per]
            y = base[:hs * ws].reshape(hs, ws)
            u = base[hs * ws:hs * ws * 5 // 4].reshape(hs // 2, ws // 2)
            v = base[hs * ws * 5 // 4:].reshape(hs // 2, ws // 2)
            return [y, u, v]
        with SangNomAAHost(clip, aac=48, dh=True) as aa:
            for f, fr in enumerate(frames):
                src = planes(arena_in, f, 1)
                for p in range(3):
                    src[p][...] = fr[p]
                dst = planes(arena_out, f, 2)
                aa.get_frame(src, dst=dst)
                _assert_frame(want[f], dst, f"pinned frame {f}")
    finally:
        unpin_host_array(arena_out)
        unpin_host_array(arena_in)
