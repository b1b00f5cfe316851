"""The anti-aliasing call on device batches and on the host ring (sn_aa_process_device_strided, sn_aa_submit_host /
sn_aa_collect_host) against the script TurnLeft().SangNom2(...).TurnRight().SangNom2(...) built from the reference's
semantics (tests/aa_script.py).  Bit-exact, tolerance zero.  The library fills its intermediate planes with 0xA5 and its
turns write only the lines the next pass keeps, so a pass that read any other line would show up here."""
import ctypes

import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2, SangNomAA, SangNomAAHost, SangNomError, capi, clip_format, synth
from tests.aa_script import Script, turned_clip
from tests.util import describe_diff, same, to_host

pytestmark = pytest.mark.gpu

VT = {1: np.uint8, 2: np.int16, 4: np.float32}  # torch has no uint16: same bits


def _assert_frame(want, got, what):
    for p, (a, b) in enumerate(zip(want, got)):
        assert same(a, b), f"{what} plane {p}: " + describe_diff(a, b)


def _to_dev(clip, frames):
    import torch
    dev = torch.device("cuda:0")
    return [torch.from_numpy(np.stack([fr[p] for fr in frames]).view(VT[clip.bytes])).pin_memory().to(dev) for p in range(clip.planes)]


def _batch(aa, clip, frames, parity=None):
    import torch
    src = _to_dev(clip, frames)
    dst = [torch.zeros_like(s) for s in src]
    torch.cuda.synchronize()
    aa.process_batch(src, dst, parity)
    aa.synchronize()
    return [[to_host(dst[p][f]).view(clip.dtype) for p in range(clip.planes)] for f in range(len(frames))]


# (format, width, height, filter kwargs, context kwargs, script kwargs, pattern, parities of the first call)
BATCH = [
    ("Y8", 128, 64, {}, {}, {}, "noise", None),
    ("Y8", 96, 80, {}, {}, {}, "noise", None),                      # the turned pass carries history
    ("Y8", 80, 96, {}, {}, {}, "noise", None),                      # the second pass carries history
    ("Y8", 200, 136, {}, {}, {}, "noise", None),                    # ragged turn tiles
    ("Y32", 132, 66, {}, {}, {}, "noise", None),
    ("Y16", 96, 64, dict(order=2), {}, {}, "noise", None),
    ("YUV420P8", 128, 64, dict(aac=48), {}, {}, "noise", None),
    ("YUV422P8", 128, 64, dict(aac=48), {}, {}, "noise", None),     # the turned clip is 4:4:0
    ("YUV420P16", 96, 64, dict(aac=48), {}, {}, "noise", None),
    ("Y8", 96, 80, {}, dict(fresh_pool=True), dict(fresh=True), "noise", None),
    ("YUV420P8", 128, 64, {}, dict(isolated_planes=True), dict(isolated=True), "noise", None),
    ("YUV420P8", 128, 64, dict(chroma=False), {}, {}, "noise", None),
    ("YUV420P8", 128, 64, dict(luma=False), {}, {}, "noise", None),
    ("Y8", 128, 64, dict(order=0), {}, {}, "noise", [1, 0, 0, 1, 1]),
    ("Y8", 128, 64, {}, dict(opt=1), dict(opt=1), "noise01", None),
    ("YUV420P8", 128, 64, {}, dict(opt=1), dict(opt=1), "noise01", None),
]


@pytest.mark.parametrize("small", ["sweep", "auto"])
@pytest.mark.parametrize("fmt,w,h,kw,ckw,skw,pattern,par", BATCH, ids=[f"{c[0]}-{c[1]}x{c[2]}-{i}" for i, c in enumerate(BATCH)])
def test_batches_match_the_script(hip_lib, fmt, w, h, kw, ckw, skw, pattern, par, small):
    """Five frames in one call, then three more on the same context: frame f is what the script gives, state carried on."""
    clip = clip_format(fmt, w, h)
    frames = [synth.frame(clip, pattern, seed=300 + i) for i in range(8)]
    parities = (par or [1] * 5) + [1, 1, 1]
    script = Script(clip, **kw, **skw)
    want = [script.frame(fr, parity=parities[f]) for f, fr in enumerate(frames)]
    if skw.get("opt") == 1:
        other = Script(clip, **kw)
        assert any(not same(a, b) for f, fr in enumerate(frames) for a, b in zip(want[f], other.frame(fr, parity=parities[f]))), \
            "opt=1 and opt=0 agree on these frames: the case shows nothing"
    sl = capi.SN_SMALL_SWEEP if small == "sweep" else capi.SN_SMALL_AUTO
    with SangNomAA(clip, max_batch=5, small_launches=sl, **kw, **ckw) as aa:
        got = _batch(aa, clip, frames[:5], parities[:5] if par else None) + _batch(aa, clip, frames[5:])
    for f in range(8):
        _assert_frame(want[f], got[f], f"frame {f}")
        for p in range(clip.planes):
            if not (kw.get("luma", True) if p == 0 else kw.get("chroma", True)):
                assert np.array_equal(got[f][p], frames[f][p]), f"frame {f}: plane {p} is not processed and must equal the source"


def test_strides_and_pitches(hip_lib):
    """Pitches larger than the row, frame strides larger than the plane, destination pre-filled: the planes are the
    script's and every byte outside them stays as it was."""
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
        fill = np.full((N, hp + 5, wp + 24), 0x5C, np.uint8)
        before.append(fill)
        dst.append(torch.from_numpy(fill.copy()).pin_memory().to(dev))
    torch.cuda.synchronize()
    with SangNomAA(clip, max_batch=N, aac=48) as aa:
        aa.process_batch(src, [d[:, :s.shape[1], :s.shape[2]] for d, s in zip(dst, src)])
        aa.synchronize()
    for p in range(3):
        hp, wp = frames[0][p].shape
        got = to_host(dst[p])
        for f in range(N):
            assert same(want[f][p], got[f, :hp, :wp]), f"frame {f} plane {p}: " + describe_diff(want[f][p], got[f, :hp, :wp])
        outside = np.ones(got.shape, bool)
        outside[:, :hp, :wp] = False
        assert np.array_equal(got[outside], before[p][outside]), f"plane {p}: bytes outside the plane were written"


def test_a_batch_beyond_the_scratch_budget_is_walked_in_chunks(hip_lib):
    """Y8 512x256: 0.4 MB of intermediates per frame, so a budget of 1 MB holds two frames and a 12-frame batch takes
    six chunks; the result is what one chunk gives (and the script's for the frames checked against it)."""
    clip = clip_format("Y8", 512, 256)
    frames = [synth.frame(clip, "noise", seed=700 + i) for i in range(12)]
    with SangNomAA(clip, max_batch=12) as aa:
        one = _batch(aa, clip, frames)
    with SangNomAA(clip, max_batch=12, scratch_budget_mb=1) as aa:
        chunked = _batch(aa, clip, frames)
    script = Script(clip)
    for f in range(12):
        _assert_frame(one[f], chunked[f], f"frame {f} (chunked against one chunk)")
        if f < 3:
            _assert_frame(script.frame(frames[f]), chunked[f], f"frame {f} (script)")


def test_full_size_frames(hip_lib):
    """Y8 3840x2160 fresh_pool, three device-resident frames: equal to the idiom composed from sn_turn_device and two
    SangNom2 contexts, and frame 1 equal to the script."""
    import torch
    clip = clip_format("Y8", 3840, 2160)
    N = 3
    frames = [synth.frame(clip, "noise", seed=900 + i) for i in range(N)]
    src = _to_dev(clip, frames)
    with SangNomAA(clip, max_batch=N, fresh_pool=True) as aa:
        dst = [torch.zeros_like(src[0])]
        torch.cuda.synchronize()
        aa.process_batch(src, dst)
        aa.synchronize()
    with SangNom2(turned_clip(clip), max_batch=N, fresh_pool=True) as first, \
            SangNom2(clip, max_batch=N, fresh_pool=True, stream=first.stream_handle()) as second:
        t1 = torch.zeros((N, 3840, 2160), dtype=torch.uint8, device=src[0].device)
        u1, t2, ref = torch.zeros_like(t1), torch.zeros_like(src[0]), torch.zeros_like(src[0])
        torch.cuda.synchronize()
        first.turn(src[0], t1, -1)
        first.process_batch([t1], [u1])
        first.turn(u1, t2, +1)
        second.process_batch([t2], [ref])
        second.synchronize()
    got, composed = to_host(dst[0]), to_host(ref)
    for f in range(N):
        assert np.array_equal(got[f], composed[f]), f"frame {f}: " + describe_diff(composed[f], got[f])
    want = Script(clip, fresh=True).frame(frames[1])
    assert same(want[0], got[1]), "frame 1: " + describe_diff(want[0], got[1])


RING = [("Y8", 128, 64, {}), ("YUV420P8", 128, 64, dict(aac=48)), ("Y16", 96, 64, {}), ("Y8", 96, 80, {})]  # 96x80: history-carrying


@pytest.mark.parametrize("depth", [1, 3, 8])
@pytest.mark.parametrize("fmt,w,h,kw", RING, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in RING])
def test_the_host_ring(hip_lib, fmt, w, h, kw, depth):
    clip = clip_format(fmt, w, h)
    frames = [synth.frame(clip, "noise", seed=40 + i) for i in range(10)]
    script = Script(clip, **kw)
    want = [script.frame(fr) for fr in frames]
    with SangNomAAHost(clip, host_depth=depth, **kw) as ring, SangNomAAHost(clip, **kw) as sync:
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
        for i, fr in enumerate(frames):
            _assert_frame(want[i], got[i], f"ring frame {i}")
            _assert_frame(sync.get_frame(fr), got[i], f"ring frame {i} against get_frame")


def test_destroying_a_context_with_frames_in_flight(hip_lib):
    clip = clip_format("Y8", 128, 64)
    frames = [synth.frame(clip, "noise", seed=5 + i) for i in range(3)]
    aa = SangNomAAHost(clip, host_depth=4)
    for fr in frames:
        aa.submit(fr)
    aa.close()  # neither hangs nor faults
    with SangNomAAHost(clip) as again:
        _assert_frame(Script(clip).frame(frames[0]), again.get_frame(frames[0]), "a new context afterwards")


def test_info_of_both_passes(hip_lib):
    clip = clip_format("Y8", 96, 80)  # the turned clip is 80 wide: not a multiple of 32
    with SangNomAA(clip, max_batch=4) as aa:
        assert aa.info(0).history_free == 0 and aa.info(1).history_free == 1
        assert aa.info(0).frames == 0 and aa.info(1).frames == 0
        _batch(aa, clip, [synth.frame(clip, "noise", seed=i) for i in range(4)])
        assert aa.info(0).frames == 4 and aa.info(1).frames == 4
        with pytest.raises(SangNomError):
            aa.info(2)
    with SangNomAA(clip_format("Y8", 80, 96)) as aa:
        assert aa.info(0).history_free == 1 and aa.info(1).history_free == 0
