"""The anti-aliasing call with an edge mask (sn_aa_create_ex3): every entry point against merge_model(source, unmasked model)
-- the numpy statement of the mask (tests/mask_model.py) over the script's frame: aa_script's without dh, the dh script plus
reduce_model with dh and a reduction --, bit for bit: device batches, strides, chunks, the host call and ring, pinned
destinations, and semi-planar, MSB and packed surfaces.  The frames are tests/mask_cases.py's, whose masks hold all three
classes (tests/test_aa_mask_cpu.py asserts it); every comparison also asserts that the expected plane is neither the source
nor the unmasked result."""
import ctypes

import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNomAA, SangNomAAHost, SangNomError, capi, clip_format
from avisynth_sangnom2_amd.filter import pin_host_array, unpin_host_array
from tests import mask_cases as mc
from tests import packed_surface_cases as pc
from tests.util import describe_diff, same, to_host

pytestmark = pytest.mark.gpu

VT = {1: np.uint8, 2: np.int16, 4: np.float32}  # torch has no uint16: same bits
MASK = dict(mask=(mc.LO, mc.HI))
FORMS = ["reduce", "plain"]  # dh + reduce, and without dh


def _assert_frame(want, got, what, source=None, unmasked=None, processed=None):
    for p, (a, b) in enumerate(zip(want, got)):
        assert a.shape == b.shape, f"{what} plane {p}: shape {b.shape}, expected {a.shape}"
        assert same(a, b), f"{what} plane {p}: " + describe_diff(a, b)
        if source is not None and (processed is None or processed[p]):
            assert not same(a, source[p]) and not same(a, unmasked[p]), f"{what} plane {p}: the expected plane is the source or the unmasked result"


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


def _form_kw(form, kernel="halfband"):
    return dict(dh=True, reduce=kernel) if form == "reduce" else {}


def _run_batches(case, form, kernel, expand, small):
    fmt, w, h, kw, ckw, skw, par = case
    clip = clip_format(fmt, w, h)
    frames, parities, res, want = mc.expected(case, kernel if form == "reduce" else None, expand)
    sl = capi.SN_SMALL_SWEEP if small == "sweep" else capi.SN_SMALL_AUTO
    with SangNomAA(clip, max_batch=5, small_launches=sl, mask_expand=expand, **MASK, **_form_kw(form, kernel), **kw, **ckw) as aa:
        m = aa.mask()
        assert (m.kind, m.lo, m.hi, m.expand) == (capi.SN_AA_MASK_SOBEL, mc.LO, mc.HI, expand)
        assert all(aa.plane_shape_out(p) == aa.plane_shape(p) for p in range(clip.planes))
        got = _batch(aa, clip, frames[:5], parities[:5] if par else None) + _batch(aa, clip, frames[5:])
    proc = mc.processed_of(case) if form == "plain" else None
    for f in range(len(frames)):
        _assert_frame(want[f], got[f], f"frame {f}", frames[f], res[f], proc)
    return frames, got


@pytest.mark.parametrize("small", ["sweep", "auto"])
@pytest.mark.parametrize("expand", mc.EXPANDS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("i", range(len(mc.BATCH)), ids=[f"{c[0]}-{c[1]}x{c[2]}-{i}" for i, c in enumerate(mc.BATCH)])
def test_batches_match_the_merged_script(hip_lib, i, form, expand, small):
    """Five frames in one call, then three more on the same context; both reduce kernels for the first case."""
    for kernel in (mc.kernel_of(i) if form == "reduce" else [None]):
        _run_batches(mc.BATCH[i], form, kernel, expand, small)


@pytest.mark.parametrize("expand", mc.EXPANDS)
def test_luma_that_is_not_processed_comes_back_as_a_copy(hip_lib, expand):
    """Without dh, luma=False: chroma is merged through its own masks, luma is the source."""
    frames, got = _run_batches(mc.LUMA_OFF, "plain", None, expand, "auto")
    for f in range(len(frames)):
        assert same(frames[f][0], got[f][0])


@pytest.mark.parametrize("form", FORMS)
def test_strides_and_pitches(hip_lib, form):
    """Pitches larger than the row, frame strides larger than the plane, destination pre-filled: nothing outside the planes is written."""
    import torch
    case = mc.BATCH[7]  # YUV420P8
    clip = clip_format(case[0], case[1], case[2])
    N = 4
    frames, _, res, want = mc.expected(case, "halfband" if form == "reduce" else None, 1)
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
    with SangNomAA(clip, max_batch=N, aac=48, **MASK, **_form_kw(form)) as aa:
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


@pytest.mark.parametrize("form", FORMS)
def test_a_tiny_scratch_budget_walks_a_batch_in_chunks(hip_lib, form):
    """Y8 512x256: 3 x 131 072 bytes of intermediates per frame without dh (a budget of 1 MB holds two frames), 1 179 648 with dh
    and a reduction (2 MB hold one): a batch of five takes three or five chunks and gives the frames one chunk gives."""
    clip = clip_format("Y8", 512, 256)
    frames = mc.frames_of("Y8", 512, 256, count=5)
    with SangNomAA(clip, max_batch=5, **MASK, **_form_kw(form)) as aa:
        one = _batch(aa, clip, frames)
    with SangNomAA(clip, max_batch=5, scratch_budget_mb=2 if form == "reduce" else 1, **MASK, **_form_kw(form)) as aa:
        chunked = _batch(aa, clip, frames)
    fr, _, res, want = mc.expected(mc.CHUNK, "halfband" if form == "reduce" else None, 1, count=2)
    for f in range(5):
        _assert_frame(one[f], chunked[f], f"frame {f} (chunked against one chunk)")
        if f < 2:
            _assert_frame(want[f], chunked[f], f"frame {f} (script)", fr[f], res[f])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("i", range(len(mc.HOST)), ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in mc.HOST])
def test_the_host_call_and_the_ring(hip_lib, i, form):
    """get_frame, then the ring: submit and collect, depth 4, 7 frames."""
    fmt, w, h, kw = mc.HOST[i]
    clip = clip_format(fmt, w, h)
    case = (fmt, w, h, kw, {}, {}, None)
    frames, _, res, want = mc.expected(case, "halfband" if form == "reduce" else None, 1, count=7)
    fkw = dict(_form_kw(form), **MASK, **kw)
    with SangNomAAHost(clip, host_depth=4, **fkw) as ring, SangNomAAHost(clip, **fkw) as sync:
        for k in range(2):
            _assert_frame(want[k], sync.get_frame(frames[k]), f"get_frame {k}", frames[k], res[k])
        n = ring.slots()
        assert 1 <= n <= 4
        got, pending, f = [], [], 0
        while len(got) < len(frames):
            while f < len(frames) and len(pending) < n:
                pending.append(ring.submit(frames[f]))
                f += 1
            got.append(ring.collect(pending.pop(0)))
        for k in range(len(frames)):
            _assert_frame(want[k], got[k], f"ring frame {k}", frames[k], res[k])


# ---- surfaces ------------------------------------------------------------------------------------------------------------------

def _semi(clip, frames, shift=0):
    import torch
    dev = torch.device("cuda:0")
    dt = clip.dtype
    return [torch.from_numpy((np.stack([fr[0] for fr in frames]).astype(dt) << shift).view(VT[clip.bytes])).pin_memory().to(dev),
            torch.from_numpy((np.stack([np.stack([fr[1], fr[2]], axis=-1) for fr in frames]).astype(dt) << shift).view(VT[clip.bytes])).pin_memory().to(dev)]


@pytest.mark.parametrize("form", FORMS)
def test_nv12_in_nv12_out(hip_lib, form):
    import torch
    case = mc.BATCH[7]
    clip = clip_format(case[0], case[1], case[2])
    frames, _, res, want = mc.expected(case, "halfband" if form == "reduce" else None, 1)
    frames, res, want = frames[:3], res[:3], want[:3]
    with SangNomAA(clip, max_batch=3, aac=48, **MASK, **_form_kw(form)) as aa:
        src = _semi(clip, frames)
        dst = [torch.full_like(t, 0x5C) for t in src]
        torch.cuda.synchronize()
        aa.process_surfaces(src, dst)
        aa.synchronize()
        i = aa.surface_info()
        assert (i.split_frames, i.merged_frames, i.copied_frames) == (3, 3, 0)
    y, uv = to_host(dst[0]), to_host(dst[1])
    for f in range(3):
        _assert_frame(want[f], [y[f], uv[f][..., 0], uv[f][..., 1]], f"NV12 frame {f}", frames[f], res[f])


@pytest.mark.parametrize("form", FORMS)
def test_planar_422_in_yuy2_out(hip_lib, form):
    import torch
    case = mc.BATCH[8]
    clip = clip_format(case[0], case[1], case[2])
    frames, _, res, want = mc.expected(case, "halfband" if form == "reduce" else None, 1)
    with SangNomAA(clip, max_batch=3, aac=48, **MASK, **_form_kw(form)) as aa:
        src = _to_dev(clip, frames[:3])
        dst = torch.full((3, 64, 256), 0x5C, dtype=torch.uint8, device=src[0].device)
        torch.cuda.synchronize()
        aa.process_surfaces(src, dst, dst_packed="yuyv")
        aa.synchronize()
    got = to_host(dst)
    for f in range(3):
        assert not same(want[f][0], frames[f][0]) and not same(want[f][0], res[f][0])
        a = pc.pack_yuyv(want[f][0], want[f][1], want[f][2], "yuyv")
        assert same(a, got[f]), f"YUY2 frame {f}: " + describe_diff(a, got[f])


def test_p010_in_planar_out_without_dh(hip_lib):
    """A SEMIPLANAR_MSB source on a 10-bit context: the planes the mask is built from are the unpacked, shifted-down ones, all lines."""
    import torch
    clip = clip_format(*mc.P010[:3])
    frames, _, res, want = mc.expected(mc.P010, None, 1, count=3)
    with SangNomAA(clip, max_batch=3, aac=48, **MASK) as aa:
        src = _semi(clip, frames, shift=6)
        dst = [torch.full((3,) + aa.plane_shape_out(p), 0x5C5C, dtype=torch.int16, device=src[0].device) for p in range(3)]
        torch.cuda.synchronize()
        aa.process_surfaces(src, dst, src_msb=True)
        aa.synchronize()
    for f in range(3):
        _assert_frame(want[f], [to_host(dst[p][f]).view(np.uint16) for p in range(3)], f"P010 frame {f}", frames[f], res[f])


# ---- unchanged paths, the getter, the refusal ----------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
def test_without_a_mask_the_call_gives_what_it_gives_today(hip_lib, form):
    case = mc.BATCH[7]
    clip = clip_format(case[0], case[1], case[2])
    frames, _, res = mc.unmasked(case, "halfband" if form == "reduce" else None)
    for kw in (dict(mask=None), {}):
        with SangNomAA(clip, max_batch=3, aac=48, **kw, **_form_kw(form)) as aa:
            assert aa.mask().kind == capi.SN_AA_MASK_NONE
            got = _batch(aa, clip, frames[:3])
        for f in range(3):
            _assert_frame(res[f], got[f], f"frame {f}")


def test_the_getter_and_the_refusal(hip_lib):
    clip = clip_format("Y8", 128, 64)
    with SangNomAA(clip, mask=(7, 201), mask_expand=0) as aa:
        m = aa.mask()
        assert (m.struct_size, m.kind, m.lo, m.hi, m.expand, list(m.reserved)) == (32, 1, 7, 201, 0, [0, 0, 0])
        short = capi.SnAAMask(struct_size=28)
        assert capi.load().sn_aa_get_mask(aa._h, ctypes.byref(short)) == capi.SN_ERR_INVALID_ARG
    with pytest.raises(SangNomError) as e:
        SangNomAA(clip, dh=True, **MASK)
    assert e.value.code == capi.SN_ERR_CONFIG and "mask needs the frame at source size" in str(e.value)
    with pytest.raises(SangNomError) as e:
        SangNomAAHost(clip, mask=(97, 96))
    assert e.value.code == capi.SN_ERR_INVALID_ARG and "sn_aa_mask.lo" in str(e.value)


@pytest.mark.parametrize("form", FORMS)
def test_pinned_and_pageable_destinations(hip_lib, form):
    """Destination planes inside memory pinned with sn_pin_host_buffer are written from the device; pageable ones through the
    staging.  Last in the file: it registers and unregisters host memory."""
    case = mc.BATCH[7]
    clip = clip_format(case[0], case[1], case[2])
    frames, _, res, want = mc.expected(case, "halfband" if form == "reduce" else None, 1)
    per = 64 * 128 * 3 // 2
    arena_in = np.zeros(3 * per, np.uint8)
    arena_out = np.zeros(3 * per, np.uint8)
    pin_host_array(arena_in)
    pin_host_array(arena_out)
    try:
        def planes(arena, f):
            base = arena[f * per:(f + 1) * per]
            return [base[:8192].reshape(64, 128), base[8192:10240].reshape(32, 64), base[10240:].reshape(32, 64)]
        with SangNomAAHost(clip, aac=48, **MASK, **_form_kw(form)) as aa:
            for f in range(3):
                src = planes(arena_in, f)
                for p in range(3):
                    src[p][...] = frames[f][p]
                dst = planes(arena_out, f)
                aa.get_frame(src, dst=dst)
                _assert_frame(want[f], dst, f"pinned frame {f}", frames[f], res[f])
                _assert_frame(want[f], aa.get_frame(frames[f]), f"pageable frame {f}")
    finally:
        unpin_host_array(arena_out)
        unpin_host_array(arena_in)
