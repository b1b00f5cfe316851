"""The anti-aliasing call with chroma merged through the luma plane's mask (sn_aa_create_ex4, SN_AA_MASK_CHROMA_LUMA): every
route against merge_model_luma(source, unmasked model) -- tests/mask_luma_model.py over the script's frame: aa_script's
without dh, the dh script plus reduce_model with dh and a reduction --, bit for bit: device batches, chunks, the host call and
ring, and semi-planar, MSB and packed surfaces.  The frames are tests/mask_luma_cases.py's, whose reduced masks hold all three
classes (tests/test_aa_mask_luma_cpu.py asserts it); every comparison also asserts that the expected chroma plane is neither
the source, nor the unmasked result, nor what the plane's own mask gives."""
import ctypes

import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNomAA, SangNomAAHost, capi, clip_format
from tests import mask_luma_cases as lc
from tests import packed_surface_cases as pc
from tests.util import describe_diff, same, to_host

pytestmark = pytest.mark.gpu

VT = {1: np.uint8, 2: np.int16, 4: np.float32}  # torch has no uint16: same bits
MASK = dict(mask=(lc.LO, lc.HI), mask_chroma="luma")
FORMS = ["reduce", "plain"]  # dh + reduce, and without dh


def _assert_frame(want, got, what, source=None, unmasked=None, own=None, processed=None):
    for p, (a, b) in enumerate(zip(want, got)):
        assert a.shape == b.shape, f"{what} plane {p}: shape {b.shape}, expected {a.shape}"
        assert same(a, b), f"{what} plane {p}: " + describe_diff(a, b)
        if source is not None and (processed is None or processed[p]):
            assert not same(a, source[p]) and not same(a, unmasked[p]), f"{what} plane {p}: the expected plane is the source or the unmasked result"
            if p:
                assert not same(a, own[p]), f"{what} plane {p}: the expected plane is what the plane's own mask gives"


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


def _run_batches(case, form, kernel, expand, mask_kw=MASK):
    """Three frames in one call, then one more on the same context."""
    fmt, w, h, kw, ckw, skw, par = case
    clip = clip_format(fmt, w, h)
    frames, parities, res, want, own = lc.expected(case, kernel if form == "reduce" else None, expand)
    with SangNomAA(clip, max_batch=3, small_launches=capi.SN_SMALL_SWEEP, mask_expand=expand, **mask_kw, **_form_kw(form, kernel), **kw, **ckw) as aa:
        got = _batch(aa, clip, frames[:3], parities[:3] if par else None) + _batch(aa, clip, frames[3:], parities[3:] if par else None)
    return frames, res, want, own, got


@pytest.mark.parametrize("expand", lc.EXPANDS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("i", range(len(lc.BATCH)), ids=[f"{c[0]}-{c[1]}x{c[2]}-{i}" for i, c in enumerate(lc.BATCH)])
def test_batches_match_the_script_merged_through_lumas_mask(hip_lib, i, form, expand):
    for kernel in (lc.kernel_of(i) if form == "reduce" else [None]):
        frames, res, want, own, got = _run_batches(lc.BATCH[i], form, kernel, expand)
        for f in range(len(frames)):
            _assert_frame(want[f], got[f], f"frame {f}", frames[f], res[f], own[f])


@pytest.mark.parametrize("expand", lc.EXPANDS)
def test_chroma_that_is_not_processed_is_copied(hip_lib, expand):
    """Without dh, chroma=False: luma through its own mask, chroma is the source."""
    frames, res, want, own, got = _run_batches(lc.CHROMA_OFF, "plain", None, expand)
    for f in range(len(frames)):
        _assert_frame(want[f], got[f], f"frame {f}", frames[f], res[f], own[f], lc.processed_of(lc.CHROMA_OFF))
        assert same(frames[f][1], got[f][1]) and same(frames[f][2], got[f][2])


@pytest.mark.parametrize("form", FORMS)
def test_a_y_clip_accepts_the_option_and_it_has_no_effect(hip_lib, form):
    frames, res, want, own, got = _run_batches(lc.Y8, form, "halfband", 1)
    for f in range(len(frames)):
        _assert_frame(own[f], got[f], f"frame {f}", frames[f], res[f], own[f])


@pytest.mark.parametrize("form", FORMS)
def test_mask_chroma_own_is_the_existing_call(hip_lib, form):
    """A context made with mask_chroma="own" gives the own-mask expectation (tests/mask_model.merge_model) of the same frames."""
    case = lc.BATCH[0]
    frames, res, want, own, got = _run_batches(case, form, "halfband", 1, dict(mask=(lc.LO, lc.HI), mask_chroma="own"))
    for f in range(len(frames)):
        _assert_frame(own[f], got[f], f"frame {f}")
        assert not same(got[f][1], want[f][1])


@pytest.mark.parametrize("form", FORMS)
def test_a_tiny_scratch_budget_walks_a_batch_in_chunks(hip_lib, form):
    """YUV420P8 512x256: 3 x 196 608 bytes of intermediates per frame without dh (a budget of 1 MB holds one frame), nine plane
    sizes with dh and a reduction (2 MB hold one): a batch of three takes three chunks and gives the frames one chunk gives."""
    case = lc.CHUNK
    clip = clip_format(*case[:3])
    frames = lc.frames_of(*case[:3], count=3)
    with SangNomAA(clip, max_batch=3, **MASK, **_form_kw(form)) as aa:
        one = _batch(aa, clip, frames)
    with SangNomAA(clip, max_batch=3, scratch_budget_mb=2 if form == "reduce" else 1, **MASK, **_form_kw(form)) as aa:
        chunked = _batch(aa, clip, frames)
    fr, _, res, want, own = lc.expected(case, "halfband" if form == "reduce" else None, 1, count=1)
    for f in range(3):
        _assert_frame(one[f], chunked[f], f"frame {f} (chunked against one chunk)")
    _assert_frame(want[0], chunked[0], "frame 0 (script)", fr[0], res[0], own[0])


@pytest.mark.parametrize("form", FORMS)
def test_the_host_call_and_the_ring(hip_lib, form):
    """get_frame, then the ring: submit and collect, depth 4."""
    fmt, w, h, kw = lc.HOST[:4]
    clip = clip_format(fmt, w, h)
    frames, _, res, want, own = lc.expected(lc.HOST, "halfband" if form == "reduce" else None, 1)
    fkw = dict(_form_kw(form), **MASK, **kw)
    with SangNomAAHost(clip, host_depth=4, **fkw) as ring, SangNomAAHost(clip, **fkw) as sync:
        for k in range(2):
            _assert_frame(want[k], sync.get_frame(frames[k]), f"get_frame {k}", frames[k], res[k], own[k])
        n = ring.slots()
        assert 1 <= n <= 4
        got, pending, f = [], [], 0
        while len(got) < len(frames):
            while f < len(frames) and len(pending) < n:
                pending.append(ring.submit(frames[f]))
                f += 1
            got.append(ring.collect(pending.pop(0)))
        for k in range(len(frames)):
            _assert_frame(want[k], got[k], f"ring frame {k}", frames[k], res[k], own[k])


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
    case = lc.NV12
    clip = clip_format(*case[:3])
    frames, _, res, want, own = lc.expected(case, "halfband" if form == "reduce" else None, 1)
    frames, res, want, own = frames[:3], res[:3], want[:3], own[:3]
    with SangNomAA(clip, max_batch=3, **case[3], **MASK, **_form_kw(form)) as aa:
        src = _semi(clip, frames)
        dst = [torch.full_like(t, 0x5C) for t in src]
        torch.cuda.synchronize()
        aa.process_surfaces(src, dst)
        aa.synchronize()
    y, uv = to_host(dst[0]), to_host(dst[1])
    for f in range(3):
        _assert_frame(want[f], [y[f], uv[f][..., 0], uv[f][..., 1]], f"NV12 frame {f}", frames[f], res[f], own[f])


@pytest.mark.parametrize("form", FORMS)
def test_p010_in_planar_out(hip_lib, form):
    """A SEMIPLANAR_MSB source on a 10-bit context: the luma plane the chroma mask is built from is the shifted-down one of the luma scratch."""
    import torch
    case = lc.P010
    clip = clip_format(*case[:3])
    frames, _, res, want, own = lc.expected(case, "halfband" if form == "reduce" else None, 1, count=3)
    with SangNomAA(clip, max_batch=3, **case[3], **MASK, **_form_kw(form)) as aa:
        src = _semi(clip, frames, shift=6)
        dst = [torch.full((3,) + aa.plane_shape_out(p), 0x5C5C, dtype=torch.int16, device=src[0].device) for p in range(3)]
        torch.cuda.synchronize()
        aa.process_surfaces(src, dst, src_msb=True)
        aa.synchronize()
    for f in range(3):
        _assert_frame(want[f], [to_host(dst[p][f]).view(np.uint16) for p in range(3)], f"P010 frame {f}", frames[f], res[f], own[f])


@pytest.mark.parametrize("form", FORMS)
def test_planar_422_in_yuy2_out(hip_lib, form):
    import torch
    case = lc.YUY2
    clip = clip_format(*case[:3])
    frames, _, res, want, own = lc.expected(case, "halfband" if form == "reduce" else None, 1)
    with SangNomAA(clip, max_batch=3, **case[3], **MASK, **_form_kw(form)) as aa:
        src = _to_dev(clip, frames[:3])
        dst = torch.full((3, 64, 256), 0x5C, dtype=torch.uint8, device=src[0].device)
        torch.cuda.synchronize()
        aa.process_surfaces(src, dst, dst_packed="yuyv")
        aa.synchronize()
    got = to_host(dst)
    for f in range(3):
        assert all(not same(want[f][p], x[f][p]) for p in (1, 2) for x in (frames, res, own))
        a = pc.pack_yuyv(want[f][0], want[f][1], want[f][2], "yuyv")
        assert same(a, got[f]), f"YUY2 frame {f}: " + describe_diff(a, got[f])


# ---- the getter ------------------------------------------------------------------------------------------------------------------

def test_mask_ex_round_trips(hip_lib):
    clip = clip_format("YUV420P8", 128, 64)
    for name, value in (("luma", capi.SN_AA_MASK_CHROMA_LUMA), ("own", capi.SN_AA_MASK_CHROMA_OWN)):
        with SangNomAA(clip, mask=(7, 201), mask_chroma=name) as aa:
            m = aa.mask_ex
            assert (m.struct_size, m.chroma, list(m.reserved)) == (32, value, [0] * 6)
            short = capi.SnAAMaskEx(struct_size=28)
            assert capi.load().sn_aa_get_mask_ex(aa._h, ctypes.byref(short)) == capi.SN_ERR_INVALID_ARG
    with SangNomAA(clip) as aa:                       # no mask: the default
        assert aa.mask_ex.chroma == capi.SN_AA_MASK_CHROMA_OWN
    with SangNomAA(clip, mask_chroma="luma") as aa:   # ... and without a mask the field is ignored
        assert aa.mask_ex.chroma == capi.SN_AA_MASK_CHROMA_OWN
