"""The anti-aliasing call with the rank repair (sn_aa_create_ex7): every entry point against tests/repair_cases.expected --
merge_model(source, repair_model(source, sharpen_model(source, unmasked model))), the stages in the library's order --, bit for
bit: device batches, chunks, the host call and ring, both fields, and semi-planar and MSB surfaces.  The frames are
tests/mask_cases.py's, on which every repaired plane has samples clamped to each bound (tests/test_aa_repair_cpu.py asserts
it); every comparison also asserts that the expected plane is not the unrepaired one, and that a plane which is not repaired is
today's, bit for bit."""
import ctypes

import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNomAA, SangNomAAHost, SangNomError, capi, clip_format
from tests import fields_cases as fc
from tests import repair_cases as rc
from tests.util import describe_diff, same, to_host

pytestmark = pytest.mark.gpu

VT = {1: np.uint8, 2: np.int16, 4: np.float32}  # torch has no uint16: same bits
LUMA_MASK_ROW = 7  # YUV420P8 128x64


def _assert_frame(want, got, what, plain=None, repaired=None):
    """plain: the unrepaired expectation; repaired[p]: whether plane p is (a plane that is not must equal it bit for bit)."""
    for p, (a, b) in enumerate(zip(want, got)):
        assert a.shape == b.shape, f"{what} plane {p}: shape {b.shape}, expected {a.shape}"
        assert same(a, b), f"{what} plane {p}: " + describe_diff(a, b)
        if plain is not None and not repaired[p]:
            assert same(b, plain[p]), f"{what} plane {p}: a plane that is not repaired differs from what the call gives without the stage"


def _assert_changed(want, plain, repaired, what):
    """On frame 0 the repair shows in every repaired plane."""
    for p in range(len(want)):
        if repaired[p]:
            assert not same(want[p], plain[p]), f"{what} plane {p}: the expected plane is the unrepaired one"


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


def _form_kw(form):
    return dict(dh=True, reduce=form) if form else {}


def _stage_kw(sharpen, mask, mask_chroma="own"):
    kw = {} if sharpen is None else dict(sharpen=sharpen[0], sharpen_chroma=sharpen[1])
    if mask is not None:
        kw.update(mask=mask[:2], mask_expand=mask[2], mask_chroma=mask_chroma)
    return kw


def _run_batches(case, form, rank, chroma, sharpen=None, mask=None, mask_chroma="own"):
    fmt, w, h, kw, ckw, skw, par = case
    clip = clip_format(fmt, w, h)
    frames, parities, plain, want = rc.expected(case, form, rank, chroma, sharpen, mask, mask_chroma=mask_chroma)
    with SangNomAA(clip, max_batch=5, repair=rank, repair_chroma=chroma, **_stage_kw(sharpen, mask, mask_chroma), **_form_kw(form), **kw, **ckw) as aa:
        s = aa.repair
        assert (s.struct_size, s.rank, s.chroma, list(s.reserved)) == (32, rank, int(chroma), [0] * 5)
        assert all(aa.plane_shape_out(p) == aa.plane_shape(p) for p in range(clip.planes))
        got = _batch(aa, clip, frames[:5], parities[:5] if par else None) + _batch(aa, clip, frames[5:])
    repaired = rc.repaired_planes(case, form, chroma)
    if mask is None:
        _assert_changed(want[0], plain[0], repaired, "frame 0")
    for f in range(len(frames)):
        _assert_frame(want[f], got[f], f"frame {f}", plain[f], repaired)
    return frames, got


@pytest.mark.parametrize("rank", rc.RANKS)
@pytest.mark.parametrize("i", range(len(rc.BATCH)), ids=[f"{c[0]}-{c[1]}x{c[2]}-{i}" for i, c in enumerate(rc.BATCH)])
def test_batches_match_the_repaired_script(hip_lib, i, rank):
    """Repair alone: five frames in one call, then three more on the same context (row 10: order 0 with mixed parities; row 11:
    opt=1), without dh and with dh and the half-band reduction (row 0: the tent too); the subsampled rows with chroma 0 and 1."""
    case = rc.BATCH[i]
    for form in rc.forms_of(case):
        for chroma in rc.chromas_of(case):
            _run_batches(case, form, rank, chroma)


@pytest.mark.parametrize("rank", rc.RANKS)
@pytest.mark.parametrize("stages", ["sharpen", "mask", "sharpen+mask"])
@pytest.mark.parametrize("i", [0, 4, 7], ids=lambda i: f"{rc.BATCH[i][0]}-{i}")
def test_behind_the_sharpening_and_before_the_mask(hip_lib, i, stages, rank):
    case = rc.BATCH[i]
    sharpen = (rc.AMOUNT, True) if "sharpen" in stages else None
    mask = rc.MASK if "mask" in stages else None
    for form in (None, "halfband"):
        _run_batches(case, form, rank, rc.chromas_of(case)[-1], sharpen, mask)


@pytest.mark.parametrize("form", [None, "halfband"])
def test_chroma_through_the_luma_mask_merges_the_repaired_planes(hip_lib, form):
    _run_batches(rc.BATCH[LUMA_MASK_ROW], form, 3, True, (rc.AMOUNT, True), rc.MASK, mask_chroma="luma")


@pytest.mark.parametrize("chroma", [False, True])
def test_luma_that_is_not_processed_comes_back_as_a_copy(hip_lib, chroma):
    """Without dh, luma=False: luma is the source whatever the stage is told; chroma is repaired only when asked."""
    for rank in rc.RANKS:
        frames, got = _run_batches(rc.LUMA_OFF, None, rank, chroma)
        for f in range(len(frames)):
            assert same(frames[f][0], got[f][0])


@pytest.mark.parametrize("i", rc.BOTH_ROWS)
def test_both_fields(hip_lib, i):
    """tests/fields_model.BothScript gives the averaged frames; the row's own sharpening and mask stand around the repair."""
    case = fc.CASES[i]
    clip = clip_format(case.fmt, case.w, case.h)
    for rank in rc.RANKS:
        frames, plain, want = rc.expected_both(i, rank, True)
        with SangNomAA(clip, max_batch=len(frames), repair=rank, repair_chroma=True, **fc.lib_kw(case)) as aa:
            assert (aa.repair.rank, aa.repair.chroma, aa.fields.mode) == (rank, 1, capi.SN_AA_FIELDS_BOTH)
            got = _batch(aa, clip, frames)
        for f in range(len(frames)):
            _assert_frame(want[f], got[f], f"rank {rank} frame {f}")
        assert not any(same(a, b) for a, b in zip(want[0], plain[0]))  # (tests/test_aa_repair_cpu.py asserts it of frame 0)


@pytest.mark.parametrize("form", [None, "halfband"])
def test_a_tiny_scratch_budget_walks_a_batch_in_chunks(hip_lib, form):
    """Y8 512x256: a plane is 131 072 bytes.  The repair adds no intermediate: three of them per frame without dh (a budget of
    1 MB holds two frames) and nine with dh and a reduction (2 MB hold one).  A batch of five takes three or five chunks and
    gives the frames one chunk gives."""
    clip = clip_format("Y8", 512, 256)
    plane = 512 * 256
    per_frame, budget = (9 * plane, 2 << 20) if form else (3 * plane, 1 << 20)
    cap = budget // per_frame
    assert cap == (1 if form else 2) and -(-5 // cap) == (5 if form else 3)
    frames, _, plain, want = rc.expected(rc.CHUNK, form, 3, False, None, rc.MASK, count=5)
    kw = dict(repair=3, **_stage_kw(None, rc.MASK), **_form_kw(form))
    with SangNomAA(clip, max_batch=5, **kw) as aa:
        one = _batch(aa, clip, frames)
    with SangNomAA(clip, max_batch=5, scratch_budget_mb=budget >> 20, **kw) as aa:
        chunked = _batch(aa, clip, frames)
    for f in range(5):
        _assert_frame(one[f], chunked[f], f"frame {f} (chunked against one chunk)")
        _assert_frame(want[f], chunked[f], f"frame {f} (script)")
        assert not same(want[f][0], plain[f][0])


@pytest.mark.parametrize("form", [None, "halfband"])
@pytest.mark.parametrize("i", range(len(rc.HOST)), ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in rc.HOST])
def test_the_host_call_and_the_ring(hip_lib, i, form):
    """get_frame, then the ring: submit and collect, depth 4, 7 frames."""
    fmt, w, h, kw = rc.HOST[i]
    clip = clip_format(fmt, w, h)
    case = (fmt, w, h, kw, {}, {}, None)
    frames, _, plain, want = rc.expected(case, form, 1, True, (rc.AMOUNT, False), rc.MASK, count=7)
    fkw = dict(_form_kw(form), repair=1, repair_chroma=True, **_stage_kw((rc.AMOUNT, False), rc.MASK), **kw)
    with SangNomAAHost(clip, host_depth=4, **fkw) as ring, SangNomAAHost(clip, **fkw) as sync:
        assert sync.repair.rank == 1 and ring.repair.chroma == 1
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
            assert not all(same(a, b) for a, b in zip(want[k], plain[k]))


# ---- surfaces ------------------------------------------------------------------------------------------------------------------

def _semi(clip, frames, shift=0):
    import torch
    dev = torch.device("cuda:0")
    dt = clip.dtype
    return [torch.from_numpy((np.stack([fr[0] for fr in frames]).astype(dt) << shift).view(VT[clip.bytes])).pin_memory().to(dev),
            torch.from_numpy((np.stack([np.stack([fr[1], fr[2]], axis=-1) for fr in frames]).astype(dt) << shift).view(VT[clip.bytes])).pin_memory().to(dev)]


@pytest.mark.parametrize("form", [None, "halfband"])
def test_nv12_in_planar_out(hip_lib, form):
    """The repair reads the planar scratch the UV plane is split into."""
    import torch
    case = rc.BATCH[LUMA_MASK_ROW]
    clip = clip_format(case[0], case[1], case[2])
    frames, _, plain, want = rc.expected(case, form, 3, True, None, rc.MASK, count=3)
    with SangNomAA(clip, max_batch=3, aac=48, repair=3, repair_chroma=True, **_stage_kw(None, rc.MASK), **_form_kw(form)) as aa:
        src = _semi(clip, frames)
        dst = [torch.full((3,) + aa.plane_shape_out(p), 0x5C, dtype=torch.uint8, device=src[0].device) for p in range(3)]
        torch.cuda.synchronize()
        aa.process_surfaces(src, dst)
        aa.synchronize()
    for f in range(3):
        _assert_frame(want[f], [to_host(dst[p][f]) for p in range(3)], f"NV12 frame {f}")
        assert not any(same(a, b) for a, b in zip(want[f], plain[f]))


@pytest.mark.parametrize("chroma", [False, True])
def test_p010_in_planar_out_without_dh(hip_lib, chroma):
    """A SEMIPLANAR_MSB source on a 10-bit context: the planes the stage reads are the unpacked, shifted-down ones, all lines."""
    import torch
    clip = clip_format(*rc.P010[:3])
    frames, _, plain, want = rc.expected(rc.P010, None, 1, chroma, None, None, count=3)
    with SangNomAA(clip, max_batch=3, aac=48, repair=1, repair_chroma=chroma) as aa:
        src = _semi(clip, frames, shift=6)
        dst = [torch.full((3,) + aa.plane_shape_out(p), 0x5C5C, dtype=torch.int16, device=src[0].device) for p in range(3)]
        torch.cuda.synchronize()
        aa.process_surfaces(src, dst, src_msb=True)
        aa.synchronize()
    _assert_changed(want[0], plain[0], [True, chroma, chroma], "P010 frame 0")
    for f in range(3):
        _assert_frame(want[f], [to_host(dst[p][f]).view(np.uint16) for p in range(3)], f"P010 frame {f}", plain[f], [True, chroma, chroma])


def test_p010_in_p010_out_with_reduce(hip_lib):
    """MSB-aligned on both sides, dh and the half-band reduction, every stage."""
    import torch
    clip = clip_format(*rc.P010[:3])
    frames, _, plain, want = rc.expected(rc.P010, "halfband", 3, True, (rc.AMOUNT, True), rc.MASK, count=3)
    with SangNomAA(clip, max_batch=3, aac=48, repair=3, repair_chroma=True, **_stage_kw((rc.AMOUNT, True), rc.MASK), **_form_kw("halfband")) as aa:
        src = _semi(clip, frames, shift=6)
        dst = [torch.full_like(t, 0x5C5C) for t in src]
        torch.cuda.synchronize()
        aa.process_surfaces(src, dst, src_msb=True, dst_msb=True)
        aa.synchronize()
    y, uv = to_host(dst[0]).view(np.uint16), to_host(dst[1]).view(np.uint16)
    assert not (y & 63).any() and not (uv & 63).any()
    for f in range(3):
        _assert_frame(want[f], [y[f] >> 6, uv[f][..., 0] >> 6, uv[f][..., 1] >> 6], f"P010 frame {f}")
        assert not any(same(a, b) for a, b in zip(want[f], plain[f]))


# ---- unchanged paths, the getter, the refusal ----------------------------------------------------------------------------------

@pytest.mark.parametrize("form", [None, "halfband"])
def test_a_context_made_through_ex6_gives_todays_frames(hip_lib, form):
    """sn_aa_create_ex6 directly, and the filter with repair=None and repair=0: the unrepaired frames."""
    case = rc.BATCH[LUMA_MASK_ROW]
    clip = clip_format(case[0], case[1], case[2])
    frames, _, plain, _ = rc.expected(case, form, 2, True, (rc.AMOUNT, False), rc.MASK, count=3)
    L = capi.load()
    for how in ("ex6", None, 0):
        with SangNomAA(clip, max_batch=3, aac=48, repair=None if how == "ex6" else how, repair_chroma=True, **_stage_kw((rc.AMOUNT, False), rc.MASK),
                       **_form_kw(form)) as aa:
            if how == "ex6":  # the same context again, made by the older entry point
                cfg = capi.SnConfig(struct_size=ctypes.sizeof(capi.SnConfig), width=clip.width, height=clip.height, bytes_per_sample=clip.bytes,
                                    bits_per_sample=clip.bits, num_planes=clip.planes, sub_w=clip.subw, sub_h=clip.subh, order=1, aa=48, aac=48,
                                    dh=int(bool(form)), luma=1, chroma=1, device=0, max_batch=3, mode=capi.SN_MODE_AUTO, host_depth=0,
                                    isolated_planes=0, fresh_pool=0, stream=None)
                pol, opts = capi.policy(), capi.options()
                aopts, amask = capi.aa_options(form or 0), capi.aa_mask(rc.MASK[:2], rc.MASK[2])
                asharpen = capi.aa_sharpen(rc.AMOUNT, False)
                L.sn_aa_destroy(aa._h)
                aa._h = ctypes.c_void_p()
                assert L.sn_aa_create_ex6(ctypes.byref(cfg), ctypes.byref(pol), ctypes.byref(opts), ctypes.byref(aopts), ctypes.byref(amask), None,
                                          ctypes.byref(asharpen), None, ctypes.byref(aa._h)) == capi.SN_OK, L.sn_aa_last_error(None)
            assert (aa.repair.rank, aa.repair.chroma) == (0, 0)
            got = _batch(aa, clip, frames)
        for f in range(3):
            _assert_frame(plain[f], got[f], f"{how}: frame {f}")


def test_the_getter_and_the_refusals(hip_lib):
    clip = clip_format("YUV420P8", 128, 64)
    with SangNomAA(clip, repair=4, repair_chroma=True) as aa:
        s = aa.repair
        assert (s.struct_size, s.rank, s.chroma, list(s.reserved)) == (32, 4, 1, [0] * 5)
        short = capi.SnAARepair(struct_size=28)
        assert capi.load().sn_aa_get_repair(aa._h, ctypes.byref(short)) == capi.SN_ERR_INVALID_ARG
    with SangNomAA(clip, repair=0, repair_chroma=True) as aa:
        assert (aa.repair.rank, aa.repair.chroma) == (0, 0)
    with pytest.raises(SangNomError) as e:
        SangNomAA(clip, dh=True, repair=1)
    assert e.value.code == capi.SN_ERR_CONFIG and "repair needs the frame at source size" in str(e.value)
    with pytest.raises(ValueError):
        SangNomAAHost(clip, repair=5)
