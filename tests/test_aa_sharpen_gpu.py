"""The anti-aliasing call with contra-sharpening (sn_aa_create_ex5): every entry point against tests/sharpen_cases.expected --
merge_model(source, sharpen_model(source, unmasked model)), the stages in the library's order --, bit for bit: device batches,
chunks, the host call and ring, and semi-planar and MSB surfaces.  The frames are tests/mask_cases.py's, on which the stage
changes most samples and its limit acts (tests/test_aa_sharpen_cpu.py asserts it); every comparison also asserts that the
expected plane is not the unsharpened one."""
import ctypes

import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNomAA, SangNomAAHost, SangNomError, capi, clip_format
from tests import mask_cases as mc
from tests import sharpen_cases as sc
from tests.util import describe_diff, same, to_host

pytestmark = pytest.mark.gpu

VT = {1: np.uint8, 2: np.int16, 4: np.float32}  # torch has no uint16: same bits
FORMS = ["reduce", "plain"]  # dh + reduce, and without dh
MASKS = [None, sc.MASK]


def _assert_frame(want, got, what, plain=None, sharpened=None):
    """plain: the unsharpened expectation; sharpened[p]: whether plane p is (a plane that is not must equal it bit for bit)."""
    for p, (a, b) in enumerate(zip(want, got)):
        assert a.shape == b.shape, f"{what} plane {p}: shape {b.shape}, expected {a.shape}"
        assert same(a, b), f"{what} plane {p}: " + describe_diff(a, b)
        if plain is not None:
            if sharpened[p]:
                assert not same(a, plain[p]), f"{what} plane {p}: the expected plane is the unsharpened one"
            else:
                assert same(b, plain[p]), f"{what} plane {p}: a plane that is not sharpened differs from what the call gives without the stage"


def _sharpened(case, form, chroma):
    proc = mc.processed_of(case) if form == "plain" else [True] * len(mc.processed_of(case))
    return [proc[p] and (p == 0 or bool(chroma)) for p in range(len(proc))]


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


def _mask_kw(mask, mask_chroma="own"):
    return {} if mask is None else dict(mask=mask[:2], mask_expand=mask[2], mask_chroma=mask_chroma)


def _run_batches(case, form, kernel, amount, chroma, mask, mask_chroma="own"):
    fmt, w, h, kw, ckw, skw, par = case
    clip = clip_format(fmt, w, h)
    frames, parities, plain, want = sc.expected(case, kernel if form == "reduce" else None, amount, chroma, mask, mask_chroma=mask_chroma)
    with SangNomAA(clip, max_batch=5, sharpen=amount, sharpen_chroma=chroma, **_mask_kw(mask, mask_chroma), **_form_kw(form, kernel), **kw, **ckw) as aa:
        s = aa.sharpen
        assert (s.struct_size, s.amount, s.chroma, list(s.reserved)) == (32, amount, int(chroma), [0] * 5)
        assert all(aa.plane_shape_out(p) == aa.plane_shape(p) for p in range(clip.planes))
        got = _batch(aa, clip, frames[:5], parities[:5] if par else None) + _batch(aa, clip, frames[5:])
    sharpened = _sharpened(case, form, chroma)
    for f in range(len(frames)):
        _assert_frame(want[f], got[f], f"frame {f}", plain[f], sharpened)
    return frames, got


@pytest.mark.parametrize("mask", MASKS, ids=["unmasked", "masked"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("i", range(len(sc.BATCH)), ids=[f"{c[0]}-{c[1]}x{c[2]}-{i}" for i, c in enumerate(sc.BATCH)])
def test_batches_match_the_sharpened_script(hip_lib, i, form, mask):
    """Five frames in one call, then three more on the same context (row 10: order 0 with mixed parities; row 11: opt=1).  The
    first row with both reduce kernels and with amount 255 too; the YUV rows with chroma 0 and 1."""
    case = sc.BATCH[i]
    yuv = clip_format(case[0], case[1], case[2]).planes == 3
    for kernel in (mc.kernel_of(i) if form == "reduce" else [None]):
        for amount in ([sc.AMOUNT, 255] if i == 0 else [sc.AMOUNT]):
            for chroma in ([False, True] if yuv else [False]):
                _run_batches(case, form, kernel, amount, chroma, mask)


@pytest.mark.parametrize("form", FORMS)
def test_chroma_through_the_luma_mask_merges_the_sharpened_planes(hip_lib, form):
    _run_batches(sc.BATCH[7], form, "halfband", sc.AMOUNT, True, sc.MASK, mask_chroma="luma")


@pytest.mark.parametrize("chroma", [False, True])
def test_luma_that_is_not_processed_comes_back_as_a_copy(hip_lib, chroma):
    """Without dh, luma=False: luma is the source whatever the stage is told; chroma is sharpened only when asked."""
    frames, got = _run_batches(sc.LUMA_OFF, "plain", None, sc.AMOUNT, chroma, sc.MASK)
    for f in range(len(frames)):
        assert same(frames[f][0], got[f][0])


@pytest.mark.parametrize("form", FORMS)
def test_a_tiny_scratch_budget_walks_a_batch_in_chunks(hip_lib, form):
    """Y8 512x256: a plane is 131 072 bytes, and the sharpened plane's intermediate makes it four of them per frame without dh (a
    budget of 1 MB holds two frames) and ten with dh and a reduction (2 MB hold one): a batch of five takes three or five
    chunks and gives the frames one chunk gives."""
    clip = clip_format("Y8", 512, 256)
    plane = 512 * 256
    per_frame, budget = (10 * plane, 2 << 20) if form == "reduce" else (4 * plane, 1 << 20)
    cap = budget // per_frame
    assert cap == (1 if form == "reduce" else 2) and -(-5 // cap) == (5 if form == "reduce" else 3)
    frames = mc.frames_of("Y8", 512, 256, count=5)
    kw = dict(sharpen=sc.AMOUNT, **_mask_kw(sc.MASK), **_form_kw(form))
    with SangNomAA(clip, max_batch=5, **kw) as aa:
        one = _batch(aa, clip, frames)
    with SangNomAA(clip, max_batch=5, scratch_budget_mb=budget >> 20, **kw) as aa:
        chunked = _batch(aa, clip, frames)
    fr, _, plain, want = sc.expected(sc.CHUNK, "halfband" if form == "reduce" else None, sc.AMOUNT, False, sc.MASK, count=2)
    for f in range(5):
        _assert_frame(one[f], chunked[f], f"frame {f} (chunked against one chunk)")
        if f < 2:
            _assert_frame(want[f], chunked[f], f"frame {f} (script)", plain[f], [True])


def test_every_stage_at_once_with_a_chunk_boundary_inside_a_field_run(hip_lib):
    """dh, the half-band reduction, the sharpening on every plane and chroma through luma's mask, order 0 with parities 1,1,0,0,1
    -- the reduction is cut into the runs {0,1}, {2,3}, {4} of equal field offset -- under a budget whose chunks cut across the
    middle run.  A frame of intermediates is T1, U1, T2, E and S of every plane, each row padded to 256 bytes: for a w x h
    plane 256 (w + 2 w + h + 2 h + h) bytes, 327 680 for the 128x64 4:2:0 frame, so 1 MB (the smallest budget there is) holds
    three frames: chunks {0,1,2} and {3,4}."""
    fmt, w, h, kw = sc.BATCH[7][:4]
    parities = [1, 1, 0, 0, 1]
    case = (fmt, w, h, dict(kw, order=0), {}, {}, parities)
    clip = clip_format(fmt, w, h)
    assert clip.bytes == 1 and max(w, 2 * w, h) <= 256  # every pitch is 256
    per_frame = sum(256 * (pw + 2 * pw + ph + 2 * ph + ph) for pw, ph in [(w, h), (w >> clip.subw, h >> clip.subh), (w >> clip.subw, h >> clip.subh)])
    cap = (1 << 20) // per_frame
    assert per_frame == 327680 and cap == 3 and parities[cap - 1] == parities[cap]  # frames 2 and 3 are one run, in two chunks
    frames, _, plain, want = sc.expected(case, "halfband", sc.AMOUNT, True, sc.MASK, count=5, mask_chroma="luma")
    kw = dict(max_batch=5, sharpen=sc.AMOUNT, sharpen_chroma=True, **_mask_kw(sc.MASK, "luma"), **_form_kw("reduce"), **case[3])
    with SangNomAA(clip, **kw) as aa:
        one = _batch(aa, clip, frames, parities)
    with SangNomAA(clip, scratch_budget_mb=1, **kw) as aa:
        chunked = _batch(aa, clip, frames, parities)
    for f in range(5):
        _assert_frame(one[f], chunked[f], f"frame {f} (chunked against one chunk)")
        _assert_frame(want[f], chunked[f], f"frame {f} (script)", plain[f], [True] * 3)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("i", range(len(sc.HOST)), ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in sc.HOST])
def test_the_host_call_and_the_ring(hip_lib, i, form):
    """get_frame, then the ring: submit and collect, depth 4, 7 frames."""
    fmt, w, h, kw = sc.HOST[i]
    clip = clip_format(fmt, w, h)
    case = (fmt, w, h, kw, {}, {}, None)
    frames, _, plain, want = sc.expected(case, "halfband" if form == "reduce" else None, sc.AMOUNT, True, sc.MASK, count=7)
    fkw = dict(_form_kw(form), sharpen=sc.AMOUNT, sharpen_chroma=True, **_mask_kw(sc.MASK), **kw)
    sharpened = [True] * clip.planes
    with SangNomAAHost(clip, host_depth=4, **fkw) as ring, SangNomAAHost(clip, **fkw) as sync:
        assert sync.sharpen.amount == sc.AMOUNT and ring.sharpen.chroma == 1
        for k in range(2):
            _assert_frame(want[k], sync.get_frame(frames[k]), f"get_frame {k}", plain[k], sharpened)
        n = ring.slots()
        assert 1 <= n <= 4
        got, pending, f = [], [], 0
        while len(got) < len(frames):
            while f < len(frames) and len(pending) < n:
                pending.append(ring.submit(frames[f]))
                f += 1
            got.append(ring.collect(pending.pop(0)))
        for k in range(len(frames)):
            _assert_frame(want[k], got[k], f"ring frame {k}", plain[k], sharpened)


# ---- surfaces ------------------------------------------------------------------------------------------------------------------

def _semi(clip, frames, shift=0):
    import torch
    dev = torch.device("cuda:0")
    dt = clip.dtype
    return [torch.from_numpy((np.stack([fr[0] for fr in frames]).astype(dt) << shift).view(VT[clip.bytes])).pin_memory().to(dev),
            torch.from_numpy((np.stack([np.stack([fr[1], fr[2]], axis=-1) for fr in frames]).astype(dt) << shift).view(VT[clip.bytes])).pin_memory().to(dev)]


@pytest.mark.parametrize("form", FORMS)
def test_nv12_in_planar_out(hip_lib, form):
    """The sharpening runs on the planar scratch the UV plane is split into."""
    import torch
    case = sc.BATCH[7]
    clip = clip_format(case[0], case[1], case[2])
    frames, _, plain, want = sc.expected(case, "halfband" if form == "reduce" else None, sc.AMOUNT, True, sc.MASK)
    with SangNomAA(clip, max_batch=3, aac=48, sharpen=sc.AMOUNT, sharpen_chroma=True, **_mask_kw(sc.MASK), **_form_kw(form)) as aa:
        src = _semi(clip, frames[:3])
        dst = [torch.full((3,) + aa.plane_shape_out(p), 0x5C, dtype=torch.uint8, device=src[0].device) for p in range(3)]
        torch.cuda.synchronize()
        aa.process_surfaces(src, dst)
        aa.synchronize()
    for f in range(3):
        _assert_frame(want[f], [to_host(dst[p][f]) for p in range(3)], f"NV12 frame {f}", plain[f], [True] * 3)


@pytest.mark.parametrize("chroma", [False, True])
def test_p010_in_planar_out_without_dh(hip_lib, chroma):
    """A SEMIPLANAR_MSB source on a 10-bit context: the planes the stage reads are the unpacked, shifted-down ones, all lines."""
    import torch
    clip = clip_format(*sc.P010[:3])
    frames, _, plain, want = sc.expected(sc.P010, None, sc.AMOUNT, chroma, sc.MASK, count=3)
    with SangNomAA(clip, max_batch=3, aac=48, sharpen=sc.AMOUNT, sharpen_chroma=chroma, **_mask_kw(sc.MASK)) as aa:
        src = _semi(clip, frames, shift=6)
        dst = [torch.full((3,) + aa.plane_shape_out(p), 0x5C5C, dtype=torch.int16, device=src[0].device) for p in range(3)]
        torch.cuda.synchronize()
        aa.process_surfaces(src, dst, src_msb=True)
        aa.synchronize()
    for f in range(3):
        _assert_frame(want[f], [to_host(dst[p][f]).view(np.uint16) for p in range(3)], f"P010 frame {f}", plain[f], [True, chroma, chroma])


def test_p010_in_p010_out_with_reduce(hip_lib):
    """MSB-aligned on both sides, dh and the half-band reduction: the sharpened 10-bit planes are valid in the destination's high bits."""
    import torch
    clip = clip_format(*sc.P010[:3])
    frames, _, plain, want = sc.expected(sc.P010, "halfband", sc.AMOUNT, True, None, count=3)
    with SangNomAA(clip, max_batch=3, aac=48, sharpen=sc.AMOUNT, sharpen_chroma=True, **_form_kw("reduce")) as aa:
        src = _semi(clip, frames, shift=6)
        dst = [torch.full_like(t, 0x5C5C) for t in src]
        torch.cuda.synchronize()
        aa.process_surfaces(src, dst, src_msb=True, dst_msb=True)
        aa.synchronize()
    y, uv = to_host(dst[0]).view(np.uint16), to_host(dst[1]).view(np.uint16)
    assert not (y & 63).any() and not (uv & 63).any()
    for f in range(3):
        _assert_frame(want[f], [y[f] >> 6, uv[f][..., 0] >> 6, uv[f][..., 1] >> 6], f"P010 frame {f}", plain[f], [True] * 3)


# ---- unchanged paths, the getter, the refusal ----------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
def test_a_context_made_through_ex4_gives_todays_frames(hip_lib, form):
    """sn_aa_create_ex4 directly, and the filter with sharpen=None and sharpen=0: the unsharpened, masked frames."""
    case = sc.BATCH[7]
    clip = clip_format(case[0], case[1], case[2])
    frames, _, plain, _ = sc.expected(case, "halfband" if form == "reduce" else None, sc.AMOUNT, True, sc.MASK)
    L = capi.load()
    for how in ("ex4", None, 0):
        with SangNomAA(clip, max_batch=3, aac=48, sharpen=None if how == "ex4" else how, **_mask_kw(sc.MASK), **_form_kw(form)) as aa:
            if how == "ex4":  # the same context again, made by the older entry point
                cfg = capi.SnConfig(struct_size=ctypes.sizeof(capi.SnConfig), width=clip.width, height=clip.height, bytes_per_sample=clip.bytes,
                                    bits_per_sample=clip.bits, num_planes=clip.planes, sub_w=clip.subw, sub_h=clip.subh, order=1, aa=48, aac=48,
                                    dh=int(form == "reduce"), luma=1, chroma=1, device=0, max_batch=3, mode=capi.SN_MODE_AUTO, host_depth=0,
                                    isolated_planes=0, fresh_pool=0, stream=None)
                pol, opts = capi.policy(), capi.options()
                aopts, amask = capi.aa_options("halfband" if form == "reduce" else 0), capi.aa_mask(sc.MASK[:2], sc.MASK[2])
                L.sn_aa_destroy(aa._h)
                aa._h = ctypes.c_void_p()
                assert L.sn_aa_create_ex4(ctypes.byref(cfg), ctypes.byref(pol), ctypes.byref(opts), ctypes.byref(aopts), ctypes.byref(amask), None,
                                          ctypes.byref(aa._h)) == capi.SN_OK, L.sn_aa_last_error(None)
            assert aa.sharpen.amount == 0
            got = _batch(aa, clip, frames[:3])
        for f in range(3):
            _assert_frame(plain[f], got[f], f"{how}: frame {f}")


def test_the_getter_and_the_refusals(hip_lib):
    clip = clip_format("YUV420P8", 128, 64)
    with SangNomAA(clip, sharpen=201, sharpen_chroma=True) as aa:
        s = aa.sharpen
        assert (s.struct_size, s.amount, s.chroma, list(s.reserved)) == (32, 201, 1, [0] * 5)
        short = capi.SnAASharpen(struct_size=28)
        assert capi.load().sn_aa_get_sharpen(aa._h, ctypes.byref(short)) == capi.SN_ERR_INVALID_ARG
    with SangNomAA(clip, sharpen=0, sharpen_chroma=True) as aa:
        assert (aa.sharpen.amount, aa.sharpen.chroma) == (0, 0)
    with pytest.raises(SangNomError) as e:
        SangNomAA(clip, dh=True, sharpen=64)
    assert e.value.code == capi.SN_ERR_CONFIG and "sharpen needs the frame at source size" in str(e.value)
    with pytest.raises(SangNomError) as e:
        SangNomAAHost(clip, sharpen=256)
    assert e.value.code == capi.SN_ERR_INVALID_ARG and "sn_aa_sharpen.amount" in str(e.value)
