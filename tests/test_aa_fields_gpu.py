"""The anti-aliasing call with both fields (sn_aa_create_ex6, fields="both") against tests/fields_model.BothScript, bit for
bit: every row of tests/fields_cases.py as a device batch, a batch walked in chunks, the host call and ring, NV12 surfaces, the
invariance against order and parity, and the getters.  tests/test_aa_fields_cpu.py asserts that the expected frames differ
from either one-field frame in most samples and that the last average rounds in half of them."""
import ctypes

import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNomAA, SangNomAAHost, capi, clip_format
from tests import fields_cases as fc
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


@pytest.mark.parametrize("i", range(len(fc.CASES)), ids=fc.IDS)
def test_batches_match_the_both_fields_script(hip_lib, i):
    """The first frame in a call of its own, the rest in one batch on the same context: the four instances carry their history
    from call to call."""
    case = fc.CASES[i]
    clip = clip_format(case.fmt, case.w, case.h)
    frames, want, _ = fc.expected(i)
    with SangNomAA(clip, max_batch=len(frames), **fc.lib_kw(case)) as aa:
        assert aa.fields.mode == capi.SN_AA_FIELDS_BOTH
        got = _batch(aa, clip, frames[:1]) + _batch(aa, clip, frames[1:])
    for f in range(len(frames)):
        _assert_frame(want[f], got[f], f"{fc.IDS[i]} frame {f}")
    for p in range(clip.planes):  # and that is not what one field gives (luma=False: a copied plane is the source either way)
        assert same(want[0][p], fc.one_field(i, 1)[p]) == (p == 0 and case.kw.get("luma") is False)


def test_a_tiny_scratch_budget_walks_a_batch_in_chunks(hip_lib):
    """Y8 328x200 (rows of the clip padded to 512 bytes, of the turned clip to 256): a frame of intermediates is T1, U1 and U1B,
    256 x 328 each, and T2 and D2, 512 x 200 each: 456 704 bytes.  1 MB, the smallest budget there is, holds two, so a batch
    of five runs in the chunks {0,1}, {2,3}, {4} and gives what one chunk gives; the first two frames also against the script."""
    clip = clip_format("Y8", 328, 200)
    per_frame = 3 * 256 * 328 + 2 * 512 * 200
    assert per_frame == 456704 and (1 << 20) // per_frame == 2
    case = fc.C("Y8", 328, 200, frames=5)
    frames = fc.frames_of(case)
    with SangNomAA(clip, max_batch=5, fields="both") as aa:
        one = _batch(aa, clip, frames)
    with SangNomAA(clip, max_batch=5, fields="both", scratch_budget_mb=1) as aa:
        chunked = _batch(aa, clip, frames)
    from tests.fields_model import BothScript
    script = BothScript(clip)
    for f in range(5):
        _assert_frame(one[f], chunked[f], f"frame {f} (chunked against one chunk)")
        if f < 2:
            _assert_frame(script.frame(frames[f]), chunked[f], f"frame {f} (script)")


@pytest.mark.parametrize("i", [fc.HISTORY_Y8, fc.YUV420, fc.STAGES_YUV], ids=["Y8-72x40", "YUV420P8", "YUV420P8-stages"])
def test_the_host_call_and_the_ring(hip_lib, i):
    """get_frame on one context, then the ring on another: submit and collect, depth 4, 6 frames."""
    case = fc.CASES[i]
    clip = clip_format(case.fmt, case.w, case.h)
    frames, want, _ = fc.expected(i, count=6)
    kw = fc.lib_kw(case)
    with SangNomAAHost(clip, host_depth=4, **kw) as ring, SangNomAAHost(clip, **kw) as sync:
        assert sync.fields.mode == 1 and ring.fields.mode == 1
        for k in range(2):
            _assert_frame(want[k], sync.get_frame(frames[k]), f"get_frame {k}")
        n = ring.slots()
        assert 1 <= n <= 4
        got, pending, f = [], [], 0
        while len(got) < len(frames):
            while f < len(frames) and len(pending) < n:
                pending.append(ring.submit(frames[f], parity=f & 1))
                f += 1
            got.append(ring.collect(pending.pop(0)))
        for k in range(len(frames)):
            _assert_frame(want[k], got[k], f"ring frame {k}")


def test_nv12_in_nv12_out(hip_lib):
    """The passes, the turn of the average and the average run on the planar scratch the UV plane is split into."""
    import torch
    case = fc.CASES[fc.YUV420]
    clip = clip_format(case.fmt, case.w, case.h)
    frames, want, _ = fc.expected(fc.YUV420)
    dev = torch.device("cuda:0")
    with SangNomAA(clip, max_batch=2, **fc.lib_kw(case)) as aa:
        src = [torch.from_numpy(np.stack([fr[0] for fr in frames])).pin_memory().to(dev),
               torch.from_numpy(np.stack([np.stack([fr[1], fr[2]], axis=-1) for fr in frames])).pin_memory().to(dev)]
        dst = [torch.full_like(t, 0x5C) for t in src]
        torch.cuda.synchronize()
        aa.process_surfaces(src, dst)
        aa.synchronize()
        si = aa.surface_info()
        assert (si.split_frames, si.merged_frames) == (2, 2)
    y, uv = to_host(dst[0]), to_host(dst[1])
    for f in range(2):
        _assert_frame(want[f], [y[f], uv[f][..., 0], uv[f][..., 1]], f"NV12 frame {f}")


def test_order_and_parity_have_no_influence(hip_lib):
    """Three frames of the history-carrying row with every order and with mixed parities: the same bytes, the model's."""
    i = fc.HISTORY_Y8
    case = fc.CASES[i]
    clip = clip_format(case.fmt, case.w, case.h)
    frames, want, _ = fc.expected(i)
    for order in (0, 1, 2):
        for parity in (None, [0, 1, 0], [0, 0, 1]):
            with SangNomAA(clip, max_batch=3, order=order, **fc.lib_kw(case)) as aa:
                got = _batch(aa, clip, frames, parity)
            for f in range(len(frames)):
                _assert_frame(want[f], got[f], f"order {order} parities {parity} frame {f}")


def test_the_getters_report_the_twins(hip_lib):
    clip = clip_format("Y8", 72, 40)
    case = fc.CASES[fc.HISTORY_Y8]
    frames = fc.frames_of(case)
    L = capi.load()
    with SangNomAA(clip, max_batch=3, fields="both") as aa:
        f = aa.fields
        assert (f.struct_size, f.mode, list(f.reserved)) == (32, capi.SN_AA_FIELDS_BOTH, [0] * 6)
        short = capi.SnAAFields(struct_size=28)
        assert L.sn_aa_get_fields(aa._h, ctypes.byref(short)) == capi.SN_ERR_INVALID_ARG
        _batch(aa, clip, frames)
        for p in (0, 1):  # a twin is an instance of its own with its pass's geometry, and has seen every frame
            a, b = aa.info(p), aa.info(p + 2)
            assert (a.out_height, a.pool_stride, a.pool_rows, a.history_free) == (b.out_height, b.pool_stride, b.pool_rows, b.history_free)
            assert a.frames == b.frames == len(frames)
            assert list(aa.parts_info(p + 2).parts) == list(aa.parts_info(p).parts)
        assert aa.info(2).out_height == 72 and aa.info(3).out_height == 40  # the turned clip's, the clip's
        info = capi.SnInfo(struct_size=ctypes.sizeof(capi.SnInfo))
        assert L.sn_aa_get_info(aa._h, 4, ctypes.byref(info)) == capi.SN_ERR_INVALID_ARG
    with SangNomAA(clip, fields="one") as aa:  # one field: no twins
        assert aa.fields.mode == capi.SN_AA_FIELDS_ONE
        info, parts = capi.SnInfo(struct_size=ctypes.sizeof(capi.SnInfo)), capi.SnPartsInfo(struct_size=ctypes.sizeof(capi.SnPartsInfo))
        for p in (2, 3):
            assert L.sn_aa_get_info(aa._h, p, ctypes.byref(info)) == capi.SN_ERR_INVALID_ARG
            assert L.sn_aa_get_parts_info(aa._h, p, ctypes.byref(parts)) == capi.SN_ERR_INVALID_ARG


def test_one_field_through_ex6_gives_todays_frames(hip_lib):
    """fields="one" (and the default) is the one-field script of the context's order."""
    i = fc.HISTORY_Y8
    case = fc.CASES[i]
    clip = clip_format(case.fmt, case.w, case.h)
    from tests.aa_script import Script
    frames = fc.frames_of(case)
    for kw in (dict(fields="one"), {}):
        script = Script(clip, order=2)
        with SangNomAA(clip, max_batch=3, order=2, **kw) as aa:
            got = _batch(aa, clip, frames)
        for f in range(len(frames)):
            _assert_frame(script.frame(frames[f]), got[f], f"{kw} frame {f}")
