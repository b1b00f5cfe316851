"""Semi-planar device surfaces -- NV12, P010 / P016, NV16, NV24 -- in and out of sn_process_device_surfaces and
sn_aa_process_device_surfaces.  The result for a semi-planar surface has to be, bit for bit, what the planar call gives on the
de-interleaved planes, re-interleaved: the expected frames are the CPU oracle's on the planar planes (tests/surface_cases.py),
interleaved by numpy.  Tolerance zero everywhere."""
import ctypes

import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2, SangNomAA, capi, clip_format, synth
from tests import layout_cases as lc
from tests import surface_cases as sc
from tests.util import describe_diff, same, to_host

pytestmark = pytest.mark.gpu

VT = {1: np.uint8, 2: np.int16, 4: np.float32}  # torch has no uint16: same bits


def _dev():
    import torch
    return torch.device("cuda:0")


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(VT[a.dtype.itemsize])).pin_memory().to(_dev())


def _planar(clip, frames):
    """Per plane a device tensor [N, H_p, W_p]."""
    return [_up(np.stack([fr[p] for fr in frames])) for p in range(clip.planes)]


def _semi(clip, frames):
    """[Y [N, H, W], UV [N, Hc, Wc, 2]]."""
    return [_up(np.stack([fr[0] for fr in frames])), _up(np.stack([sc.interleave(fr[1], fr[2]) for fr in frames]))]


def _empty(clip, n, shape_of, semi, fill=0x5C):
    import torch
    dt = {1: torch.uint8, 2: torch.int16, 4: torch.float32}[clip.bytes]
    shapes = [(n,) + tuple(shape_of(0)), (n,) + tuple(shape_of(1)) + (2,)] if semi else [(n,) + tuple(shape_of(p)) for p in range(clip.planes)]
    out = []
    for s in shapes:
        t = torch.empty(s, dtype=torch.uint8, device=_dev()) if clip.bytes == 1 else torch.empty(s, dtype=dt, device=_dev())
        t.view(torch.uint8).fill_(fill)
        out.append(t)
    return out


def _host_frames(clip, tensors, n):
    """Device surfaces of either layout -> per frame the PLANAR planes on the host."""
    host = [to_host(t).view(clip.dtype) for t in tensors]
    if len(host) == 2 and host[1].ndim == 4:
        host = [host[0], host[1][..., 0], host[1][..., 1]]
    return [[host[p][f] for p in range(len(host))] for f in range(n)]


def _assert_frames(want, got, what):
    assert len(want) == len(got)
    for f, (a, b) in enumerate(zip(want, got)):
        assert len(a) == len(b), f"{what} frame {f}: {len(b)} planes"
        for p, (x, y) in enumerate(zip(a, b)):
            assert x.shape == y.shape, f"{what} frame {f} plane {p}: shape {y.shape}, expected {x.shape}"
            assert same(x, y), f"{what} frame {f} plane {p}: " + describe_diff(x, y)


def _context(case, **extra):
    kw = dict(max_batch=case.n, mode=case.mode)
    if case.path == "sweep":
        kw["small_launches"] = capi.SN_SMALL_SWEEP
    kw.update(extra)
    return SangNom2(clip_format(case.fmt, case.w, case.h), **case.kw, **case.ckw, **kw)


def _run(flt, clip, frames, par, src_semi=True, dst_semi=True):
    import torch
    n = len(frames)
    src = _semi(clip, frames) if src_semi else _planar(clip, frames)
    dst = _empty(clip, n, flt.plane_shape_out, dst_semi)
    torch.cuda.synchronize()
    flt.process_surfaces(src, dst, par)
    flt.synchronize()
    return _host_frames(clip, dst, n), src


def _info(flt):
    i = flt.surface_info()
    return i.scratch_bytes, i.split_frames, i.merged_frames, i.copied_frames


IDS = [c.id for c in sc.PARITY]


@pytest.mark.parametrize("case", sc.PARITY, ids=IDS)
def test_semi_planar_in_and_out_matches_the_oracle(hip_lib, case):
    clip, frames, par, want = sc.expected(case)
    with _context(case) as flt:
        got, _ = _run(flt, clip, frames, par)
        _assert_frames(want, got, case.id)
        i, s = flt.info(), flt.surface_info()
        assert i.frames == case.n
        assert (s.split_frames, s.merged_frames, s.copied_frames) == (case.n, case.n, 0)
        assert s.scratch_bytes == sc.scratch_frame_bytes(clip, bool(case.kw.get("dh"))) * case.n
        if case.path == "sweep":
            assert (i.fused_frames, i.banded_frames) == (case.n, 0), (i.fused_frames, i.banded_frames)
            assert i.uv_sweeps == (1 if case.uv_sweep else 0)
        if case.path == "pool":
            assert i.fused_frames == 0


@pytest.mark.parametrize("case", sc.PARITY, ids=IDS)
def test_same_library_two_routes(hip_lib, case):
    """process_surfaces on semi-planar surfaces against process_batch on the planar tensors, a context each: no oracle involved."""
    import torch
    clip, frames, par, _ = sc.expected(case)
    with _context(case) as a, _context(case) as b:
        got, _ = _run(a, clip, frames, par)
        src = _planar(clip, frames)
        dst = _empty(clip, case.n, b.plane_shape_out, False)
        torch.cuda.synchronize()
        b.process_batch(src, dst, par)
        b.synchronize()
        _assert_frames(_host_frames(clip, dst, case.n), got, case.id)


@pytest.mark.parametrize("src_semi,dst_semi", [(True, False), (False, True)], ids=["semi-to-planar", "planar-to-semi"])
@pytest.mark.parametrize("case", sc.MIXED, ids=[c.id for c in sc.MIXED])
def test_mixed_layouts(hip_lib, case, src_semi, dst_semi):
    clip, frames, par, want = sc.expected(case)
    with _context(case) as flt:
        got, _ = _run(flt, clip, frames, par, src_semi, dst_semi)
        _assert_frames(want, got, case.id)
        s = flt.surface_info()
        assert (s.split_frames, s.merged_frames, s.copied_frames) == (case.n if src_semi else 0, case.n if dst_semi else 0, 0)


# ---- layouts as callers have them ----------------------------------------------------------------------------------------------

def _alloc_up(alloc):
    import torch
    t = torch.from_numpy(alloc).pin_memory().to(_dev())
    assert t.data_ptr() % 256 == 0
    return t


def _surface_views(ts, layouts):
    """[Y [n, rows, w], UV [n, rows, cw, 2]] views into the device allocations."""
    import torch
    out = []
    for p, (t, L) in enumerate(zip(ts, layouts)):
        flat = t if L.B == 1 else t.view(torch.int16)
        if p == 0:
            v = flat.as_strided((L.n, L.rows, L.w), (L.stride // L.B, L.pitch // L.B, 1), L.base // L.B)
        else:
            v = flat.as_strided((L.n, L.rows, L.w // 2, 2), (L.stride // L.B, L.pitch // L.B, 2, 1), L.base // L.B)
        assert v.data_ptr() == t.data_ptr() + L.base
        out.append(v)
    return out


@pytest.mark.parametrize("arrangement", sc.ARRANGEMENTS, ids=[f"{s}-to-{d}" for s, d in sc.ARRANGEMENTS])
@pytest.mark.parametrize("case", sc.LAYOUTS, ids=[c.id for c in sc.LAYOUTS])
def test_layouts_as_callers_have_them(hip_lib, case, arrangement):
    """UV planes at an odd byte (8-bit) / at 2 mod 4 (16-bit), pitches that are no multiple of 4, slack between frames, against
    64-byte aligned padded lines on the other side: exact output, every byte outside the destination rows keeps its guard
    value, the source allocation is unchanged."""
    import torch
    clip, frames, par, want = sc.expected(case)
    shapes, _ = lc.shapes_of(clip)
    sl = sc.surface_layouts(arrangement[0], shapes, clip.bytes, case.n)
    dl = sc.surface_layouts(arrangement[1], shapes, clip.bytes, case.n)
    odd = sl if arrangement[0] == "odd" else dl
    assert odd[1].base % (2 * clip.bytes) and odd[1].pitch % (2 * clip.bytes) and all(a.pitch != b.pitch and a.stride != b.stride for a, b in zip(sl, dl))
    up = lc.source_batch(sl, [sc.semi(fr) for fr in frames], clip.dtype)
    ts, td = [_alloc_up(a) for a in up], [_alloc_up(a) for a in lc.destination_batch(dl)]
    torch.cuda.synchronize()
    with _context(case) as flt:
        flt.process_surfaces(_surface_views(ts, sl), _surface_views(td, dl), par)
        flt.synchronize()
    lc.assert_clean(f"{case.id} {arrangement[0]} -> {arrangement[1]}", [to_host(t) for t in td], dl, [sc.semi(fr) for fr in want], clip.dtype,
                    [to_host(t) for t in ts], up)


@pytest.mark.parametrize("case", sc.KEPT, ids=[c.id for c in sc.KEPT])
def test_only_the_kept_lines_of_the_source_are_needed(hip_lib, case):
    """The split reads the lines the pass keeps and nothing else: the other lines of the source UV plane hold another pattern."""
    clip, frames, par, want = sc.expected(case)
    off = 0 if case.kw["order"] == 1 else 1
    other = synth.frame(clip, "checker", seed=9)
    spoiled = []
    for fr in frames:
        u, v = fr[1].copy(), fr[2].copy()
        u[1 - off::2], v[1 - off::2] = other[1][1 - off::2], other[2][1 - off::2]
        assert not same(u, fr[1])
        spoiled.append([fr[0], u, v])
    with _context(case) as flt:
        got, _ = _run(flt, clip, spoiled, par)
    _assert_frames(want, got, case.id)


@pytest.mark.parametrize("src_semi,dst_semi", [(True, True), (True, False), (False, True)], ids=["semi-to-semi", "semi-to-planar", "planar-to-semi"])
def test_unprocessed_chroma_is_copied_or_converted(hip_lib, src_semi, dst_semi):
    case = sc.COPIED
    clip, frames, par, want = sc.expected(case)
    for f in range(case.n):
        assert same(want[f][1], frames[f][1]) and same(want[f][2], frames[f][2])
    with _context(case) as flt:
        got, _ = _run(flt, clip, frames, par, src_semi, dst_semi)
        _assert_frames(want, got, case.id)
        assert _info(flt) == (0, 0, 0, case.n), _info(flt)
        assert flt.info().frames == case.n


def test_chroma_only_through_the_pool_path(hip_lib):
    case = sc.CHROMA_ONLY
    clip, frames, par, want = sc.expected(case)
    with _context(case) as flt:
        got, _ = _run(flt, clip, frames, par)
        _assert_frames(want, got, case.id)
        assert flt.info().fused_frames == 0 and _info(flt)[1:] == (case.n, case.n, 0)


def test_a_batch_beyond_the_scratch_budget_takes_chunks(hip_lib):
    """The scratch holds min(max_batch, a sixteenth of the budget / one frame) frames: three of the four under 1 MiB, so the
    call walks two chunks, in order -- the clip carries history from frame to frame."""
    case = sc.CHUNKED
    clip, frames, par, want = sc.expected(case)
    cap = sc.scratch_frames(clip, case.n, 1)
    assert 1 <= cap < case.n
    with _context(case, scratch_budget_mb=1) as flt:
        assert flt.info().history_free == 0
        got, _ = _run(flt, clip, frames, par)
        _assert_frames(want, got, case.id)
        assert _info(flt) == (cap * sc.scratch_frame_bytes(clip), case.n, case.n, 0), _info(flt)


@pytest.mark.parametrize("fmt,dh", sc.AA, ids=[f"{f}-dh{int(d)}" for f, d in sc.AA])
def test_anti_aliasing_call(hip_lib, fmt, dh):
    import torch
    clip, frames, want = sc.expected_aa(fmt, dh)
    n = len(frames)
    with SangNomAA(clip, max_batch=n, aac=48, dh=dh) as aa:
        src, dst = _semi(clip, frames), _empty(clip, n, aa.plane_shape_out, True)
        torch.cuda.synchronize()
        aa.process_surfaces(src, dst)
        aa.synchronize()
        _assert_frames(want, _host_frames(clip, dst, n), f"{fmt} dh={dh}")
        s = aa.surface_info()
        assert (s.scratch_bytes, s.split_frames, s.merged_frames, s.copied_frames) == (sc.scratch_frame_bytes_aa(clip, dh) * n, n, n, 0)


@pytest.mark.parametrize("case", sc.PLANAR, ids=[c.id for c in sc.PLANAR])
def test_planar_through_the_new_call(hip_lib, case):
    import torch
    clip, frames, par, want = sc.expected(case)
    with _context(case) as a, _context(case) as b:
        got, _ = _run(a, clip, frames, par, False, False)
        src, dst = _planar(clip, frames), _empty(clip, case.n, b.plane_shape_out, False)
        torch.cuda.synchronize()
        b.process_batch(src, dst, par)
        b.synchronize()
        _assert_frames(_host_frames(clip, dst, case.n), got, case.id)
        _assert_frames(want, got, case.id)
        assert _info(a) == (0, 0, 0, 0)


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def _raw(flt, n, src, dst):
    return flt._lib.sn_process_device_surfaces(flt._h, n, ctypes.byref(src), ctypes.byref(dst), None), flt._lib.sn_last_error(flt._h).decode()


def _described(tensors, B, semi):
    return capi.surfaces(capi.SN_LAYOUT_SEMIPLANAR if semi else capi.SN_LAYOUT_PLANAR, [t.data_ptr() for t in tensors],
                         [t.stride(1) * B for t in tensors], [t.stride(0) * B for t in tensors])


def test_refusals_name_the_field_and_leave_the_context_usable(hip_lib):
    import torch
    case = sc.MIXED[0]
    clip, frames, par, want = sc.expected(case)
    cw, B, n = clip.width >> 1, clip.bytes, case.n
    with _context(case) as flt:
        src, dst = _semi(clip, frames), _empty(clip, n, flt.plane_shape_out, True)
        extra = torch.zeros(16, dtype=torch.uint8, device=_dev())
        torch.cuda.synchronize()

        def good():
            dst[0].fill_(0x5C), dst[1].fill_(0x5C)
            flt.process_surfaces(src, dst, par)
            flt.synchronize()
            _assert_frames(want, _host_frames(clip, dst, n), "after a refusal")

        def bad(change, code, word):
            s, d = _described(src, B, True), _described(dst, B, True)
            change(s, d)
            rc, text = _raw(flt, n, s, d)
            assert rc == code and word in text, (rc, text)
            good()

        def plane2(s, d):
            s.plane[2] = extra.data_ptr()

        def pitch(s, d):
            d.pitch[1] = 2 * cw * B - B

        def null_plane(s, d):
            s.plane[1] = None
        bad(plane2, capi.SN_ERR_INVALID_ARG, "plane[2]")
        bad(pitch, capi.SN_ERR_INVALID_ARG, "pitch[1]")
        bad(null_plane, capi.SN_ERR_INVALID_ARG, "plane[1]")
        bad(lambda s, d: setattr(s, "layout", 7), capi.SN_ERR_INVALID_ARG, "layout")
        bad(lambda s, d: setattr(d, "struct_size", 64), capi.SN_ERR_INVALID_ARG, "struct_size")
        bad(lambda s, d: setattr(d, "reserved", 1), capi.SN_ERR_INVALID_ARG, "reserved")
        assert flt.surface_info().split_frames == 6 * n  # only the good calls ran


@pytest.mark.parametrize("fmt,word", [("Y8", "num_planes"), ("YUV420PS", "bytes_per_sample")])
def test_surfaces_that_do_not_exist_are_unsupported(hip_lib, fmt, word):
    """SN_LAYOUT_SEMIPLANAR on a Y-only context and on a float clip; a planar call follows on the same context."""
    import torch
    case = sc.Case(fmt, 64, 32)
    clip, frames, par, want = sc.expected(case)
    with _context(case) as flt:
        src, dst = _planar(clip, frames), _empty(clip, case.n, flt.plane_shape_out, False)
        torch.cuda.synchronize()
        s, d = _described(src[:2] if clip.planes > 1 else src + src, clip.bytes, True), _described(dst, clip.bytes, False)
        rc, text = _raw(flt, case.n, s, d)
        assert rc == capi.SN_ERR_UNSUPPORTED and word in text, (rc, text)
        flt.process_surfaces(src, dst, par)
        flt.synchronize()
        _assert_frames(want, _host_frames(clip, dst, case.n), fmt)
        assert _info(flt) == (0, 0, 0, 0)
