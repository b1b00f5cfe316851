"""Packed 4:2:2 device surfaces -- YUY2 / UYVY, Y210 / Y212 / Y216, v210 (SN_LAYOUT_PACKED_*) -- in and out of
sn_process_device_surfaces and sn_aa_process_device_surfaces.  One rule: the destination holds what the planar call gives on
the unpacked planes, packed as the destination's layout says.  The expected frames are the CPU oracle's on the planar LSB-aligned
frames, packed by numpy (tests/packed_surface_cases.py); every source carries junk where it must be ignored.  Tolerance zero."""
import ctypes

import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2, SangNomAA, capi, clip_format
from tests import layout_cases as lc
from tests import msb_surface_cases as mc
from tests import packed_surface_cases as pc
from tests import surface_cases as sc
from tests import test_surfaces_gpu as sg  # its device helpers: upload, empty destinations, read-back, comparison
from tests.util import describe_diff, same, to_host

pytestmark = pytest.mark.gpu

NP_VIEW = {1: np.uint8, 2: np.int16, 4: np.int32}  # torch has no uint16 / uint32: same bits


def _context(case, **extra):
    kw = dict(max_batch=case.n, mode=case.mode)
    if case.path == "sweep":
        kw["small_launches"] = capi.SN_SMALL_SWEEP
    kw.update(extra)
    return SangNom2(clip_format(case.fmt, case.w, case.h), **case.kw, **case.ckw, **kw)


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(NP_VIEW[a.dtype.itemsize])).pin_memory().to(sg._dev())


def _keywords(side):
    packed, _, msb = pc.side_kind(side)
    return (pc.order_of(side) if packed else None), msb


def _source(clip, frames, side):
    """The LSB-aligned planar frames as a device source of that side: a packed layout, "planar", "planar_msb" or "nv16"."""
    if side in pc.LAYOUTS:
        return _up(np.stack(pc.pack_frames(side, clip, frames, source=True)))
    words = mc.msb_source(frames, mc.shift_of(clip)) if side.endswith("_msb") else frames
    return sg._semi(clip, words) if side == "nv16" else sg._planar(clip, words)


def _destination(clip, n, shape_of, side):
    import torch
    if side not in pc.LAYOUTS:
        return sg._empty(clip, n, shape_of, side == "nv16")
    h, w = shape_of(0)
    if side == "v210":
        t = torch.empty((n, h, 4 * pc.v210_blocks(w)), dtype=torch.int32, device=sg._dev())
    else:
        t = torch.empty((n, h, 2 * w), dtype={1: torch.uint8, 2: torch.int16}[clip.bytes], device=sg._dev())
    t.view(torch.uint8).fill_(0x5C)
    return t


def _assert_destination(clip, want, dst, side, what):
    """want: the expected LSB-aligned planar frames; dst: the device destination of that side."""
    if side in pc.LAYOUTS:
        got = to_host(dst).view(pc.packed_dtype(side, clip))
        for f, a in enumerate(pc.pack_frames(side, clip, want)):
            assert a.shape == got[f].shape, f"{what} frame {f}: shape {got[f].shape}, expected {a.shape}"
            assert same(a, got[f]), f"{what} frame {f} ({side}): " + describe_diff(a, got[f])
        return
    sg._assert_frames(mc.up(want, mc.shift_of(clip)) if side.endswith("_msb") else want, sg._host_frames(clip, dst, len(want)), what)


def _run(flt, clip, frames, par, src, dst, want, what):
    import torch
    ts, td = _source(clip, frames, src), _destination(clip, len(frames), flt.plane_shape_out, dst)
    (sp, sm), (dp, dm) = _keywords(src), _keywords(dst)
    torch.cuda.synchronize()
    flt.process_surfaces(ts, td, par, src_msb=sm, dst_msb=dm, src_packed=sp, dst_packed=dp)
    flt.synchronize()
    _assert_destination(clip, want, td, dst, what)
    return ts, td


def _counters(flt):
    i = flt.surface_info()
    return i.split_frames, i.merged_frames, i.copied_frames


def _check_parity(case, layout):
    clip, frames, par, want = pc.expected(case)
    dh = bool(case.kw.get("dh"))
    what = f"{case.id} {layout}"
    with _context(case) as flt:
        _run(flt, clip, frames, par, layout, layout, want, what)
        i, s = flt.info(), flt.surface_info()
        assert i.frames == case.n and _counters(flt) == (case.n, case.n, 0), (i.frames, _counters(flt))
        assert s.scratch_bytes == pc.scratch_frame_bytes(clip, layout, layout, dh=dh) * case.n
        if case.path == "sweep":
            assert (i.fused_frames, i.banded_frames) == (case.n, 0), (i.fused_frames, i.banded_frames)
    return clip, want


@pytest.mark.parametrize("case,layout", pc.PARITY, ids=[f"{c.id}-{layout}" for c, layout in pc.PARITY])
def test_packed_in_and_out_matches_the_oracle(hip_lib, case, layout):
    _check_parity(case, layout)


@pytest.mark.parametrize("layout", pc.OUT_OF_RANGE_LAYOUTS)
def test_samples_above_the_range_lose_their_high_bits(hip_lib, layout):
    """The oracle's frames hold samples above 1023: a v210 field is sample & 0x3FF, a Y210 word the low 16 bits of sample << 6."""
    clip, want = _check_parity(pc.OUT_OF_RANGE, layout)
    assert pc.exceeds_range(clip, want)


@pytest.mark.parametrize("bits,sides", [(b, s) for b in (8, 10) for s in pc.MIXED_SIDES[b]],
                         ids=[f"{b}bit-{s}-to-{d}" for b in (8, 10) for s, d in pc.MIXED_SIDES[b]])
def test_mixed_sides(hip_lib, bits, sides):
    case = pc.MIXED[bits]
    clip, frames, par, want = pc.expected(case)
    src, dst = sides
    with _context(case) as flt:
        _run(flt, clip, frames, par, src, dst, want, f"{case.id} {src} -> {dst}")
        split = case.n if src in pc.LAYOUTS or src == "nv16" else 0
        merged = case.n if dst in pc.LAYOUTS or dst == "nv16" else 0
        assert _counters(flt) == (split, merged, 0), _counters(flt)
        assert flt.surface_info().scratch_bytes == pc.scratch_frame_bytes(clip, src, dst) * case.n
        assert flt.info().frames == case.n


@pytest.mark.parametrize("layout", pc.COPIED_LAYOUTS)
@pytest.mark.parametrize("case", pc.COPIED, ids=[c.id for c in pc.COPIED])
def test_planes_that_are_only_copied(hip_lib, case, layout):
    """chroma=False; luma=False: the planes that are not processed equal the source's with the junk gone -- low bits of an MSB
    source, bits 30-31 and the fields of missing pixels of a v210 one -- and never reach a pass."""
    clip, frames, par, want = pc.expected(case)
    luma, chroma = case.kw.get("luma", True), case.kw.get("chroma", True)
    for f in range(case.n):
        assert all(same(want[f][p], frames[f][p]) for p in range(3) if not (luma if p == 0 else chroma))
    with _context(case) as flt:
        _run(flt, clip, frames, par, layout, layout, want, f"{case.id} {layout}")
        assert _counters(flt) == (case.n, case.n, 0 if chroma else case.n), _counters(flt)
        assert flt.surface_info().scratch_bytes == pc.scratch_frame_bytes(clip, layout, layout) * case.n
        assert flt.info().frames == case.n


# ---- layouts as callers have them ----------------------------------------------------------------------------------------------

def _packed_view(t, L, layout, clip):
    import torch
    size = 4 if layout == "v210" else clip.bytes
    flat = t if size == 1 else t.view({2: torch.int16, 4: torch.int32}[size])
    v = flat.as_strided((L.n, L.rows, L.row // size), (L.stride // size, L.pitch // size, 1), L.base // size)
    assert v.data_ptr() == t.data_ptr() + L.base
    return v


def _as_bytes(packed):
    return [[a.view(np.uint8).reshape(a.shape[0], -1)] for a in packed]


@pytest.mark.parametrize("arrangement", sc.ARRANGEMENTS, ids=[f"{s}-to-{d}" for s, d in sc.ARRANGEMENTS])
@pytest.mark.parametrize("case,layout", pc.CALLER_LAYOUTS, ids=[f"{c.id}-{layout}" for c, layout in pc.CALLER_LAYOUTS])
def test_layouts_as_callers_have_them(hip_lib, case, layout, arrangement):
    """A surface at an offset and a pitch that are aligned to the unit only (one sample, one v210 block per access) against
    64-byte aligned padded lines (16 bytes per access), both ways: exact output, every byte outside the destination rows keeps
    its guard value, the source allocation is unchanged."""
    import torch
    clip, frames, par, want = pc.expected(case)
    sl, dl = (pc.caller_layout(name, layout, clip, clip.height, case.n) for name in arrangement)
    odd = sl if arrangement[0] == "odd" else dl
    unit = 4 if layout == "v210" else clip.bytes
    assert odd.base % 16 and odd.pitch % 16 and odd.base % unit == 0 and odd.pitch % unit == 0 and odd.stride % unit == 0
    up = lc.source_batch([sl], _as_bytes(pc.pack_frames(layout, clip, frames, source=True)), np.uint8)
    ts, td = sg._alloc_up(up[0]), sg._alloc_up(lc.destination_batch([dl])[0])
    sp, sm = _keywords(layout)
    torch.cuda.synchronize()
    with _context(case) as flt:
        flt.process_surfaces(_packed_view(ts, sl, layout, clip), _packed_view(td, dl, layout, clip), par, src_msb=sm, dst_msb=sm,
                             src_packed=sp, dst_packed=sp)
        flt.synchronize()
    lc.assert_clean(f"{case.id} {layout} {arrangement[0]} -> {arrangement[1]}", [to_host(td)], [dl], _as_bytes(pc.pack_frames(layout, clip, want)),
                    np.uint8, [to_host(ts)], up)


# ---- chunks and scratch --------------------------------------------------------------------------------------------------------

def test_a_batch_beyond_the_scratch_budget_takes_chunks(hip_lib):
    """Under 1 MiB the scratch holds fewer than the four frames: the call walks chunks, in order -- the clip carries history."""
    case, layout = pc.CHUNKED
    clip, frames, par, want = pc.expected(case)
    per_frame = pc.scratch_frame_bytes(clip, layout, layout)
    cap = mc.scratch_frames(per_frame, case.n, 1)
    assert 1 <= cap < case.n
    with _context(case, scratch_budget_mb=1) as flt:
        assert flt.info().history_free == 0
        _run(flt, clip, frames, par, layout, layout, want, case.id)
        assert flt.surface_info().scratch_bytes == cap * per_frame and _counters(flt) == (case.n, case.n, 0)


def test_packed_scratch_joins_the_scratch_a_context_already_holds(hip_lib):
    """A context that has served NV16 holds U and V in and out; its first packed call gives that back and takes the union --
    with both luma planes --, and an NV16 call after that still gives the right frames."""
    case = pc.REFIT
    clip, frames, par, want = pc.expected(case)
    nv16 = sc.scratch_frame_bytes(clip)
    both = pc.scratch_frame_bytes(clip, "yuyv", "yuyv")
    assert 0 < nv16 < both
    with _context(case) as flt:
        for side, per_frame in (("nv16", nv16), ("yuyv", both), ("nv16", both)):
            _run(flt, clip, frames, par, side, side, want, f"{case.id} {side}")
            assert flt.surface_info().scratch_bytes == per_frame * case.n
        assert _counters(flt) == (3 * case.n, 3 * case.n, 0) and flt.info().frames == 3 * case.n


# ---- the anti-aliasing call ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,layout,dh", pc.AA, ids=[f"{f}-{layout}-dh{int(d)}" for f, layout, d in pc.AA])
def test_anti_aliasing_call(hip_lib, fmt, layout, dh):
    clip, frames, want = sc.expected_aa(fmt, dh)
    n = len(frames)
    with SangNomAA(clip, max_batch=n, aac=48, dh=dh) as aa:
        _run(aa, clip, frames, None, layout, layout, want, f"{fmt} {layout} dh={dh}")
        i = aa.surface_info()
        per_frame = pc.scratch_frame_bytes(clip, layout, layout, dh=dh, aa=True)
        assert (i.scratch_bytes, i.split_frames, i.merged_frames, i.copied_frames) == (per_frame * n, n, n, 0)


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def _described(t, layout):
    size = t.element_size()
    return capi.surfaces(layout, [t.data_ptr()], [t.stride(1) * size], [t.stride(0) * size])


def _described_planar(tensors, B):
    return capi.surfaces(capi.SN_LAYOUT_PLANAR, [t.data_ptr() for t in tensors], [t.stride(1) * B for t in tensors], [t.stride(0) * B for t in tensors])


def _raw(flt, n, src, dst):
    return flt._lib.sn_process_device_surfaces(flt._h, n, ctypes.byref(src), ctypes.byref(dst), None), flt._lib.sn_last_error(flt._h).decode()


def _refused_then_planar(case, layouts):
    """Every layout of `layouts` as source and as destination of a context that cannot take it: SN_ERR_UNSUPPORTED naming layout;
    a planar call follows on the same context and gives the right frames."""
    import torch
    clip, frames, par, want = sc.expected(case)
    with _context(case) as flt:
        src, dst = sg._planar(clip, frames), sg._empty(clip, case.n, flt.plane_shape_out, False)
        one = torch.zeros((case.n, clip.height, 16 * clip.width), dtype=torch.uint8, device=sg._dev())  # room for any packed row
        torch.cuda.synchronize()
        for layout in layouts:
            for packed_src in (True, False):
                s = _described(one, layout) if packed_src else _described_planar(src, clip.bytes)
                d = _described_planar(dst, clip.bytes) if packed_src else _described(one, layout)
                rc, text = _raw(flt, case.n, s, d)
                assert rc == capi.SN_ERR_UNSUPPORTED and "layout" in text, (layout, rc, text)
        flt.process_surfaces(src, dst, par)
        flt.synchronize()
        sg._assert_frames(want, sg._host_frames(clip, dst, case.n), case.id)
        assert sg._info(flt) == (0, 0, 0, 0) and flt.info().frames == case.n


@pytest.mark.parametrize("case", pc.REFUSED_CONTEXTS, ids=[c.id for c in pc.REFUSED_CONTEXTS])
def test_packed_layouts_need_a_422_context_with_integer_samples(hip_lib, case):
    _refused_then_planar(case, [capi.SN_LAYOUT_PACKED_YUYV, capi.SN_LAYOUT_PACKED_UYVY, capi.SN_LAYOUT_PACKED_V210])


def test_msb_forms_need_sixteen_bit_words(hip_lib):
    _refused_then_planar(pc.V210_REFUSED[0], [capi.SN_LAYOUT_PACKED_YUYV_MSB, capi.SN_LAYOUT_PACKED_UYVY_MSB])


@pytest.mark.parametrize("case", pc.V210_REFUSED, ids=[c.id for c in pc.V210_REFUSED])
def test_v210_needs_a_ten_bit_context(hip_lib, case):
    _refused_then_planar(case, [capi.SN_LAYOUT_PACKED_V210])


@pytest.mark.parametrize("layout", ["yuyv", "v210"])
def test_refusals_name_the_field_and_leave_the_context_usable(hip_lib, layout):
    """plane[1] set, a pitch one unit below the row, a v210 pitch that is no multiple of 4, values that are no layouts: refused;
    every good call in between gives the right frames and only the good calls are counted."""
    import torch
    case = pc.MIXED[10 if layout == "v210" else 8]
    clip, frames, par, want = pc.expected(case)
    n = case.n
    code = capi.PACKED_LAYOUTS[(layout, False)]
    unit = 4 if layout == "v210" else clip.bytes
    with _context(case) as flt:
        src, dst = _source(clip, frames, layout), _destination(clip, n, flt.plane_shape_out, layout)
        extra = torch.zeros(16, dtype=torch.uint8, device=sg._dev())
        torch.cuda.synchronize()
        calls = [0]

        def good():
            dst.view(torch.uint8).fill_(0x5C)
            flt.process_surfaces(src, dst, par, src_packed=layout, dst_packed=layout)
            flt.synchronize()
            _assert_destination(clip, want, dst, layout, "after a refusal")
            calls[0] += 1

        def bad(change, word):
            a, b = _described(src, code), _described(dst, code)
            change(a, b)
            rc, text = _raw(flt, n, a, b)
            assert rc == capi.SN_ERR_INVALID_ARG and word in text, (rc, text)
            good()

        def plane1(a, b):
            a.plane[1] = extra.data_ptr()

        def short_pitch(a, b):
            b.pitch[0] = pc.row_bytes(layout, clip.width, clip.bytes) - unit

        def crooked_pitch(a, b):
            a.pitch[0] = a.pitch[0] + 2
        good()
        bad(plane1, "plane[1]")
        bad(short_pitch, "pitch[0]")
        if layout == "v210":
            bad(crooked_pitch, "pitch[0]")
        for value in (5, 6, 13):
            bad(lambda a, b: setattr(b, "layout", value), "layout")
        assert _counters(flt) == (calls[0] * n, calls[0] * n, 0) and flt.info().frames == calls[0] * n
