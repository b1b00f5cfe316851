"""MSB-aligned device surfaces -- P010 / P012 as the 10- and 12-bit clips they are (SN_LAYOUT_PLANAR_MSB,
SN_LAYOUT_SEMIPLANAR_MSB) -- in and out of sn_process_device_surfaces and sn_aa_process_device_surfaces.  One rule: with ss and
ds the shifts of the two sides the destination holds what the call gives on src >> ss, shifted left by ds.  The expected frames
are the CPU oracle's on the LSB-aligned frames (tests/msb_surface_cases.py), shifted and interleaved by numpy; every MSB source
carries random non-zero low bits, which must never reach the output.  Tolerance zero everywhere."""
import ctypes

import pytest

from avisynth_sangnom2_amd import SangNom2, SangNomAA, capi, clip_format
from tests import layout_cases as lc
from tests import msb_surface_cases as mc
from tests import surface_cases as sc
from tests import test_surfaces_gpu as sg  # its device helpers: upload, empty destinations, read-back, comparison
from tests.util import to_host

pytestmark = pytest.mark.gpu

SEMI_MSB = (True, True)


def _context(case, **extra):
    kw = dict(max_batch=case.n, mode=case.mode)
    if case.path == "sweep":
        kw["small_launches"] = capi.SN_SMALL_SWEEP
    kw.update(extra)
    return SangNom2(clip_format(case.fmt, case.w, case.h), **case.kw, **case.ckw, **kw)


def _run(flt, clip, frames, par, src=SEMI_MSB, dst=SEMI_MSB, want=None):
    """The LSB-aligned frames through process_surfaces with src / dst = (semi-planar, MSB); the frames read back as planar
    planes, and `want` aligned as the destination is."""
    import torch
    s, n = mc.shift_of(clip), len(frames)
    words = mc.msb_source(frames, s) if src[1] else frames
    ts = sg._semi(clip, words) if src[0] else sg._planar(clip, words)
    td = sg._empty(clip, n, flt.plane_shape_out, dst[0])
    torch.cuda.synchronize()
    flt.process_surfaces(ts, td, par, src_msb=src[1], dst_msb=dst[1])
    flt.synchronize()
    return sg._host_frames(clip, td, n), (mc.up(want, s) if dst[1] else want) if want is not None else None


def _counters(flt):
    i = flt.surface_info()
    return i.split_frames, i.merged_frames, i.copied_frames


@pytest.mark.parametrize("case", mc.PARITY, ids=[c.id for c in mc.PARITY])
def test_msb_in_and_out_matches_the_oracle(hip_lib, case):
    clip, frames, par, want = mc.expected(case)
    dh = bool(case.kw.get("dh"))
    with _context(case) as flt:
        got, want = _run(flt, clip, frames, par, want=want)
        sg._assert_frames(want, got, case.id)
        i, s = flt.info(), flt.surface_info()
        assert i.frames == case.n and _counters(flt) == (case.n, case.n, 0)
        assert s.scratch_bytes == mc.scratch_frame_bytes(clip, True, True, True, dh=dh) * case.n
        if case.path == "sweep":
            assert (i.fused_frames, i.banded_frames) == (case.n, 0), (i.fused_frames, i.banded_frames)
        if case.path == "pool":
            assert i.fused_frames == 0


def test_a_batch_beyond_the_scratch_budget_takes_chunks(hip_lib):
    """Luma and chroma scratch together obey the sixteenth-of-the-budget rule: two of the four frames under 1 MiB, so the call
    walks two chunks, in order -- the clip carries history from frame to frame."""
    case = mc.CHUNKED
    clip, frames, par, want = mc.expected(case)
    per_frame = mc.scratch_frame_bytes(clip, True, True, True)
    cap = mc.scratch_frames(per_frame, case.n, 1)
    assert 1 <= cap < case.n
    with _context(case, scratch_budget_mb=1) as flt:
        assert flt.info().history_free == 0
        got, want = _run(flt, clip, frames, par, want=want)
        sg._assert_frames(want, got, case.id)
        assert flt.surface_info().scratch_bytes == cap * per_frame and _counters(flt) == (case.n, case.n, 0)


def test_the_luma_scratch_joins_chroma_scratch_a_context_already_holds(hip_lib):
    """A context that has served LSB-aligned semi-planar surfaces holds chroma scratch only; its first call with an MSB source
    gives that back and takes chroma and luma under the same rule.  Both calls, and an LSB call after them, give the right frames."""
    case = mc.MIXED
    clip, frames, par, want = mc.expected(case)
    chroma, both = mc.scratch_frame_bytes(clip, True, False, True), mc.scratch_frame_bytes(clip, True, True, True)
    assert 0 < chroma < both
    with _context(case) as flt:
        for sides, per_frame in (((True, False), chroma), ((True, True), both), ((True, False), both)):
            got, expect = _run(flt, clip, frames, par, sides, sides, want)
            sg._assert_frames(expect, got, f"{case.id} {sides}")
            assert flt.surface_info().scratch_bytes == per_frame * case.n
        assert _counters(flt) == (3 * case.n, 3 * case.n, 0) and flt.info().frames == 3 * case.n


@pytest.mark.parametrize("sides", mc.MIXED_SIDES, ids=["p010-to-planar", "planar-to-p010", "planar-msb-to-p016", "p010-to-planar-msb"])
def test_mixed_sides(hip_lib, sides):
    case = mc.MIXED
    clip, frames, par, want = mc.expected(case)
    src, dst = sides[:2], sides[2:]
    with _context(case) as flt:
        got, want = _run(flt, clip, frames, par, src, dst, want)
        sg._assert_frames(want, got, f"{case.id} {sides}")
        assert _counters(flt) == (case.n if src[0] else 0, case.n if dst[0] else 0, 0)
        assert flt.surface_info().scratch_bytes == mc.scratch_frame_bytes(clip, src[0], src[1], dst[0]) * case.n
        assert flt.info().frames == case.n


@pytest.mark.parametrize("case", mc.LUMA_ONLY, ids=[c.id for c in mc.LUMA_ONLY])
def test_a_luma_clip_planar_msb_both_sides(hip_lib, case):
    """No chroma scratch at all: one luma plane per frame.  The wide clip runs in column parts."""
    clip, frames, par, want = mc.expected(case)
    with _context(case) as flt:
        got, want = _run(flt, clip, frames, par, (False, True), (False, True), want)
        sg._assert_frames(want, got, case.id)
        assert flt.surface_info().scratch_bytes == mc.roundup256(case.w * 2) * case.h * case.n and _counters(flt) == (0, 0, 0)
        if case.ckw.get("column_parts"):
            p = flt.parts_info()
            assert (p.part_frames, p.part_fallbacks) == (case.n, 0), (p.part_frames, p.part_fallbacks)
            assert flt.info().fused_frames == case.n


@pytest.mark.parametrize("sides", mc.COPIED_SIDES, ids=["msb-to-msb", "msb-to-lsb"])
@pytest.mark.parametrize("case", mc.COPIED, ids=[c.id for c in mc.COPIED])
def test_planes_that_are_only_copied_are_masked(hip_lib, case, sides):
    """chroma=False: the UV plane goes from src to dst as a plane of 2 cw samples; luma=False: the luma plane does.  Between two
    MSB sides that is the mask -- the source's low bits are set --, towards an LSB side the shift down."""
    clip, frames, par, want = mc.expected(case)
    luma, chroma = case.kw.get("luma", True), case.kw.get("chroma", True)
    for f in range(case.n):
        assert all(sg.same(want[f][p], frames[f][p]) for p in range(3) if not (luma if p == 0 else chroma))
    with _context(case) as flt:
        got, want = _run(flt, clip, frames, par, (True, sides[0]), (True, sides[1]), want)
        sg._assert_frames(want, got, f"{case.id} {sides}")
        assert _counters(flt) == ((case.n, case.n, 0) if chroma else (0, 0, case.n)), _counters(flt)
        assert flt.surface_info().scratch_bytes == mc.scratch_frame_bytes(clip, True, True, True, luma=luma, chroma=chroma) * case.n
        assert flt.info().frames == case.n


@pytest.mark.parametrize("arrangement", sc.ARRANGEMENTS, ids=[f"{s}-to-{d}" for s, d in sc.ARRANGEMENTS])
@pytest.mark.parametrize("case", mc.LAYOUTS, ids=[c.id for c in mc.LAYOUTS])
def test_layouts_as_callers_have_them(hip_lib, case, arrangement):
    """Planes at 2 mod 4 with pitches that are no multiple of 4 (one sample per access) against 64-byte aligned padded lines (16
    bytes per access), both ways: exact output, every byte outside the destination rows keeps its guard value -- the pitch
    padding of a destination that is shifted up in place included --, the source allocation is unchanged."""
    import torch
    clip, frames, par, want = mc.expected(case)
    s = mc.shift_of(clip)
    shapes, _ = lc.shapes_of(clip)
    sl = sc.surface_layouts(arrangement[0], shapes, clip.bytes, case.n)
    dl = sc.surface_layouts(arrangement[1], shapes, clip.bytes, case.n)
    up = lc.source_batch(sl, [sc.semi(fr) for fr in mc.msb_source(frames, s)], clip.dtype)
    ts, td = [sg._alloc_up(a) for a in up], [sg._alloc_up(a) for a in lc.destination_batch(dl)]
    torch.cuda.synchronize()
    with _context(case) as flt:
        flt.process_surfaces(sg._surface_views(ts, sl), sg._surface_views(td, dl), par, src_msb=True, dst_msb=True)
        flt.synchronize()
    lc.assert_clean(f"{case.id} {arrangement[0]} -> {arrangement[1]}", [to_host(t) for t in td], dl, [sc.semi(fr) for fr in mc.up(want, s)],
                    clip.dtype, [to_host(t) for t in ts], up)


@pytest.mark.parametrize("fmt,dh", mc.AA, ids=[f"{f}-dh{int(d)}" for f, d in mc.AA])
def test_anti_aliasing_call(hip_lib, fmt, dh):
    import torch
    clip, frames, want = mc.expected_aa(fmt, dh)
    n, s = len(frames), mc.shift_of(clip)
    with SangNomAA(clip, max_batch=n, aac=48, dh=dh) as aa:
        src, dst = sg._semi(clip, mc.msb_source(frames, s)), sg._empty(clip, n, aa.plane_shape_out, True)
        torch.cuda.synchronize()
        aa.process_surfaces(src, dst, src_msb=True, dst_msb=True)
        aa.synchronize()
        sg._assert_frames(mc.up(want, s), sg._host_frames(clip, dst, n), f"{fmt} dh={dh}")
        i = aa.surface_info()
        per_frame = sc.scratch_frame_bytes_aa(clip, dh) + mc.roundup256(clip.width * 2) * clip.height
        assert (i.scratch_bytes, i.split_frames, i.merged_frames, i.copied_frames) == (per_frame * n, n, n, 0)


def test_on_a_sixteen_bit_context_the_msb_layouts_are_the_plain_ones(hip_lib):
    """Shift 0: SN_LAYOUT_SEMIPLANAR_MSB gives the frames of SN_LAYOUT_SEMIPLANAR, the oracle's, and takes no luma scratch."""
    case = mc.SIXTEEN
    clip, frames, par, want = mc.expected(case)
    assert mc.shift_of(clip) == 0
    with _context(case) as a, _context(case) as b:
        got, _ = _run(a, clip, frames, par)
        plain, _ = _run(b, clip, frames, par, (True, False), (True, False))
        sg._assert_frames(plain, got, case.id)
        sg._assert_frames(want, got, case.id)
        assert a.surface_info().scratch_bytes == b.surface_info().scratch_bytes == sc.scratch_frame_bytes(clip) * case.n


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def _described(tensors, layout):
    B = tensors[0].element_size()
    return capi.surfaces(layout, [t.data_ptr() for t in tensors], [t.stride(1) * B for t in tensors], [t.stride(0) * B for t in tensors])


def _raw(flt, n, src, dst):
    return flt._lib.sn_process_device_surfaces(flt._h, n, ctypes.byref(src), ctypes.byref(dst), None), flt._lib.sn_last_error(flt._h).decode()


@pytest.mark.parametrize("case", mc.REFUSED, ids=[c.id for c in mc.REFUSED])
@pytest.mark.parametrize("layout", [capi.SN_LAYOUT_PLANAR_MSB, capi.SN_LAYOUT_SEMIPLANAR_MSB], ids=["planar-msb", "semiplanar-msb"])
def test_msb_layouts_need_sixteen_bit_words(hip_lib, case, layout):
    """An _MSB layout on an 8-bit and on a float context, as source and as destination; a planar call follows on the same context."""
    import torch
    clip, frames, par, want = mc.expected(case)
    semi = layout == capi.SN_LAYOUT_SEMIPLANAR_MSB
    with _context(case) as flt:
        src, dst = sg._planar(clip, frames), sg._empty(clip, case.n, flt.plane_shape_out, False)
        torch.cuda.synchronize()
        for msb_src in (True, False):
            s = _described(src[:2] if semi and msb_src else src, layout if msb_src else capi.SN_LAYOUT_PLANAR)
            d = _described(dst[:2] if semi and not msb_src else dst, capi.SN_LAYOUT_PLANAR if msb_src else layout)
            rc, text = _raw(flt, case.n, s, d)
            assert rc == capi.SN_ERR_UNSUPPORTED and "layout" in text, (rc, text)
        flt.process_surfaces(src, dst, par)
        flt.synchronize()
        sg._assert_frames(want, sg._host_frames(clip, dst, case.n), case.id)
        assert sg._info(flt) == (0, 0, 0, 0) and flt.info().frames == case.n


def test_refusals_leave_the_context_usable(hip_lib):
    """plane[2] set with SN_LAYOUT_SEMIPLANAR_MSB, a pitch below the UV row and a layout beyond the enum: refused as for
    SN_LAYOUT_SEMIPLANAR; every good call in between gives the right frames and only the good calls are counted."""
    import torch
    case = mc.MIXED
    clip, frames, par, want = mc.expected(case)
    s, n = mc.shift_of(clip), case.n
    want = mc.up(want, s)
    with _context(case) as flt:
        src, dst = sg._semi(clip, mc.msb_source(frames, s)), sg._empty(clip, n, flt.plane_shape_out, True)
        extra = torch.zeros(16, dtype=torch.uint8, device=sg._dev())
        torch.cuda.synchronize()

        def good():
            dst[0].fill_(0x5C5C), dst[1].fill_(0x5C5C)
            flt.process_surfaces(src, dst, par, src_msb=True, dst_msb=True)
            flt.synchronize()
            sg._assert_frames(want, sg._host_frames(clip, dst, n), "after a refusal")

        def bad(change, code, word):
            a, b = _described(src, capi.SN_LAYOUT_SEMIPLANAR_MSB), _described(dst, capi.SN_LAYOUT_SEMIPLANAR_MSB)
            change(a, b)
            rc, text = _raw(flt, n, a, b)
            assert rc == code and word in text, (rc, text)
            good()

        def plane2(a, b):
            a.plane[2] = extra.data_ptr()

        def pitch(a, b):
            b.pitch[1] = 2 * (clip.width >> 1) * clip.bytes - clip.bytes
        bad(plane2, capi.SN_ERR_INVALID_ARG, "plane[2]")
        bad(pitch, capi.SN_ERR_INVALID_ARG, "pitch[1]")
        bad(lambda a, b: setattr(a, "layout", 4), capi.SN_ERR_INVALID_ARG, "layout")
        bad(lambda a, b: setattr(b, "layout", -1), capi.SN_ERR_INVALID_ARG, "layout")
        assert _counters(flt) == (4 * n, 4 * n, 0) and flt.info().frames == 4 * n
