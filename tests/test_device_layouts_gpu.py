"""Device planes as callers lay them out, through every sweep (sn_process_device_strided, sn_turn_device).

Every other GPU test hands the sweeps tight planes fresh from the allocator: 256-byte aligned bases, pitch == row, frame
stride == plane, the same layout on both sides, U and V alike.  Here the planes are views into padded allocations in the two
layouts of tests/layout_cases.py, source in one and destination in the other, and a launch has to
  * give the oracle's frames, bit for bit,
  * leave every byte of the destination allocation that belongs to no plane as it was (a store past column w-1, a row
    addressed with the other side's or the other plane's pitch, a frame stride taken from the wrong side), and
  * leave the source allocation as it was, whatever its padding held (0xFF: 255, 65535, NaN -- a load past column w-1 that
    reached the result would show).
Each case asserts the sn_info counter that proves its path ran, so that none passes on a fallback.
"""
import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2, SangNomError, capi, clip_format, synth
from oracle.oracle import Oracle
from tests import layout_cases as lc
from tests.util import describe_diff, oracle_cfg, same, to_host

pytestmark = pytest.mark.gpu

ARR_IDS = [f"{s}-to-{d}" for s, d in lc.ARRANGEMENTS]


def _upload(alloc):
    import torch
    t = torch.from_numpy(alloc).pin_memory().to(torch.device("cuda:0"))
    assert t.data_ptr() % 256 == 0  # what the layouts' alignment classes are relative to
    return t


def _tview(t, L):
    """The [n, rows, w] view of a plane inside its device allocation (the library is handed its pointer, pitch and stride)."""
    import torch
    tdt = {1: torch.uint8, 2: torch.int16, 4: torch.float32}[L.B]
    flat = t if L.B == 1 else t.view(tdt)
    v = flat.as_strided((L.n, L.rows, L.w), (L.stride // L.B, L.pitch // L.B, 1), L.base // L.B)
    assert v.data_ptr() == t.data_ptr() + L.base
    return v


def _launch(run, sl, dl, frames, dtype):
    """Builds both batches, calls run(src views, dst views), returns (dst allocations, source after, source uploaded)."""
    import torch
    up = lc.source_batch(sl, frames, dtype)
    ts, td = [_upload(a) for a in up], [_upload(a) for a in lc.destination_batch(dl)]
    torch.cuda.synchronize()
    run([_tview(t, L) for t, L in zip(ts, sl)], [_tview(t, L) for t, L in zip(td, dl)])
    return [to_host(t) for t in td], [to_host(t) for t in ts], up


def _context(case, mode="fused", **extra):
    return SangNom2(clip_format(case.fmt, case.w, case.h), max_batch=case.n, mode=mode, **case.kw, **case.ckw, **extra)


def _run(case, arrangement, pattern, flt):
    clip, frames, want = lc.expected(case, pattern)
    sl, dl = lc.layouts_of(case, arrangement)
    for p in range(clip.planes):
        assert (lc.fused_layout_ok(sl[p], dl[p]) or not case.fused) and sl[p].pitch != dl[p].pitch and sl[p].stride != dl[p].stride

    def run(src, dst):
        flt.process_batch(src, dst, list(case.parities))
        flt.synchronize()
    got, after, up = _launch(run, sl, dl, frames, clip.dtype)
    lc.assert_clean(f"{case.id} {arrangement[0]} -> {arrangement[1]} {pattern}", got, dl, want, clip.dtype, after, up)


@pytest.mark.parametrize("arrangement", lc.ARRANGEMENTS, ids=ARR_IDS)
@pytest.mark.parametrize("case", lc.SWEEPS, ids=[c.id for c in lc.SWEEPS])
def test_whole_plane_sweeps(hip_lib, case, arrangement):
    """The 8-bit, 16-bit and float sweeps of planes on their own, the coupled 4:2:0 sweeps, U and V as one sweep, padded
    sweeps, isolated planes, column parts and the SSE2 arithmetic: mode="fused", small_launches pinned to the sweeps."""
    for pattern in case.patterns:
        with _context(case, small_launches=capi.SN_SMALL_SWEEP) as flt:
            assert flt.info().fused_eligible == 1
            if case.parts:
                flt.debug_set_column_parts(case.parts, 0)
            if case.path == "parts":
                assert flt.parts_info().parts[0] >= 2
            _run(case, arrangement, pattern, flt)
            i = flt.info()
            assert (i.frames, i.fused_frames, i.banded_frames, i.chained_frames) == (case.n, case.n, 0, 0), (i.frames, i.fused_frames, i.banded_frames)
            if case.path != "sse2":  # (8-bit 4:2:0 in the SSE2 arithmetic: either form of the chroma sweeps)
                assert i.uv_sweeps == (1 if case.path == "uv" else 0)
            if case.path == "parts":
                pi = flt.parts_info()
                assert pi.part_frames == case.n, pi.part_frames
                if pattern == "noise":  # (converges within the ghost: tests/test_column_parts_cpu.py)
                    assert pi.part_fallbacks == 0, pi.part_fallbacks


@pytest.mark.parametrize("arrangement", lc.ARRANGEMENTS, ids=ARR_IDS)
@pytest.mark.parametrize("case", lc.BANDS, ids=[c.id for c in lc.BANDS])
def test_row_bands(hip_lib, case, arrangement):
    """A launch of two frames cut into six row bands (4:2:0: the luma plane; chroma by the pool kernels)."""
    for pattern in case.patterns:
        with _context(case, mode="auto", small_launches=capi.SN_SMALL_AUTO) as flt:
            flt.set_bands(6, 0)
            _run(case, arrangement, pattern, flt)
            i = flt.info()
            assert (i.frames, i.banded_frames) == (2, 2), (i.frames, i.banded_frames)
            if pattern == "noise":
                assert i.band_fallbacks == 0, i.band_fallbacks


@pytest.mark.parametrize("arrangement", lc.ARRANGEMENTS, ids=ARR_IDS)
@pytest.mark.parametrize("case", lc.POOL, ids=[c.id for c in lc.POOL])
def test_pool_path_and_chain(hip_lib, case, arrangement):
    """The pool kernels: asked for outright, and as the only path of history-carrying clips (one oracle instance through the
    batch) -- frame by frame, and as a chain of passes."""
    for pattern in case.patterns:
        with _context(case, mode="pool" if case.path == "pool" else "auto") as flt:
            assert flt.info().history_free == (1 if case.path == "pool" else 0)
            _run(case, arrangement, pattern, flt)
            i = flt.info()
            assert (i.frames, i.fused_frames, i.banded_frames) == (case.n, 0, 0), (i.frames, i.fused_frames, i.banded_frames)
            assert i.chained_frames == (case.n if case.path == "chain" else 0), i.chained_frames


@pytest.mark.parametrize("arrangement", lc.ARRANGEMENTS, ids=ARR_IDS)
@pytest.mark.parametrize("direction", (1, -1), ids=("right", "left"))
@pytest.mark.parametrize("fmt,w,h", lc.TURNS, ids=[f"{t[0]}-{t[1]}x{t[2]}" for t in lc.TURNS])
def test_turns(hip_lib, fmt, w, h, direction, arrangement):
    """sn_turn_device: source [N, H, W] and destination [N, W, H], each padded in its own layout, against np.rot90."""
    clip = clip_format(fmt, w, h)
    n = lc.NFRAMES
    frames = [synth.frame(clip, "noise", seed=700 + i) for i in range(n)]
    want = [[np.ascontiguousarray(np.rot90(fr[0], -1 if direction > 0 else 1))] for fr in frames]
    sl = lc.batch_layout(arrangement[0], [(h, w)], clip.bytes, n)
    dl = lc.batch_layout(arrangement[1], [(w, h)], clip.bytes, n)
    with SangNom2(clip) as flt:
        def run(src, dst):
            flt.turn(src[0], dst[0], direction)
            flt.synchronize()
        got, after, up = _launch(run, sl, dl, frames, clip.dtype)
    lc.assert_clean(f"turn {fmt} {w}x{h} {direction} {arrangement[0]} -> {arrangement[1]}", got, dl, want, clip.dtype, after, up)


# ---- planes of 2 GiB and more ---------------------------------------------------------------------------------------------

LARGE = [("dst", 31), ("dst", 32), ("src", 32)]  # which side is wide, and the power of two its 64 rows just exceed


def _count_not(t, fill, chunk=1 << 28):
    """Bytes of a device tensor of bytes that differ from `fill`, counted on the device a chunk at a time."""
    return sum(int((t[i:i + chunk] != fill).sum().item()) for i in range(0, t.numel(), chunk))


@pytest.mark.parametrize("side,bits", LARGE, ids=[f"{s}-above-2^{b}" for s, b in LARGE])
def test_planes_of_2_gib_and_more(hip_lib, side, bits):
    """A 64 x 64 column window of a very wide device surface: 64 rows whose pitch is a multiple of 64 with 64 * pitch just
    above 2^31 or 2^32.  The sweeps address a plane through a 32-bit buffer range and 32-bit row offsets, so
    fused_layout_ok hands such planes to the pool kernels (64-bit row pointers); the required behaviour is the oracle's
    plane and nothing written outside it -- or SN_ERR_INVALID_ARG naming the limit, never a silently different plane."""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 12 << 30:
        pytest.skip(f"{free >> 20} MiB of device memory free, the case needs 12 GiB")
    dev = torch.device("cuda:0")
    clip = clip_format("Y8", 64, 64)
    frame = synth.frame(clip, "noise", seed=900)
    want = Oracle(oracle_cfg(clip)).process(frame, parity=1)
    P = (1 << (bits - 6)) + 64
    assert P % 64 == 0 and 0 < 64 * P - (1 << bits) <= 4096
    fill = lc.FILL_DST if side == "dst" else lc.FILL_SRC
    big = torch.empty(64 * P, dtype=torch.uint8, device=dev)  # (whole pitches: what a descriptor of pitch * rows bytes would span)
    big.fill_(fill)
    wide = big.as_strided((1, 64, 64), (64 * P, P, 1))
    tight = torch.full((1, 64, 64), lc.FILL_DST, dtype=torch.uint8, device=dev)
    src, dst = (tight, wide) if side == "dst" else (wide, tight)
    src.copy_(torch.from_numpy(frame[0]).pin_memory().to(dev).unsqueeze(0))
    inside_before = int((wide != fill).sum().item())
    torch.cuda.synchronize()
    try:
        with SangNom2(clip, mode="fused") as flt:
            try:
                flt.process_batch([src], [dst], [1])
                flt.synchronize()
            except SangNomError as e:
                assert e.code == capi.SN_ERR_INVALID_ARG and "2^31" in str(e), str(e)
                return
        got = to_host(dst[0].contiguous())
        assert same(want[0], got), describe_diff(want[0], got)
        inside = int((wide != fill).sum().item())
        changed = _count_not(big, fill)
        assert changed == inside, f"{changed - inside} bytes outside the plane differ from the fill"
        if side == "src":
            assert inside == inside_before and same(frame[0], to_host(src[0].contiguous()))
    finally:
        del big, wide, tight, src, dst
        torch.cuda.empty_cache()

