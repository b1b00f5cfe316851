"""The shortest and the narrowest planes through every route of the library, bit-exact against the CPU oracle.

Which kernels serve a launch is decided on the host by rules over the planes' geometry, and every such rule has a boundary at
the lower end: a plane with no interpolated row, a pool of one row, a chroma plane too short for the one-sweep form, fewer rows
than two bands.  tests/small_plane_cases.py restates the rules and derives a case on each side of every boundary from them;
tests/test_small_planes_cpu.py checks that table.  Here every case runs on the device:

  a  column parts: wide 16-bit and float planes with no row, one row, two rows -- host frame, host ring, device batch
  b  whole-plane sweeps of eight waves at heights 2 and 4, as device batches, with dh, and in the SSE2 arithmetic
  c  coupled 4:2:0 / 4:2:2 sweeps whose chroma has no row, one row, two rows; the hand-off rows themselves
  d  U and V as one sweep on both sides of its row condition
  e  row bands on both sides of the band count
  f  the pool path with a pool of one row and of two, at every stage-2 schedule; the pool's contents
  g  chains of a history-carrying batch on both sides of their conditions
  h  planes narrower than 32 columns, and clips whose chroma is one or two columns wide
  i  decoder and capture surfaces of a few pixels
  j  the anti-aliasing call on planes whose turned form is a few columns wide

Every case feeds frames of different content and both parities, compares float planes on their bit patterns, and asserts from
the context's counters that the intended route served it -- or, on the far side of a rule, that it did not.
"""
import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2, SangNomAA, capi, clip_format
from oracle.oracle import Oracle
from oracle.sangnom_numpy import NumpySangNom
from tests import small_plane_cases as sp
from tests import sse2_sweep_cases as ssc
from tests.util import describe_diff, oracle_cfg, same, to_host

pytestmark = pytest.mark.gpu

SWEEP = dict(small_launches=capi.SN_SMALL_SWEEP)


def _kw_id(*dicts):
    return "".join(f"-{k}{int(v)}" for d in dicts for k, v in d.items())


def _assert_frames(want, got, what):
    assert len(want) == len(got), what
    for f, (a, b) in enumerate(zip(want, got)):
        for p, (x, y) in enumerate(zip(a, b)):
            assert x.shape == y.shape and same(x, y), f"{what} frame {f} plane {p}: " + describe_diff(x, y)


def _batch(flt, clip, frames, par):
    import torch
    dev, n = torch.device("cuda:0"), len(frames)
    src = sp.to_torch(frames, clip, dev)
    dst = [torch.zeros((n,) + flt.plane_shape_out(p), dtype=src[p].dtype, device=dev) for p in range(clip.planes)]
    torch.cuda.synchronize()
    flt.process_batch(src, dst, par)
    flt.synchronize()
    return [[to_host(dst[p][f]).view(clip.dtype) for p in range(clip.planes)] for f in range(n)]


def _ring(flt, frames, par, depth):
    got = []
    for i in range(0, len(frames), depth):  # as many frames in flight as the ring holds
        slots = [flt.submit(fr, parity=pa) for fr, pa in zip(frames[i:i + depth], par[i:i + depth])]
        got += [flt.collect(s) for s in slots]
    return got


def _run(flt, clip, frames, par, way):
    if way == "host":
        return [flt.get_frame(fr, parity=pa) for fr, pa in zip(frames, par)]
    if way.startswith("ring"):
        return _ring(flt, frames, par, int(way[4:]))
    return _batch(flt, clip, frames, par)


def _way_kw(way, n):
    return dict(host_depth=int(way[4:])) if way.startswith("ring") else dict(max_batch=n) if way == "batch" else {}


# ---- a. column parts -------------------------------------------------------------------------------------------------------------

PARTS_IDS = [f"{c[0]}-{c[1]}x{c[2]}" + _kw_id(c[3], c[4]) for c in sp.PARTS]


@pytest.mark.parametrize("way", sp.PARTS_WAYS)
@pytest.mark.parametrize("case", sp.PARTS, ids=PARTS_IDS)
def test_wide_planes_with_no_row_one_row_and_two_rows(hip_lib, case, way):
    """A plane marked for column parts is cut when it has a row to interpolate (part_frames counts the launch, no frame falls
    back) and runs on the pool path's assemble when it has none (part_frames does not count it, no sweep is launched for it).
    Either way a mode="fused" context serves the clip and says fused_eligible = 1."""
    fmt, w, h, kw, ckw = case
    clip, frames, par, want = sp.expected(fmt, w, h, kw, ckw)
    n = len(frames)
    planes = sp.planes_of(clip, kw)
    cut = [on and sp.parts_marked(clip.bytes, pw) and sp.nr(ho) >= 1 for pw, ho, on in planes]
    swept = [on and (c or sp.sweep_plane_ok(clip.bytes, pw)) for (pw, ho, on), c in zip(planes, cut)]
    with SangNom2(clip, mode="fused", column_parts=1, **_way_kw(way, n), **kw, **ckw) as flt:
        assert flt.info().fused_eligible == 1
        pi = flt.parts_info()
        assert [pi.parts[p] >= 2 for p in range(clip.planes)] == cut, list(pi.parts)
        got = _run(flt, clip, frames, par, way)
        _assert_frames(want, got, f"{fmt} {w}x{h} {way}")
        i, pi = flt.info(), flt.parts_info()
        assert i.fused_frames == (n if any(swept) else 0), (i.fused_frames, swept)
        assert pi.part_frames == (n if any(cut) else 0) and pi.part_fallbacks == 0, (pi.part_frames, pi.part_fallbacks)
        assert i.banded_frames == 0 and i.chained_frames == 0
        if way == "batch":
            assert i.frames == n


@pytest.mark.parametrize("case", sp.PARTS_FORCED, ids=[f"{c[0]}-{c[1]}x{c[2]}-{c[3]}parts" for c in sp.PARTS_FORCED])
def test_forced_parts_on_a_plane_of_one_row(hip_lib, case):
    fmt, w, h, parts = case
    clip, frames, par, want = sp.expected(fmt, w, h)
    n = len(frames)
    with SangNom2(clip, mode="fused", column_parts=1, max_batch=n) as flt:
        assert list(flt.parts_info().parts) == [0, 0, 0]
        flt.debug_set_column_parts(parts, 0)
        assert flt.parts_info().parts[0] == parts
        _assert_frames(want, _batch(flt, clip, frames, par), f"{fmt} {w}x{h} {parts} parts")
        i, pi = flt.info(), flt.parts_info()
        assert i.fused_frames == n and pi.part_frames == n and pi.part_fallbacks == 0, (i.fused_frames, pi.part_frames, pi.part_fallbacks)


# ---- b. whole-plane sweeps of eight waves ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sp.WIDE, ids=[f"{c[0]}-{c[1]}x{c[2]}" + _kw_id(c[3]) for c in sp.WIDE])
def test_the_widest_sweeps_at_two_and_four_lines_as_device_batches(hip_lib, case):
    fmt, w, h, kw = case
    clip, frames, par, want = sp.expected(fmt, w, h, kw)
    n = len(frames)
    with SangNom2(clip, mode="fused", max_batch=n, **kw) as flt:
        _assert_frames(want, _batch(flt, clip, frames, par), f"{fmt} {w}x{h} {kw}")
        i = flt.info()
        assert i.fused_eligible == 1 and i.frames == n and i.fused_frames == n and i.banded_frames == 0, (i.fused_frames, i.banded_frames)


@pytest.mark.parametrize("case", sp.WIDE_SSE2, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in sp.WIDE_SSE2])
def test_the_sse2_sweeps_at_two_and_four_lines(hip_lib, case):
    """opt=1 with sse2_sweeps=1 against the numpy model of the reference's SSE2 path."""
    fmt, w, h = case
    clip = clip_format(fmt, w, h)
    frames, par = sp.frames_of(clip, 3, patterns=("noise01", "checker2", "noise")), sp.parities_of(3)
    want = ssc.want(clip, {}, frames, par, 1)
    for way in ("host", "batch"):
        with SangNom2(clip, mode="fused", opt=1, sse2_sweeps=1, **_way_kw(way, 3)) as flt:
            _assert_frames(want, _run(flt, clip, frames, par, way), f"{fmt} {w}x{h} opt=1 {way}")
            i = flt.info()
            assert i.fused_eligible == 1 and i.fused_frames == 3 and i.banded_frames == 0


# ---- c. coupled sweeps -------------------------------------------------------------------------------------------------------------

def _chroma_rows(clip, kw):
    planes = sp.planes_of(clip, kw)
    return sp.nr(planes[1][1]), sp.bh(planes[0][1])


@pytest.mark.parametrize("case", sp.COUPLED, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in sp.COUPLED])
def test_coupled_sweeps_whose_chroma_has_no_row_one_row_two_rows(hip_lib, case):
    fmt, w, h = case
    kw = dict(aac=48)
    clip, frames, par, want = sp.expected(fmt, w, h, kw)
    n = len(frames)
    nr_c, b = _chroma_rows(clip, kw)
    for way in ("host", "batch"):
        with SangNom2(clip, mode="fused", **_way_kw(way, n), **kw) as flt:
            _assert_frames(want, _run(flt, clip, frames, par, way), f"{fmt} {w}x{h} {way}")
            i = flt.info()
            assert i.fused_eligible == 1 and i.fused_frames == n and i.banded_frames == 0, (i.fused_frames, i.banded_frames)
            assert i.coupled_rows == sp.reach(nr_c, b) + 1, i.coupled_rows
            assert i.uv_sweeps == 0  # too short for U and V as one sweep


@pytest.mark.parametrize("case", sp.HANDOFF, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in sp.HANDOFF])
def test_hand_off_rows_of_short_coupled_sweeps_match_the_shared_pool(hip_lib, case):
    """What the luma sweep leaves for U and the U sweep for V is what the reference's shared pool holds at those points, inside
    the dependency cone of the chroma planes (tests/test_gpu_parity.py has the same check from 48 lines up)."""
    fmt, w, h = case
    kw = dict(aa=48, aac=48)
    clip = clip_format(fmt, w, h)
    nr_c, b = _chroma_rows(clip, kw)
    w_c = w // 2
    with SangNom2(clip, mode="fused", chroma_sweeps=1, **kw) as flt:
        rows = flt.info().coupled_rows
        assert rows == sp.reach(nr_c, b) + 1
        for f, src in enumerate(sp.frames_of(clip, 2)):
            model = NumpySangNom(width=w, height=h, bytes=clip.bytes, bits=clip.bits, planes=3, subw=1, subh=1, **kw)
            pools = []
            for p in (0, 1):
                d = np.zeros_like(src[p])
                d[0::2] = src[p][0::2]  # order=1 keeps the even lines
                model._plane(d, 0, p)
                pools.append(model.pool.copy())
            flt.get_frame(src, parity=f & 1)
            for which, last, extra in ((0, rows - 1, 6), (1, min(nr_c + 1, b - 1), 0)):
                got = flt.read_coupled_rows(which)[:, 1:last + 1]
                exp = pools[which][:, 1:last + 1, :w]
                if clip.bytes == 4:
                    got, exp = got.view(np.uint32), np.ascontiguousarray(exp, dtype=np.float32).view(np.uint32)
                got, exp = got.astype(np.int64), exp.astype(np.int64)
                q, x = np.arange(1, last + 1)[:, None], np.arange(w)[None, :]
                cone = (x < w_c + 3 * (nr_c - q + 2) + extra) & ((x >= w_c) | (q > nr_c))
                assert cone.any()
                bad = np.argwhere((got != exp) & cone[None])
                assert len(bad) == 0, f"frame {f} hand-off {which}: {len(bad)} samples differ, first (buffer, row - 1, x) {bad[:4].tolist()}"
        i = flt.info()
        assert i.fused_frames == 2 and i.uv_sweeps == 0


# ---- d. U and V as one sweep -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sp.UV, ids=[f"{c[0]}-{c[1]}x{c[2]}" + ("-dh" if c[3] else "") for c in sp.UV])
def test_u_and_v_as_one_sweep_on_both_sides_of_its_row_condition(hip_lib, case):
    fmt, w, h, dh = case
    kw = dict(aac=48, dh=True) if dh else dict(aac=48)
    clip, frames, par, want = sp.expected(fmt, w, h, kw)
    n = len(frames)
    near = sp.uv_rows_ok(*_chroma_rows(clip, kw))
    for policy, one_sweep in (({}, near), (dict(chroma_sweeps=1), False)):
        with SangNom2(clip, mode="fused", **policy, **kw) as flt:
            _assert_frames(want, _run(flt, clip, frames, par, "host"), f"{fmt} {w}x{h} {kw} {policy}")
            i = flt.info()
            assert i.fused_frames == n and i.banded_frames == 0
            assert i.uv_sweeps == (1 if one_sweep else 0), (i.uv_sweeps, near, policy)


# ---- e. row bands ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("warm", sp.BAND_WARMS)
@pytest.mark.parametrize("case", sp.BANDS, ids=[f"{c[0]}-{c[1]}x{c[2]}-b{c[3]}" for c in sp.BANDS])
def test_row_bands_on_both_sides_of_the_band_count(hip_lib, case, warm):
    """Auto mode, the default small-launch policy, bands forced.  Below two bands of eight rows the frame is not cut at all; from
    there on it is, and with the default run-up -- which reaches row 1 from every band of these short planes -- no frame fails
    the check.  A run-up of one row may fail it (the pool kernels redo the frame); the output is the oracle's either way."""
    fmt, w, h, forced = case
    clip, frames, par, want = sp.expected(fmt, w, h)
    n = len(frames)
    nb = sp.band_count(sp.nr(h), forced)
    with SangNom2(clip) as flt:
        flt.set_bands(forced, warm)
        _assert_frames(want, _run(flt, clip, frames, par, "host"), f"{fmt} {w}x{h} {forced} bands, run-up {warm}")
        i = flt.info()
        assert i.banded_frames == (n if nb else 0), (i.banded_frames, nb)
        if nb == 0 or warm == 0:
            assert i.band_fallbacks == 0, i.band_fallbacks
        else:
            assert 0 <= i.band_fallbacks <= n, i.band_fallbacks


# ---- f. the pool path --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sp.POOL, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in sp.POOL])
def test_pool_path_with_a_pool_of_one_row_and_of_two(hip_lib, case):
    fmt, w, h = case
    clip, frames, par, want = sp.expected(fmt, w, h)
    with SangNom2(clip, mode="pool") as flt:
        assert bool(flt.info().history_free) == (w % 32 == 0)
        _assert_frames(want, _run(flt, clip, frames, par, "host"), f"{fmt} {w}x{h} pool")
        i = flt.info()
        assert i.fused_frames == 0 and i.banded_frames == 0 and i.chained_frames == 0
        assert i.pool_rows == sp.bh(h) + 1 and i.pool_stride == sp.pool_stride(w)


@pytest.mark.parametrize("case", sp.POOL_CONTENTS, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in sp.POOL_CONTENTS])
def test_pool_contents_of_the_shortest_pools(hip_lib, case):
    """The pool itself after every frame, rows 0 and bh and the columns right of the plane included."""
    fmt, w, h = case
    clip = clip_format(fmt, w, h)
    ora = Oracle(oracle_cfg(clip))
    with SangNom2(clip, mode="pool") as flt:
        for f, src in enumerate(sp.frames_of(clip, 3)):
            want, got = ora.process(src, parity=f & 1), flt.get_frame(src, parity=f & 1)
            _assert_frames([want], [got], f"{fmt} {w}x{h} frame {f}")
            a, b = ora.pool(), flt.read_pool(0)
            assert a.shape == b.shape and same(a, b), f"{fmt} {w}x{h}: pool differs after frame {f}"
        assert flt.info().fused_frames == 0


# ---- g. chains ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chain", sp.CHAIN_POLICIES)
@pytest.mark.parametrize("case", sp.CHAINS, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in sp.CHAINS])
def test_chains_on_both_sides_of_their_conditions(hip_lib, case, chain):
    fmt, w, h, kw = case
    n = sp.CHAIN_FRAMES
    clip, frames, par, want = sp.expected(fmt, w, h, kw, n=n)
    chained = sp.chain_ok(clip, kw)
    with SangNom2(clip, max_batch=n, chain=chain, **kw) as flt:
        assert flt.info().history_free == 0
        _assert_frames(want, _batch(flt, clip, frames, par), f"{fmt} {w}x{h} chain={chain}")
        i = flt.info()
        assert i.frames == n and i.chained_frames == (n if chained else 0), (i.chained_frames, chained)
        assert i.fused_frames == 0 and i.banded_frames == 0 and i.chain_redone == 0


# ---- h. narrow planes --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fresh", [False, True], ids=["shared", "fresh"])
@pytest.mark.parametrize("case", sp.NARROW, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in sp.NARROW])
def test_planes_narrower_than_32_columns(hip_lib, case, fresh):
    """Host frames and a device batch.  Such a clip carries history (its pool stride is 32): the pool path, frame by frame, against
    one oracle instance.  With fresh_pool nothing is carried; 8 and 24 columns then take the padded sweep over the stride."""
    fmt, w, h = case
    ckw = dict(fresh_pool=True) if fresh else {}
    clip, frames, par, want = sp.expected(fmt, w, h, {}, ckw)
    n = len(frames)
    padded = fresh and w % 8 == 0
    for way in ("host", "batch"):
        with SangNom2(clip, **SWEEP, **_way_kw(way, n), **ckw) as flt:
            i = flt.info()
            assert (i.history_free, i.fused_eligible, i.pool_stride) == (int(fresh), int(padded), 32)
            _assert_frames(want, _run(flt, clip, frames, par, way), f"{fmt} {w}x{h} {ckw} {way}")
            i = flt.info()
            assert i.fused_frames == (n if padded else 0), (i.fused_frames, padded)
            assert i.banded_frames == 0 and i.chained_frames == 0


@pytest.mark.parametrize("case", sp.NARROW_CLIPS, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in sp.NARROW_CLIPS])
def test_clips_whose_chroma_is_one_or_two_columns_wide(hip_lib, case):
    fmt, w, h = case
    kw = dict(aac=48)
    clip, frames, par, want = sp.expected(fmt, w, h, kw)
    n = len(frames)
    for way in ("host", "batch"):
        with SangNom2(clip, **SWEEP, **_way_kw(way, n), **kw) as flt:
            assert flt.info().fused_eligible == 0
            _assert_frames(want, _run(flt, clip, frames, par, way), f"{fmt} {w}x{h} {way}")
            i = flt.info()
            assert i.fused_frames == 0 and i.banded_frames == 0 and i.chained_frames == 0


# ---- i. surfaces -------------------------------------------------------------------------------------------------------------------

SEMI = {"planar": (False, False), "semi": (True, False), "semi_msb": (True, True)}


@pytest.mark.parametrize("case", sp.SURFACES, ids=[f"{c[0]}-{c[1]}x{c[2]}-{c[3]}-to-{c[4]}" for c in sp.SURFACES])
def test_surfaces_of_a_few_pixels(hip_lib, case):
    """The numpy models of the layouts are those of the surface tests (tests/surface_cases.py, tests/msb_surface_cases.py,
    tests/packed_surface_cases.py), driven through their device helpers."""
    from tests import test_msb_surfaces_gpu as mg
    from tests import test_packed_surfaces_gpu as pg
    from tests import test_surfaces_gpu as sg
    fmt, w, h, src, dst = case
    clip, frames, par, want = sp.expected(fmt, w, h)
    n = len(frames)
    what = f"{fmt} {w}x{h} {src} -> {dst}"
    with SangNom2(clip, max_batch=n) as flt:
        if src in SEMI and dst in SEMI:
            got, expect = mg._run(flt, clip, frames, par, SEMI[src], SEMI[dst], want)
            sg._assert_frames(expect, got, what)
        else:
            pg._run(flt, clip, frames, par, src, dst, want, what)
        i, s = flt.info(), flt.surface_info()
        assert i.frames == n and i.fused_frames == 0 and i.banded_frames == 0
        assert (s.split_frames, s.merged_frames, s.copied_frames) == (n if src != "planar" else 0, n if dst != "planar" else 0, 0)


# ---- j. the anti-aliasing call -----------------------------------------------------------------------------------------------------

def _aa_batch(aa, clip, frames, par, dh):
    import torch
    dev, n = torch.device("cuda:0"), len(frames)
    src = sp.to_torch(frames, clip, dev)
    dst = [torch.zeros((n,) + aa.plane_shape_out(p), dtype=src[p].dtype, device=dev) for p in range(clip.planes)]
    torch.cuda.synchronize()
    aa.process_batch(src, dst, par)
    aa.synchronize()
    return [[to_host(dst[p][f]).view(clip.dtype) for p in range(clip.planes)] for f in range(n)]


def _sweeps_serve(clip):
    return clip.width % 32 == 0 and (clip.planes == 1 or (clip.width >> clip.subw) % 8 == 0)


@pytest.mark.parametrize("case", sp.AA, ids=[f"{c[0]}-{c[1]}x{c[2]}" + ("-dh" if c[3] else "") for c in sp.AA])
def test_anti_aliasing_call_on_planes_a_few_columns_wide_one_way_or_the_other(hip_lib, case):
    fmt, w, h, dh = case
    clip, frames, par, want = sp.expected_aa(fmt, w, h, dh, aac=48)
    n = len(frames)
    with SangNomAA(clip, max_batch=n, dh=dh, aac=48, **SWEEP) as aa:
        _assert_frames(want, _aa_batch(aa, clip, frames, par, dh), f"{fmt} {w}x{h} dh={dh}")
        for k, (pass_clip, _) in enumerate(sp.aa_pass_clips(fmt, w, h, dh)):
            i = aa.info(k)
            assert i.frames == n and i.fused_frames == (n if _sweeps_serve(pass_clip) else 0), (k, i.frames, i.fused_frames)
            assert i.banded_frames == 0


def test_the_enlargement_of_a_two_line_clip_runs_its_second_pass_in_parts(hip_lib):
    fmt, w, h = sp.AA_PARTS
    clip, frames, par, want = sp.expected_aa(fmt, w, h, True)
    n = len(frames)
    with SangNomAA(clip, max_batch=n, dh=True, column_parts=1, **SWEEP) as aa:
        assert aa.info(1).fused_eligible == 1 and aa.parts_info(1).parts[0] >= 2 and aa.parts_info(0).parts[0] == 0
        _assert_frames(want, _aa_batch(aa, clip, frames, par, True), f"{fmt} {w}x{h} enlargement")
        pi = aa.parts_info(1)
        assert aa.info(1).fused_frames == n and pi.part_frames == n and pi.part_fallbacks == 0, (pi.part_frames, pi.part_fallbacks)
        assert aa.info(0).fused_frames == 0  # the turned clip is two columns wide
