"""The fused sweeps in the SSE2 arithmetic (opt=1 with sn_policy.sse2_sweeps = 1) on the GPU: 16-bit planes on their own,
padded sweeps, row bands, the pool-coupled sweeps of 4:2:0 / 4:2:2 in 8 and 16 bits, U and V as one sweep, the hand-off
rows and the anti-aliasing call.

Everything is bit-exact, tolerance zero, against the reference's own opt=1 outputs (tests/golden/sse2_*.npz) and the numpy
model that reproduces them (tests/sse2_model.py).  Cases come from tests/sse2_sweep_cases.py; every 8-bit and 16-bit case
asserts first (sc.expected) that the model's opt=1 output differs from its opt=0 output on the input, so a sweep that kept
the wrapping arithmetic cannot pass.  Without the knob the same contexts report and run as before (the pool kernels).
"""
import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2, SangNomAA, SangNomError, capi, clip_format, synth
from tests import sse2_model as sm
from tests import sse2_sweep_cases as sc
from tests.aa_script import Script
from tests.util import describe_diff, same, to_host

pytestmark = pytest.mark.gpu

ON = dict(opt=1, sse2_sweeps=1)
# how a context is asked to run (tests/test_sse2_mode_gpu.py, PATHS), plus the whole-plane sweeps demanded outright
PATHS = {"fused": dict(mode="fused"), "sweep": dict(small_launches=capi.SN_SMALL_SWEEP), "auto": {}, "pool": dict(mode="pool")}


def _assert_frames(want, got, what):
    for p, (a, b) in enumerate(zip(want, got)):
        assert same(a, b), f"{what} plane {p}: " + describe_diff(a, b)


def _batch(flt, clip, frames, parities):
    import torch
    dev, n = torch.device("cuda:0"), len(frames)
    src = sc.to_torch(frames, clip, dev)
    dst = [torch.zeros((n,) + flt.plane_shape_out(p), dtype=src[p].dtype, device=dev) for p in range(clip.planes)]
    torch.cuda.synchronize()
    flt.process_batch(src, dst, parities)
    flt.synchronize()
    return [[to_host(dst[p][f]).view(clip.dtype) for p in range(clip.planes)] for f in range(n)]


# ---- 1. the reference's own outputs through the sweeps --------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.FIXTURES)
def test_reference_fixture_through_the_sweeps(hip_lib, name):
    meta, frames, out1, _ = sm.load_fixture(name)
    clip, n = clip_format(meta["fmt"], meta["width"], meta["height"]), meta["nframes"]
    with SangNom2(clip, mode="fused", **ON, **meta["kw"]) as flt:
        assert flt.info().fused_eligible == 1
        for f, src in enumerate(frames):
            _assert_frames(out1[f], flt.get_frame(src, parity=meta["parity"][f]), f"{name} frame {f}")
        assert flt.info().fused_frames == n
    with SangNom2(clip, mode="fused", max_batch=n, **ON, **meta["kw"]) as flt:
        for f, got in enumerate(_batch(flt, clip, frames, meta["parity"])):
            _assert_frames(out1[f], got, f"{name} batch frame {f}")
        assert flt.info().fused_frames == n


def test_history_carrying_fixture_is_unchanged_by_the_knob(hip_lib):
    meta, frames, out1, _ = sm.load_fixture(sc.FIXTURE_NOT_ELIGIBLE)
    clip = clip_format(meta["fmt"], meta["width"], meta["height"])
    with SangNom2(clip, **ON, **meta["kw"]) as flt:
        assert flt.info().fused_eligible == 0
        for f, src in enumerate(frames):
            _assert_frames(out1[f], flt.get_frame(src, parity=meta["parity"][f]), f"frame {f}")
    with pytest.raises(SangNomError, match="not eligible"):  # the ordinary message, not the arithmetic's
        SangNom2(clip, mode="fused", **ON, **meta["kw"])


# ---- 2. reporting ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,w,h,kw", sc.REPORTING, ids=[f"{c[0]}-{'iso' if c[3].get('isolated_planes') else 'shared'}" for c in sc.REPORTING])
def test_the_knob_decides_where_the_planes_run(hip_lib, fmt, w, h, kw):
    sweep = capi.SN_SMALL_SWEEP
    clip = clip_format(fmt, w, h)
    src = synth.frame(clip, "noise01", seed=1)
    with SangNom2(clip, small_launches=sweep, **ON, **kw) as flt:
        assert flt.info().fused_eligible == 1
        assert flt.get_policy().sse2_sweeps == 1
        flt.get_frame(src)
        i = flt.info()
        assert i.frames == 1 and i.fused_frames == 1 and i.banded_frames == 0
        flt.set_policy(sse2_sweeps=0)  # read at creation only: ignored, and reported as created
        assert flt.get_policy().sse2_sweeps == 1 and flt.info().fused_eligible == 1
        flt.get_frame(src)
        assert flt.info().fused_frames == 2
    with SangNom2(clip, mode="fused", **ON, **kw) as flt:
        flt.get_frame(src)
        assert flt.info().fused_frames == 1
    for off in (dict(sse2_sweeps=0), {}):  # as today
        with SangNom2(clip, opt=1, small_launches=sweep, **off, **kw) as flt:
            assert flt.info().fused_eligible == 0 and flt.get_policy().sse2_sweeps == 0
            flt.set_policy(sse2_sweeps=1)
            assert flt.get_policy().sse2_sweeps == 0 and flt.info().fused_eligible == 0
            flt.get_frame(src)
            i = flt.info()
            assert i.frames == 1 and i.fused_frames == 0 and i.banded_frames == 0
        with pytest.raises(SangNomError, match="SN_ARITH_SSE2") as ei:
            SangNom2(clip, opt=1, mode="fused", **off, **kw)
        assert ei.value.code == capi.SN_ERR_UNSUPPORTED
    want0 = None
    for knob in (1, 0):  # no effect in the default arithmetic
        with SangNom2(clip, opt=0, small_launches=sweep, sse2_sweeps=knob, **kw) as flt:
            assert flt.info().fused_eligible == 1 and hip_lib.sn_get_arithmetic(flt._h) == capi.SN_ARITH_CXX
            got = flt.get_frame(src)
            assert flt.info().fused_frames == 1
        if want0 is None:
            want0 = got
        _assert_frames(want0, got, "opt=0 with and without the knob")


def test_the_knob_has_no_effect_on_a_float_context(hip_lib):
    clip = clip_format("Y32", 256, 32)
    src = synth.frame(clip, "noise", seed=2)
    out = []
    for knob in (0, 1):
        with SangNom2(clip, opt=1, sse2_sweeps=knob, mode="fused") as flt:
            assert flt.info().fused_eligible == 1
            out.append(flt.get_frame(src))
    _assert_frames(out[0], out[1], "float")


# ---- 3. 16-bit planes on their own ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("case", sc.PLAIN16, ids=[sc.case_id(c) for c in sc.PLAIN16])
def test_16_bit_planes_on_their_own_match_the_model(hip_lib, case, path):
    fmt, w, h, kw, ckw, n, pattern = case
    clip, frames, parities, want = sc.expected(fmt, w, h, kw, ckw, n, pattern)
    with SangNom2(clip, **ON, **kw, **ckw, **PATHS[path]) as flt:
        assert flt.info().fused_eligible == 1
        for f, src in enumerate(frames):
            _assert_frames(want[f], flt.get_frame(src, parity=parities[f]), f"frame {f}")
        i = flt.info()
        assert i.frames == n
        if path in ("fused", "sweep"):
            assert i.fused_frames == n and i.banded_frames == 0
        if path == "pool":
            assert i.fused_frames == 0


# ---- 4. padded sweeps of fresh pools ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["auto", "fused"])
@pytest.mark.parametrize("fmt,w,h,kw,pattern", sc.PADDED16, ids=[f"{c[0]}-{c[1]}x{c[2]}-{c[4]}" for c in sc.PADDED16])
def test_padded_16_bit_sweeps_of_fresh_pools_match_the_model(hip_lib, fmt, w, h, kw, pattern, mode):
    n = 3
    clip, frames, parities, want = sc.expected(fmt, w, h, kw, dict(fresh_pool=True), n, pattern, (1, 0, 1))
    assert all((w >> (clip.subw if p else 0)) % 8 == 0 and (w >> (clip.subw if p else 0)) % 32 != 0 for p in range(clip.planes))
    with SangNom2(clip, fresh_pool=True, mode=mode, small_launches=capi.SN_SMALL_SWEEP, **ON, **kw) as flt:
        assert flt.info().fused_eligible == 1 and flt.info().history_free == 1
        for f, src in enumerate(frames):  # one frame per launch
            _assert_frames(want[f], flt.get_frame(src, parity=parities[f]), f"frame {f}")
        i = flt.info()
        assert i.frames == n and i.fused_frames == n and i.banded_frames == 0, "the padded sweep did not serve these frames"
    with SangNom2(clip, fresh_pool=True, mode=mode, max_batch=n, small_launches=capi.SN_SMALL_SWEEP, **ON, **kw) as flt:  # ... and a batch
        for f, got in enumerate(_batch(flt, clip, frames, parities)):
            _assert_frames(want[f], got, f"batch frame {f}")
        i = flt.info()
        assert i.fused_frames == n and i.banded_frames == 0


# ---- 5. row bands -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,w,h,kw", sc.BANDS, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in sc.BANDS])
def test_row_bands_in_the_mode_agree_with_every_other_path(hip_lib, fmt, w, h, kw):
    """SN_MODE_AUTO with bands forced, switched off or left to the shipped policy, and SN_MODE_POOL: one answer, the
    model's.  With the knob on these clips are really cut into bands (4:2:0: the luma plane, the chroma planes follow on the
    pool kernels), which without it they never are."""
    clip, frames, parities, want = sc.expected(fmt, w, h, kw, {}, sc.BANDS_FRAMES, sc.BANDS_PATTERN, (1, 1))
    for mode, bands in (("auto", 4), ("auto", -1), ("auto", 0), ("pool", 0)):
        with SangNom2(clip, mode=mode, **ON, **kw) as flt:
            if bands:
                flt.set_bands(bands)
            for f, src in enumerate(frames):
                _assert_frames(want[f], flt.get_frame(src, parity=parities[f]), f"{mode} bands {bands} frame {f}")
            i = flt.info()
            if bands > 0:
                assert i.banded_frames == len(frames) and i.fused_frames == len(frames), "the forced bands did not run"
                assert i.band_fallbacks == 0
            if bands < 0 or mode == "pool":
                assert i.banded_frames == 0


def test_a_band_whose_check_fails_is_redone_in_the_mode(hip_lib):
    """A run-up of one row cannot forget the guessed state: the check fails and the guarded pool kernels redo the frame,
    in the context's arithmetic."""
    fmt, w, h, kw = sc.BANDS[0]
    clip, frames, parities, want = sc.expected(fmt, w, h, kw, {}, sc.BANDS_FRAMES, sc.BANDS_PATTERN, (1, 1))
    with SangNom2(clip, **ON, **kw) as flt:
        flt.set_bands(4, warm_rows=1)
        for f, src in enumerate(frames):
            _assert_frames(want[f], flt.get_frame(src, parity=parities[f]), f"frame {f}")
        i = flt.info()
        assert i.banded_frames == len(frames) and i.band_fallbacks > 0


# ---- 6. pool-coupled sweeps ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chroma_sweeps", [0, 1])
@pytest.mark.parametrize("case", sc.COUPLED, ids=[sc.case_id(c) for c in sc.COUPLED])
def test_pool_coupled_sweeps_match_the_model(hip_lib, case, chroma_sweeps):
    """Luma, U and V of clips whose subsampled chroma shares the luma pool, as three sweeps with two hand-off pools
    (chroma_sweeps=1; 16-bit always) or -- 8-bit, where the geometry allows -- luma and ONE sweep for U and V (chroma_sweeps=0):
    the one-sweep form has instances of the SSE2 arithmetic, so sn_info.uv_sweeps is 1 there."""
    fmt, w, h, kw, ckw, n, pattern = case
    clip, frames, parities, want = sc.expected(fmt, w, h, kw, ckw, n, pattern)
    with SangNom2(clip, mode="fused", chroma_sweeps=chroma_sweeps, **ON, **kw, **ckw) as flt:
        for f, src in enumerate(frames):
            _assert_frames(want[f], flt.get_frame(src, parity=parities[f]), f"frame {f}")
        i = flt.info()
        assert i.frames == n and i.fused_frames == n and i.banded_frames == 0
        one_sweep = clip.bytes == 1 and chroma_sweeps == 0 and not ckw and _uv_geometry(clip)
        assert i.uv_sweeps == (1 if one_sweep else 0)
    if n > 1 and not ckw:  # ... and the frames as one batch
        with SangNom2(clip, mode="fused", chroma_sweeps=chroma_sweeps, max_batch=n, **ON, **kw) as flt:
            for f, got in enumerate(_batch(flt, clip, frames, parities)):
                _assert_frames(want[f], got, f"batch frame {f}")
            assert flt.info().fused_frames == n


def _uv_geometry(clip):
    """Geometries U and V run as one sweep on (fused_uv_ok, sn_fused_u8_uv.hip): at least six chroma row pairs for the
    skew of two steps, and no more chroma rows than the pool has below row 0."""
    nr_c = (clip.height >> clip.subh) // 2 - 1
    return nr_c >= 6 and nr_c <= (clip.height + 1) // 2 - 1


# ---- 7. hand-off rows ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chroma_sweeps", [0, 1])
@pytest.mark.parametrize("fmt,w,h", sc.HANDOFF, ids=[c[0] for c in sc.HANDOFF])
def test_hand_off_rows_match_the_models_shared_pool(hip_lib, fmt, w, h, chroma_sweeps):
    """What the luma sweep leaves for U (and, as two chroma sweeps, U for V) is sample for sample what the SSE2 path's shared
    pool holds at those points: saturated sums, which the final planes alone show only above the aa threshold."""
    kw = dict(aa=48, aac=48)
    clip, frames, _, _ = sc.expected(fmt, w, h, kw, {}, 1, sc.HANDOFF_PATTERN, (1,), sc.HANDOFF_SEED)
    src = frames[0]
    m = sm.model_for(1, w, h, bytes=clip.bytes, bits=clip.bits, planes=3, subw=1, subh=1, **kw)
    base = sm.model_for(0, w, h, bytes=clip.bytes, bits=clip.bits, planes=3, subw=1, subh=1, **kw)
    pools, pools0 = [], []
    for p in (0, 1):
        for mod, keep in ((m, pools), (base, pools0)):
            d = np.zeros_like(src[p])
            d[0::2] = src[p][0::2]  # order=1 keeps the even lines
            mod._plane(d, 0, p)
            keep.append(mod.pool.copy())
    with SangNom2(clip, mode="fused", chroma_sweeps=chroma_sweeps, **ON, **kw) as flt:
        flt.get_frame(src)
        rows = flt.info().coupled_rows
        nr_c, bh, w_c = h // 4 - 1, (h + 1) // 2, w // 2
        assert rows == min(nr_c + 2, bh - 1) + 1
        hand_offs = ((0, rows - 1, 6), (1, min(nr_c + 1, bh - 1), 0))
        for which, last, extra in hand_offs[:2 if chroma_sweeps == 1 else 1]:
            got = flt.read_coupled_rows(which)[:, 1:last + 1].astype(np.int64)
            exp = np.asarray(pools[which][:, 1:last + 1, :w]).astype(np.int64)
            q = np.arange(1, last + 1)[:, None]
            x = np.arange(w)[None, :]
            cone = (x < w_c + 3 * (nr_c - q + 2) + extra) & ((x >= w_c) | (q > nr_c))  # what is handed on (sn_fused_v3_common.h)
            assert cone.any()
            assert ((np.asarray(pools0[which][:, 1:last + 1, :w]).astype(np.int64) != exp) & cone[None]).any(), "the two arithmetics agree on these rows"
            bad = np.argwhere((got != exp) & cone[None])
            assert len(bad) == 0, f"hand-off {which}: {len(bad)} samples differ, first (buffer,row-1,x) {bad[:4].tolist()}"


# ---- 8. the anti-aliasing call ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,w,h,kw", sc.AA, ids=[c[0] for c in sc.AA])
def test_anti_aliasing_call_with_the_knob(hip_lib, fmt, w, h, kw):
    import torch
    clip = clip_format(fmt, w, h)
    frames = sc.frames_of(clip, sc.AA_PATTERN, sc.AA_FRAMES, sc.AA_SEED)
    s1, s0 = Script(clip, opt=1, fresh=True, **kw), Script(clip, opt=0, fresh=True, **kw)
    want = [s1.frame(fr) for fr in frames]
    assert sc.differs(want, [s0.frame(fr) for fr in frames]), "this case cannot tell the SSE2 arithmetic from the default"
    dev = torch.device("cuda:0")
    with SangNomAA(clip, max_batch=1, fresh_pool=True, **ON, **kw) as aa:
        assert aa.info(0).fused_eligible == 1 and aa.info(1).fused_eligible == 1
        for f, fr in enumerate(frames):
            src = sc.to_torch([fr], clip, dev)
            dst = [torch.zeros_like(s) for s in src]
            torch.cuda.synchronize()
            aa.process_batch(src, dst)
            aa.synchronize()
            _assert_frames(want[f], [to_host(dst[p][0]).view(clip.dtype) for p in range(clip.planes)], f"frame {f}")
    with SangNomAA(clip, max_batch=1, fresh_pool=True, opt=1, **kw) as aa:  # without the knob: as before
        assert aa.info(0).fused_eligible == aa.info(1).fused_eligible == (1 if clip.bytes == 1 else 0)
