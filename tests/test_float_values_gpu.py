"""The float code of the library -- the fused sweep (sn_fused_f32_v3.hip: plain, padded, coupled 4:2:0 / 4:2:2, row bands)
and the float instances of the pool kernels, the chain and the anti-aliasing call -- bit-exact against the CPU oracle on the
sample values the generic patterns never feed: negative and out-of-range samples, k / 255, denormals, -0.0, a ladder minimum
equal to the threshold, huge finite samples and non-finite ones (tests/float_cases.py; test_float_values_cpu.py shows what
each input reaches in the reference).  No tolerance anywhere: float planes are compared on their bit patterns.

Every path runs at the smallest shape that still reaches it: one wave; a second wave that is nearly empty (real ghosts);
several waves (parked buffers in LDS); a padded sweep of one and of two strips' worth of lanes; 4:2:0 with the chroma region
ending inside a strip (the packed and the fetch rows) and 4:2:2; six row bands with the default run-up and with a run-up from
the top of the plane; the pool kernels and the chain on clips whose pool carries history (100 and 104 columns: no multiple of 32).
"""
import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2, SangNomAA, capi, clip_format
from oracle.oracle import Oracle
from tests import float_cases as fc
from tests.aa_script import Script
from tests.util import describe_diff, oracle_cfg, same, to_host

pytestmark = pytest.mark.gpu

PLAIN = (("Y32", 64, 24), ("Y32", 544, 24), ("Y32", 1536, 16))
PADDED = (("Y32", 72, 24), ("Y32", 200, 24))
COUPLED = (("YUV420PS", 64, 40), ("YUV420PS", 1024, 40), ("YUV422PS", 576, 28))
BANDS = (("Y32", 480, 200, (6, 0)), ("Y32", 480, 200, (6, 100)))
HISTORY = ("Y32", 100, 40)  # the pool carries state from frame to frame: the pool kernels, pass by pass
CHAIN = ("Y32", 104, 40)    # ... and a width of whole lanes (8 columns), which a batch runs as a chain of passes
AA_CALL = ("Y32", 96, 64)

_ids = lambda s: f"{s[0]}-{s[1]}x{s[2]}" + (f"-bands{s[3][1]}" if len(s) > 3 else "")


def _assert_planes(want, got, what):
    for p in range(len(want)):
        assert same(want[p], got[p]), f"{what} plane {p}: " + describe_diff(want[p], got[p])


def _check(fmt, w, h, kw, pattern, mode="fused", bands=None, fresh=False, n=fc.NFRAMES, slope_aa=None):
    """`n` frames of one filter instance against one oracle instance (fresh: against a new one per frame, which is what
    sn_config.fresh_pool promises), parities 0 and 1, and the path asserted through info()."""
    clip = clip_format(fmt, w, h)
    ora = Oracle(oracle_cfg(clip, **kw))
    with SangNom2(clip, mode="auto" if bands else mode, fresh_pool=fresh, **kw) as flt:
        if bands:
            flt.set_bands(*bands)
        if mode == "fused":
            assert flt.info().fused_eligible == 1
        for f, src in enumerate(fc.frames(clip, pattern, n=n, aa=slope_aa)):
            if fresh:
                ora = Oracle(oracle_cfg(clip, **kw))
            want = ora.process(src, parity=f & 1)
            got = flt.get_frame(src, parity=f & 1)
            _assert_planes(want, got, f"{fmt} {w}x{h} {kw} {pattern} {mode} bands={bands} frame {f}")
            if pattern == "negzero":
                assert all((g.view(np.uint32) == 0x80000000).all() for g in got)
        info = flt.info()
        if bands:
            assert info.banded_frames == n
            # a run-up that reaches the top of the plane (h / 2 kept lines) gives every band the exact state: no frame may be
            # redone by the pool kernels, and what was compared is the band instances' own output
            assert info.band_fallbacks == 0 or bands[1] < h // 2, (pattern, info.band_fallbacks)
        elif mode == "fused":
            assert info.fused_frames == n and info.banded_frames == 0
        else:
            assert info.fused_frames == 0 and info.banded_frames == 0
    return info


@pytest.mark.parametrize("aa", fc.AA)
@pytest.mark.parametrize("shape", PLAIN, ids=_ids)
def test_plain_sweep(hip_lib, shape, aa):
    for pattern in fc.PATTERNS:
        _check(*shape, dict(order=1, aa=aa), pattern)


@pytest.mark.parametrize("aa", fc.AA)
@pytest.mark.parametrize("shape", PADDED, ids=_ids)
def test_padded_sweep(hip_lib, shape, aa):
    """A plane narrower than its pool stride on a pool zeroed per frame: costs are multiplied by 1 or 0."""
    for pattern in fc.PATTERNS:
        _check(*shape, dict(order=1, aa=aa), pattern, fresh=True)


@pytest.mark.parametrize("aa", fc.AA)
@pytest.mark.parametrize("shape", COUPLED, ids=_ids)
def test_coupled_sweeps(hip_lib, shape, aa):
    """Luma and chroma share the pool: the chroma sweeps select, lane by lane, between their own costs and what luma left."""
    for pattern in fc.PATTERNS:
        _check(*shape, dict(order=1, aa=aa, aac=aa), pattern)


@pytest.mark.parametrize("aa", fc.AA)
@pytest.mark.parametrize("shape", BANDS, ids=_ids)
def test_row_bands(hip_lib, shape, aa):
    for pattern in fc.PATTERNS:
        _check(*shape[:3], dict(order=1, aa=aa), pattern, bands=shape[3])


@pytest.mark.parametrize("aa", fc.AA)
def test_pool_kernels_carrying_history(hip_lib, aa):
    for pattern in fc.PATTERNS:
        _check(*HISTORY, dict(order=1, aa=aa), pattern, mode="pool", n=3)


def _to_dev(frames):
    import torch
    return [torch.from_numpy(np.stack([fr[0] for fr in frames])).pin_memory().to(torch.device("cuda:0"))]


@pytest.mark.parametrize("aa", fc.AA)
@pytest.mark.parametrize("shape", (HISTORY, CHAIN), ids=_ids)
def test_device_batch_carrying_history(hip_lib, shape, aa):
    """A batch of four frames of a history-carrying clip equals frame after frame of ONE oracle instance: at 100 columns pass
    by pass through the pool kernels (the chain takes planes of whole lanes, 8 columns), at 104 as one chain of passes
    (k_smooth_f32_chain)."""
    import torch
    clip = clip_format(*shape)
    N = 4
    for pattern in fc.PATTERNS:
        frames = fc.frames(clip, pattern, n=N)
        ora = Oracle(oracle_cfg(clip, aa=aa))
        with SangNom2(clip, max_batch=N, aa=aa) as flt:
            assert flt.info().history_free == 0
            src = _to_dev(frames)
            dst = [torch.zeros((N,) + flt.plane_shape_out(0), dtype=torch.float32, device=src[0].device)]
            torch.cuda.synchronize()
            flt.process_batch(src, dst)
            flt.synchronize()
            assert flt.info().chained_frames == (N if shape is CHAIN else 0), "the chain of passes did not run"
            assert flt.info().fused_frames == 0
            for f in range(N):
                _assert_planes(ora.process(frames[f]), [to_host(dst[0][f])], f"batch {shape} aa={aa} {pattern} frame {f}")


@pytest.mark.parametrize("aa", fc.AA)
def test_anti_aliasing_call(hip_lib, aa):
    """TurnLeft().SangNom2().TurnRight().SangNom2() in one call, the frames staying on the device, against the script."""
    import torch
    clip = clip_format(*AA_CALL)
    for pattern in fc.PATTERNS:
        frames = fc.frames(clip, pattern)
        script = Script(clip, aa=aa)
        with SangNomAA(clip, max_batch=len(frames), small_launches=capi.SN_SMALL_SWEEP, aa=aa) as call:
            src = _to_dev(frames)
            dst = [torch.zeros_like(src[0])]
            torch.cuda.synchronize()
            call.process_batch(src, dst)
            call.synchronize()
            assert call.info(0).fused_frames == len(frames) and call.info(1).fused_frames == len(frames)
        for f, fr in enumerate(frames):
            _assert_planes(script.frame(fr), [to_host(dst[0][f])], f"anti-aliasing call aa={aa} {pattern} frame {f}")


@pytest.mark.parametrize("aa", fc.SLOPE_AA)
def test_a_minimum_equal_to_the_threshold_is_not_above_it(hip_lib, aa):
    """`minbuf > aaf` is strict (SangNom2.cpp:211).  On the slope the smoothed minimum of the first interpolated row IS the
    threshold: a `>=` anywhere would interpolate straight down instead of along buffer 5."""
    for shape in PLAIN:
        _check(*shape, dict(order=1, aa=aa), "slope", slope_aa=aa)
    for shape in PADDED:
        _check(*shape, dict(order=1, aa=aa), "slope", fresh=True, slope_aa=aa)
    for shape in BANDS:
        _check(*shape[:3], dict(order=1, aa=aa), "slope", bands=shape[3], slope_aa=aa)
    for shape in COUPLED:  # the slope is the luma plane; chroma is signed noise
        _check(*shape, dict(order=1, aa=aa, aac=aa), "slope", slope_aa=aa)


HUGE_WAYS = {"fused": dict(mode="fused"), "pool": dict(mode="pool"), "bands": dict(bands=(6, 100)), "bands-from-the-top": dict(bands=(6, 200))}


@pytest.mark.parametrize("way", sorted(HUGE_WAYS))
def test_huge_finite_samples(hip_lib, way):
    """Samples beyond FLT_MAX / 4 are finite, yet the reference's 4 * p1 is an infinity of its own before 5 * p2 is added; a
    fused multiply-add keeps the sum finite and narrows the cone of infinite cost by a column.  Every output sample is
    finite (test_float_values_cpu.py), so every sample is compared.  Row bands twice: an infinite cost never decays, so with
    a run-up of 100 of the plane's 200 rows the lower bands' guessed state stays wrong, their check says so and the frame is
    redone by the pool kernels (the result must be right all the same); with a run-up of 200 rows every band starts at the top
    and the band instances' own output is what is compared."""
    fmt, w, h = fc.HUGE_SHAPE
    _check(fmt, w, h, dict(order=1, aa=128), "huge", **HUGE_WAYS[way])


def _check_non_finite(shape, kw, **how):
    fmt, w, h, every = shape
    clip = clip_format(fmt, w, h)
    bands = how.pop("bands", None)
    with SangNom2(clip, **how, **kw) as flt:
        if bands:
            flt.set_bands(*bands)
        frames = fc.frames(clip, "nonfinite", every=every)
        for f, src in enumerate(frames):
            want, written = fc.written_by_reference(clip, src, parity=f & 1, **kw)
            got = flt.get_frame(src, parity=f & 1)
            for p in range(len(want)):
                fc.assert_defined_samples_match(want[p], written[p], got[p], f"{fmt} {w}x{h} {how} frame {f} plane {p}")
        info = flt.info()
        if bands:
            assert info.banded_frames == len(frames)
        else:
            assert info.fused_frames == len(frames) and info.banded_frames == 0


def test_non_finite_samples_in_the_plain_sweep(hip_lib):
    _check_non_finite(fc.NONFINITE_PLAIN, {}, mode="fused")


def test_non_finite_samples_in_the_padded_sweep(hip_lib):
    """An infinite cost times the padding's zero would be a NaN: the padding lanes must not see the plane's costs."""
    _check_non_finite(fc.NONFINITE_PADDED, {}, mode="fused", fresh_pool=True)


def test_non_finite_samples_in_the_coupled_sweeps(hip_lib):
    """The chroma sweeps take stale luma values lane by lane: an infinity or a NaN of luma's must arrive where the reference
    reads it and nowhere else."""
    _check_non_finite(fc.NONFINITE_COUPLED, dict(aac=48), mode="fused")


def test_non_finite_samples_in_row_bands(hip_lib):
    _check_non_finite(fc.NONFINITE_BANDS, {}, mode="auto", bands=(6, 100))
