"""Column parts on the GPU (sn_options.column_parts = 1): 16-bit and float planes wider than one workgroup of the sweeps
holds, swept as 2..N windows whose seams are checked (sn_fused_v3_common.h kParts, sn_band.hip k_parts_verify).

Everything is bit-exact against the CPU oracle (float planes on their bit patterns), in batches of three frames with different
content, and contexts are created with mode="fused": without the feature a 3872-wide 16-bit clip is not eligible and creation
itself fails.  Where the inputs are those on which the reference alone converges within the ghost
(tests/test_column_parts_cpu.py) no frame may take the fallback; the fallback has tests of its own, forced (a seam 8 columns
from a window's end) and natural (checker2, the fixed point of the floor).
"""
import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2, SangNomAA, SangNomError, capi, clip_format, synth
from oracle.oracle import Oracle
from tests import column_parts_cases as cc
from tests import float_cases as fc
from tests import sse2_sweep_cases as sc
from tests.aa_dh_script import Script
from tests.util import describe_diff, oracle_cfg, same, to_host

pytestmark = pytest.mark.gpu

ON = dict(mode="fused", column_parts=1)
TRIPLES = (("noise", "sine", "edges"), ("checker", "noise", "sine"))  # three frames of different content; all four patterns


def _assert_frames(want, got, what):
    for p, (a, b) in enumerate(zip(want, got)):
        assert same(a, b), f"{what} plane {p}: " + describe_diff(a, b)


def _batch(flt, clip, frames, parities):
    import torch
    dev, n = torch.device("cuda:0"), len(frames)
    src = cc.to_torch(frames, clip, dev)
    dst = [torch.zeros((n,) + flt.plane_shape_out(p), dtype=src[p].dtype, device=dev) for p in range(clip.planes)]
    torch.cuda.synchronize()
    flt.process_batch(src, dst, parities)
    flt.synchronize()
    return [[to_host(dst[p][f]).view(clip.dtype) for p in range(clip.planes)] for f in range(n)]


def _run_case(case, patterns, parities=cc.PARITIES):
    fmt, w, h, kw, ckw = case
    clip, frames, want = cc.expected(fmt, w, h, kw, ckw, patterns, parities)
    n = len(frames)
    with SangNom2(clip, max_batch=n, **ON, **kw, **ckw) as flt:
        assert flt.info().fused_eligible == 1
        pi = flt.parts_info()
        assert pi.parts[0] >= 2 and pi.ghost_columns == cc.GHOST[clip.bytes], (list(pi.parts), pi.ghost_columns)
        got = _batch(flt, clip, frames, parities)
        for f in range(n):
            _assert_frames(want[f], got[f], f"{cc.case_id(case)} {patterns[f]} frame {f}")
        i, pi = flt.info(), flt.parts_info()
        assert i.frames == n and i.fused_frames == n and i.banded_frames == 0
        assert pi.part_frames == n and pi.part_fallbacks == 0, (pi.part_frames, pi.part_fallbacks)


# ---- 1. natural widths ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("patterns", TRIPLES, ids=["-".join(t) for t in TRIPLES])
@pytest.mark.parametrize("case", cc.NATURAL, ids=[cc.case_id(c) for c in cc.NATURAL])
def test_wide_planes_in_parts_match_the_oracle(hip_lib, case, patterns):
    _run_case(case, patterns)


@pytest.mark.parametrize("case", cc.ORDERS, ids=[cc.case_id(c) for c in cc.ORDERS])
def test_orders_parities_and_dh(hip_lib, case):
    _run_case(case, TRIPLES[0], parities=(0, 1, 0))


# ---- 2. forced parts on narrow planes: middle windows with two seams ---------------------------------------------------------

@pytest.mark.parametrize("parts", cc.FORCED_PARTS)
@pytest.mark.parametrize("shape", cc.FORCED, ids=[f"{s[0]}-{s[1]}x{s[2]}" for s in cc.FORCED])
def test_forced_parts_on_a_narrow_plane(hip_lib, shape, parts):
    fmt, w, h = shape
    for patterns in TRIPLES:
        clip, frames, want = cc.expected(fmt, w, h, {}, {}, patterns)
        with SangNom2(clip, max_batch=len(frames), **ON) as flt:
            assert list(flt.parts_info().parts) == [0, 0, 0]  # fits one workgroup: not cut on its own
            flt.debug_set_column_parts(parts, 0)
            assert flt.parts_info().parts[0] == parts
            got = _batch(flt, clip, frames, cc.PARITIES)
            for f in range(len(frames)):
                _assert_frames(want[f], got[f], f"{fmt} {parts} parts {patterns[f]} frame {f}")
            pi = flt.parts_info()
            assert pi.part_frames == len(frames) and pi.part_fallbacks == 0, (pi.part_frames, pi.part_fallbacks)
            flt.debug_set_column_parts(0, 0)
            assert list(flt.parts_info().parts) == [0, 0, 0]
        with SangNom2(clip, mode="fused") as flt:  # the hook needs the option
            with pytest.raises(SangNomError):
                flt.debug_set_column_parts(parts, 0)


# ---- 3. forced fallback ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [cc.WIDE_Y16, ("Y32", 512, 64)], ids=["Y16-3872x32", "Y32-512x64-forced"])
def test_a_seam_next_to_a_window_end_sends_every_frame_to_the_pool_path(hip_lib, shape):
    fmt, w, h = shape
    patterns = ("noise",) * 3
    clip, frames, want = cc.expected(fmt, w, h, {}, {}, patterns)
    n = len(frames)
    with SangNom2(clip, max_batch=n, **ON) as flt:
        flt.debug_set_column_parts(0 if w > 3840 else 2, 8)
        assert flt.parts_info().ghost_columns == 8
        got = _batch(flt, clip, frames, cc.PARITIES)
        for f in range(n):
            _assert_frames(want[f], got[f], f"{fmt} ghost 8 frame {f}")
        pi = flt.parts_info()
        assert pi.part_frames == n and pi.part_fallbacks == n, (pi.part_frames, pi.part_fallbacks)
        # the pause: the next launch does not try the parts again (a wide plane goes to the pool path)
        got = _batch(flt, clip, frames, cc.PARITIES)
        for f in range(n):
            _assert_frames(want[f], got[f], f"{fmt} paused frame {f}")
        i, pi = flt.info(), flt.parts_info()
        assert pi.part_frames == n and pi.part_fallbacks == n
        assert i.frames == 2 * n and i.fused_frames == (n if w > 3840 else 2 * n)


# ---- 4. natural fallback --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["Y16", "Y32"])
def test_only_the_fixed_point_frame_falls_back(hip_lib, fmt):
    patterns = ("noise", cc.FIXED_POINT, "noise")
    # 128 lines: the clamp's error travels three columns per row and has to reach the seam (at 32 lines it does not, and the
    # parts are exact: tests/test_column_parts_cpu.py runs this pattern at the same height)
    clip, frames, want = cc.expected(fmt, 3872, 128, {}, {}, patterns)
    with SangNom2(clip, max_batch=3, **ON) as flt:
        got = _batch(flt, clip, frames, cc.PARITIES)
        for f in range(3):
            _assert_frames(want[f], got[f], f"{fmt} {patterns[f]} frame {f}")
        pi = flt.parts_info()
        assert pi.part_frames == 3 and pi.part_fallbacks == 1, (pi.part_frames, pi.part_fallbacks)


# ---- 5. the SSE2 arithmetic -----------------------------------------------------------------------------------------------

def test_opt_1_with_sse2_sweeps(hip_lib):
    """noise01 saturates the SangNom value and the box: the SSE2 model's frames differ from the default arithmetic's
    (sc.expected asserts it), so parts that kept the wrapping arithmetic cannot pass."""
    fmt, w, h = cc.WIDE_Y16
    clip, frames, parities, want = sc.expected(fmt, w, h, {}, {}, 3, "noise01")
    with SangNom2(clip, max_batch=3, opt=1, sse2_sweeps=1, **ON) as flt:
        assert flt.info().fused_eligible == 1 and flt.parts_info().parts[0] >= 2
        got = _batch(flt, clip, frames, parities)
        for f in range(3):
            _assert_frames(want[f], got[f], f"opt=1 frame {f}")
        pi = flt.parts_info()
        assert flt.info().fused_frames == 3 and pi.part_frames == 3 and pi.part_fallbacks == 0, pi.part_fallbacks
    with pytest.raises(SangNomError, match="SN_ARITH_SSE2"):  # without the knob such a clip has no sweeps, parts or not
        SangNom2(clip, opt=1, **ON)


# ---- 6. special floats ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("parts", (2, 3))
def test_special_floats_in_forced_parts(hip_lib, parts):
    """Non-finite and huge samples (tests/float_cases.py): an infinite or NaN cost never decays, so a window may well fail the
    check -- the result is exact either way, wherever the reference writes at all."""
    clip = clip_format("Y32", 512, 64)
    for pattern, kw in (("nonfinite", {}), ("huge", dict(aa=128))):
        with SangNom2(clip, **ON, **kw) as flt:
            flt.debug_set_column_parts(parts, 0)
            for f, src in enumerate(fc.frames(clip, pattern)):
                got = flt.get_frame(src, parity=f & 1)
                if pattern == "nonfinite":
                    want, written = fc.written_by_reference(clip, src, parity=f & 1, **kw)
                    fc.assert_defined_samples_match(want[0], written[0], got[0], f"{parts} parts {pattern} frame {f}")
                else:
                    want = Oracle(oracle_cfg(clip, **kw)).process(src, parity=f & 1)
                    _assert_frames(want, got, f"{parts} parts {pattern} frame {f}")
            assert flt.info().frames == fc.NFRAMES


# ---- 7. the anti-aliasing call with dh ------------------------------------------------------------------------------------

def test_the_second_pass_of_the_enlargement_runs_in_parts(hip_lib):
    import torch
    fmt, w, h = cc.AA_DH
    clip = clip_format(fmt, w, h)
    frames = cc.frames_of(clip, TRIPLES[0])
    script = Script(clip)
    want = [script.frame(fr) for fr in frames]
    dev = torch.device("cuda:0")
    with SangNomAA(clip, max_batch=3, small_launches=capi.SN_SMALL_SWEEP, dh=True, column_parts=1) as aa:
        assert aa.info(1).fused_eligible == 1 and aa.parts_info(1).parts[0] >= 2 and aa.parts_info(0).parts[0] == 0
        src = cc.to_torch(frames, clip, dev)
        dst = [torch.zeros((3, 2 * h, 2 * w), dtype=src[0].dtype, device=dev)]
        torch.cuda.synchronize()
        aa.process_batch(src, dst)
        aa.synchronize()
        for f in range(3):
            _assert_frames(want[f], [to_host(dst[0][f]).view(clip.dtype)], f"enlargement frame {f}")
        pi = aa.parts_info(1)
        assert aa.info(1).fused_frames == 3 and pi.part_frames == 3 and pi.part_fallbacks == 0, (pi.part_frames, pi.part_fallbacks)


# ---- 8. the host ring -----------------------------------------------------------------------------------------------------

def test_the_host_ring(hip_lib):
    fmt, w, h = cc.WIDE_Y16
    clip, frames, want = cc.expected(fmt, w, h, {}, {}, ("noise", "edges"), parities=(1, 1))
    with SangNom2(clip, host_depth=2, **ON) as flt:
        slots = [flt.submit(fr) for fr in frames]
        got = [flt.collect(s) for s in slots]
        for f in range(2):
            _assert_frames(want[f], got[f], f"ring frame {f}")
        pi = flt.parts_info()
        assert flt.info().fused_frames == 2 and pi.part_frames == 2 and pi.part_fallbacks == 0, (pi.part_frames, pi.part_fallbacks)
    with SangNom2(clip, **ON) as flt:  # and the synchronous host call
        _assert_frames(want[0], flt.get_frame(frames[0]), "synchronous frame")
        assert flt.parts_info().part_frames == 1 and flt.parts_info().part_fallbacks == 0


# ---- 9. option off --------------------------------------------------------------------------------------------------------

def test_without_the_option_nothing_changes(hip_lib):
    fmt, w, h = cc.WIDE_Y16
    clip = clip_format(fmt, w, h)
    with SangNom2(clip, small_launches=capi.SN_SMALL_SWEEP) as flt:
        assert flt.info().fused_eligible == 0
        pi = flt.parts_info()
        assert (list(pi.parts), pi.ghost_columns, pi.part_frames, pi.part_fallbacks) == ([0, 0, 0], 0, 0, 0)
        flt.get_frame(synth.frame(clip, "noise", seed=1))
        assert flt.info().fused_frames == 0 and flt.parts_info().part_frames == 0
    with pytest.raises(SangNomError, match="not eligible"):
        SangNom2(clip, mode="fused")
    # 8-bit contexts accept the option; it has no effect there
    with SangNom2(clip_format("Y8", 256, 32), **ON) as flt:
        assert list(flt.parts_info().parts) == [0, 0, 0]
    # a wide 4:2:0 clip whose chroma shares the luma pool stays on the pool path and says so
    with SangNom2(clip_format("YUV420P16", 4096, 32), aac=48, column_parts=1) as flt:
        assert flt.info().fused_eligible == 0 and list(flt.parts_info().parts) == [0, 0, 0]
