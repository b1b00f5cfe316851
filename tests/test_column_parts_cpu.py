"""sn_options.column_parts without a GPU: the field took the place of a reserved word (same struct size, same ABI version),
a value other than 0 / 1 is refused before any device is touched, the new symbols exist -- and the convergence argument the
column parts rest on, checked with the numpy oracle on cropped windows: a window that clamps at an inner edge
is wrong only within a few dozen columns of it, the seam columns of two overlapping windows agree with the library's ghost
and differ when the seam lies 8 columns from a window's end, and agreement never comes with wrong own columns."""
import ctypes

import pytest

from avisynth_sangnom2_amd import capi, synth
from tests import column_parts_cases as cc


def _cfg(**kw):
    base = dict(struct_size=ctypes.sizeof(capi.SnConfig), width=64, height=32, bytes_per_sample=1, bits_per_sample=8,
                num_planes=1, sub_w=0, sub_h=0, order=1, aa=48, aac=0, dh=0, luma=1, chroma=1, device=0, max_batch=1, mode=0,
                host_depth=0, isolated_planes=0, fresh_pool=0, stream=None)
    base.update(kw)
    return capi.SnConfig(**base)


def test_the_option_took_a_reserved_word(hip_lib):
    assert ctypes.sizeof(capi.SnOptions) == 32
    assert capi.SnOptions.column_parts.offset == 8 and capi.SnOptions.reserved.offset == 12
    assert hip_lib.sn_abi_version() == 4
    assert ctypes.sizeof(capi.SnPartsInfo) == 40 and capi.SnPartsInfo.part_frames.offset == 24
    o = capi.options(capi.SN_ARITH_SSE2, column_parts=1)
    assert (o.struct_size, o.arithmetic, o.column_parts, list(o.reserved)) == (32, 1, 1, [0] * 5)
    assert capi.options().column_parts == 0


def test_the_new_symbols_exist(hip_lib):
    for name in ("sn_get_parts_info", "sn_aa_get_parts_info", "sn_debug_set_column_parts"):
        assert name in capi.EXPORTS and hasattr(hip_lib, name)
    header = open(capi.LIB_PATH.replace("avisynth_sangnom2_amd/libsangnom_hip.so", "include/sangnom_hip.h")).read()
    assert "int32_t column_parts;" in header and "int32_t reserved[5];" in header


def test_a_value_other_than_0_or_1_is_refused_with_the_field_named(hip_lib):
    h = ctypes.c_void_p()
    cfg = _cfg(width=4096, bytes_per_sample=2, bits_per_sample=16)
    for bad in (2, -1):
        o = capi.options(column_parts=bad)
        assert hip_lib.sn_create_ex(ctypes.byref(cfg), None, ctypes.byref(o), ctypes.byref(h)) == capi.SN_ERR_INVALID_ARG
        assert b"sn_options.column_parts" in hip_lib.sn_last_error(None)
        assert not h.value


# ---- the convergence check --------------------------------------------------------------------------------------------

_PATTERNS = cc.CONVERGING + (cc.FIXED_POINT,)
_W, _H = cc.CPU_SHAPE
_SEAM = _W // 2


@pytest.mark.parametrize("fmt", list(cc.FORMATS))
def test_windows_converge_within_the_ghost(fmt, record_property):
    """The default ghost: the two windows agree around the seam on every pattern the GPU tests feed, except on checker2 at
    8-bit, 16-bit and float -- the fixed point of the floor, where they must differ (the natural fallback).  Agreement implies
    exact own columns and an exact output.  The deepest wrong column of each pattern goes into the test report: the
    library's ghost is that of 540 pool rows plus 16, DESIGN.md 4.6."""
    bytes, bits = cc.FORMATS[fmt]
    ghost = cc.GHOST[bytes]
    for pattern in _PATTERNS:
        plane = synth.plane(_H, _W, bytes, bits, pattern, cc.SEED)
        r = cc.seam_check(plane, bytes, bits, _SEAM, ghost)
        record_property(f"deepest_wrong_column_{fmt}_{pattern}", r["deepest"])
        print(f"{fmt} {pattern}: deepest wrong column {r['deepest']}, seam agrees: {r['agree']}")
        fixed_point = pattern == cc.FIXED_POINT and fmt != "10-bit"
        assert r["agree"] == (not fixed_point), (fmt, pattern, r)
        if r["agree"]:
            assert r["own_exact"] and r["out_exact"], (fmt, pattern, r)
            assert r["deepest"] + 8 <= ghost, (fmt, pattern, r)  # the compared columns reach 8 beyond the seam
        else:
            assert r["deepest"] > ghost - 8, (fmt, pattern, r)


@pytest.mark.parametrize("fmt", list(cc.FORMATS))
def test_a_seam_8_columns_from_the_window_end_is_caught(fmt):
    """The forced case of the GPU tests (sn_debug_set_column_parts(parts, 8)): the left window's seam columns lie in what its
    clamp spoils, so the check must fail on every pattern -- and with it the left window's own columns are wrong."""
    bytes, bits = cc.FORMATS[fmt]
    for pattern in _PATTERNS:
        plane = synth.plane(_H, _W, bytes, bits, pattern, cc.SEED)
        r = cc.seam_check(plane, bytes, bits, _SEAM, cc.GHOST[bytes], seam_from_left_end=8)
        assert not r["agree"], (fmt, pattern, r)
        assert not r["own_exact"], (fmt, pattern, r)


def test_the_sse2_arithmetic_converges_on_its_gpu_input(record_property):
    """opt=1 with sse2_sweeps=1 runs the parts on noise01 (tests/sse2_sweep_cases.py: the input on which the two arithmetics
    differ most): the saturating box forgets as the wrapping one does."""
    from tests import sse2_sweep_cases as sc
    for seed in (sc.SEED, sc.SEED + 1, sc.SEED + 2):
        plane = synth.plane(_H, _W, 2, 16, "noise01", seed * 3)  # synth.frame's seed of plane 0
        r = cc.seam_check(plane, 2, 16, _SEAM, cc.GHOST[2], run=cc.sse2_pool)
        record_property(f"deepest_wrong_column_sse2_noise01_{seed}", r["deepest"])
        assert r["agree"] and r["own_exact"] and r["out_exact"] and r["deepest"] + 8 <= cc.GHOST[2], r
        assert not cc.seam_check(plane, 2, 16, _SEAM, cc.GHOST[2], seam_from_left_end=8, run=cc.sse2_pool)["agree"]
