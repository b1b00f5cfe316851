"""The contra-sharpening of the anti-aliasing call, the parts that need no GPU: the ABI of sn_aa_sharpen and the three new
symbols, the refusals made before a device is touched, the numpy model (tests/sharpen_model.py) pinned by answers derived
by hand, and the condition that keeps the GPU tests from passing trivially: in every plane of the frames they use the stage
changes at least half of the samples and its limit acts on at least 1 % of them."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from avisynth_sangnom2_amd import capi, clip_format
from tests import sharpen_cases as sc
from tests.sharpen_model import sharpen_model, sharpen_plane, sharpen_terms
from tests.util import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sn_aa_create_ex5", "sn_aa_get_sharpen", "sn_contra_sharpen_device")


def _cfg(**kw):
    base = dict(struct_size=ctypes.sizeof(capi.SnConfig), width=64, height=32, bytes_per_sample=1, bits_per_sample=8, num_planes=1, sub_w=0,
                sub_h=0, order=1, aa=48, aac=0, dh=0, luma=1, chroma=1, device=0, max_batch=1, mode=0, host_depth=0, isolated_planes=0,
                fresh_pool=0, stream=None)
    base.update(kw)
    return capi.SnConfig(**base)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------

def test_sn_aa_sharpen_as_a_c_compiler_lays_it_out(tmp_path):
    src = tmp_path / "layout.c"
    fields = ("struct_size", "amount", "chroma", "reserved")
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sangnom_hip.h"\n'
                   'int main(void) { printf("%d ' + "%d " * len(fields) + '\\n", (int)sizeof(sn_aa_sharpen), '
                   + ", ".join(f"(int)offsetof(sn_aa_sharpen, {f})" for f in fields) + "); return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    assert [int(x) for x in out] == [32, 0, 4, 8, 12]
    M = capi.SnAASharpen
    assert ctypes.sizeof(M) == 32
    assert [getattr(M, f).offset for f in fields] == [0, 4, 8, 12]
    s = capi.aa_sharpen(64, True)
    assert (s.struct_size, s.amount, s.chroma, list(s.reserved)) == (32, 64, 1, [0] * 5)
    assert (capi.aa_sharpen().amount, capi.aa_sharpen(None, True).amount) == (0, 0)


def test_the_three_symbols_are_declared_exported_and_mirrored(hip_lib):
    header = open(os.path.join(ROOT, "include", "sangnom_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), f"{name} is not declared"
        assert hasattr(hip_lib, name), f"libsangnom_hip.so does not export {name}"
        assert name in capi.EXPORTS + capi.EXPORTS_NUMBERED and getattr(hip_lib, name).argtypes, f"capi.py does not mirror {name}"
    assert hip_lib.sn_abi_version() == 4
    assert re.search(r"#define SN_ABI_VERSION 4\b", header)
    assert "launch_contra_sharpen" in open(os.path.join(ROOT, "avisynth_sangnom2_amd", "csrc", "sn_internal.h")).read()
    assert "sn_sharpen.hip" in open(os.path.join(ROOT, "avisynth_sangnom2_amd", "csrc", "Makefile")).read()


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def _create(hip_lib, cfg, sharpen, aopt=None):
    h = ctypes.c_void_p()
    rc = hip_lib.sn_aa_create_ex5(ctypes.byref(cfg), None, None, ctypes.byref(aopt) if aopt is not None else None, None, None,
                                  ctypes.byref(sharpen) if sharpen is not None else None, ctypes.byref(h))
    assert not h.value
    return rc, hip_lib.sn_aa_last_error(None).decode()


def _sharpen(**kw):
    base = dict(struct_size=ctypes.sizeof(capi.SnAASharpen), amount=64, chroma=0)
    base.update(kw)
    return capi.SnAASharpen(**base)


@pytest.mark.parametrize("kw,field", [(dict(struct_size=28), "struct_size"), (dict(struct_size=0), "struct_size"), (dict(struct_size=28, amount=0), "struct_size"),
                                      (dict(amount=-1), "amount"), (dict(amount=256), "amount"), (dict(chroma=2), "chroma"), (dict(chroma=-1), "chroma")])
def test_a_bad_struct_is_refused_naming_the_field(hip_lib, kw, field):
    rc, msg = _create(hip_lib, _cfg(), _sharpen(**kw))
    assert rc == capi.SN_ERR_INVALID_ARG and "sn_aa_sharpen." + field in msg, msg


def test_reserved_words_and_the_source_size_rule(hip_lib):
    for word in range(5):
        s = _sharpen()
        s.reserved[word] = 1
        rc, msg = _create(hip_lib, _cfg(), s)
        assert rc == capi.SN_ERR_INVALID_ARG and "sn_aa_sharpen.reserved" in msg
    for chroma in (0, 1):
        rc, msg = _create(hip_lib, _cfg(dh=1), _sharpen(chroma=chroma))
        assert rc == capi.SN_ERR_CONFIG
        assert msg == "SangNomAA: sharpen needs the frame at source size (dh=false, or dh=true with reduce)"
    # amount 0: the other fields are ignored -- the call gets as far as the device (or succeeds where there is one)
    h = ctypes.c_void_p()
    off = _sharpen(amount=0, chroma=7)
    off.reserved[3] = 9
    rc = hip_lib.sn_aa_create_ex5(ctypes.byref(_cfg(dh=1)), None, None, None, None, None, ctypes.byref(off), ctypes.byref(h))
    assert rc in (capi.SN_OK, capi.SN_ERR_HIP, capi.SN_ERR_NO_DEVICE), hip_lib.sn_aa_last_error(None).decode()
    if h.value:
        hip_lib.sn_aa_destroy(h)
    assert hip_lib.sn_aa_get_sharpen(None, ctypes.byref(_sharpen())) == capi.SN_ERR_INVALID_ARG
    assert hip_lib.sn_contra_sharpen_device(None, 64, 1, None, 0, 0, None, 0, 0, 1, 1, None, 0, 0) == capi.SN_ERR_INVALID_ARG


# ---- the model, pinned by hand ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,bits,value", [(np.uint8, 8, 255), (np.uint8, 8, 77), (np.uint16, 10, 1023), (np.uint16, 16, 65535), (np.float32, 32, 0.3)])
def test_a_constant_result_comes_back_unchanged(dtype, bits, value):
    """R constant: h = 4 R, B = (16 R + 8) >> 4 = R, d = 0 -- whatever the source holds."""
    rng = np.random.default_rng(1)
    R = np.full((9, 14), value, dtype)
    S = (rng.random((9, 14)) * (1.0 if dtype == np.float32 else (1 << bits) - 1)).astype(dtype)
    for amount in (1, 64, 255):
        assert same(sharpen_plane(S, R, amount, bits), R)


def test_where_the_filter_changed_nothing_the_result_comes_back_unchanged():
    """S == R: every S - R is 0, so mn = mx = 0 and c = 0, for any content."""
    rng = np.random.default_rng(2)
    for dtype, bits in ((np.uint8, 8), (np.uint16, 10), (np.uint16, 16), (np.float32, 32)):
        R = (rng.random((11, 17)) * (1.0 if dtype == np.float32 else (1 << bits) - 1)).astype(dtype)
        for amount in (1, 64, 255):
            assert same(sharpen_plane(R.copy(), R, amount, bits), R)
            d1 = sharpen_terms(R, R, amount, bits)[0]
            assert amount == 1 or (d1 != 0).mean() > 0.5  # ... and not because there was nothing to add (at amount 1, |d| < 64 adds nothing)


# Every row the same, so the vertical [1 2 1] gives 4 h and B = (4 h + 8) >> 4 = (h + 2) >> 2.
#   column      0   1   2   3   4   5    6    7    8 ...
#   R          40  40  40  40  40  80  160  200  200        a softened step
#   h         160 160 160 160 200 360  600  760  800
#   B          40  40  40  40  50  90  150  190  200
#   d           0   0   0   0 -10 -10  +10  +10    0
#   D = S - R   0   0   0  +3   0  +6  -12   +4    0        (S = 40 40 40 43 40 86 148 204 200)
#   mn          0   0   0   0   0 -12  -12  -12    0        over columns x - 1 .. x + 1, with 0
#   mx          0   0  +3  +3  +6  +6   +6   +4   +4
# amount 64 (d1 = d):   column 4: d1 = -10 but every nearby S - R is >= 0: cut to 0;  column 5: -10 >= mn: the full d1;
#                       column 6: +10 cut to mx = 6;  column 7: +10 cut to mx = 4
# amount 255 (d1 = sgn(d) (2550 >> 6) = +-39):  column 5 cut to mn = -12, columns 6 and 7 as before, column 4 still 0
# amount 1 (d1 = 10 >> 6 = 0): nothing
STEP_R = [40, 40, 40, 40, 40, 80, 160, 200, 200, 200, 200, 200]
STEP_S = [40, 40, 40, 43, 40, 86, 148, 204, 200, 200, 200, 200]
STEP_OUT = {64: [40, 40, 40, 40, 40, 70, 166, 204, 200, 200, 200, 200], 255: [40, 40, 40, 40, 40, 68, 166, 204, 200, 200, 200, 200], 1: STEP_R}


@pytest.mark.parametrize("amount", [64, 255, 1])
@pytest.mark.parametrize("dtype,scale", [(np.uint8, 1), (np.uint16, 1), (np.float32, 1 / 256)])
def test_a_step_by_hand(dtype, scale, amount):
    """... as rows and, transposed, as columns; as 8-bit and 16-bit samples, and as float samples x / 256: every value of the
    table is then exact in single precision, and as every h of it is a multiple of 4 the float B = v / 16 is the integer one.
    Only d1 differs, which is not truncated for float samples: +-10 * 255 / 64 = +-39.84375 meets the same limits, and +-10 / 64 =
    +-0.15625 is added in full where the limit has its sign (columns 5, 6 and 7) and cut to 0 in column 4."""
    R = np.tile((np.array(STEP_R) * scale).astype(dtype), (5, 1))
    S = np.tile((np.array(STEP_S) * scale).astype(dtype), (5, 1))
    row = STEP_OUT[amount]
    if dtype == np.float32 and amount == 1:
        row = [40, 40, 40, 40, 40, 80 - 0.15625, 160 + 0.15625, 200 + 0.15625, 200, 200, 200, 200]
    want = np.tile((np.array(row) * scale).astype(dtype), (5, 1))
    bits = 8 if dtype == np.uint8 else 16
    got = sharpen_plane(S, R, amount, bits)
    assert same(got, want), (got[2], want[2])
    got_t = sharpen_plane(np.ascontiguousarray(S.T), np.ascontiguousarray(R.T), amount, bits)
    assert same(got_t, np.ascontiguousarray(want.T))
    if dtype != np.float32:
        d1, mn, mx, c = sharpen_terms(S, R, amount, bits)
        k = {64: 10, 255: 39, 1: 0}[amount]
        assert list(d1[2]) == [0, 0, 0, 0, -k, -k, k, k, 0, 0, 0, 0]
        assert list(mn[2]) == [0, 0, 0, 0, 0, -12, -12, -12, 0, 0, 0, 0] and list(mx[2]) == [0, 0, 3, 3, 6, 6, 6, 4, 4, 0, 0, 0]


def test_the_clamp_to_the_clip_at_10_bit():
    """amount 255, rows the same.
    upper: R = 1000 1000 1000 1020 1000 ..., S = 1000 1000 1023 1020 1023 ...: at column 3 h = 4040, B = 4042 >> 2 = 1010, d = 10,
           d1 = 2550 >> 6 = 39, mx = 23: c = 23 and 1043 is clamped to 1023; at column 2 d = 1000 - (4022 >> 2) = -5, mn = 0: c = 0.
    lower: R = 20 20 20 2 20 ..., S = 20 20 0 2 0 ...: at column 3 h = 44, B = 46 >> 2 = 11, d = -9, d1 = -(2295 >> 6) = -35,
           mn = -20: c = -20 and -18 is clamped to 0; at column 2 d = 20 - (64 >> 2) = 4, mx = 0: c = 0."""
    R = np.tile(np.array([1000, 1000, 1000, 1020, 1000, 1000, 1000], np.uint16), (4, 1))
    S = np.tile(np.array([1000, 1000, 1023, 1020, 1023, 1000, 1000], np.uint16), (4, 1))
    assert list(sharpen_plane(S, R, 255, 10)[1]) == [1000, 1000, 1000, 1023, 1000, 1000, 1000]
    assert list(sharpen_plane(S, R, 255, 16)[1]) == [1000, 1000, 1000, 1043, 1000, 1000, 1000]
    R = np.tile(np.array([20, 20, 20, 2, 20, 20, 20], np.uint16), (4, 1))
    S = np.tile(np.array([20, 20, 0, 2, 0, 20, 20], np.uint16), (4, 1))
    assert list(sharpen_plane(S, R, 255, 10)[1]) == [20, 20, 20, 0, 20, 20, 20]
    # R itself above the clip's range (a wider container, without reduce): clamped too
    R = np.full((4, 6), 1500, np.uint16)
    assert np.all(sharpen_plane(R, R, 64, 10) == 1023)


def special_planes():
    """(S, R, expected) of 8 x 16 float samples, amount 64 (k = 1): R is 0.5 and S equals R except where listed below; the
    listed places are three or more samples apart, so their 3 x 3 neighbourhoods do not meet.  Where R is 0.5 all around,
    h = 2, v = 8, B = 0.5, d = +0, c = 0: a copy.
      (1, 1)  R = NaN (payload 0x1234), S = 0.5: d1 is NaN at it and around it: copies, the NaN with its payload.
      (1, 5)  R = +inf, S = +inf: at it d = inf - inf = NaN: a copy.  Around it B = +inf, d1 = -inf, the only S - R that is not
              0 is NaN (ignored), so mn = 0 and c = 0: copies.
      (1, 9)  R = -inf, S = 0.5: a copy at it.  Around it B = -inf, d1 = +inf, mx = S - R = +inf: c = +inf, out = +inf.
      (1, 13) R = -0.0, S = -1.0: h = (0.5 + 0.5) + (-0.0 + -0.0) = 1, v = (2 + 2) + (1 + 1) = 6, B = 0.375, d1 = -0.375, mn = -1:
              out = -0.0 + -0.375 = -0.375.  Around it d1 > 0 and mx = 0: copies.
      (5, 2)  R = 1.0, S = +inf: h = (0.5 + 0.5) + (1 + 1) = 3, v = (2 + 2) + (3 + 3) = 10, B = 0.625, d1 = 0.375, mx = +inf: out = 1.375.
              Around it d1 < 0 and mn = 0: copies.
      (5, 6)  R = 1.0, S = -inf: d1 = 0.375, mx = 0: a copy.  Around it mn = -inf, so the full d1: beside it h = (0.5 + 1) + 1 = 2.5,
              v = (2 + 2) + (2.5 + 2.5) = 9, B = 0.5625, out = 0.5 - 0.0625 = 0.4375, above and below it v = (2 + 3) + (2 + 2) = 9 as well;
              diagonally v = (2.5 + 2) + (2 + 2) = 8.5, B = 0.53125, out = 0.46875.
      (5, 10) R = 1.0, S = NaN, and S(5, 11) = 0.75: at (5, 10) the NaN is ignored, mx = 0.25, d1 = 0.375: out = 1.25.  Around it
              d1 < 0 and mn = 0: copies.
      (5, 14) S = -0.0: d1 = +0 there and around it: copies."""
    R = np.full((8, 16), 0.5, np.float32)
    R.view(np.uint32)[1, 1] = 0x7FC01234
    R[1, 5], R[1, 9], R[1, 13] = np.inf, -np.inf, -0.0
    R[5, 2] = R[5, 6] = R[5, 10] = 1.0
    S = R.copy()
    S[1, 1], S[1, 9], S[1, 13] = 0.5, 0.5, -1.0
    S[5, 2], S[5, 6], S[5, 10], S[5, 11], S[5, 14] = np.inf, -np.inf, np.nan, 0.75, -0.0
    want = R.copy()
    want[0:3, 8:11] = np.inf
    want[1, 9] = -np.inf
    want[1, 13] = -0.375
    want[5, 2] = 1.375
    want[4:7, 5:8] = 0.46875
    want[4, 6] = want[6, 6] = want[5, 5] = want[5, 7] = 0.4375
    want[5, 6] = 1.0
    want[5, 10] = 1.25
    return S, R, want


def test_nan_infinities_and_negative_zero_by_hand():
    S, R, want = special_planes()
    got = sharpen_plane(S, R, 64, 32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert got.view(np.uint32)[1, 1] == 0x7FC01234 and np.isnan(got).sum() == 1  # the one NaN of R, copied; none generated
    assert np.signbit(got[1, 13]) and got.view(np.uint32)[5, 14] == R.view(np.uint32)[5, 14]
    # ... and with the planes exchanged no NaN is generated either: every NaN of the output is one of R's, bit for bit
    got = sharpen_plane(R, S, 64, 32)
    nan = np.isnan(got)
    assert np.array_equal(nan, np.isnan(S)) and np.array_equal(got.view(np.uint32)[nan], S.view(np.uint32)[nan])


def test_chroma_and_processed_select_the_planes():
    rng = np.random.default_rng(3)
    S = [rng.integers(0, 256, (8, 12)).astype(np.uint8) for _ in range(3)]
    R = [rng.integers(0, 256, (8, 12)).astype(np.uint8) for _ in range(3)]
    sharp = [sharpen_plane(s, r, 64, 8) for s, r in zip(S, R)]
    assert all(not same(a, b) for a, b in zip(sharp, R))
    out = sharpen_model(S, R, 64, False, 8)
    assert same(out[0], sharp[0]) and out[1] is R[1] and out[2] is R[2]
    out = sharpen_model(S, R, 64, True, 8, [False, True, True])
    assert out[0] is R[0] and same(out[1], sharp[1]) and same(out[2], sharp[2])


# ---- the frames of the GPU tests -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(sc.BATCH)), ids=[f"{c[0]}-{c[1]}x{c[2]}-{i}" for i, c in enumerate(sc.BATCH)])
def test_the_stage_changes_the_frames_of_the_gpu_tests_and_its_limit_acts(i):
    """Frame 0 of every row, without dh and with dh and the half-band reduction, every plane, amount 64: at least half of the
    samples differ from R, and at least 1 % are limited (c is neither d1 nor 0).  In the first row without dh the class "cut to
    0" (c == 0 although d1 != 0) is not empty."""
    case = sc.BATCH[i]
    bits = clip_format(case[0], case[1], case[2]).bits
    for form in (None, "halfband"):
        frames, _, res = sc.unmasked(case, form, count=1)
        for p, (S, R) in enumerate(zip(frames[0], res[0])):
            d1, mn, mx, c = sharpen_terms(S, R, sc.AMOUNT, bits)
            out = sharpen_plane(S, R, sc.AMOUNT, bits)
            changed = (out != R).mean()
            limited = ((c != d1) & (c != 0)).mean()
            cut0 = ((c == 0) & (d1 != 0)).mean()
            print(f"{case[0]} {case[1]}x{case[2]} form {form} plane {p}: changed {changed:.3f} limited {limited:.3f} cut to 0 {cut0:.3f}")
            assert changed >= 0.5 and limited >= 0.01, f"form {form} plane {p}: changed {changed:.3f}, limited {limited:.3f}"
            if i == 0 and form is None:
                assert cut0 > 0


@pytest.mark.parametrize("i", [0, 4, 7], ids=lambda i: f"{sc.BATCH[i][0]}-{i}")
def test_the_expected_frames_differ_from_the_unsharpened_ones(i):
    case = sc.BATCH[i]
    for form in (None, "halfband"):
        for mask in (None, sc.MASK):
            frames, _, plain, want = sc.expected(case, form, sc.AMOUNT, True, mask, count=2)
            for f in range(2):
                for p in range(len(frames[f])):
                    assert not same(want[f][p], plain[f][p]), f"form {form} mask {mask} frame {f} plane {p}: the expected plane is the unsharpened one"
            if len(frames[0]) == 3:  # chroma = 0: planes 1 and 2 are the unsharpened expectation
                _, _, plain0, want0 = sc.expected(case, form, sc.AMOUNT, False, mask, count=2)
                assert same(want0[0][0], want[0][0]) and same(want0[0][1], plain0[0][1]) and same(want0[0][2], plain0[0][2])
