"""The edge mask of the anti-aliasing call, the parts that need no GPU: the ABI of sn_aa_mask and the three new symbols,
the refusals made before a device is touched, the numpy model (tests/mask_model.py) pinned by answers derived by hand, and
the condition that keeps the GPU tests from passing trivially: every plane of every frame they use holds all three classes
of the mask, and the expected frame differs from both the source and the unmasked result."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from avisynth_sangnom2_amd import capi
from tests import mask_cases as mc
from tests.mask_model import edge_mask, mask_plane, merge_plane, sobel_e

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(**kw):
    base = dict(struct_size=ctypes.sizeof(capi.SnConfig), width=64, height=32, bytes_per_sample=1, bits_per_sample=8, num_planes=1, sub_w=0,
                sub_h=0, order=1, aa=48, aac=0, dh=0, luma=1, chroma=1, device=0, max_batch=1, mode=0, host_depth=0, isolated_planes=0,
                fresh_pool=0, stream=None)
    base.update(kw)
    return capi.SnConfig(**base)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------

def test_sn_aa_mask_as_a_c_compiler_lays_it_out(tmp_path):
    src = tmp_path / "layout.c"
    fields = ("struct_size", "kind", "lo", "hi", "expand", "reserved")
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sangnom_hip.h"\n'
                   'int main(void) { printf("%d ' + "%d " * len(fields) + '%d %d\\n", (int)sizeof(sn_aa_mask), '
                   + ", ".join(f"(int)offsetof(sn_aa_mask, {f})" for f in fields) + ", SN_AA_MASK_NONE, SN_AA_MASK_SOBEL); return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    assert [int(x) for x in out] == [32, 0, 4, 8, 12, 16, 20, 0, 1]
    M = capi.SnAAMask
    assert ctypes.sizeof(M) == 32
    assert [getattr(M, f).offset for f in fields] == [0, 4, 8, 12, 16, 20]
    assert (capi.SN_AA_MASK_NONE, capi.SN_AA_MASK_SOBEL) == (0, 1)


def test_the_three_symbols_are_declared_exported_and_mirrored(hip_lib):
    header = open(os.path.join(ROOT, "include", "sangnom_hip.h")).read()
    for name in ("sn_aa_create_ex3", "sn_aa_get_mask", "sn_mask_merge_device"):
        assert re.search(r"\bint " + name + r"\(", header), f"{name} is not declared"
        assert hasattr(hip_lib, name), f"libsangnom_hip.so does not export {name}"
        assert name in capi.EXPORTS + capi.EXPORTS_NUMBERED and getattr(hip_lib, name).argtypes, f"capi.py does not mirror {name}"
    assert hip_lib.sn_abi_version() == 4
    assert re.search(r"#define SN_ABI_VERSION 4\b", header)
    assert "launch_mask_merge" in open(os.path.join(ROOT, "avisynth_sangnom2_amd", "csrc", "sn_internal.h")).read()
    assert "sn_mask.hip" in open(os.path.join(ROOT, "avisynth_sangnom2_amd", "csrc", "Makefile")).read()


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def _create(hip_lib, cfg, mask, aopt=None):
    h = ctypes.c_void_p()
    rc = hip_lib.sn_aa_create_ex3(ctypes.byref(cfg), None, None, ctypes.byref(aopt) if aopt is not None else None,
                                  ctypes.byref(mask) if mask is not None else None, ctypes.byref(h))
    assert not h.value
    return rc, hip_lib.sn_aa_last_error(None).decode()


def _mask(**kw):
    base = dict(struct_size=ctypes.sizeof(capi.SnAAMask), kind=capi.SN_AA_MASK_SOBEL, lo=16, hi=96, expand=1)
    base.update(kw)
    return capi.SnAAMask(**base)


@pytest.mark.parametrize("kw,field", [(dict(struct_size=28), "struct_size"), (dict(struct_size=0), "struct_size"), (dict(kind=2), "kind"),
                                      (dict(kind=-1), "kind"), (dict(lo=-1), "lo"), (dict(lo=256, hi=256), "lo"), (dict(hi=256), "hi"),
                                      (dict(hi=-1, lo=0), "hi"), (dict(lo=97), "lo"), (dict(expand=2), "expand"), (dict(expand=-1), "expand")])
def test_bad_masks_are_refused_naming_the_field(hip_lib, kw, field):
    rc, msg = _create(hip_lib, _cfg(), _mask(**kw))
    assert rc == capi.SN_ERR_INVALID_ARG and "sn_aa_mask." + field in msg, msg


def test_reserved_words_and_the_source_size_rule(hip_lib):
    for word in range(3):
        m = _mask()
        m.reserved[word] = 1
        rc, msg = _create(hip_lib, _cfg(), m)
        assert rc == capi.SN_ERR_INVALID_ARG and "sn_aa_mask.reserved" in msg
    rc, msg = _create(hip_lib, _cfg(dh=1), _mask())
    assert rc == capi.SN_ERR_CONFIG
    assert msg == "SangNomAA: mask needs the frame at source size (dh=false, or dh=true with reduce)"
    # kind 0: the other fields are ignored -- the call gets as far as the device (or succeeds where there is one)
    h = ctypes.c_void_p()
    none = _mask(kind=capi.SN_AA_MASK_NONE, lo=999, hi=-5, expand=7)
    none.reserved[1] = 3
    rc = hip_lib.sn_aa_create_ex3(ctypes.byref(_cfg(dh=1)), None, None, None, ctypes.byref(none), ctypes.byref(h))
    assert rc in (capi.SN_OK, capi.SN_ERR_HIP, capi.SN_ERR_NO_DEVICE), hip_lib.sn_aa_last_error(None).decode()
    if h.value:
        hip_lib.sn_aa_destroy(h)
    assert hip_lib.sn_aa_get_mask(None, ctypes.byref(_mask())) == capi.SN_ERR_INVALID_ARG
    assert hip_lib.sn_mask_merge_device(None, ctypes.byref(_mask()), 1, None, 0, 0, None, 0, 0, 1, 1, None, 0, 0) == capi.SN_ERR_INVALID_ARG


# ---- the model, pinned by hand ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,bits,value", [(np.uint8, 8, 255), (np.uint8, 8, 77), (np.uint16, 10, 1023), (np.uint16, 16, 65535), (np.float32, 32, 0.3)])
def test_a_constant_plane_has_an_empty_mask(dtype, bits, value):
    S = np.full((9, 14), value, dtype)
    R = np.zeros((9, 14), dtype)
    for expand in (0, 1):
        assert not edge_mask(S, 0, 0, expand, bits).any()
        assert np.array_equal(merge_plane(S, R, 0, 0, expand, bits), S)
        assert not mask_plane(S, 0, 0, expand, bits).any()


@pytest.mark.parametrize("dtype,bits,a,d", [(np.uint8, 8, 100, 40), (np.uint8, 8, 0, 255), (np.uint16, 10, 400, 160), (np.uint16, 16, 0, 65535),
                                            (np.float32, 32, 0.25, 0.25)])
def test_a_step_of_height_d_gives_e_equal_d_beside_it(dtype, bits, a, d):
    """Columns 0..5 hold a, columns 6.. hold a + d: gx = 4 (a + d) - 4 a in columns 5 and 6 and nothing else anywhere, so
    e = d there and 0 elsewhere; the transposed plane gives the same through gy."""
    S = np.full((10, 13), a, dtype)
    S[:, 6:] = a + d
    want = np.zeros((10, 13), S.dtype if dtype == np.float32 else np.int64)
    want[:, 5:7] = d
    assert np.array_equal(sobel_e(S, bits), want)
    assert np.array_equal(sobel_e(np.ascontiguousarray(S.T), bits), want.T)


def test_equal_thresholds_give_a_binary_mask_and_expansion_widens_one_column_to_three():
    """Rows of 0 0 0 30 40 40 40: e = S(x + 1) - S(x - 1) = 0 0 30 40 10 0 0.  lo = hi = 35: only column 3 is above."""
    S = np.tile(np.array([0, 0, 0, 30, 40, 40, 40], np.uint8), (6, 1))
    assert np.array_equal(sobel_e(S)[2], [0, 0, 30, 40, 10, 0, 0])
    m = edge_mask(S, 35, 35, 0)
    assert np.array_equal(m, np.tile([0, 0, 0, 256, 0, 0, 0], (6, 1)))
    assert np.array_equal(edge_mask(S, 35, 35, 1), np.tile([0, 0, 256, 256, 256, 0, 0], (6, 1)))
    m = edge_mask(S, 10, 10, 0)  # e = 10 is not above lo
    assert np.array_equal(m[0], [0, 0, 256, 256, 0, 0, 0])
    # a corner sample of 200, where the clamp repeats it: at (0, 0) col(-1) = row(-1) = 200 + 400 + 0, e = 1200 >> 2 = 300; at (0, 1)
    # gx = 600 and gy = 200 (the repeated row above), e = 200; at (1, 1) gx = gy = 200, e = 100; two samples away nothing
    S = np.zeros((7, 7), np.uint8)
    S[0, 0] = 200
    assert np.array_equal(sobel_e(S)[:3, :3], [[300, 200, 0], [200, 100, 0], [0, 0, 0]])
    want = np.zeros((7, 7), np.int64)
    want[:2, :2] = 256
    assert np.array_equal(edge_mask(S, 99, 99, 0), want)
    want[:3, :3] = 256  # the maximum over clamped coordinates adds nothing outside the plane's own 3 x 3
    assert np.array_equal(edge_mask(S, 99, 99, 1), want)


def test_mask_0_gives_the_source_and_mask_256_the_result():
    rng = np.random.default_rng(5)
    for dtype, bits in ((np.uint8, 8), (np.uint16, 10), (np.uint16, 16), (np.float32, 32)):
        mx = 1.0 if dtype == np.float32 else (1 << bits) - 1
        S = np.zeros((8, 12), dtype)
        S[:, 6:] = mx
        R = (rng.random((8, 12)) * mx).astype(dtype)
        out = merge_plane(S, R, 20, 20, 0, bits)
        m = edge_mask(S, 20, 20, 0, bits)
        assert set(np.unique(m)) == {0, 256}
        assert np.array_equal(out[m == 0], S[m == 0]) and np.array_equal(out[m == 256], R[m == 256])
        assert np.array_equal(mask_plane(S, 20, 20, 0, bits)[m == 256], np.full(int((m == 256).sum()), mx, dtype))


def test_one_ramp_value_by_hand():
    """lo 16, hi 96 and a step of 40 (8-bit), 160 (10-bit), 0.25 (float):
    8-bit:  m = (40 - 16) * 256 / 80 = 76.8 -> 76;  S 100, R 200: (100 * 180 + 200 * 76 + 128) >> 8 = 33328 >> 8 = 130
    10-bit: m = (160 - 64) * 256 / 320 = 76.8 -> 76;  S 400, R 800: (400 * 180 + 800 * 76 + 128) >> 8 = 132928 >> 8 = 519
    float:  m = int((0.25 - 16 / 255) * 256 / (80 / 255)) = int(152.8) = 152;  S 0.25, R 0.75: 0.25 + 0.5 * (152 / 256) = 0.546875
    and the mask plane: (76 * 255 + 128) >> 8 = 76, (76 * 1023 + 128) >> 8 = 304, 152 / 256 = 0.59375."""
    for dtype, bits, a, d, r, m_want, out_want, mask_want in ((np.uint8, 8, 100, 40, 200, 76, 130, 76), (np.uint16, 10, 400, 160, 800, 76, 519, 304),
                                                              (np.float32, 32, 0.25, 0.25, 0.75, 152, 0.546875, 0.59375)):
        S = np.full((6, 12), a, dtype)
        S[:, 6:] = a + d
        R = np.full((6, 12), r, dtype)
        assert edge_mask(S, 16, 96, 0, bits)[3, 5] == m_want
        assert merge_plane(S, R, 16, 96, 0, bits)[3, 5] == dtype(out_want)
        assert mask_plane(S, 16, 96, 0, bits)[3, 5] == dtype(mask_want)
        assert merge_plane(S, R, 16, 96, 0, bits)[3, 2] == dtype(a)


def test_a_nan_keeps_the_source_and_an_infinity_takes_the_result():
    S = np.full((7, 9), 0.5, np.float32)
    S[3, 2] = np.nan
    S[3, 6] = np.inf
    m = edge_mask(S, 16, 96, 0)
    assert not m[2:5, 1:4].any()          # e is NaN around the NaN, and 0 at it
    assert m[3, 6] == 0 and m[2:5, 5:8].sum() == 8 * 256


# ---- the frames of the GPU tests -------------------------------------------------------------------------------------------------

def _classes(m):
    n = m.size
    return (m == 0).sum() / n, ((m > 0) & (m < 256)).sum() / n, (m == 256).sum() / n


ALL_CASES = mc.BATCH + [mc.LUMA_OFF, mc.CHUNK, mc.P010] + [(c[0], c[1], c[2], c[3], {}, {}, None) for c in mc.HOST]


@pytest.mark.parametrize("i", range(len(ALL_CASES)), ids=[f"{c[0]}-{c[1]}x{c[2]}-{i}" for i, c in enumerate(ALL_CASES)])
def test_every_plane_of_the_gpu_tests_frames_holds_all_three_classes(i):
    from avisynth_sangnom2_amd import clip_format
    case = ALL_CASES[i]
    bits = clip_format(case[0], case[1], case[2]).bits
    for f, fr in enumerate(mc.frames_of(case[0], case[1], case[2])):
        for p, S in enumerate(fr):
            for expand in mc.EXPANDS:
                c = _classes(edge_mask(S, mc.LO, mc.HI, expand, bits))
                print(f"{case[0]} {case[1]}x{case[2]} frame {f} plane {p} expand {expand}: " + " / ".join(f"{x:.2f}" for x in c))
                assert min(c) >= 0.05, f"frame {f} plane {p} expand {expand}: classes {c}"


@pytest.mark.parametrize("i", [0, 4, 6, 7], ids=lambda i: f"{mc.BATCH[i][0]}-{i}")
def test_the_expected_frames_differ_from_the_source_and_from_the_unmasked_result(i):
    """On the first two frames of a case of every sample type, for both forms of the call (the GPU tests assert the same of
    every frame they compare)."""
    case = mc.BATCH[i]
    for form in (None, "halfband"):
        for expand in mc.EXPANDS:
            frames, _, res, want = mc.expected(case, form, expand, count=2)
            for f in range(2):
                for p in range(len(frames[f])):
                    assert not np.array_equal(want[f][p], frames[f][p]), f"form {form} frame {f} plane {p}: the expected plane is the source"
                    assert not np.array_equal(want[f][p], res[f][p]), f"form {form} frame {f} plane {p}: the expected plane is the unmasked result"
