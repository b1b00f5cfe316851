"""Chroma merged through the luma plane's mask, the parts that need no GPU: the ABI of sn_aa_mask_ex and the three new
symbols, the refusals made before a device is touched, the numpy model (tests/mask_luma_model.py) pinned by answers derived
by hand, and the condition that keeps the GPU tests from passing trivially: the reduced mask mc of every frame they use
holds at least 5 % of each class, and the expected frame differs from the source, from the unmasked result and from what
every plane's own mask gives."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNomAAHost, SangNomError, capi, clip_format
from tests import mask_luma_cases as lc
from tests.mask_luma_model import chroma_mask, mask_plane_luma, merge_plane_luma, reduce_mask
from tests.mask_model import edge_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(**kw):
    base = dict(struct_size=ctypes.sizeof(capi.SnConfig), width=64, height=32, bytes_per_sample=1, bits_per_sample=8, num_planes=3, sub_w=1,
                sub_h=1, order=1, aa=48, aac=0, dh=0, luma=1, chroma=1, device=0, max_batch=1, mode=0, host_depth=0, isolated_planes=0,
                fresh_pool=0, stream=None)
    base.update(kw)
    return capi.SnConfig(**base)


def _mask(**kw):
    base = dict(struct_size=ctypes.sizeof(capi.SnAAMask), kind=capi.SN_AA_MASK_SOBEL, lo=40, hi=96, expand=1)
    base.update(kw)
    return capi.SnAAMask(**base)


def _ex(**kw):
    base = dict(struct_size=ctypes.sizeof(capi.SnAAMaskEx), chroma=capi.SN_AA_MASK_CHROMA_LUMA)
    base.update(kw)
    return capi.SnAAMaskEx(**base)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------

def test_sn_aa_mask_ex_as_a_c_compiler_lays_it_out(tmp_path):
    src = tmp_path / "layout.c"
    fields = ("struct_size", "chroma", "reserved")
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sangnom_hip.h"\n'
                   'int main(void) { printf("%d ' + "%d " * len(fields) + '%d %d\\n", (int)sizeof(sn_aa_mask_ex), '
                   + ", ".join(f"(int)offsetof(sn_aa_mask_ex, {f})" for f in fields) + ", SN_AA_MASK_CHROMA_OWN, SN_AA_MASK_CHROMA_LUMA); return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    assert [int(x) for x in out] == [32, 0, 4, 8, 0, 1]
    M = capi.SnAAMaskEx
    assert ctypes.sizeof(M) == 32
    assert [getattr(M, f).offset for f in fields] == [0, 4, 8]
    assert (capi.SN_AA_MASK_CHROMA_OWN, capi.SN_AA_MASK_CHROMA_LUMA) == (0, 1)


def test_the_three_symbols_are_declared_exported_and_mirrored(hip_lib):
    header = open(os.path.join(ROOT, "include", "sangnom_hip.h")).read()
    for name in ("sn_aa_create_ex4", "sn_aa_get_mask_ex", "sn_mask_merge_luma_device"):
        assert re.search(r"\bint " + name + r"\(", header), f"{name} is not declared"
        assert hasattr(hip_lib, name), f"libsangnom_hip.so does not export {name}"
        assert name in capi.EXPORTS + capi.EXPORTS_NUMBERED and getattr(hip_lib, name).argtypes, f"capi.py does not mirror {name}"
    assert hip_lib.sn_abi_version() == 4
    assert re.search(r"#define SN_ABI_VERSION 4\b", header)
    assert "launch_mask_merge_luma" in open(os.path.join(ROOT, "avisynth_sangnom2_amd", "csrc", "sn_internal.h")).read()


def test_aa_mask_ex_of_capi():
    assert capi.aa_mask_ex().chroma == 0 and capi.aa_mask_ex("own").chroma == 0 and capi.aa_mask_ex("luma").chroma == 1
    assert capi.aa_mask_ex("luma").struct_size == 32
    for bad in ("chroma", 1, None, True, "LUMA"):
        with pytest.raises(ValueError):
            capi.aa_mask_ex(bad)


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def _create(hip_lib, cfg, mask, ex):
    h = ctypes.c_void_p()
    rc = hip_lib.sn_aa_create_ex4(ctypes.byref(cfg), None, None, None, ctypes.byref(mask) if mask is not None else None,
                                  ctypes.byref(ex) if ex is not None else None, ctypes.byref(h))
    assert not h.value
    return rc, hip_lib.sn_aa_last_error(None).decode()


@pytest.mark.parametrize("kw,field", [(dict(struct_size=28), "struct_size"), (dict(struct_size=0), "struct_size"), (dict(chroma=2), "chroma"),
                                      (dict(chroma=-1), "chroma")])
def test_a_bad_mask_ex_is_refused_naming_the_field(hip_lib, kw, field):
    rc, msg = _create(hip_lib, _cfg(), _mask(), _ex(**kw))
    assert rc == capi.SN_ERR_INVALID_ARG and "sn_aa_mask_ex." + field in msg, msg


def test_reserved_words_and_the_luma_rule(hip_lib):
    for word in range(6):
        ex = _ex()
        ex.reserved[word] = 1
        rc, msg = _create(hip_lib, _cfg(), _mask(), ex)
        assert rc == capi.SN_ERR_INVALID_ARG and "sn_aa_mask_ex.reserved" in msg
    rc, msg = _create(hip_lib, _cfg(luma=0), _mask(), _ex())
    assert rc == capi.SN_ERR_CONFIG
    assert msg == "SangNomAA: a luma-derived chroma mask needs luma processed (luma=true)"
    # the struct_size is looked at even without a mask
    for mask in (None, _mask(kind=capi.SN_AA_MASK_NONE)):
        rc, msg = _create(hip_lib, _cfg(), mask, _ex(struct_size=28))
        assert rc == capi.SN_ERR_INVALID_ARG and "sn_aa_mask_ex.struct_size" in msg
    assert hip_lib.sn_aa_get_mask_ex(None, ctypes.byref(_ex())) == capi.SN_ERR_INVALID_ARG
    assert hip_lib.sn_mask_merge_luma_device(None, ctypes.byref(_mask()), 1, None, 0, 0, 1, 1, None, None, None, None, None, None, 1, 1,
                                             None, None, None) == capi.SN_ERR_INVALID_ARG


def test_without_a_mask_the_other_fields_of_mask_ex_are_ignored(hip_lib):
    """kind 0 or mask NULL: the call gets as far as the device (or succeeds where there is one), luma=0 included."""
    for mask in (None, _mask(kind=capi.SN_AA_MASK_NONE)):
        ex = _ex(chroma=7)
        ex.reserved[3] = 5
        h = ctypes.c_void_p()
        rc = hip_lib.sn_aa_create_ex4(ctypes.byref(_cfg(luma=0)), None, None, None, ctypes.byref(mask) if mask is not None else None, ctypes.byref(ex),
                                      ctypes.byref(h))
        assert rc in (capi.SN_OK, capi.SN_ERR_HIP, capi.SN_ERR_NO_DEVICE), hip_lib.sn_aa_last_error(None).decode()
        if h.value:
            hip_lib.sn_aa_destroy(h)


def test_the_python_constructor_reports_the_luma_rule_and_bad_names(hip_lib):
    clip = clip_format("YUV420P8", 128, 64)
    with pytest.raises(SangNomError) as e:
        SangNomAAHost(clip, luma=False, mask=(40, 96), mask_chroma="luma")
    assert e.value.code == capi.SN_ERR_CONFIG and "a luma-derived chroma mask needs luma processed" in str(e.value)
    with pytest.raises(ValueError):
        SangNomAAHost(clip, mask=(40, 96), mask_chroma="both")


# ---- the model, pinned by hand ---------------------------------------------------------------------------------------------------

def _step(at, shape=(8, 16), lo=50, hi=200):
    S = np.full(shape, lo, np.uint8)
    S[:, at:] = hi
    return S


def test_a_vertical_luma_step_by_hand():
    """Luma columns 0..5 hold 50 and 6.. hold 200: e = 150 in columns 5 and 6, so with lo = hi = 100 m_L = 256 there and 0
    elsewhere.  4:2:2 and 4:2:0: chroma column 2 is the mean over luma columns 4, 5 and column 3 over 6, 7: (256 + 1) >> 1 = 128
    each (4:2:0: (512 + 2) >> 2).  4:1:1: chroma column 1 covers luma 4..7, two columns of four: (512 + 2) >> 2 = 128."""
    L = _step(6)
    mL = edge_mask(L, 100, 100, 0)
    want = np.zeros(L.shape, np.int64)
    want[:, 5:7] = 256
    assert np.array_equal(mL, want)
    for sw, sh in ((1, 0), (1, 1)):
        mc = chroma_mask(L, 100, 100, 0, 8, sw, sh)
        assert mc.shape == (8 >> sh, 8)
        assert np.array_equal(mc, np.tile([0, 0, 128, 128, 0, 0, 0, 0], (8 >> sh, 1)))
    assert np.array_equal(chroma_mask(L, 100, 100, 0, 8, 2, 0), np.tile([0, 128, 0, 0], (8, 1)))
    # the step between columns 6 | 7: m_L = 256 in 6 and 7, the whole block of chroma column 3
    for sw, sh in ((1, 0), (1, 1)):
        assert np.array_equal(chroma_mask(_step(7), 100, 100, 0, 8, sw, sh), np.tile([0, 0, 0, 256, 0, 0, 0, 0], (8 >> sh, 1)))
    # and the merge: S where mc = 0, R where it is 256, (S 128 + R 128 + 128) >> 8 at 128
    S = np.full((4, 8), 10, np.uint8)
    R = np.full((4, 8), 201, np.uint8)
    assert np.array_equal(merge_plane_luma(L, S, R, 100, 100, 0, 8, 1, 1), np.tile([10, 10, 106, 106, 10, 10, 10, 10], (4, 1)))
    assert np.array_equal(merge_plane_luma(_step(7), S, R, 100, 100, 0, 8, 1, 1), np.tile([10, 10, 10, 201, 10, 10, 10, 10], (4, 1)))
    assert np.array_equal(mask_plane_luma(L, 100, 100, 0, 8, 1, 1)[0], [0, 0, 128, 128, 0, 0, 0, 0])  # (128 * 255 + 128) >> 8 = 128
    assert np.array_equal(mask_plane_luma(L.astype(np.uint16) << 2, 100, 100, 0, 10, 1, 1)[0], [0, 0, 512, 512, 0, 0, 0, 0])  # (128 * 1023 + 128) >> 8


def test_block_means_by_hand():
    m = np.zeros((4, 8), np.int64)
    m[1, 3] = 256                      # one sample of 256 in a 2 x 2 block: (256 + 2) >> 2 = 64; in a 1 x 2 block 128; in 4 x 4 (256 + 8) >> 4 = 16
    m[2, 6] = 76                       # one ramp value of 76: (76 + 2) >> 2 = 19 in a 2 x 2 block, (76 + 1) >> 1 = 38 in a 1 x 2 block
    assert np.array_equal(reduce_mask(m, 1, 1), [[0, 64, 0, 0], [0, 0, 0, 19]])
    assert np.array_equal(reduce_mask(m, 1, 0), [[0, 0, 0, 0], [0, 128, 0, 0], [0, 0, 0, 38], [0, 0, 0, 0]])
    assert np.array_equal(reduce_mask(m, 0, 1), [[0, 0, 0, 128, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 38, 0]])
    assert np.array_equal(reduce_mask(m, 2, 2), [[16, (76 + 8) >> 4]])
    assert reduce_mask(m, 0, 0) is not m and np.array_equal(reduce_mask(m, 0, 0), m)
    for sw in range(3):
        for sh in range(3):
            assert np.all(reduce_mask(np.full((8, 8), 256), sw, sh) == 256) and not reduce_mask(np.zeros((8, 8), np.int64), sw, sh).any()
            assert np.all(reduce_mask(np.full((8, 8), 255), sw, sh) == 255)


def test_without_subsampling_mc_is_the_luma_mask():
    from avisynth_sangnom2_amd import synth
    for dtype, bits in ((np.uint8, 8), (np.uint16, 10), (np.float32, 32)):
        L = synth.plane(24, 40, np.dtype(dtype).itemsize, bits, "edges", 921)
        for expand in (0, 1):
            assert np.array_equal(chroma_mask(L, 40, 96, expand, bits, 0, 0), edge_mask(L, 40, 96, expand, bits))


def test_a_nan_in_float_luma_keeps_the_chroma_source():
    L = np.full((8, 12), 0.5, np.float32)
    L[3, 2] = np.nan
    L[3, 8] = np.inf
    mc = chroma_mask(L, 40, 96, 0, 32, 1, 1)
    assert not mc[:, :2].any()                   # e is NaN around the NaN: m_L = 0 there
    # the ring of 256 around the infinity (rows 2..4, columns 7..9, 0 at the infinity itself), cut by the blocks: chroma (1, 3) holds
    # luma (2, 7) and (3, 7), chroma (1, 4) holds (2, 8), (2, 9) and (3, 9)
    assert mc[1, 3] == (2 * 256 + 2) >> 2 and mc[1, 4] == (3 * 256 + 2) >> 2


# ---- the frames of the GPU tests -------------------------------------------------------------------------------------------------

def _classes(m):
    n = m.size
    return (m == 0).sum() / n, ((m > 0) & (m < 256)).sum() / n, (m == 256).sum() / n


ALL_SIZES = sorted({c[:3] for c in lc.BATCH + [lc.CHROMA_OFF, lc.CHUNK]} | set(lc.EXTRA_SIZES))


@pytest.mark.parametrize("fmt,w,h", ALL_SIZES, ids=[f"{f}-{w}x{h}" for f, w, h in ALL_SIZES])
def test_mc_of_every_frame_of_the_gpu_tests_holds_all_three_classes(fmt, w, h):
    clip = clip_format(fmt, w, h)
    for f, fr in enumerate(lc.frames_of(fmt, w, h)):
        for expand in lc.EXPANDS:
            mc = chroma_mask(fr[0], lc.LO, lc.HI, expand, clip.bits, clip.subw, clip.subh)
            c = _classes(mc)
            differs = [float((mc != edge_mask(fr[p], lc.LO, lc.HI, expand, clip.bits)).mean()) for p in (1, 2)]
            print(f"{fmt} {w}x{h} frame {f} expand {expand}: " + " / ".join(f"{x:.3f}" for x in c) + f"; differs from the own masks on {differs}")
            assert min(c) >= 0.05, f"frame {f} expand {expand}: classes {c}"
            assert min(differs) >= 0.25, f"frame {f} expand {expand}: mc is nearly the plane's own mask"


@pytest.mark.parametrize("i", [0, 2, 3, 4], ids=lambda i: f"{lc.BATCH[i][0]}-{i}")
def test_the_expected_frames_differ_from_the_source_the_unmasked_result_and_the_own_mask_expectation(i):
    """On the first two frames of a case of every sample type and subsampling, for both forms of the call (the GPU tests
    assert the same of every frame they compare)."""
    case = lc.BATCH[i]
    for form in (None, "halfband"):
        for expand in lc.EXPANDS:
            frames, _, res, want, own = lc.expected(case, form, expand, count=2)
            for f in range(2):
                assert np.array_equal(want[f][0], own[f][0]), "luma is merged through its own mask"
                for p in (1, 2):
                    what = f"form {form} expand {expand} frame {f} plane {p}"
                    assert not np.array_equal(want[f][p], frames[f][p]), what + ": the expected plane is the source"
                    assert not np.array_equal(want[f][p], res[f][p]), what + ": the expected plane is the unmasked result"
                    assert not np.array_equal(want[f][p], own[f][p]), what + ": the expected plane is the own-mask expectation"
