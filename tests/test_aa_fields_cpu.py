"""The both-fields mode of the anti-aliasing call, the parts that need no GPU: the ABI of sn_aa_fields and the new symbols,
the refusals made before a device is touched, the model of avg (tests/fields_model.py) pinned by answers worked out by hand,
the plan of the mode (tests/c/aa_fields_plan_check.cpp on the host compiler), and the conditions that keep the GPU tests from
passing trivially: on frame 0 of every row the expected frame differs from either one-field frame in at least half of the
samples, and the last average sees an odd sum in at least a quarter of them."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from avisynth_sangnom2_amd import capi, clip_format, synth
from tests import fields_cases as fc
from tests.fields_model import BothScript, merge_plane, processed_planes
from tests.util import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avisynth_sangnom2_amd", "csrc")
NAMES = ("sn_aa_create_ex6", "sn_aa_get_fields", "sn_merge_device", "sn_turn_merge_device")


def _cfg(**kw):
    base = dict(struct_size=ctypes.sizeof(capi.SnConfig), width=64, height=32, bytes_per_sample=1, bits_per_sample=8, num_planes=1, sub_w=0,
                sub_h=0, order=1, aa=48, aac=0, dh=0, luma=1, chroma=1, device=0, max_batch=1, mode=0, host_depth=0, isolated_planes=0,
                fresh_pool=0, stream=None)
    base.update(kw)
    return capi.SnConfig(**base)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------

def test_sn_aa_fields_as_a_c_compiler_lays_it_out(tmp_path):
    src = tmp_path / "layout.c"
    fields = ("struct_size", "mode", "reserved")
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sangnom_hip.h"\n'
                   'int main(void) { printf("%d ' + "%d " * len(fields) + '%d %d\\n", (int)sizeof(sn_aa_fields), '
                   + ", ".join(f"(int)offsetof(sn_aa_fields, {f})" for f in fields) + ", SN_AA_FIELDS_ONE, SN_AA_FIELDS_BOTH); return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    assert [int(x) for x in out] == [32, 0, 4, 8, 0, 1]
    M = capi.SnAAFields
    assert ctypes.sizeof(M) == 32 and [getattr(M, f).offset for f in fields] == [0, 4, 8]
    f = capi.aa_fields("both")
    assert (f.struct_size, f.mode, list(f.reserved)) == (32, capi.SN_AA_FIELDS_BOTH, [0] * 6)
    assert (capi.aa_fields().mode, capi.aa_fields("one").mode) == (0, 0)
    with pytest.raises(ValueError):
        capi.aa_fields("top")


def test_the_new_symbols_are_declared_exported_and_mirrored(hip_lib):
    header = open(os.path.join(ROOT, "include", "sangnom_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), f"{name} is not declared"
        assert hasattr(hip_lib, name), f"libsangnom_hip.so does not export {name}"
        assert name in capi.EXPORTS + capi.EXPORTS_NUMBERED and getattr(hip_lib, name).argtypes, f"capi.py does not mirror {name}"
    assert "sn_aa_create_ex6" in capi.EXPORTS_NUMBERED
    assert hip_lib.sn_abi_version() == 4
    assert re.search(r"#define SN_ABI_VERSION 4\b", header)
    internal = open(os.path.join(CSRC, "sn_internal.h")).read()
    assert "launch_merge" in internal and "launch_turn_merge" in internal
    assert "sn_merge.hip" in open(os.path.join(CSRC, "Makefile")).read()


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def _create(hip_lib, cfg, fields, aopt=None):
    h = ctypes.c_void_p()
    rc = hip_lib.sn_aa_create_ex6(ctypes.byref(cfg), None, None, ctypes.byref(aopt) if aopt is not None else None, None, None, None,
                                  ctypes.byref(fields) if fields is not None else None, ctypes.byref(h))
    assert not h.value
    return rc, hip_lib.sn_aa_last_error(None).decode()


def _fields(**kw):
    base = dict(struct_size=ctypes.sizeof(capi.SnAAFields), mode=capi.SN_AA_FIELDS_BOTH)
    base.update(kw)
    return capi.SnAAFields(**base)


@pytest.mark.parametrize("kw,field", [(dict(struct_size=28), "struct_size"), (dict(struct_size=0), "struct_size"), (dict(struct_size=36, mode=0), "struct_size"),
                                      (dict(mode=-1), "mode"), (dict(mode=2), "mode")])
def test_a_bad_struct_is_refused_naming_the_field(hip_lib, kw, field):
    rc, msg = _create(hip_lib, _cfg(), _fields(**kw))
    assert rc == capi.SN_ERR_INVALID_ARG and "sn_aa_fields." + field in msg, msg


def test_reserved_words_and_the_dh_rule(hip_lib):
    for word in range(6):
        f = _fields()
        f.reserved[word] = 1
        rc, msg = _create(hip_lib, _cfg(), f)
        assert rc == capi.SN_ERR_INVALID_ARG and "sn_aa_fields.reserved" in msg
    rc, msg = _create(hip_lib, _cfg(dh=1), _fields())
    assert (rc, msg) == (capi.SN_ERR_CONFIG, "SangNomAA: both fields needs dh=false")
    rc, msg = _create(hip_lib, _cfg(dh=1), _fields(), capi.aa_options("halfband"))  # reduce needs dh, and falls with it
    assert (rc, msg) == (capi.SN_ERR_CONFIG, "SangNomAA: both fields needs dh=false")
    rc, msg = _create(hip_lib, _cfg(), _fields(), capi.aa_options("tent"))
    assert (rc, msg) == (capi.SN_ERR_CONFIG, "SangNomAA: reduce needs dh=true")
    assert hip_lib.sn_aa_get_fields(None, ctypes.byref(_fields())) == capi.SN_ERR_INVALID_ARG
    assert hip_lib.sn_merge_device(None, 1, None, 0, 0, None, 0, 0, 1, 1, None, 0, 0) == capi.SN_ERR_INVALID_ARG
    assert hip_lib.sn_turn_merge_device(None, 1, 1, None, 0, 0, None, 0, 0, 1, 1, None, 0, 0) == capi.SN_ERR_INVALID_ARG


@pytest.mark.parametrize("dh", [0, 1])
def test_one_field_with_junk_in_the_other_words_gets_as_far_as_the_device(hip_lib, dh):
    h = ctypes.c_void_p()
    one = _fields(mode=capi.SN_AA_FIELDS_ONE)
    for word in range(6):
        one.reserved[word] = 9 + word
    rc = hip_lib.sn_aa_create_ex6(ctypes.byref(_cfg(dh=dh)), None, None, None, None, None, None, ctypes.byref(one), ctypes.byref(h))
    assert rc in (capi.SN_OK, capi.SN_ERR_HIP, capi.SN_ERR_NO_DEVICE), hip_lib.sn_aa_last_error(None).decode()
    if h.value:
        hip_lib.sn_aa_destroy(h)


def test_the_filter_classes_take_the_keyword():
    from avisynth_sangnom2_amd import SangNomAA, SangNomAAHost, SangNomError
    clip = clip_format("Y8", 64, 32)
    for cls in (SangNomAA, SangNomAAHost):
        with pytest.raises(SangNomError) as e:
            cls(clip, dh=True, fields="both")
        assert e.value.code == capi.SN_ERR_CONFIG and "both fields needs dh=false" in str(e.value)
        with pytest.raises(ValueError):
            cls(clip, fields="neither")


# ---- the model, pinned by hand ---------------------------------------------------------------------------------------------------

def _f32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)


@pytest.mark.parametrize("dtype,a,b,want", [(np.uint8, 0, 1, 1), (np.uint8, 255, 255, 255), (np.uint8, 254, 255, 255), (np.uint8, 7, 7, 7),
                                            (np.uint16, 65535, 65534, 65535), (np.uint16, 65535, 65535, 65535), (np.uint16, 1023, 0, 512),
                                            (np.uint16, 32768, 32767, 32768)])
def test_integer_averages_round_up_and_do_not_overflow(dtype, a, b, want):
    for x, y in ((a, b), (b, a)):
        got = merge_plane(np.array([[x]], dtype), np.array([[y]], dtype))
        assert got.dtype == dtype and int(got[0, 0]) == want


def test_float_averages_and_the_one_nan():
    m = lambda a, b: merge_plane(np.asarray(a, np.float32).reshape(1, 1), np.asarray(b, np.float32).reshape(1, 1)).view(np.uint32)[0, 0]
    assert m(0.25, 0.5) == _f32(0x3EC00000).view(np.uint32)[0] and _f32(0x3EC00000)[0] == np.float32(0.375)
    assert m(np.inf, -np.inf) == 0x7FC00000
    payload = _f32(0xFFC12345)  # a negative quiet NaN with a payload
    assert m(payload, 1.0) == 0x7FC00000 and m(1.0, payload) == 0x7FC00000
    assert m(_f32(0x7F812345), 1.0) == 0x7FC00000  # a signalling one
    assert m(-0.0, -0.0) == 0x80000000
    assert m(np.inf, np.inf) == 0x7F800000 and m(-np.inf, 5.0) == 0xFF800000
    big = np.float32(3.0e38)
    assert m(big, big) == 0x7F800000  # the sum overflows before the halving: (a + b) * 0.5f in that order
    tiny = _f32(0x00000001)  # the smallest denormal: 2 tiny * 0.5 = tiny, denormals are kept
    assert m(tiny, tiny) == 0x00000001


# ---- the plan --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_of_both_fields_matches_lines_written_out_by_hand(tmp_path, sanitized):
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else []
    exe = str(tmp_path / ("aa_fields_plan_check" + ("_san" if sanitized else "")))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC, *extra,
                           os.path.join(ROOT, "tests", "c", "aa_fields_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-3000:], r.stderr[-2000:])


# ---- the GPU frames are not trivial ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(fc.CASES)), ids=fc.IDS)
def test_the_expected_frames_tell_both_fields_from_one_and_a_rounding_average_from_a_truncating_one(i):
    case = fc.CASES[i]
    clip = clip_format(case.fmt, case.w, case.h)
    proc = processed_planes(clip.planes, case.kw)
    frames, want, last = fc.expected(i)
    for p in range(clip.planes):
        if not proc[p]:
            assert same(want[0][p], frames[0][p])
            continue
        d1 = float((want[0][p] != fc.one_field(i, 1)[p]).mean())
        d2 = float((want[0][p] != fc.one_field(i, 2)[p]).mean())
        print(f"{fc.IDS[i]} plane {p}: differs from order 1 in {d1:.3f}, from order 2 in {d2:.3f} of the samples", end="")
        if clip.bytes < 4:
            odd = float((((last[0][p].astype(np.int64) + last[1][p]) & 1) == 1).mean())
            print(f", a + b odd in {odd:.3f}")
        else:
            print()
        assert d1 >= 0.5 and d2 >= 0.5
        if clip.bytes < 4:
            assert odd >= 0.25


# ---- order and parity have no influence ------------------------------------------------------------------------------------------

def test_the_model_gives_one_answer_for_every_order_and_parity():
    clip = clip_format("Y8", 72, 40)
    frames = [synth.frame(clip, "noise", seed=411 + f) for f in range(3)]
    ref = None
    for order in (0, 1, 2):
        for parities in ([1, 1, 1], [0, 0, 0], [0, 1, 0]):
            script = BothScript(clip, order=order)
            got = [script.frame(fr, parity=q) for fr, q in zip(frames, parities)]
            if ref is None:
                ref = got
            assert all(same(a[0], b[0]) for a, b in zip(ref, got)), (order, parities)
