"""Anti-aliasing at source size, the parts that need no GPU: the ABI of sn_aa_options and the three new symbols, the
refusals made before a device is touched, and the numpy model of the reduction (tests/reduce_model.py) against the dh
script (tests/aa_dh_script.py): the ox / oy mapping, constants, and that the half-band kernel's clamp acts on both sides."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from avisynth_sangnom2_amd import capi, clip_format, synth
from tests.aa_dh_script import Script, kept_offset
from tests.reduce_model import reduce_model, reduce_plane, reduce_unclamped

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(**kw):
    base = dict(struct_size=ctypes.sizeof(capi.SnConfig), width=64, height=32, bytes_per_sample=1, bits_per_sample=8, num_planes=1, sub_w=0,
                sub_h=0, order=1, aa=48, aac=0, dh=1, luma=1, chroma=1, device=0, max_batch=1, mode=0, host_depth=0, isolated_planes=0,
                fresh_pool=0, stream=None)
    base.update(kw)
    return capi.SnConfig(**base)


def test_sn_aa_options_as_a_c_compiler_lays_it_out(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sangnom_hip.h"\n'
                   'int main(void) { printf("%d %d %d %d %d %d\\n", (int)sizeof(sn_aa_options), (int)offsetof(sn_aa_options, struct_size),\n'
                   '(int)offsetof(sn_aa_options, reduce), (int)offsetof(sn_aa_options, reserved), SN_AA_REDUCE_TENT, SN_AA_REDUCE_HALFBAND); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    assert [int(x) for x in out] == [32, 0, 4, 8, 1, 2]
    assert ctypes.sizeof(capi.SnAAOptions) == 32 and capi.SnAAOptions.reduce.offset == 4 and capi.SnAAOptions.reserved.offset == 8
    assert (capi.SN_AA_REDUCE_NONE, capi.SN_AA_REDUCE_TENT, capi.SN_AA_REDUCE_HALFBAND) == (0, 1, 2)


def test_the_three_symbols_are_declared_exported_and_mirrored(hip_lib):
    header = open(os.path.join(ROOT, "include", "sangnom_hip.h")).read()
    for name in ("sn_aa_create_ex2", "sn_aa_get_reduce", "sn_reduce_device"):
        assert re.search(r"\bint " + name + r"\(", header), f"{name} is not declared"
        assert hasattr(hip_lib, name), f"libsangnom_hip.so does not export {name}"
        assert name in capi.EXPORTS + capi.EXPORTS_NUMBERED and getattr(hip_lib, name).argtypes, f"capi.py does not mirror {name}"
    assert hip_lib.sn_abi_version() == 4
    assert re.search(r"#define SN_ABI_VERSION 4\b", header)
    assert hip_lib.sn_aa_get_reduce(None) == -1


def _create(hip_lib, cfg, aopt):
    h = ctypes.c_void_p()
    rc = hip_lib.sn_aa_create_ex2(ctypes.byref(cfg), None, None, ctypes.byref(aopt) if aopt is not None else None, ctypes.byref(h))
    assert not h.value
    return rc, hip_lib.sn_aa_last_error(None).decode()


def test_refusals_that_need_no_device(hip_lib):
    size = ctypes.sizeof(capi.SnAAOptions)
    rc, msg = _create(hip_lib, _cfg(dh=0), capi.SnAAOptions(struct_size=size, reduce=1))
    assert rc == capi.SN_ERR_CONFIG and "reduce needs dh" in msg
    rc, msg = _create(hip_lib, _cfg(), capi.SnAAOptions(struct_size=size, reduce=3))
    assert rc == capi.SN_ERR_INVALID_ARG and "reduce" in msg
    rc, msg = _create(hip_lib, _cfg(), capi.SnAAOptions(struct_size=size, reduce=-1))
    assert rc == capi.SN_ERR_INVALID_ARG and "reduce" in msg
    for word in range(6):
        o = capi.SnAAOptions(struct_size=size, reduce=1)
        o.reserved[word] = 1
        rc, msg = _create(hip_lib, _cfg(), o)
        assert rc == capi.SN_ERR_INVALID_ARG and "reserved" in msg
    rc, msg = _create(hip_lib, _cfg(), capi.SnAAOptions(struct_size=size - 4, reduce=1))
    assert rc == capi.SN_ERR_INVALID_ARG and "struct_size" in msg
    with pytest.raises(ValueError):
        capi.aa_options("box")


POINT = [("Y8", dict(order=1), 1), ("Y8", dict(order=2), 1), ("Y8", dict(order=0), 1), ("Y8", dict(order=0), 0),
         ("YUV420P8", dict(order=1, aac=48), 1), ("YUV420P8", dict(order=2, aac=48), 1), ("YUV420P8", dict(order=0, aac=48), 1),
         ("YUV420P8", dict(order=0, aac=48), 0)]


@pytest.mark.parametrize("fmt,kw,parity", POINT, ids=[f"{c[0]}-order{c[1]['order']}-parity{c[2]}" for c in POINT])
def test_point_taps_return_the_source_frame(fmt, kw, parity):
    """The source sample (x, y) lies at E[2y + off][2x + 1 - off]: the model with taps [1] gives the source frame back."""
    clip = clip_format(fmt, 128, 64)
    fr = synth.frame(clip, "noise", seed=11)
    E = Script(clip, **kw).frame(fr, parity=parity)
    got = reduce_model(E, "point", order=kw["order"], parity=parity, bits=8)
    for p in range(clip.planes):
        assert got[p].shape == fr[p].shape and np.array_equal(got[p], fr[p]), f"plane {p}"
    assert kept_offset(kw["order"], parity) == (kw["order"] - 1 if kw["order"] else 1 - parity)


@pytest.mark.parametrize("kernel", ["tent", "halfband"])
@pytest.mark.parametrize("dtype,bits,value", [(np.uint8, 8, 255), (np.uint8, 8, 77), (np.uint16, 10, 1023), (np.uint16, 16, 65535), (np.uint16, 16, 1),
                                              (np.float32, 32, 0.3), (np.float32, 32, -1.5)])
def test_a_constant_plane_reduces_to_itself(kernel, dtype, bits, value):
    E = np.full((24, 36), value, dtype)
    for ox in (0, 1):
        for oy in (0, 1):
            got = reduce_plane(E, kernel, ox, oy, bits)
            assert got.shape == (12, 18) and got.dtype == E.dtype
            assert np.array_equal(got, np.full((12, 18), value, dtype))


@pytest.mark.parametrize("fmt,w,h,below,above", [("Y8", 128, 64, True, 255), ("Y16", 96, 64, True, 65535), ("Y10", 64, 48, False, 1023)])
def test_the_half_band_clamp_acts_on_checker_frames(fmt, w, h, below, above):
    clip = clip_format(fmt, w, h)
    E = Script(clip).frame(synth.frame(clip, "checker", seed=0))[0]
    v = (reduce_unclamped(E, "halfband", 1, 0) + 512) >> 10
    print(f"{fmt}: unclamped half-band result min {v.min()} max {v.max()}")
    assert v.max() > above
    if below:
        assert v.min() < 0
    got = reduce_plane(E, "halfband", 1, 0, clip.bits)
    assert got.min() >= 0 and got.max() <= above
