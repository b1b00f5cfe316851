"""sn_policy.sse2_sweeps without a GPU: the field took the place of a reserved word (same struct, same ABI version), a value
other than 0 / 1 is refused before a device is touched, and every case of tests/sse2_sweep_cases.py is one on which the SSE2
model and the opt=0 oracle give different pixels (so a sweep that kept the wrapping arithmetic cannot pass the GPU tests)."""
import ctypes

import pytest

from avisynth_sangnom2_amd import capi
from tests import sse2_sweep_cases as sc


def _cfg(**kw):
    base = dict(struct_size=ctypes.sizeof(capi.SnConfig), width=64, height=32, bytes_per_sample=1, bits_per_sample=8,
                num_planes=1, sub_w=0, sub_h=0, order=1, aa=48, aac=0, dh=0, luma=1, chroma=1, device=0, max_batch=1, mode=0,
                host_depth=0, isolated_planes=0, fresh_pool=0, stream=None)
    base.update(kw)
    return capi.SnConfig(**base)


def test_the_policy_struct_keeps_its_size_and_layout(hip_lib):
    assert ctypes.sizeof(capi.SnPolicy) == 32
    assert capi.SnPolicy.sse2_sweeps.offset == 24 and capi.SnPolicy.reserved.offset == 28  # reserved[0] of the previous release
    assert capi.SnPolicy.chroma_sweeps.offset == 20
    assert hip_lib.sn_abi_version() == 4


def test_the_knob_defaults_to_the_previous_kernels():
    assert capi.POLICY_DEFAULTS["sse2_sweeps"] == 0
    assert capi.policy().sse2_sweeps == 0 and capi.policy(sse2_sweeps=1).sse2_sweeps == 1


@pytest.mark.parametrize("bad", [2, -1, 7])
def test_a_value_other_than_0_or_1_is_refused_before_a_device_is_touched(hip_lib, bad):
    h = ctypes.c_void_p()
    cfg = _cfg()
    pol = capi.policy(sse2_sweeps=bad)
    assert hip_lib.sn_create_with_policy(ctypes.byref(cfg), ctypes.byref(pol), ctypes.byref(h)) == capi.SN_ERR_INVALID_ARG
    assert b"sn_policy" in hip_lib.sn_last_error(None)
    opts = capi.options(capi.SN_ARITH_SSE2)
    assert hip_lib.sn_create_ex(ctypes.byref(cfg), ctypes.byref(pol), ctypes.byref(opts), ctypes.byref(h)) == capi.SN_ERR_INVALID_ARG
    assert b"sn_policy" in hip_lib.sn_last_error(None)


@pytest.mark.parametrize("case", list(sc.every_case()), ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-{c[6]}")
def test_the_model_tells_the_arithmetics_apart_on_every_case(case):
    fmt, w, h, kw, ckw, n, pattern, parities = case
    sc.expected(fmt, w, h, kw, ckw, n, pattern, parities)  # asserts it for 8-bit and 16-bit clips


def test_the_model_tells_the_arithmetics_apart_on_the_hand_off_and_anti_aliasing_inputs():
    from tests.aa_script import Script
    from avisynth_sangnom2_amd import clip_format
    for fmt, w, h in sc.HANDOFF:
        sc.expected(fmt, w, h, dict(aa=48, aac=48), {}, 1, sc.HANDOFF_PATTERN, (1,), sc.HANDOFF_SEED)
    for fmt, w, h, kw in sc.AA:
        clip = clip_format(fmt, w, h)
        frames = sc.frames_of(clip, sc.AA_PATTERN, sc.AA_FRAMES, sc.AA_SEED)
        s1, s0 = Script(clip, opt=1, fresh=True, **kw), Script(clip, opt=0, fresh=True, **kw)
        assert sc.differs([s1.frame(fr) for fr in frames], [s0.frame(fr) for fr in frames])
