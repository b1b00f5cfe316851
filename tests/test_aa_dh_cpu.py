"""The anti-aliasing call with dh (enlargement by two in both directions), as far as it can be checked without a GPU:
the creation checks that come before any device is touched, and the script the GPU tests compare against
(tests/aa_dh_script.py) on the CPU oracle."""
import ctypes

import numpy as np
import pytest

from avisynth_sangnom2_amd import capi, clip_format, synth
from tests.aa_dh_script import Script, kept_offset
from tests.util import same


def _cfg(width, height, **kw):
    f = dict(struct_size=ctypes.sizeof(capi.SnConfig), width=width, height=height, bytes_per_sample=1, bits_per_sample=8, num_planes=1,
             sub_w=0, sub_h=0, order=1, aa=48, aac=0, dh=1, luma=1, chroma=1, device=0, max_batch=1, mode=capi.SN_MODE_AUTO)
    f.update(kw)
    return capi.SnConfig(**f)


def test_an_odd_width_is_the_turned_clips_odd_height(hip_lib):
    """The turned clip is validated first, as SangNom2 validates it, before any device is touched: with or without a GPU."""
    h = ctypes.c_void_p()
    cfg = _cfg(63, 32)
    assert hip_lib.sn_aa_create(ctypes.byref(cfg), ctypes.byref(h)) == capi.SN_ERR_CONFIG
    assert not h.value
    assert hip_lib.sn_aa_last_error(None).decode() == "SangNom2: height must be even."
    assert hip_lib.sn_abi_version() == 4


@pytest.mark.parametrize("order,parity", [(1, 1), (2, 1), (0, 1), (0, 0)])
def test_the_script_keeps_the_source_samples(order, parity):
    clip = clip_format("Y8", 128, 64)
    fr = synth.frame(clip, "noise", seed=11)
    out = Script(clip, order=order).frame(fr, parity=parity)
    assert out[0].shape == (128, 256)
    off = kept_offset(order, parity)
    assert np.array_equal(out[0][off::2, (1 - off)::2], fr[0])
    assert not np.array_equal(out[0][(1 - off)::2, off::2], fr[0]), "the other lattice holds interpolated samples"


def test_dh_forces_the_planes_in_the_script():
    clip = clip_format("YUV420P8", 128, 64)
    fr = synth.frame(clip, "noise", seed=12)
    a = Script(clip, aac=48, luma=False).frame(fr)
    b = Script(clip, aac=48).frame(fr)
    assert [x.shape for x in a] == [(128, 256), (64, 128), (64, 128)]
    for p in range(3):
        assert same(a[p], b[p]), f"plane {p}"
