"""The plugin function SangNomAA(clip, ..., mask=true, mluma=true): host/sn_host_test drives sangnom::AAFilter with
SN_HOST_TEST_MASK=lo,hi,expand and SN_HOST_TEST_MASK_LUMA=1, synchronously ("aa:1") and over the host ring ("aa:4"), without
dh and with dh and a reduction.  The frames equal merge_model_luma(source, the script's frame) (tests/mask_luma_model.py,
tests/mask_luma_cases.py); the constructor error needs no GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

from avisynth_sangnom2_amd import clip_format
from tests import mask_luma_cases as lc
from tests.util import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "host", "sn_host_test")


def _run(tmp_path, clip, kw, frames, mask, extra, reduce=0, luma=1):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), "sn_host_test"])
    hdr = [clip.width, clip.height, clip.bytes, clip.bits, clip.planes, clip.subw, clip.subh, kw.get("order", 1), kw.get("aa", 48), kw.get("aac", 0),
           int(kw.get("dh", False)), luma, 1, len(frames)]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<14i", *hdr))
        for fr in frames:
            f.write(struct.pack("<i", 1))
            for pl in fr:
                f.write(np.ascontiguousarray(pl).tobytes())
    env = dict(os.environ, SN_HOST_TEST_SWEEPS="1", SN_HOST_TEST_MASK=mask, SN_HOST_TEST_MASK_LUMA="1")
    if reduce:
        env["SN_HOST_TEST_REDUCE"] = str(reduce)
    r = subprocess.run([BIN, fin, fout, extra], capture_output=True, text=True, timeout=300, env=env)
    return r, fout


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["reduce", "plain"])
@pytest.mark.parametrize("how", ["aa:4", "aa:1"])
def test_frames_equal_the_model(tmp_path, how, form):
    fmt, w, h, kw = lc.HOST[:4]
    clip = clip_format(fmt, w, h)
    frames, _, res, want, own = lc.expected(lc.HOST, "halfband" if form == "reduce" else None, 1)
    r, fout = _run(tmp_path, clip, dict(kw, dh=form == "reduce"), frames, f"{lc.LO},{lc.HI},1", how, reduce=2 if form == "reduce" else 0)
    assert r.returncode == 0, (r.stdout, r.stderr)
    raw = np.fromfile(fout, dtype=np.uint8)
    pos = 0
    for f, fr in enumerate(frames):
        for p, wpl in enumerate(want[f]):
            got = raw[pos:pos + wpl.nbytes].view(wpl.dtype).reshape(wpl.shape)
            pos += wpl.nbytes
            assert same(wpl, got), f"{fmt} {how} frame {f} plane {p}"
            assert not same(wpl, fr[p]) and not same(wpl, res[f][p])
            assert p == 0 or not same(wpl, own[f][p]), "the expected plane is what the plane's own mask gives"
    assert pos == raw.size, "the frames are not of source size"


def test_luma_false_is_a_constructor_error(tmp_path):
    """Checked before any device is touched, so this runs without a GPU."""
    r, _ = _run(tmp_path, clip_format("YUV420P8", 128, 64), {}, [], "40,96,1", "aa", luma=0)
    assert r.returncode == 3 and r.stdout.strip() == "SangNomAA: a luma-derived chroma mask needs luma processed (luma=true)", \
        (r.returncode, r.stdout, r.stderr)
