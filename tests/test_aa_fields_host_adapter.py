"""The plugin function SangNomAA(clip, ..., both): host/sn_host_test drives sangnom::AAFilter with SN_HOST_TEST_FIELDS=both,
synchronously ("aa:1") and over the host ring ("aa:4").  The frames equal tests/fields_model.BothScript's
(tests/fields_cases.py), whatever order and parity the frames are sent with; the constructor error needs no GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

from avisynth_sangnom2_amd import clip_format
from tests import fields_cases as fc
from tests.util import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "host", "sn_host_test")


def _run(tmp_path, clip, kw, frames, extra, fields="both", parities=None):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), "sn_host_test"])
    hdr = [clip.width, clip.height, clip.bytes, clip.bits, clip.planes, clip.subw, clip.subh, kw.get("order", 1), kw.get("aa", 48), kw.get("aac", 0),
           int(kw.get("dh", False)), 1, 1, len(frames)]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<14i", *hdr))
        for k, fr in enumerate(frames):
            f.write(struct.pack("<i", parities[k] if parities else 1))
            for pl in fr:
                f.write(np.ascontiguousarray(pl).tobytes())
    env = dict(os.environ, SN_HOST_TEST_SWEEPS="1", SN_HOST_TEST_FIELDS=fields)
    r = subprocess.run([BIN, fin, fout, extra], capture_output=True, text=True, timeout=300, env=env)
    return r, fout


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["aa:4", "aa:1"])
@pytest.mark.parametrize("i,order", [(fc.HISTORY_Y8, 1), (fc.HISTORY_Y8, 0), (fc.YUV420, 2)], ids=["Y8-72x40", "Y8-72x40-order0", "YUV420P8-order2"])
def test_both_fields_frames_equal_the_model(tmp_path, i, order, how):
    case = fc.CASES[i]
    clip = clip_format(case.fmt, case.w, case.h)
    frames, want, _ = fc.expected(i, count=5)
    r, fout = _run(tmp_path, clip, dict(case.kw, order=order), frames, how, parities=[1, 0, 0, 1, 0])
    assert r.returncode == 0, (r.stdout, r.stderr)
    raw = np.fromfile(fout, dtype=np.uint8)
    pos = 0
    for f in range(len(frames)):
        for p, wpl in enumerate(want[f]):
            got = raw[pos:pos + wpl.nbytes].view(wpl.dtype).reshape(wpl.shape)
            pos += wpl.nbytes
            assert same(wpl, got), f"{case.fmt} {how} frame {f} plane {p}"
    assert pos == raw.size, "the frames are not of source size"
    assert not same(want[0][0], fc.one_field(i, 1)[0])  # (tests/test_aa_fields_cpu.py has the figures)


def test_both_fields_with_dh_is_a_constructor_error(tmp_path):
    """Checked before any device is touched, so this runs without a GPU."""
    r, _ = _run(tmp_path, clip_format("Y8", 128, 64), dict(dh=True), [], "aa")
    assert r.returncode == 3 and r.stdout.strip() == "SangNomAA: both fields needs dh=false", (r.returncode, r.stdout, r.stderr)
