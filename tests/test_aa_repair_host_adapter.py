"""The plugin function SangNomAA(clip, ..., repair, repairc): host/sn_host_test drives sangnom::AAFilter with
SN_HOST_TEST_REPAIR=rank,chroma, synchronously ("aa:1") and over the host ring ("aa:4"), without dh and with dh and a
reduction.  The frames equal repair_model(source, the script's frame) (tests/repair_model.py, tests/repair_cases.py); the
constructor errors need no GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

from avisynth_sangnom2_amd import clip_format
from tests import repair_cases as rc
from tests.util import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "host", "sn_host_test")
RANK = 3


def _run(tmp_path, clip, kw, frames, repair, extra, reduce=0):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), "sn_host_test"])
    hdr = [clip.width, clip.height, clip.bytes, clip.bits, clip.planes, clip.subw, clip.subh, kw.get("order", 1), kw.get("aa", 48), kw.get("aac", 0),
           int(kw.get("dh", False)), 1, 1, len(frames)]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<14i", *hdr))
        for fr in frames:
            f.write(struct.pack("<i", 1))
            for pl in fr:
                f.write(np.ascontiguousarray(pl).tobytes())
    env = dict(os.environ, SN_HOST_TEST_SWEEPS="1", SN_HOST_TEST_REPAIR=repair)
    if reduce:
        env["SN_HOST_TEST_REDUCE"] = str(reduce)
    r = subprocess.run([BIN, fin, fout, extra], capture_output=True, text=True, timeout=300, env=env)
    return r, fout


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["reduce", "plain"])
@pytest.mark.parametrize("how", ["aa:4", "aa:1"])
@pytest.mark.parametrize("i,chroma", [(0, 0), (1, 1), (1, 0)], ids=["Y8", "YUV420P8-chroma", "YUV420P8-luma"])
def test_repaired_frames_equal_the_model(tmp_path, i, chroma, how, form):
    fmt, w, h, kw = rc.HOST[i]
    clip = clip_format(fmt, w, h)
    frames, _, plain, want = rc.expected((fmt, w, h, kw, {}, {}, None), "halfband" if form == "reduce" else None, RANK, bool(chroma), count=7)
    frames, plain, want = frames[:5], plain[:5], want[:5]
    r, fout = _run(tmp_path, clip, dict(kw, dh=form == "reduce"), frames, f"{RANK},{chroma}", how, reduce=2 if form == "reduce" else 0)
    assert r.returncode == 0, (r.stdout, r.stderr)
    raw = np.fromfile(fout, dtype=np.uint8)
    pos = 0
    for f in range(len(frames)):
        for p, wpl in enumerate(want[f]):
            got = raw[pos:pos + wpl.nbytes].view(wpl.dtype).reshape(wpl.shape)
            pos += wpl.nbytes
            assert same(wpl, got), f"{fmt} {how} frame {f} plane {p}"
            assert same(wpl, plain[f][p]) == (p > 0 and not chroma)  # a plane that is not repaired is the script's, every other one is not
    assert pos == raw.size, "the frames are not of source size"


@pytest.mark.parametrize("repair,kw,message", [
    ("2,0", dict(dh=True), "SangNomAA: repair needs the frame at source size (dh=false, or dh=true with reduce)"),
    ("5,0", {}, "SangNomAA: sn_aa_repair.rank must be 0 (off) or 1..4"),
    ("-1,1", {}, "SangNomAA: sn_aa_repair.rank must be 0 (off) or 1..4"),
])
def test_a_bad_repair_is_a_constructor_error(tmp_path, repair, kw, message):
    """Checked before any device is touched, so this runs without a GPU."""
    r, _ = _run(tmp_path, clip_format("Y8", 128, 64), kw, [], repair, "aa")
    assert r.returncode == 3 and r.stdout.strip() == message, (r.returncode, r.stdout, r.stderr)
