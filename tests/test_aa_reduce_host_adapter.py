"""The plugin function SangNomAA(clip, ..., dh=true, reduce=1 | 2) as a drop-in anti-aliaser: host/sn_host_test drives
sangnom::AAFilter with SN_HOST_TEST_REDUCE, synchronously ("aa:1") and over the host ring ("aa:4").  The frames come back
at SOURCE size and equal the dh script reduced by tests/reduce_model.py; the alpha of a YUVA clip passes through 1:1."""
import os
import struct
import subprocess

import numpy as np
import pytest

from avisynth_sangnom2_amd import clip_format, synth
from tests.aa_dh_script import Script
from tests.reduce_model import reduce_model
from tests.util import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "host", "sn_host_test")
KERNEL = {1: "tent", 2: "halfband"}


def _run(tmp_path, clip, kw, frames, reduce, extra):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), "sn_host_test"])
    hdr = [clip.width, clip.height, clip.bytes, clip.bits, clip.planes, clip.subw, clip.subh, kw.get("order", 1), kw.get("aa", 48), kw.get("aac", 0),
           int(kw.get("dh", True)), 1, 1, len(frames)]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<14i", *hdr))
        for fr in frames:
            f.write(struct.pack("<i", 1))
            for pl in fr:
                f.write(np.ascontiguousarray(pl).tobytes())
    env = dict(os.environ, SN_HOST_TEST_SWEEPS="1", SN_HOST_TEST_REDUCE=str(reduce))
    r = subprocess.run([BIN, fin, fout, extra], capture_output=True, text=True, timeout=300, env=env)
    return r, fout


_WANT = {}  # format -> (frames, the dh script's frames): computed once, left unchanged


def _script_frames(fmt):
    if fmt not in _WANT:
        clip = clip_format(fmt, 128, 64)
        frames = [synth.frame(clip, "noise", seed=11 + i) for i in range(5)]
        script = Script(clip, aac=48)
        _WANT[fmt] = (frames, [script.frame(fr) for fr in frames])
    return _WANT[fmt]


@pytest.mark.gpu
@pytest.mark.parametrize("reduce", [1, 2])
@pytest.mark.parametrize("how", ["aa:4", "aa:1"])
@pytest.mark.parametrize("fmt", ["Y8", "YUV420P8"])
def test_frames_of_source_size_equal_the_model(tmp_path, fmt, how, reduce):
    clip = clip_format(fmt, 128, 64)
    frames, E = _script_frames(fmt)
    r, fout = _run(tmp_path, clip, dict(aac=48), frames, reduce, how)
    assert r.returncode == 0, (r.stdout, r.stderr)
    raw = np.fromfile(fout, dtype=np.uint8)
    pos = 0
    for f, fr in enumerate(frames):
        want = reduce_model(E[f], KERNEL[reduce])
        for p, wpl in enumerate(want):
            assert wpl.shape == fr[p].shape
            got = raw[pos:pos + wpl.nbytes].view(wpl.dtype).reshape(wpl.shape)
            pos += wpl.nbytes
            assert same(wpl, got), f"{fmt} {how} frame {f} plane {p}"
    assert pos == raw.size, "the frames are not of source size"


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["aa:4", "aa:1"])
def test_alpha_comes_back_unchanged(tmp_path, how):
    clip = clip_format("YUV420P8", 128, 64)
    frames, E = _script_frames("YUV420P8")
    rng = np.random.default_rng(12)
    alphas = [rng.integers(0, 256, (64, 128), dtype=np.uint8) for _ in frames]
    yuva = clip_format("YUV420P8", 128, 64)
    yuva.planes = 4
    r, fout = _run(tmp_path, yuva, dict(aac=48), [list(fr) + [al] for fr, al in zip(frames, alphas)], 1, how)
    assert r.returncode == 0, (r.stdout, r.stderr)
    raw = np.fromfile(fout, dtype=np.uint8)
    pos = 0
    for f in range(len(frames)):
        for p, wpl in enumerate(reduce_model(E[f], "tent") + [alphas[f]]):
            got = raw[pos:pos + wpl.nbytes].view(wpl.dtype).reshape(wpl.shape)
            pos += wpl.nbytes
            assert same(wpl, got), f"{how} frame {f} plane {p}"
    assert pos == raw.size


@pytest.mark.parametrize("reduce", [1, 2])
def test_reduce_without_dh_is_a_constructor_error(tmp_path, reduce):
    """Checked before any device is touched, so this runs without a GPU."""
    r, _ = _run(tmp_path, clip_format("Y8", 128, 64), dict(dh=False), [], reduce, "aa")
    assert r.returncode == 3 and r.stdout.strip() == "SangNomAA: reduce needs dh=true", (r.returncode, r.stdout, r.stderr)
