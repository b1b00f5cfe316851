"""SangNomAA(dh=true) of the plugin (sangnom::AAFilter with Args::dh), with and without look-ahead, driven through
host/sn_host_test the way a script engine drives it, against the script
TurnLeft().SangNom2(dh=true).TurnRight().SangNom2(dh=true) from the reference's semantics: frames twice as wide and
twice as high come back, written with the filter's own clip info."""
import os
import struct
import subprocess

import numpy as np
import pytest

from avisynth_sangnom2_amd import clip_format, synth
from tests.aa_dh_script import Script
from tests.util import same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "host", "sn_host_test")


def _run(tmp_path, clip, kw, frames, extra, fresh=False):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), "sn_host_test"])
    hdr = [clip.width, clip.height, clip.bytes, clip.bits, clip.planes, clip.subw, clip.subh, kw.get("order", 1), kw.get("aa", 48),
           kw.get("aac", 0), 1, 1, 1, len(frames)]  # the dh word is set
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<14i", *hdr))
        for fr in frames:
            f.write(struct.pack("<i", 1))
            for pl in fr:
                f.write(np.ascontiguousarray(pl).tobytes())
    env = dict(os.environ, SN_HOST_TEST_SWEEPS="1")
    if fresh:
        env["SN_HOST_TEST_FRESH"] = "1"
    r = subprocess.run([BIN, fin, fout, *[str(x) for x in extra]], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout, r.stderr)
    return np.fromfile(fout, dtype=np.uint8)


def _check(raw, wants, what):
    pos = 0
    for i, want in enumerate(wants):
        for p, wpl in enumerate(want):
            assert pos + wpl.nbytes <= raw.size, f"{what} request {i} plane {p}: the output file ends after {raw.size} bytes"
            got = raw[pos:pos + wpl.nbytes].view(wpl.dtype).reshape(wpl.shape)
            pos += wpl.nbytes
            assert same(wpl, got), f"{what} request {i} plane {p}"
    assert pos == raw.size


@pytest.mark.parametrize("la", [4, 1])
@pytest.mark.parametrize("fmt,w,h,kw,fresh", [("Y8", 128, 64, {}, False), ("YUV420P8", 128, 64, dict(aac=48), False), ("Y8", 96, 80, {}, True)],
                         ids=["y8", "yuv420p8", "y8-96x80-fresh"])
def test_enlargement_matches_the_script(tmp_path, fmt, w, h, kw, fresh, la):
    clip = clip_format(fmt, w, h)
    frames = [synth.frame(clip, "noise", seed=210 + i) for i in range(7)]
    script = Script(clip, fresh=fresh, **kw)
    want = [script.frame(fr) for fr in frames]
    assert want[0][0].shape == (2 * h, 2 * w)
    _check(_run(tmp_path, clip, kw, frames, [f"aa:{la}"], fresh=fresh), want, f"{fmt} aa:{la} dh")


@pytest.mark.parametrize("la", [4, 1])
def test_alpha_fills_a_block_of_two_by_two(tmp_path, la):
    w, h = 128, 64
    clip = clip_format("YUV420P8", w, h)
    rng = np.random.default_rng(3)
    frames = []
    for i in range(4):
        frames.append(list(synth.frame(clip, "noise", seed=270 + i)) + [rng.integers(0, 256, (h, w), dtype=np.uint8)])
    yuva = clip_format("YUV420P8", w, h)
    yuva.planes = 4
    script = Script(clip, aac=48)
    want = [script.frame(fr[:3]) + [np.repeat(np.repeat(fr[3], 2, axis=0), 2, axis=1)] for fr in frames]
    _check(_run(tmp_path, yuva, dict(aac=48), frames, [f"aa:{la}"]), want, f"yuva aa:{la} dh")
