"""The C++ host-side adapter (host/sangnom2_filter.hpp) with the script argument opt=1: sangnom::Filter passes it on as
SN_ARITH_SSE2, and GetFrame gives what the reference gives with opt=1 (tests/golden/sse2_*.npz, written by the reference
itself).  opt=0 and opt=-1 stay its C++ arithmetic."""
import os
import struct
import subprocess

import numpy as np
import pytest

from avisynth_sangnom2_amd import clip_format
from tests import sse2_model as sm
from tests.util import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "host", "sn_host_test")


def _run(tmp_path, meta, frames, opt, extra=()):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), "sn_host_test"])
    kw = meta["kw"]
    hdr = [meta["width"], meta["height"], meta["bytes"], meta["bits"], meta["planes"], meta["subw"], meta["subh"],
           kw["order"], kw["aa"], kw["aac"], int(kw["dh"]), 1, 1, len(frames)]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<14i", *hdr))
        for fr, par in zip(frames, meta["parity"]):
            f.write(struct.pack("<i", par))
            for pl in fr:
                f.write(np.ascontiguousarray(pl).tobytes())
    env = dict(os.environ, SN_HOST_TEST_OPT=str(opt))
    r = subprocess.run([BIN, fin, fout, *[str(x) for x in extra]], capture_output=True, text=True, timeout=300, env=env)
    return r, fout


def test_opt_out_of_range_carries_the_reference_text(tmp_path):
    """Validation happens before any device is touched, so this runs without a GPU."""
    meta, frames, _, _ = sm.load_fixture("sse2_y8_top")
    r, _ = _run(tmp_path, meta, [], 2)
    assert r.returncode == 3 and r.stdout.strip() == "SangNom2: opt must be between -1..2.", (r.returncode, r.stdout, r.stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sse2_y8_top", "sse2_y8_w100_3frames", "sse2_y8_order0", "sse2_y16", "sse2_yuv420p8", "sse2_yuv444ps_dh"])
@pytest.mark.parametrize("opt", [1, 0, -1])
def test_getframe_with_opt_matches_the_reference(tmp_path, name, opt):
    meta, frames, out1, out0 = sm.load_fixture(name)
    r, fout = _run(tmp_path, meta, frames, opt)
    assert r.returncode == 0, (r.stdout, r.stderr)
    raw = np.fromfile(fout, dtype=np.uint8)
    pos = 0
    for f, want in enumerate(out1 if opt == 1 else out0):
        for p, wpl in enumerate(want):
            got = raw[pos:pos + wpl.nbytes].view(wpl.dtype).reshape(wpl.shape)
            pos += wpl.nbytes
            assert same(wpl, got), f"{name} opt {opt} frame {f} plane {p}"
    assert pos == raw.size


@pytest.mark.gpu
def test_getframe_over_the_host_ring_with_opt_1(tmp_path):
    meta, frames, out1, _ = sm.load_fixture("sse2_yuv420p8")  # history-free: look-ahead applies
    r, fout = _run(tmp_path, meta, frames, 1, extra=(4,))
    assert r.returncode == 0, (r.stdout, r.stderr)
    raw = np.fromfile(fout, dtype=np.uint8)
    want = np.concatenate([pl.ravel().view(np.uint8) for fr in out1 for pl in fr])
    assert np.array_equal(raw, want)
