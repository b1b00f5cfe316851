"""The C++ host-side adapter (host/sangnom2_filter.hpp) with Args::column_parts: sangnom::Filter passes it on as
sn_options.column_parts, and GetFrame of a 16-bit clip wider than one workgroup of the sweeps gives the oracle's frame.  The
test program asks for the whole-plane sweeps (SN_HOST_TEST_SWEEPS), so the single frame runs in column parts and not on the
pool path; `$SANGNOM_COLUMN_PARTS` reaches the same field."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import column_parts_cases as cc
from tests.util import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "host", "sn_host_test")


def _run(tmp_path, clip, frames, parities, extra=(), env=None):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), "sn_host_test"])
    hdr = [clip.width, clip.height, clip.bytes, clip.bits, clip.planes, clip.subw, clip.subh, 1, 48, 0, 0, 1, 1, len(frames)]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<14i", *hdr))
        for fr, par in zip(frames, parities):
            f.write(struct.pack("<i", par))
            for pl in fr:
                f.write(np.ascontiguousarray(pl).tobytes())
    r = subprocess.run([BIN, fin, fout, *[str(x) for x in extra]], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, SN_HOST_TEST_SWEEPS="1", **(env or {})))
    return r, fout


def test_a_bad_value_is_refused_by_the_library(tmp_path):
    """Validation happens before any device is touched, so this runs without a GPU."""
    fmt, w, h = cc.WIDE_Y16
    clip, frames, _ = cc.expected(fmt, w, h, {}, {}, ("noise",), parities=(1,))
    r, _ = _run(tmp_path, clip, [], [], env=dict(SANGNOM_COLUMN_PARTS="2"))
    assert r.returncode == 3 and "sn_options.column_parts" in r.stdout, (r.returncode, r.stdout, r.stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["argument", "environment"])
def test_getframe_of_a_wide_clip_in_column_parts(tmp_path, how):
    fmt, w, h = cc.WIDE_Y16
    clip, frames, want = cc.expected(fmt, w, h, {}, {}, ("noise",), parities=(1,))
    r, fout = _run(tmp_path, clip, frames, (1,), extra=("parts",) if how == "argument" else (),
                   env=dict(SANGNOM_COLUMN_PARTS="1") if how == "environment" else None)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = np.fromfile(fout, dtype=clip.dtype).reshape(want[0][0].shape)
    assert same(want[0][0], got)
