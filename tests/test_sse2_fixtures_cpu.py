"""CPU tests of the reference-written fixtures (tests/golden/sse2_*.npz, SSE2_FIXTURES.md) and of the numpy model of
the SSE2 arithmetic mode (tests/sse2_model.py).  No GPU.

* the model reproduces every opt=1 output of the reference bit for bit (pool history across frames included);
* the existing numpy oracle reproduces every opt=0 output bit for bit: the first reference-written pin of opt=0;
* no fixture tests nothing: where the two paths can differ, the reference's two outputs differ in every plane.
"""
import numpy as np
import pytest

from oracle.sangnom_numpy import NumpySangNom
from tests import sse2_model as sm
from tests.util import describe_diff, same

NAMES = sm.fixture_names()


def test_the_fixture_set_is_complete():
    fmts = {}
    for n in NAMES:
        meta = sm.load_fixture(n)[0]
        fmts.setdefault(meta["fmt"], []).append(meta)
    assert {"Y8", "Y10", "Y16", "YUV420P8", "YUV420P16", "YUV444PS"} <= set(fmts)
    y8 = fmts["Y8"]
    assert any(m["width"] == 64 and m["height"] == 32 and m["kw"]["order"] == 1 for m in y8)
    assert any(m["width"] == 100 and m["nframes"] == 3 for m in y8)
    assert any(m["kw"]["order"] == 0 and set(m["parity"]) == {0, 1} for m in y8)
    assert all(m["kw"]["aa"] == 48 and m["kw"]["aac"] == 48 for m in fmts["YUV420P8"])
    assert all(m["kw"]["dh"] for m in fmts["YUV444PS"])


@pytest.mark.parametrize("name", NAMES)
def test_model_reproduces_the_references_opt1_output(name):
    meta, frames, out1, _ = sm.load_fixture(name)
    m = sm.Sse2SangNom(meta["width"], meta["height"], **sm.model_kwargs(meta))
    for f, src in enumerate(frames):  # one instance, frames in order: the pool carries over
        got = m.get_frame(src, parity=meta["parity"][f])
        for p, (a, b) in enumerate(zip(got, out1[f])):
            assert same(a, b), f"{name} frame {f} plane {p}: " + describe_diff(a, b)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_references_opt0_output(name):
    meta, frames, _, out0 = sm.load_fixture(name)
    m = NumpySangNom(meta["width"], meta["height"], **sm.model_kwargs(meta))
    for f, src in enumerate(frames):
        got = m.get_frame(src, parity=meta["parity"][f])
        for p, (a, b) in enumerate(zip(got, out0[f])):
            assert same(a, b), f"{name} frame {f} plane {p}: " + describe_diff(a, b)


@pytest.mark.parametrize("name", NAMES)
def test_c_oracle_reproduces_the_references_opt0_output(name):
    """The C oracle (what the GPU suite compares the default mode with) against the same opt=0 outputs."""
    from oracle.oracle import Config, Oracle
    meta, frames, _, out0 = sm.load_fixture(name)
    kw = sm.model_kwargs(meta)
    ora = Oracle(Config(width=meta["width"], height=meta["height"], **kw))
    for f, src in enumerate(frames):
        got = ora.process(src, parity=meta["parity"][f])
        for p, (a, b) in enumerate(zip(got, out0[f])):
            assert same(a, b), f"{name} frame {f} plane {p}: " + describe_diff(a, b)


@pytest.mark.parametrize("name", NAMES)
def test_no_fixture_tests_nothing(name):
    meta, _, out1, out0 = sm.load_fixture(name)
    per_plane = [sum(int((out1[f][p].view(np.uint8) != out0[f][p].view(np.uint8)).sum()) for f in range(meta["nframes"]))
                 for p in range(meta["planes"])]
    if meta["bytes"] == 4:  # float: the reference's two paths are the same arithmetic
        assert per_plane == [0] * meta["planes"]
        assert not meta["expect_diff"]
    elif meta["bits"] in (8, 16):
        assert meta["expect_diff"] and all(v > 0 for v in per_plane), per_plane
    else:  # 9..15 bits: only a negative SangNom sum can differ, and rarely does (SSE2_FIXTURES.md)
        assert (sum(per_plane) > 0) == meta["expect_diff"]
    assert per_plane == meta["differing_per_plane"]


def test_the_set_exercises_both_deltas():
    total = dict(sg_negative=0, sg_above=0, box_above=0)
    for name in NAMES:
        meta, frames, _, _ = sm.load_fixture(name)
        m = sm.Sse2SangNom(meta["width"], meta["height"], **sm.model_kwargs(meta))
        for f, src in enumerate(frames):
            m.get_frame(src, parity=meta["parity"][f])
        for k in total:
            total[k] += m.events[k]
    assert all(v > 0 for v in total.values()), total


def test_known_answers():
    """Known answers that follow from the reference's text, through the helpers the model computes with, through the model
    and the oracle themselves, and through a whole plane."""
    # the SangNom value s = 4 p1 + 5 p2 - p3
    assert int(sm.sg_cxx(0, 0, 255)) == 224 and int(sm.sg_sse2(0, 0, 255)) == 255        # s = -255
    assert int(sm.sg_cxx(255, 255, 0)) == 30 and int(sm.sg_sse2(255, 255, 0)) == 255      # s >> 3 = 286
    assert int(sm.sg_sse2(10, 20, 30)) == int(sm.sg_cxx(10, 20, 30)) == 13                # in range: the same
    assert int(sm.sg_cxx(0, 0, 65535, 2)) == 57344 and int(sm.sg_sse2(0, 0, 65535, 2)) == 65535
    assert int(sm.sg_sse2(0, 0, 1023, 2)) == 65535   # MAXT is the container's, whatever the bit depth
    # a box over seven three-row sums of 765
    assert int(sm.box_cxx(7 * 765)) == 78 and int(sm.box_sse2(7 * 765)) == 255
    assert int(sm.box_cxx(7 * 3 * 65535, 2)) == (7 * 3 * 65535 // 16) % 65536 and int(sm.box_sse2(7 * 3 * 65535, 2)) == 65535
    # the same through the classes
    m1, m0 = sm.Sse2SangNom(32, 8), NumpySangNom(32, 8)
    p1, p2, p3 = np.array([0, 255, 10]), np.array([0, 255, 20]), np.array([255, 0, 30])
    assert m1._sg(p1, p2, p3).tolist() == [255, 255, 13] and m0._sg(p1, p2, p3).tolist() == [224, 30, 13]
    assert m1.events == dict(sg_negative=1, sg_above=1, box_above=0)
    m16 = sm.Sse2SangNom(32, 8, bytes=2, bits=10)
    assert m16._sg(np.array([0]), np.array([0]), np.array([1023])).tolist() == [65535]
    # ... and a plane whose kept lines alternate 0 / 255: every cost of the centre buffer is 255, so its pool row 1 is
    # (0 + 255 + 255) * 7 / 16 = 223 in both arithmetics and row 2 is (223 + 255 + 255) * 7 / 16 = 320: 255 saturated, 64 wrapped
    for m, row2 in ((sm.Sse2SangNom(32, 12), 255), (NumpySangNom(32, 12), 64)):
        src = np.zeros((12, 32), np.uint8)
        src[2::4] = 255  # order 1 keeps the even lines
        m.get_frame([src])
        assert int(m.pool[4, 1, 16]) == 223 and int(m.pool[4, 2, 16]) == row2
