"""Numpy model of the SSE2 arithmetic mode (SN_ARITH_SSE2: the reference's opt=1 / default path).  TEST INFRASTRUCTURE ONLY.

The reference's SSE2 path computes the same pixels as its C++ path (opt=0, oracle/sangnom_numpy.py) except in two
narrowing steps of the 8-bit and 9..16-bit code, where it saturates to the container (MAXT = 255 / 65535, whatever the
bit depth) and the C++ path wraps modulo 2^(8 * sizeof T):

1. the SangNom value  s = 4 p1 + 5 p2 - p3:  MAXT when s < 0, else min(s >> 3, MAXT)   (a logical shift in a lane twice
   as wide, then an unsigned-saturating pack); used by stage 1 and again by stage 3;
2. the box of stage 2:  min(sum >> 4, MAXT).

Float is the same in both paths.  sg_sse2 / box_sse2 below are those two steps, and the class overrides
oracle/sangnom_numpy.py with them (sg_cxx / box_cxx restate what the oracle does, for the known answers); the box narrowing
is inline in NumpySangNom._plane, so that method is restated here.  `events` counts, per instance, how often each of the
three ways the two paths can part was met (tests use it to show that a case exercises the mode).
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.sangnom_numpy import F32, NumpySangNom  # noqa: E402


def sg_cxx(p1, p2, p3, bytes=1):
    """SangNom value of the C++ path for integer samples."""
    return ((4 * p1 + 5 * p2 - p3) >> 3) % (1 << (8 * bytes))


def sg_sse2(p1, p2, p3, bytes=1):
    """SangNom value of the SSE2 path for integer samples."""
    maxt = (1 << (8 * bytes)) - 1
    s = 4 * np.asarray(p1, dtype=np.int64) + 5 * np.asarray(p2, dtype=np.int64) - np.asarray(p3, dtype=np.int64)
    return np.where(s < 0, maxt, np.minimum(s >> 3, maxt))


def box_cxx(total, bytes=1):
    return (total // 16) % (1 << (8 * bytes))


def box_sse2(total, bytes=1):
    return np.minimum(np.asarray(total, dtype=np.int64) >> 4, (1 << (8 * bytes)) - 1)


class Sse2SangNom(NumpySangNom):
    """One filter instance of the reference run with opt=1 (zero-filled shared pool, frames in call order)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.events = dict(sg_negative=0, sg_above=0, box_above=0)

    def _sg(self, p1, p2, p3):
        if self.is_float:
            return super()._sg(p1, p2, p3)
        s = 4 * p1 + 5 * p2 - p3
        self.events["sg_negative"] += int((s < 0).sum())
        self.events["sg_above"] += int(((s >> 3) > self.M - 1).sum())
        return sg_sse2(p1, p2, p3, self.bytes)

    def _plane(self, dst, offset, plane):
        h, w = dst.shape
        wt = np.float32 if self.is_float else np.int64
        K = dst[offset::2].astype(wt)
        nr = h // 2 - 1
        P = self.pool
        for y in range(nr):  # stage 1
            tc, tn, f1, f2, b1, b2 = self._candidates(K[y], K[y + 1])
            d = [tc[-3] - tn[3], tc[-2] - tn[2], tc[-1] - tn[1], f1 - f2, tc[0] - tn[0],
                 b1 - b2, tc[1] - tn[-1], tc[2] - tn[-2], tc[3] - tn[-3]]
            for b in range(9):
                P[b, y + 1, :w] = np.abs(d[b])
        se = self.stride_e
        for b in range(9):  # stage 2: in place, top to bottom, the whole pool stride
            for r in range(1, self.bh):
                S = (P[b, r - 1] + P[b, r]) + P[b, r + 1]
                Sp = np.pad(S, 3, mode="edge")
                acc = Sp[0:se] + Sp[1:se + 1]
                for k in range(2, 7):
                    acc = acc + Sp[k:se + k]
                if self.is_float:
                    P[b, r] = acc / F32(16)
                else:
                    self.events["box_above"] += int(((acc >> 4) > self.M - 1).sum())
                    P[b, r] = box_sse2(acc, self.bytes)
        thr = self.thr[plane]
        out_rows = []
        for y in range(nr):  # stage 3
            tc, tn, f1, f2, b1, b2 = self._candidates(K[y], K[y + 1])
            v = P[:, y + 1, :w]
            m = v.min(axis=0)
            cands = [
                (5, self._avg(b1, b2)), (3, self._avg(f1, f2)),
                (6, self._avg(tc[1], tn[-1])), (2, self._avg(tc[-1], tn[1])),
                (7, self._avg(tc[2], tn[-2])), (1, self._avg(tc[-2], tn[2])),
                (8, self._avg(tc[3], tn[-3])), (0, self._avg(tc[-3], tn[3])),
            ]
            res = cands[-1][1].copy()
            for bidx, val in reversed(cands[:-1]):
                res = np.where(v[bidx] == m, val, res)
            res = np.where((v[4] == m) | (m > thr), self._avg(tc[0], tn[0]), res)
            out_rows.append(res)
        for y in range(nr):
            dst[offset + 2 * y + 1] = out_rows[y].astype(self.dtype)


def model_for(arithmetic, *a, **kw):
    """arithmetic 0: the opt=0 oracle, 1: the SSE2 model."""
    return (Sse2SangNom if arithmetic else NumpySangNom)(*a, **kw)


# ---- the reference-written fixtures (tests/golden/sse2_*.npz, SSE2_FIXTURES.md) ---------------------------------------
GOLDEN = os.path.join(ROOT, "tests", "golden")


def fixture_names():
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("sse2_") and f.endswith(".npz"))


def load_fixture(name):
    """-> (meta, frames, out1, out0): per frame a list of planes; meta: fmt, width, height, bytes, bits, planes, subw,
    subh, kw (order, aa, aac, dh), parity (per frame), pattern, seed0, expect_diff.  The opt=0 outputs are stored as
    `out_f*_p*`, the key the older fixtures use, so the existing golden-vector tests read these files too."""
    import json
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    n, p = meta["nframes"], meta["planes"]
    get = lambda key: [[z[f"{key}_f{f}_p{q}"] for q in range(p)] for f in range(n)]  # noqa: E731
    return meta, get("in"), get("out1"), get("out")


def model_kwargs(meta):
    return dict(bytes=meta["bytes"], bits=meta["bits"], planes=meta["planes"], subw=meta["subw"], subh=meta["subh"],
                order=meta["kw"]["order"], aa=meta["kw"]["aa"], aac=meta["kw"]["aac"], dh=bool(meta["kw"]["dh"]))
