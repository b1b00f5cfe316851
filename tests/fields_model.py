"""The both-fields anti-aliasing call (sangnom_hip.h, "Both fields") from its definition: avg per sample type, and the script
A(A(c.TurnLeft()).TurnRight()) with A(c) = avg(SangNom2(c, order=1), SangNom2(c, order=2)) -- four filter instances of
tests/aa_script._Pass (two for the turned clip, two for the clip, each with its own pool and history) around numpy.rot90."""
import numpy as np

from tests.aa_script import _Pass, turned_clip

NAN = np.uint32(0x7FC00000)


def merge_plane(a, b):
    """avg(a, b): integers (a + b + 1) >> 1 without overflow; float (a + b) * 0.5f in single precision, in that order, every NaN
    result as the one pattern 0x7FC00000."""
    assert a.dtype == b.dtype and a.shape == b.shape
    if a.dtype == np.float32:
        with np.errstate(all="ignore"):
            s = (a + b).astype(np.float32)
            r = (s * np.float32(0.5)).astype(np.float32)
        bits = r.view(np.uint32).copy()
        bits[np.isnan(r)] = NAN
        return bits.view(np.float32)
    return ((a.astype(np.uint32) + b.astype(np.uint32) + 1) >> 1).astype(a.dtype)


def processed_planes(planes, kw):
    return [bool(kw.get("luma", True))] + [bool(kw.get("chroma", True))] * (planes - 1)


class BothScript:
    """`order` among the keywords and the parity of a frame are accepted and have no influence: the twins are orders 1 and 2.
    A plane that is not processed is a copy of the source."""

    def __init__(self, clip, opt=0, isolated=False, fresh=False, **kw):
        kw = {k: v for k, v in kw.items() if k != "order"}
        self.proc = processed_planes(clip.planes, kw)
        self.first = [_Pass(turned_clip(clip), dict(kw, order=o), opt, isolated, fresh) for o in (1, 2)]
        self.second = [_Pass(clip, dict(kw, order=o), opt, isolated, fresh) for o in (1, 2)]
        self.last = None  # the two results of the last frame's second pass, for the tests that look at what the last average sees

    def _both(self, passes, planes):
        a, b = (p.run([pl.copy() for pl in planes], 1) for p in passes)
        return a, b, [merge_plane(x, y) if on else pl.copy() for x, y, pl, on in zip(a, b, planes, self.proc)]

    def frame(self, planes, parity=1):
        _, _, m1 = self._both(self.first, [np.ascontiguousarray(np.rot90(pl, k=1)) for pl in planes])
        a, b, out = self._both(self.second, [np.ascontiguousarray(np.rot90(pl, k=-1)) for pl in m1])
        self.last = (a, b)
        return out
