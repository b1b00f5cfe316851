"""The enlargement script TurnLeft().SangNom2(..., dh=true).TurnRight().SangNom2(..., dh=true) from the reference's
semantics: two filter instances with dh=True around numpy.rot90, kept alive across frames.  The first instance is made
for the turned clip (H wide, W high; 2W high out), the second for the clip turned back, 2W wide and H high, with the
clip's own chroma subsampling; its output is 2W x 2H.  dh forces every plane through both passes, so luma / chroma play
no part.  opt=1 uses the SSE2 model (tests/sse2_model.py); `fresh` a new instance per plane and frame, `isolated` one
instance per plane."""
import numpy as np

from avisynth_sangnom2_amd import ClipFormat
from oracle.oracle import Oracle
from tests import sse2_model as sm
from tests.aa_script import turned_clip
from tests.util import oracle_cfg


def widened_clip(clip):
    """The second pass's clip: the first pass's output turned back."""
    return ClipFormat(width=2 * clip.width, height=clip.height, bytes=clip.bytes, bits=clip.bits, planes=clip.planes, subw=clip.subw, subh=clip.subh)


class _Pass:
    """One SangNom2(dh=true) instance of the script (or one per plane / per plane and frame)."""

    def __init__(self, clip, kw, opt, isolated, fresh):
        self.clip, self.kw, self.opt, self.isolated, self.fresh = clip, kw, opt, isolated or fresh, fresh
        self.inst = {}

    def _make(self, clip, kw):
        if self.opt == 1:
            m = sm.model_for(1, clip.width, clip.height, bytes=clip.bytes, bits=clip.bits, planes=clip.planes, subw=clip.subw, subh=clip.subh,
                             order=kw.get("order", 1), aa=kw.get("aa", 48), aac=kw.get("aac", 0), luma=kw.get("luma", True),
                             chroma=kw.get("chroma", True), dh=True)
            return lambda planes, parity: m.get_frame(planes, parity=parity)
        o = Oracle(oracle_cfg(clip, **dict(kw, dh=True)))
        return lambda planes, parity: o.process(planes, parity=parity)

    def run(self, planes, parity):
        if not self.isolated:
            if None not in self.inst:
                self.inst[None] = self._make(self.clip, self.kw)
            return self.inst[None](planes, parity)
        out = []
        for p, pl in enumerate(planes):  # every plane: dh forces them
            if self.fresh or p not in self.inst:
                y = ClipFormat(width=pl.shape[1], height=pl.shape[0], bytes=self.clip.bytes, bits=self.clip.bits)
                self.inst[p] = self._make(y, dict(order=self.kw.get("order", 1), aa=self.kw.get("aa", 48) if p == 0 else self.kw.get("aac", 0)))
            out.append(self.inst[p]([pl], parity)[0])
        return out


class Script:
    def __init__(self, clip, opt=0, isolated=False, fresh=False, **kw):
        self.first = _Pass(turned_clip(clip), kw, opt, isolated, fresh)
        self.second = _Pass(widened_clip(clip), kw, opt, isolated, fresh)

    def frame(self, planes, parity=1):
        a = self.first.run([np.ascontiguousarray(np.rot90(pl, k=1)) for pl in planes], parity)
        return self.second.run([np.ascontiguousarray(np.rot90(pl, k=-1)) for pl in a], parity)


def kept_offset(order, parity):
    """Where the source samples reappear: dst[off::2, (1 - off)::2] (order 1 / 2: off = 0 / 1; order 0: from the parity)."""
    return order - 1 if order else (0 if parity else 1)
