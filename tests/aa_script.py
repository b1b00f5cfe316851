"""The anti-aliasing script TurnLeft().SangNom2(...).TurnRight().SangNom2(...) from the reference's semantics: two filter
instances (one for the turned clip, one for the clip) around numpy.rot90, kept alive across frames.  opt=1 uses the SSE2
model (tests/sse2_model.py); `fresh` a new instance per plane and frame, `isolated` one instance per plane."""
import numpy as np

from avisynth_sangnom2_amd import ClipFormat
from oracle.oracle import Oracle
from tests import sse2_model as sm
from tests.util import oracle_cfg


def turned_clip(clip):
    return ClipFormat(width=clip.height, height=clip.width, bytes=clip.bytes, bits=clip.bits, planes=clip.planes, subw=clip.subh, subh=clip.subw)


class _Pass:
    """One SangNom2 instance of the script (or one per plane / per plane and frame)."""

    def __init__(self, clip, kw, opt, isolated, fresh):
        self.clip, self.kw, self.opt, self.isolated, self.fresh = clip, kw, opt, isolated or fresh, fresh
        self.inst = {}

    def _make(self, clip, kw):
        if self.opt == 1:
            m = sm.model_for(1, clip.width, clip.height, bytes=clip.bytes, bits=clip.bits, planes=clip.planes, subw=clip.subw, subh=clip.subh,
                             order=kw.get("order", 1), aa=kw.get("aa", 48), aac=kw.get("aac", 0), luma=kw.get("luma", True),
                             chroma=kw.get("chroma", True))
            return lambda planes, parity: m.get_frame(planes, parity=parity)
        o = Oracle(oracle_cfg(clip, **kw))
        return lambda planes, parity: o.process(planes, parity=parity)

    def run(self, planes, parity):
        if not self.isolated:
            if None not in self.inst:
                self.inst[None] = self._make(self.clip, self.kw)
            return self.inst[None](planes, parity)
        out = []
        for p, pl in enumerate(planes):
            on = self.kw.get("luma", True) if p == 0 else self.kw.get("chroma", True)
            if not on:
                out.append(pl.copy())
                continue
            if self.fresh or p not in self.inst:
                y = ClipFormat(width=pl.shape[1], height=pl.shape[0], bytes=self.clip.bytes, bits=self.clip.bits)
                self.inst[p] = self._make(y, dict(order=self.kw.get("order", 1), aa=self.kw.get("aa", 48) if p == 0 else self.kw.get("aac", 0)))
            out.append(self.inst[p]([pl], parity)[0])
        return out


class Script:
    def __init__(self, clip, opt=0, isolated=False, fresh=False, **kw):
        self.first = _Pass(turned_clip(clip), kw, opt, isolated, fresh)
        self.second = _Pass(clip, kw, opt, isolated, fresh)

    def frame(self, planes, parity=1):
        a = self.first.run([np.ascontiguousarray(np.rot90(pl, k=1)) for pl in planes], parity)
        return self.second.run([np.ascontiguousarray(np.rot90(pl, k=-1)) for pl in a], parity)
