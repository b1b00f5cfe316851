"""Semi-planar device surfaces (NV12, P010 / P016, NV16, NV24): the case table and the expected frames of
tests/test_surfaces_gpu.py.  TEST INFRASTRUCTURE ONLY.

A semi-planar frame is [Y, UV] with UV[y, x] = (U[y, x], V[y, x]).  What the library has to give for such a surface is what
it gives for the planar frame, re-interleaved, so the expected frames come from the CPU oracle on the de-interleaved planes
(the SSE2 model for opt=1; tests/aa_script.py and tests/aa_dh_script.py for the anti-aliasing call) and numpy interleaves them.
Every case is a batch of frames with different content -- noise, edges, sine, then noise again -- from one oracle instance,
so history-carrying clips are checked across the frames of a call."""
from dataclasses import dataclass, field

import numpy as np

from avisynth_sangnom2_amd import clip_format, synth
from tests import layout_cases as lc
from tests.util import oracle_cfg

PATTERNS = ("noise", "edges", "sine", "noise")
SEED = 2100  # frame i: SEED + i


def interleave(u, v):
    """U and V [..., H, W] -> the UV plane as [..., H, W, 2]."""
    return np.ascontiguousarray(np.stack([u, v], axis=-1))


def uv_rows(u, v):
    """... as rows of 2 W samples: [..., H, 2 W]."""
    uv = interleave(u, v)
    return uv.reshape(uv.shape[:-2] + (2 * uv.shape[-2],))


def semi(frame):
    """A planar frame [Y, U, V] -> [Y, UV rows]."""
    return [frame[0], uv_rows(frame[1], frame[2])]


@dataclass(frozen=True)
class Case:
    """fmt w x h, the filter's arguments kw, the context's ckw; path: "sweep" (mode="fused", the counters must say so),
    "pool" (mode="pool") or "auto"."""
    fmt: str
    w: int
    h: int
    kw: dict = field(default_factory=dict)
    ckw: dict = field(default_factory=dict)
    n: int = 3
    pattern: str = ""      # one pattern for every frame instead of PATTERNS
    parities: tuple = ()   # () = all 1
    path: str = "auto"
    uv_sweep: bool = False  # U and V must have run as one sweep

    @property
    def id(self):
        opts = "".join(f"-{k}{int(v)}" for k, v in {**self.kw, **self.ckw}.items())
        return f"{self.fmt}-{self.w}x{self.h}{opts}" + (f"-n{self.n}" if self.n != 3 else "")

    @property
    def mode(self):
        return {"sweep": "fused", "pool": "pool", "auto": "auto"}[self.path]

    @property
    def par(self):
        return list(self.parities) if self.parities else [1] * self.n


C = Case
PARITY = [
    C("YUV420P8", 256, 64, dict(aac=48), path="sweep", uv_sweep=True),  # U and V as one sweep
    C("YUV420P8", 640, 32, dict(aac=48), path="sweep", uv_sweep=True),
    C("YUV422P8", 256, 32, path="sweep", uv_sweep=True),                # NV16
    C("YUV444P8", 64, 32),                                              # NV24
    C("YUV420P16", 256, 64, dict(aac=48), path="sweep"),                # P016: coupled 16-bit sweeps, low bits set
    C("YUV420P10", 256, 64, dict(aac=48), path="sweep"),
    C("YUV420P8", 96, 32, dict(aac=48), path="pool"),                   # chroma 48 wide
    C("YUV420P8", 100, 40, n=4),                                        # history-carrying; a UV row of 100 bytes: the ragged tail
    C("YUV420P8", 128, 40, {}, dict(isolated_planes=True), path="sweep"),
    C("YUV420P8", 208, 40, {}, dict(fresh_pool=True), path="sweep"),
    C("YUV420P8", 128, 24, dict(dh=True)),
    C("YUV420P16", 128, 32, dict(order=0), parities=(0, 1, 0)),
    C("YUV420P16", 128, 32, {}, dict(opt=1, sse2_sweeps=1), pattern="noise01"),
]
MIXED = [C("YUV420P8", 256, 64, dict(aac=48)), C("YUV420P16", 256, 64, dict(aac=48))]
LAYOUTS = [C("YUV420P8", 256, 64, dict(aac=48)), C("YUV420P8", 100, 40, n=4), C("YUV420P16", 256, 64, dict(aac=48))]
KEPT = [C("YUV420P8", 256, 64, dict(order=1)), C("YUV420P8", 256, 64, dict(order=2))]
COPIED = C("YUV420P8", 256, 64, dict(chroma=False))
CHROMA_ONLY = C("YUV420P8", 256, 64, dict(luma=False, aac=30), path="pool")
CHUNKED = C("YUV420P8", 100, 40, n=4)
AA = [(fmt, dh) for fmt in ("YUV420P8", "YUV420P16") for dh in (False, True)]  # 128 x 64
PLANAR = [C("Y8", 64, 32), C("YUV420P8", 256, 64)]


def frames_of(case):
    clip = clip_format(case.fmt, case.w, case.h)
    return clip, [synth.frame(clip, case.pattern or PATTERNS[i % len(PATTERNS)], seed=SEED + i) for i in range(case.n)]


_cache = {}


def expected(case):
    """(clip, planar frames, parities, the expected planar frames), computed once per session and left unchanged."""
    if case.id in _cache:
        return _cache[case.id]
    clip, frames = frames_of(case)
    isolated, fresh = bool(case.ckw.get("isolated_planes")), bool(case.ckw.get("fresh_pool"))
    if case.ckw.get("opt") == 1:
        from tests import sse2_sweep_cases as sc
        want = sc.want(clip, case.kw, frames, case.par, 1, isolated, fresh)
        assert sc.differs(want, sc.want(clip, case.kw, frames, case.par, 0, isolated, fresh)), "this case cannot tell the arithmetics apart"
    elif isolated or fresh:
        from oracle.oracle import Oracle
        keep, want = {}, []
        for fr, par in zip(frames, case.par):
            planes = []
            for p in range(clip.planes):
                if fresh or p not in keep:
                    pc = clip_format(lc.Y_OF[(clip.bytes, clip.bits)], clip.width >> (clip.subw if p else 0), clip.height >> (clip.subh if p else 0))
                    k = {x: y for x, y in case.kw.items() if x != "aac"}
                    k["aa"] = case.kw.get("aa", 48) if p == 0 else case.kw.get("aac", 0)
                    keep[p] = Oracle(oracle_cfg(pc, **k))
                planes.append(keep[p].process([fr[p]], parity=par)[0])
            want.append(planes)
    else:
        from oracle.oracle import Oracle
        ora = Oracle(oracle_cfg(clip, **case.kw))
        want = [ora.process(fr, parity=par) for fr, par in zip(frames, case.par)]
    for fr in list(want) + list(frames):
        for pl in fr:
            pl.setflags(write=False)
    _cache[case.id] = (clip, frames, case.par, want)
    return _cache[case.id]


def expected_aa(fmt, dh, n=3, w=128, h=64):
    """(clip, planar frames, the script's frames) of the anti-aliasing call on fmt 128 x 64, aac = 48."""
    key = ("aa", fmt, dh, n, w, h)
    if key not in _cache:
        from tests import aa_dh_script, aa_script
        clip = clip_format(fmt, w, h)
        frames = [synth.frame(clip, PATTERNS[i % len(PATTERNS)], seed=SEED + 50 + i) for i in range(n)]
        script = (aa_dh_script if dh else aa_script).Script(clip, aac=48)
        want = [script.frame(fr) for fr in frames]
        for fr in list(want) + list(frames):
            for pl in fr:
                pl.setflags(write=False)
        _cache[key] = (clip, frames, want)
    return _cache[key]


# ---- layouts as callers have them (the allocation and guard helpers are tests/layout_cases.py's) -------------------------------

def odd_layout(p, w, rows, B, n):
    """Nothing aligned beyond the sample size: base B (3 + 2 p) -- an odd byte for 8-bit samples, 2 mod 4 for 16-bit ones --,
    pitch row + B (5 + 2 p) -- odd / 2 mod 4 where the row is a multiple of 4 bytes --, and 7 samples of slack between frames."""
    row = w * B
    pitch = row + B * (5 + 2 * p)
    return lc.PlaneLayout("odd", B * (3 + 2 * p), pitch, (rows + 2) * pitch + 7 * B, row, rows, n, B)


SURFACE_LAYOUTS = ("odd", "lines")
ARRANGEMENTS = (("odd", "lines"), ("lines", "odd"))  # (source, destination); "lines" is 64-byte aligned: the 16-byte path


def surface_layouts(name, shapes, B, n):
    """Layouts of [Y, UV] for the planar shapes [(rows, w) of Y, of U]: the UV plane has 2 w samples per row."""
    (yr, yw), (cr, cw) = shapes[0], shapes[1]
    make = odd_layout if name == "odd" else (lambda p, w, rows, B, n: lc.plane_layout(name, p, w, rows, B, n))
    return [make(0, yw, yr, B, n), make(1, 2 * cw, cr, B, n)]


def scratch_frame_bytes(clip, dh=False):
    """Chroma scratch per frame, as include/sangnom_hip.h documents it: U and V in the source's and in the destination's chroma
    geometry, pitches rounded up to 256 bytes."""
    cw, ch = clip.width >> clip.subw, clip.height >> clip.subh
    pitch = (cw * clip.bytes + 255) // 256 * 256
    return 2 * (pitch * ch + pitch * (2 * ch if dh else ch))


def scratch_frame_bytes_aa(clip, dh):
    """... of the anti-aliasing call: with dh its destination is twice as wide and twice as high."""
    cw, ch = clip.width >> clip.subw, clip.height >> clip.subh
    k = 2 if dh else 1
    return 2 * ((cw * clip.bytes + 255) // 256 * 256 * ch + (k * cw * clip.bytes + 255) // 256 * 256 * k * ch)


def scratch_frames(clip, max_batch, budget_mb, dh=False):
    """Frames the scratch holds: min(max_batch, a sixteenth of the budget / one frame), at least one."""
    return max(1, min(max_batch, (budget_mb << 20) // 16 // scratch_frame_bytes(clip, dh)))
