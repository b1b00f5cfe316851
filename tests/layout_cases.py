"""Device planes as callers lay them out (tests/test_device_layouts_gpu.py runs them on the device,
tests/test_device_layouts_cpu.py checks the helpers themselves).  TEST INFRASTRUCTURE ONLY.

A plane of a batch lives inside ONE allocation of bytes: frame f's row y starts at base + f * stride + y * pitch and is `row`
bytes long.  Every byte of the allocation that belongs to no row is padding: source padding is filled with 0xFF (255, 65535,
a NaN in float), destination padding with 0x5C, and after a launch the destination's padding must still be 0x5C, the source
allocation what was uploaded, and every plane the oracle's.  Two layouts, per plane p (B bytes per sample, row = w_p * B,
rows of that plane):

  odd8   base 8; pitch row + 8 + 16 p (8 mod 16 wherever the row is a multiple of 16, U's and V's differ); frame stride
         (rows + 3) * pitch (8 mod 16 with it: rows is even) -- everything 8-byte aligned and nothing 16-byte aligned
  lines  what a frame server hands over: base 64; pitch roundup(row, 64) + 64 (1 + p); frame stride (rows + 2) * pitch

A case runs in both ARRANGEMENTS, source in one layout and destination in the other, so the two sides never agree on a pitch
or a frame stride; in the first every source pitch is below its destination pitch.  All offsets are relative to the start
of the allocation, which the device tests assert to be 256-byte aligned.
"""
from dataclasses import dataclass, field

import numpy as np

from avisynth_sangnom2_amd import clip_format, synth
from tests.util import describe_diff, oracle_cfg, same

FILL_SRC, FILL_DST = 0xFF, 0x5C
LAYOUTS = ("odd8", "lines")
ARRANGEMENTS = (("odd8", "lines"), ("lines", "odd8"))  # (source layout, destination layout)
NFRAMES, PARITIES = 3, (1, 0, 1)  # an odd count: the last frame of a workgroup's group of frames is a repeated one
PATTERNS = ("noise", "edges")
Y_OF = {(1, 8): "Y8", (2, 10): "Y10", (2, 16): "Y16", (4, 32): "Y32"}
VIEW_DTYPE = {1: np.uint8, 2: np.int16, 4: np.float32}  # torch has no uint16: same bits as int16


@dataclass(frozen=True)
class PlaneLayout:
    """Where the n frames of one plane lie inside their allocation; everything in bytes but rows, n and B."""
    name: str
    base: int
    pitch: int
    stride: int
    row: int
    rows: int
    n: int
    B: int

    @property
    def nbytes(self):  # the last frame has its full stride: whatever follows its rows is padding like any other
        return self.base + self.n * self.stride

    @property
    def w(self):
        return self.row // self.B


def plane_layout(name, p, w, rows, B, n):
    row = w * B
    if name == "odd8":
        pitch = row + 8 + 16 * p
        return PlaneLayout(name, 8, pitch, (rows + 3) * pitch, row, rows, n, B)
    if name == "lines":
        pitch = (row + 63) // 64 * 64 + 64 * (1 + p)
        return PlaneLayout(name, 64, pitch, (rows + 2) * pitch, row, rows, n, B)
    raise ValueError(name)


def batch_layout(name, shapes, B, n):
    """shapes: (rows, w) per plane, as SangNom2.plane_shape_in / plane_shape_out give them."""
    return [plane_layout(name, p, w, rows, B, n) for p, (rows, w) in enumerate(shapes)]


def fused_layout_ok(src, dst):
    """sn_fused_select.hip's alignment condition on one plane (the size limit is far away from every case here)."""
    return all(v % 8 == 0 for L in (src, dst) for v in (L.base, L.pitch, L.stride))


def view(alloc, L, dtype):
    """The frames of a plane inside its allocation (a numpy array of bytes) as an [n, rows, w] view."""
    assert alloc.dtype == np.uint8 and alloc.ndim == 1 and alloc.size == L.nbytes and np.dtype(dtype).itemsize == L.B
    return np.ndarray((L.n, L.rows, L.w), dtype=dtype, buffer=alloc.data, offset=L.base, strides=(L.stride, L.pitch, L.B))


def source_batch(layouts, frames, dtype):
    """Per plane an allocation of 0xFF bytes with the frames' planes copied into the views."""
    out = []
    for p, L in enumerate(layouts):
        a = np.full(L.nbytes, FILL_SRC, dtype=np.uint8)
        v = view(a, L, dtype)
        for f, fr in enumerate(frames):
            v[f] = fr[p]
        out.append(a)
    return out


def destination_batch(layouts):
    return [np.full(L.nbytes, FILL_DST, dtype=np.uint8) for L in layouts]


def outside_mask(L):
    """True for every byte of the allocation that belongs to no row of no frame."""
    m = np.ones(L.nbytes, dtype=bool)
    v = np.ndarray((L.n, L.rows, L.row), dtype=bool, buffer=m.data, offset=L.base, strides=(L.stride, L.pitch, 1))
    v[...] = False
    return m


def where_is(L, off):
    """What the byte at `off` of the allocation is, in words (for the checker's reports)."""
    if off < L.base:
        return f"byte {off}: {L.base - off} before the base"
    f, r = divmod(off - L.base, L.stride)
    y, x = divmod(r, L.pitch)
    if f >= L.n:
        return f"byte {off}: behind the last frame's stride"
    if y >= L.rows:
        return f"byte {off}: between frames {f} and {f + 1}, {y - L.rows} pitches and {x} bytes behind frame {f}'s last row"
    if x >= L.row:
        return f"byte {off}: {x - L.row} right of row {y} of frame {f}"
    return f"byte {off}: column byte {x} of row {y} of frame {f}"


def problems(dst_allocs, dst_layouts, want, dtype, src_after=None, src_uploaded=None, limit=4):
    """What is wrong with a finished launch, as a list of lines (empty: nothing).  want[f][p]: the expected planes."""
    out = []
    for p, (a, L) in enumerate(zip(dst_allocs, dst_layouts)):
        got = view(a, L, VIEW_DTYPE[L.B]).view(dtype)
        for f in range(L.n):
            if not same(want[f][p], got[f]):
                out.append(f"frame {f} plane {p}: " + describe_diff(want[f][p], got[f]))
        bad = np.flatnonzero((a != FILL_DST) & outside_mask(L))
        for off in bad[:limit]:
            out.append(f"plane {p} destination padding written (0x{a[off]:02x}): " + where_is(L, int(off)))
        if len(bad) > limit:
            out.append(f"plane {p} destination padding: {len(bad)} bytes written in all")
    if src_after is not None:
        for p, (a, b) in enumerate(zip(src_after, src_uploaded)):
            bad = np.flatnonzero(a != b)
            if len(bad):
                out.append(f"plane {p} source allocation changed in {len(bad)} bytes, first at {int(bad[0])}")
    return out


def assert_clean(what, *a, **kw):
    found = problems(*a, **kw)
    assert not found, what + ": " + "; ".join(found)


# ---- the case matrix ------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Case:
    """One configuration: fmt w x h, the filter's arguments kw, the context's ckw, and the path it is meant to reach."""
    path: str
    fmt: str
    w: int
    h: int
    kw: dict = field(default_factory=dict)
    ckw: dict = field(default_factory=dict)
    n: int = NFRAMES
    patterns: tuple = PATTERNS
    parts: int = 0       # > 0: debug_set_column_parts(parts, 0)
    fused: bool = True   # False: a width the sweeps do not take (only the sample-size alignment matters)

    @property
    def id(self):
        opts = "".join(f"-{k}{int(v)}" for k, v in {**self.kw, **self.ckw}.items())
        return f"{self.path}-{self.fmt}-{self.w}x{self.h}{opts}" + (f"-parts{self.parts}" if self.parts else "")

    @property
    def parities(self):
        return tuple((f + 1) & 1 for f in range(self.n))  # 1, 0, 1, ...


C = Case
U8 = [C("u8", "Y8", 32, 8), C("u8", "Y8", 544, 24, dict(order=2)), C("u8", "Y8", 4096, 16), C("u8", "Y8", 64, 16, dict(dh=True, order=0))]
COUPLED8 = [C("coupled8", "YUV420P8", 128, 40, dict(aac=48), dict(chroma_sweeps=1))]
UV = [C("uv", "YUV420P8", 256, 64, dict(aac=48)), C("uv", "YUV420P8", 640, 32, dict(aac=48)), C("uv", "YUV422P8", 256, 32),
      C("uv", "YUV420P8", 256, 64, dict(aac=48, dh=True))]
U16 = [C("u16", "Y16", 64, 24), C("u16", "Y10", 544, 24, dict(aa=20)), C("u16", "Y16", 64, 16, dict(dh=True)),
       C("u16", "YUV420P16", 128, 40, dict(aac=48)), C("u16", "YUV444P16", 64, 24)]
F32 = [C("f32", "Y32", 64, 24), C("f32", "Y32", 544, 24, dict(order=2)), C("f32", "YUV420PS", 128, 40, dict(aac=48)),
       C("f32", "YUV444PS", 64, 24, dict(dh=True))]
PADDED = [C("padded", "Y8", 104, 24, {}, dict(fresh_pool=True)), C("padded", "YUV420P8", 208, 40, dict(aac=48), dict(fresh_pool=True)),
          C("padded", "Y16", 104, 24, {}, dict(fresh_pool=True)), C("padded", "Y32", 104, 24, {}, dict(fresh_pool=True))]
ISOLATED = [C("isolated", "YUV420P8", 128, 40, dict(aac=48), dict(isolated_planes=True))]
BANDS = [C("bands", "Y8", 480, 200, n=2), C("bands", "Y16", 480, 200, n=2), C("bands", "YUV420P8", 960, 320, n=2)]
PARTS = [C("parts", fmt, 512, 64, {}, dict(column_parts=1), parts=k) for fmt in ("Y16", "Y32") for k in (2, 3)] + \
        [C("parts", "Y16", 3872, 32, {}, dict(column_parts=1))]
SSE2 = [C("sse2", "Y8", 64, 24, {}, dict(opt=1, sse2_sweeps=1), patterns=("noise01",)),
        C("sse2", "YUV420P8", 256, 64, {}, dict(opt=1, sse2_sweeps=1), patterns=("noise01",))]
# the pool kernels of a clip the sweeps would take; two history-carrying clips (one oracle instance through all four frames:
# neither has every processed plane a multiple of 8 wide, so their frames go one at a time); and one whose frames run as a
# chain of passes (sn_info.chained_frames)
POOL = [C("pool", "YUV420P8", 96, 32, dict(aac=48)), C("history", "Y8", 100, 40, n=4, fused=False),
        C("history", "YUV420P8", 104, 40, dict(aac=48), n=4, fused=False), C("chain", "YUV420P8", 112, 40, dict(aac=48), n=4, fused=False)]
SWEEPS = U8 + COUPLED8 + UV + U16 + F32 + PADDED + ISOLATED + PARTS + SSE2
ALL = SWEEPS + BANDS + POOL

TURNS = [("Y8", 200, 136), ("Y16", 70, 34), ("Y32", 64, 32)]


def shapes_of(clip, dh=False):
    """((rows, w) per plane of the source, ... of the destination), as SangNom2.plane_shape_in / plane_shape_out."""
    src = [(clip.height >> (clip.subh if p else 0), clip.width >> (clip.subw if p else 0)) for p in range(min(clip.planes, 3))]
    return src, [(2 * r if dh else r, w) for r, w in src]


def layouts_of(case, arrangement):
    """(source layouts, destination layouts) of a case in one arrangement."""
    clip = clip_format(case.fmt, case.w, case.h)
    s, d = shapes_of(clip, bool(case.kw.get("dh")))
    return batch_layout(arrangement[0], s, clip.bytes, case.n), batch_layout(arrangement[1], d, clip.bytes, case.n)


_cache = {}


def expected(case, pattern, seed0=500):
    """(clip, frames, the expected frames) of a case on one pattern, computed once per session and left unchanged: one oracle
    instance through all frames; isolated_planes: one per plane; fresh_pool: a new one per plane and frame; opt=1: the model
    of the reference's SSE2 arithmetic (tests/sse2_sweep_cases.py, which also asserts that the default arithmetic differs)."""
    key = (case.id, pattern)
    if key in _cache:
        return _cache[key]
    clip = clip_format(case.fmt, case.w, case.h)
    if case.ckw.get("opt") == 1:
        from tests import sse2_sweep_cases as sc
        _, frames, _, want = sc.expected(case.fmt, case.w, case.h, case.kw, {}, case.n, pattern, case.parities, seed0)
        _cache[key] = (clip, frames, want)
        return _cache[key]
    from oracle.oracle import Oracle
    frames = [synth.frame(clip, pattern, seed=seed0 + i) for i in range(case.n)]
    isolated, fresh = bool(case.ckw.get("isolated_planes")), bool(case.ckw.get("fresh_pool"))
    if isolated or fresh:
        def plane_oracle(p):
            pc = clip_format(Y_OF[(clip.bytes, clip.bits)], clip.width >> (clip.subw if p else 0), clip.height >> (clip.subh if p else 0))
            k = {x: y for x, y in case.kw.items() if x != "aac"}
            k["aa"] = case.kw.get("aa", 48) if p == 0 else case.kw.get("aac", 0)
            return Oracle(oracle_cfg(pc, **k))
        keep = {}
        want = []
        for fr, par in zip(frames, case.parities):
            planes = []
            for p in range(clip.planes):
                if fresh or p not in keep:
                    keep[p] = plane_oracle(p)
                planes.append(keep[p].process([fr[p]], parity=par)[0])
            want.append(planes)
    else:
        ora = Oracle(oracle_cfg(clip, **case.kw))
        want = [ora.process(fr, parity=par) for fr, par in zip(frames, case.parities)]
    for fr in want:
        for pl in fr:
            pl.setflags(write=False)
    _cache[key] = (clip, frames, want)
    return _cache[key]
