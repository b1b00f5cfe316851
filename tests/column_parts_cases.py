"""Shared inputs of the column-parts tests (sn_options.column_parts).  TEST INFRASTRUCTURE ONLY.

Two things live here:

  * the convergence check on the CPU: a plane is split at a seam, each side is cropped to a window that reaches `ghost`
    columns beyond the seam, and the windows run through an oracle as planes of their own -- which is what a column part is
    on the device.  `seam_check` says whether the two windows agree on the smoothed values of the 16 columns around the seam
    (what k_parts_verify compares), whether each window's own columns are exact, and how deep the wrong columns reach from
    each window's inner edge;
  * the case tables of tests/test_column_parts_gpu.py, and the expected frames (the C oracle, computed once).

Formats are (bytes, bits): 8-bit is here for the record only, the library cuts 16-bit and float planes.
"""
import numpy as np

from avisynth_sangnom2_amd import clip_format, synth
from oracle.oracle import Oracle
from oracle.sangnom_numpy import NumpySangNom
from tests.util import oracle_cfg

GHOST = {1: 64, 2: 64, 4: 96}  # the library's ghost per sample size (sn_route.h: kPartsGhost16 / kPartsGhost32); 8-bit: for the record
FORMATS = {"8-bit": (1, 8), "10-bit": (2, 10), "16-bit": (2, 16), "float": (4, 32)}
CONVERGING = ("noise", "sine", "edges", "checker")  # what the GPU tests feed where no frame may take the fallback
FIXED_POINT = "checker2"                            # never converges (8-bit, 16-bit, float): the natural fallback
SEED = 3          # synth.plane(..., seed=SEED) of the CPU check
CPU_SHAPE = (512, 128)  # width, height: 64 pool rows


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def numpy_pool(plane, bytes, bits, aa=48):
    """(output plane, smoothed rows [9, nr, w]) of a Y plane through the numpy oracle."""
    h, w = plane.shape
    m = NumpySangNom(w, h, bytes=bytes, bits=bits, aa=aa)
    out = m.get_frame([plane])[0]
    nr = h // 2 - 1
    return out, np.ascontiguousarray(m.pool[:, 1:nr + 1, :w]).astype(plane.dtype)


def sse2_pool(plane, bytes, bits, aa=48):
    """The same in the reference's SSE2 arithmetic (tests/sse2_model.py), for opt=1 with sse2_sweeps=1."""
    from tests import sse2_model as sm
    h, w = plane.shape
    m = sm.model_for(1, w, h, bytes=bytes, bits=bits, aa=aa)
    out = m.get_frame([plane])[0]
    nr = h // 2 - 1
    return out, np.ascontiguousarray(m.pool[:, 1:nr + 1, :w]).astype(plane.dtype)


def c_pool(plane, bytes, bits, aa=48):
    """The same through the C oracle (fast enough for planes of 540 pool rows)."""
    h, w = plane.shape
    o = Oracle(oracle_cfg(clip_format({(1, 8): "Y8", (2, 10): "Y10", (2, 16): "Y16", (4, 32): "Y32"}[(bytes, bits)], w, h), aa=aa))
    out = o.process([plane])[0]
    nr = h // 2 - 1
    return out, o.pool()[:, 1:nr + 1, :w].copy()


def seam_check(plane, bytes, bits, seam, ghost, seam_from_left_end=None, run=numpy_pool):
    """Split `plane` at column `seam` into windows [0, seam + ghost) and [seam - ghost, w).  seam_from_left_end (the test
    hook's ghost_columns): the windows stay, the seam moves to that distance from the left window's end."""
    h, w = plane.shape
    out_t, pool_t = run(plane, bytes, bits)
    le, rs = seam + ghost, seam - ghost  # left window's end, right window's start
    m = seam if seam_from_left_end is None else le - seam_from_left_end
    out_l, pool_l = run(np.ascontiguousarray(plane[:, :le]), bytes, bits)
    out_r, pool_r = run(np.ascontiguousarray(plane[:, rs:]), bytes, bits)
    agree = np.array_equal(_bits(pool_l[:, :, m - 8:m + 8]), _bits(pool_r[:, :, m - 8 - rs:m + 8 - rs]))
    own = (np.array_equal(_bits(pool_l[:, :, :m]), _bits(pool_t[:, :, :m])) and
           np.array_equal(_bits(pool_r[:, :, m - rs:]), _bits(pool_t[:, :, m:])))
    out = (np.array_equal(_bits(out_l[:, :m]), _bits(out_t[:, :m])) and np.array_equal(_bits(out_r[:, m - rs:]), _bits(out_t[:, m:])))
    # deepest wrong column, counted from the window's inner edge (1 = the edge column itself)
    bad_l = np.nonzero((_bits(pool_l) != _bits(pool_t[:, :, :le])).any(axis=(0, 1)))[0]
    bad_r = np.nonzero((_bits(pool_r) != _bits(pool_t[:, :, rs:])).any(axis=(0, 1)))[0]
    deep = max(int(le - bad_l.min()) if len(bad_l) else 0, int(bad_r.max()) + 1 if len(bad_r) else 0)
    return dict(agree=agree, own_exact=own, out_exact=out, deepest=deep)


# ---- GPU cases ------------------------------------------------------------------------------------------------------------
NFRAMES = 3
PARITIES = (1, 0, 1)
# (format, width, height, filter kwargs, context kwargs)
NATURAL = [
    ("Y16", 3872, 32, {}, {}), ("Y10", 3872, 32, {}, {}), ("Y32", 3872, 32, {}, {}),
    ("Y16", 4096, 64, {}, {}), ("Y10", 4096, 64, {}, {}), ("Y32", 4096, 64, {}, {}),
    ("Y16", 8192, 16, {}, {}), ("Y32", 8192, 16, {}, {}),
    ("YUV444P16", 3872, 32, dict(aac=48), {}),
    ("YUV420P16", 4096, 64, dict(aac=48), dict(isolated_planes=True)),
    ("YUV420PS", 4096, 64, dict(aac=48), dict(isolated_planes=True)),
]
# orders with mixed parity and dh, on one shape each
ORDERS = [("Y16", 3872, 32, dict(order=0), {}), ("Y32", 3872, 32, dict(order=1), {}), ("Y16", 4096, 64, dict(order=2), {}),
          ("Y16", 3872, 16, dict(dh=True), {})]
FORCED = [("Y16", 512, 64), ("Y32", 512, 64)]
FORCED_PARTS = (2, 3, 4)
WIDE_Y16 = ("Y16", 3872, 32)
AA_DH = ("Y16", 1952, 32)  # the second pass is 3904 wide


def case_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}" + "".join(f"-{k}{int(v)}" for k, v in {**c[3], **c[4]}.items()) if len(c) > 3 else f"{c[0]}-{c[1]}x{c[2]}"


def frames_of(clip, patterns, seed0=SEED):
    """One frame per pattern, every frame with its own seed."""
    return [synth.frame(clip, pat, seed=seed0 + i) for i, pat in enumerate(patterns)]


_cache = {}


def expected(fmt, w, h, kw, ckw, patterns, parities=PARITIES, seed0=SEED):
    """(clip, frames, the oracle's frames) of a case, computed once per session and left unchanged.  isolated_planes: every
    plane through an oracle instance of its own, as the option promises."""
    key = (fmt, w, h, tuple(sorted(kw.items())), tuple(sorted(ckw.items())), tuple(patterns), tuple(parities), seed0)
    if key not in _cache:
        clip = clip_format(fmt, w, h)
        frames = frames_of(clip, patterns, seed0)
        if ckw.get("isolated_planes"):
            oras = []
            for p in range(clip.planes):
                pc = clip_format({2: "Y16", 4: "Y32"}[clip.bytes], clip.width >> (clip.subw if p else 0), clip.height >> (clip.subh if p else 0))
                k = dict(kw)
                k["aa"] = kw.get("aa", 48) if p == 0 else kw.get("aac", 0)
                k.pop("aac", None)
                oras.append(Oracle(oracle_cfg(pc, **k)))
            want = [[oras[p].process([fr[p]], parity=par)[0] for p in range(clip.planes)] for fr, par in zip(frames, parities)]
        else:
            ora = Oracle(oracle_cfg(clip, **kw))
            want = [ora.process(fr, parity=par) for fr, par in zip(frames, parities)]
        for fr in want:
            for pl in fr:
                pl.setflags(write=False)
        _cache[key] = (clip, frames, want)
    return _cache[key]


def to_torch(frames, clip, dev):
    """Frames -> per plane a device tensor [N, H, W] (torch has no uint16: same bits as int16)."""
    import torch
    vt = {1: np.uint8, 2: np.int16, 4: np.float32}[clip.bytes]
    return [torch.from_numpy(np.stack([fr[p] for fr in frames]).view(vt)).pin_memory().to(dev) for p in range(clip.planes)]
