"""Packed 4:2:2 device surfaces (SN_LAYOUT_PACKED_*: YUY2 / UYVY, Y210 / Y212 / Y216, v210): the numpy model of the layouts, the
case table, the sources and the expected frames of tests/test_packed_surfaces_cpu.py and tests/test_packed_surfaces_gpu.py.
TEST INFRASTRUCTURE ONLY.

One rule defines the result (include/sangnom_hip.h): the destination holds what the planar call gives on the unpacked planes --
MSB words shifted down, v210 fields extracted --, packed as the destination's layout says (MSB shift up, v210 mask).  So the
planar LSB-aligned frames are tests/surface_cases.py's, their expected frames the CPU oracle's on them (the SSE2 model for
opt=1, tests/aa_script.py / tests/aa_dh_script.py for the anti-aliasing call), and numpy packs both.  Every source carries junk
where it must be ignored: MSB sources random non-zero low bits, v210 sources random bits 30-31 and random fields for the
pixels at and beyond the width."""
import numpy as np

from avisynth_sangnom2_amd import clip_format, synth
from tests import msb_surface_cases as mc
from tests import surface_cases as sc

C = sc.Case
LAYOUTS = ("yuyv", "uyvy", "yuyv_msb", "uyvy_msb", "v210")
JUNK_SEED = 4242


# ---- the layouts in numpy ------------------------------------------------------------------------------------------------------

def order_of(layout):
    return layout.split("_")[0]


def is_msb(layout):
    return layout.endswith("_msb")


def pack_yuyv(y, u, v, order="yuyv"):
    """Planes [..., H, W], [..., H, W / 2] x 2 of one dtype -> rows of 2 W samples."""
    out = np.empty(y.shape[:-1] + (2 * y.shape[-1],), dtype=y.dtype)
    iy, ic = (0, 1) if order == "yuyv" else (1, 0)
    out[..., iy::2] = y
    out[..., ic::4] = u
    out[..., ic + 2::4] = v
    return out


def unpack_yuyv(rows, order="yuyv"):
    iy, ic = (0, 1) if order == "yuyv" else (1, 0)
    return [np.ascontiguousarray(rows[..., iy::2]), np.ascontiguousarray(rows[..., ic::4]), np.ascontiguousarray(rows[..., ic + 2::4])]


V210_Y = ((0, 1), (1, 0), (1, 2), (2, 1), (3, 0), (3, 2))  # pixel k of a block: (word, field)
V210_U = ((0, 0), (1, 1), (2, 2))
V210_V = ((0, 2), (2, 0), (3, 1))


def v210_blocks(w):
    return (w + 5) // 6


def pack_v210(y, u, v, junk_seed=None):
    """uint16 planes [..., H, W], [..., H, W / 2] x 2 -> rows of 4 ceil(W / 6) uint32 words: every field sample & 0x3FF, bits 30-31
    and the fields of pixels >= W zero -- or, with junk_seed, random (what a source may hold there)."""
    w, nb = y.shape[-1], v210_blocks(y.shape[-1])
    lead = y.shape[:-1]

    def padded(pl, n):
        out = np.zeros(lead + (n,), dtype=np.uint32)
        out[..., :pl.shape[-1]] = pl.astype(np.uint32) & 0x3FF
        if junk_seed is not None and n > pl.shape[-1]:
            r = synth.splitmix64(np.arange(out[..., pl.shape[-1]:].size, dtype=np.uint64), junk_seed + n)
            out[..., pl.shape[-1]:] = (r >> np.uint64(9)).astype(np.uint32).reshape(out[..., pl.shape[-1]:].shape) & 0x3FF
        return out.reshape(lead + (nb, -1))
    yy, uu, vv = padded(y, 6 * nb), padded(u, 3 * nb), padded(v, 3 * nb)
    words = np.zeros(lead + (nb, 4), dtype=np.uint32)
    for table, pl in ((V210_Y, yy), (V210_U, uu), (V210_V, vv)):
        for k, (word, field) in enumerate(table):
            words[..., word] |= pl[..., k] << np.uint32(10 * field)
    if junk_seed is not None:
        r = synth.splitmix64(np.arange(words.size, dtype=np.uint64), junk_seed)
        words |= ((r >> np.uint64(7)).astype(np.uint32).reshape(words.shape) & 3) << np.uint32(30)
    return words.reshape(lead + (4 * nb,))


def unpack_v210(rows, w):
    nb = rows.shape[-1] // 4
    words = rows.reshape(rows.shape[:-1] + (nb, 4)).astype(np.uint32)

    def plane(table, n):
        out = np.stack([(words[..., word] >> np.uint32(10 * field)) & 0x3FF for word, field in table], axis=-1)
        return np.ascontiguousarray(out.reshape(rows.shape[:-1] + (-1,))[..., :n].astype(np.uint16))
    return [plane(V210_Y, w), plane(V210_U, w // 2), plane(V210_V, w // 2)]


def row_bytes(layout, w, B):
    return 16 * v210_blocks(w) if layout == "v210" else 2 * w * B


def packed_dtype(layout, clip):
    return np.uint32 if layout == "v210" else clip.dtype


def pack_frames(layout, clip, frames, source=False, seed=JUNK_SEED):
    """LSB-aligned planar frames -> per frame ONE packed array.  source: with the junk a source may carry; otherwise what a
    destination has to hold (an MSB word keeps the low 16 bits of sample << shift, a v210 field sample & 0x3FF)."""
    s = mc.shift_of(clip) if is_msb(layout) else 0
    out = []
    for f, fr in enumerate(frames):
        if layout == "v210":
            out.append(pack_v210(fr[0], fr[1], fr[2], seed + f if source else None))
            continue
        planes = mc.msb_source([fr], s, seed + f)[0] if source and s else mc.up([fr], s)[0] if s else fr
        out.append(pack_yuyv(planes[0], planes[1], planes[2], order_of(layout)))
    for a in out:
        a.setflags(write=False)
    return out


def unpack_frames(layout, clip, packed):
    """... and back to LSB-aligned planar frames (junk dropped)."""
    s = mc.shift_of(clip) if is_msb(layout) else 0
    if layout == "v210":
        return [unpack_v210(a, clip.width) for a in packed]
    return [[pl >> s if s else pl for pl in unpack_yuyv(a, order_of(layout))] for a in packed]


# ---- the case table ------------------------------------------------------------------------------------------------------------

P8, P10, P12, P16 = "YUV422P8", "YUV422P10", "YUV422P12", "YUV422P16"
PARITY = [
    (C(P8, 256, 32, path="sweep", uv_sweep=True), "yuyv"),
    (C(P8, 256, 32, path="sweep", uv_sweep=True), "uyvy"),
    (C(P8, 64, 16), "yuyv"),                                   # exactly two vectors of 32 pixels
    (C(P8, 64, 16), "uyvy"),
    (C(P8, 100, 40, n=4), "yuyv"),                             # history-carrying; three vectors and two pixel pairs behind them
    (C(P8, 128, 24, dict(dh=True)), "yuyv"),
    (C(P8, 128, 32, dict(order=0), parities=(0, 1, 0)), "uyvy"),  # two field offsets in one call
    (C(P8, 128, 40, {}, dict(isolated_planes=True)), "yuyv"),
    (C(P8, 128, 32, {}, dict(opt=1, sse2_sweeps=1), pattern="noise01"), "yuyv"),  # (surface_cases asserts the arithmetics differ)
    (C(P16, 256, 32), "yuyv"),                                 # Y216: low bits set
    (C(P10, 256, 32), "yuyv_msb"),                             # Y210
    (C(P12, 100, 40, n=4), "uyvy_msb"),                        # v216-style Y212; vectors of 16 pixels, then pairs
    (C(P10, 96, 16), "v210"),                                  # two whole groups
    (C(P10, 98, 16), "v210"),                                  # ... and a block of 2 pixels
    (C(P10, 100, 40, n=4), "v210"),                            # ... of 4 pixels; history-carrying
    (C(P10, 384, 32, path="sweep"), "v210"),
    (C(P8, 4128, 8, n=1), "yuyv"),                             # 129 vectors: more than one workgroup along a row
    (C(P10, 3168, 8, n=1), "v210"),                            # 66 groups
]
# interpolated samples above 2^bits - 1: the v210 mask and the MSB shift drop their high bits
OUT_OF_RANGE = C(P10, 96, 16, dict(aa=48, aac=48), pattern="noise01")
OUT_OF_RANGE_SEED = 7
OUT_OF_RANGE_LAYOUTS = ("v210", "yuyv_msb")

MIXED = {8: C(P8, 256, 32), 10: C(P10, 256, 32)}
# (source, destination): a packed layout, "planar", "planar_msb" or "nv16"
MIXED_SIDES = {
    8: [("yuyv", "planar"), ("planar", "uyvy"), ("yuyv", "uyvy"), ("yuyv", "nv16"), ("nv16", "yuyv")],
    10: [("v210", "yuyv_msb"), ("yuyv_msb", "planar"), ("planar_msb", "v210"), ("yuyv_msb", "nv16"), ("nv16", "v210")],
}
COPIED = [C(P10, 128, 32, dict(chroma=False)), C(P10, 128, 32, dict(luma=False, aac=30))]
COPIED_LAYOUTS = ("yuyv_msb", "v210")
CALLER_LAYOUTS = [(C(P8, 256, 64), "yuyv"), (C(P8, 100, 40, n=4), "yuyv"), (C(P10, 256, 64), "yuyv_msb"), (C(P10, 100, 40, n=4), "yuyv_msb"),
                  (C(P10, 256, 64), "v210"), (C(P10, 100, 40, n=4), "v210")]
CHUNKED = (C(P8, 100, 40, n=4), "yuyv")
REFIT = C(P8, 256, 32)
AA = [(P8, "yuyv", False), (P8, "yuyv", True), (P10, "v210", False), (P10, "v210", True)]  # 128 x 64
REFUSED_CONTEXTS = [C("YUV420P8", 64, 32), C("YUV444P8", 64, 32), C("Y8", 64, 32), C("YUV422PS", 64, 32)]
V210_REFUSED = [C(P8, 64, 32), C(P12, 64, 32), C(P16, 64, 32)]

_cache = {}


def expected(case):
    """(clip, LSB-aligned planar frames, parities, the expected LSB-aligned planar frames), once per session."""
    if case is OUT_OF_RANGE:
        if "oor" not in _cache:
            from oracle.oracle import Oracle
            from tests.util import oracle_cfg
            clip = clip_format(case.fmt, case.w, case.h)
            frames = [synth.frame(clip, case.pattern, seed=OUT_OF_RANGE_SEED + i) for i in range(case.n)]
            ora = Oracle(oracle_cfg(clip, **case.kw))
            want = [ora.process(fr, parity=par) for fr, par in zip(frames, case.par)]
            for fr in want + frames:
                for pl in fr:
                    pl.setflags(write=False)
            _cache["oor"] = (clip, frames, case.par, want)
        return _cache["oor"]
    return mc.expected(case) if case.ckw.get("opt") == 1 and clip_format(case.fmt, case.w, case.h).bytes == 2 else sc.expected(case)


def exceeds_range(clip, frames):
    return max(int(pl.max()) for fr in frames for pl in fr) > (1 << clip.bits) - 1


# ---- scratch -------------------------------------------------------------------------------------------------------------------

def side_kind(side):
    """(packed, semi-planar, MSB-aligned) of a side name."""
    return side in LAYOUTS, side == "nv16", side.endswith("_msb")


def scratch_frame_bytes(clip, src, dst, dh=False, aa=False):
    """Scratch per frame of a call with a packed side, as include/sangnom_hip.h has it: U and V in for a packed, MSB-aligned or
    semi-planar source, Y in for a packed or MSB-aligned one; U and V out for a packed or semi-planar destination, Y out for a
    packed one; pitches rounded up to 256.  dh doubles the destination's height, in the anti-aliasing call its width as well."""
    (sp, ss, sm), (dp, dsemi, _) = side_kind(src), side_kind(dst)
    assert sp or dp
    sm = sm and mc.shift_of(clip) != 0
    w, h, B = clip.width, clip.height, clip.bytes
    W, H = (2 * w if dh and aa else w), (2 * h if dh else h)
    R = mc.roundup256
    total = 0
    if sp or ss or sm:
        total += 2 * R(w // 2 * B) * h
    if sp or sm:
        total += R(w * B) * h
    if dp or dsemi:
        total += 2 * R(W // 2 * B) * H
    if dp:
        total += R(W * B) * H
    return total


# ---- layouts as callers have them ----------------------------------------------------------------------------------------------

def caller_layout(name, layout, clip, rows, n):
    """Where the n packed frames lie inside ONE allocation (tests/layout_cases.PlaneLayout, rows of bytes).
    odd:   nothing aligned beyond the unit (the sample; 4 bytes for v210) -- base 3 units (v210: 4 = 4 mod 16), pitch row + 5
           units (v210: row + 4 * 5), slack between frames;
    lines: 64-byte aligned padded lines."""
    from tests import layout_cases as lc
    unit = 4 if layout == "v210" else clip.bytes
    row = row_bytes(layout, clip.width, clip.bytes)
    if name == "odd":
        base = 4 if layout == "v210" else 3 * unit
        pitch = row + 5 * unit
        return lc.PlaneLayout("odd", base, pitch, (rows + 2) * pitch + 7 * unit, row, rows, n, 1)
    pitch = (row + 63) // 64 * 64 + 64
    return lc.PlaneLayout("lines", 64, pitch, (rows + 2) * pitch, row, rows, n, 1)
