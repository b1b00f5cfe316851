"""Widths, heights and inputs that walk the geometry of the fused sweeps (tests/test_sweep_geometry_gpu.py runs them on the
device, tests/test_sweep_geometry_cpu.py checks the table itself).  TEST INFRASTRUCTURE ONLY.

Every fused sweep kernel is a template over its wave count NW, and NW follows from the width alone (csrc/sn_sweep_args.h):
a lane holds 8 columns, strip 0 holds 62 real lanes, every later strip 60, a plane of at most 64 lanes is one strip; the
16-bit and float sweeps put one strip on a wave, the 8-bit sweep two (wave k holds strips k and k + NW, so an odd strip count
leaves the last wave's high half dead).  The table below is derived from that formula instead of being chosen case by case:

  WAVE_WIDTHS   the narrowest and the widest plane, a multiple of 32 wide, of every strip count the type has instances for
  EDGE_WIDTHS   the last column on every lane that is 3 mod 4 of a first wave, of a second one, and on the third wave's two lanes
  PADDED        (width, pool stride) of fresh_pool planes a multiple of 8 and not of 32 wide: the lines end 1 .. 3 lanes before
                the sweep does, in the same strip and -- strides 992, 1472, 3392, 3872, 7232 -- in the strip before the last
  HEIGHTS       nothing to interpolate, one interpolated row, and a row loop that ends at each position of the five-row seam block
  COUPLED*      4:2:0 / 4:2:2 clips whose pool-coupled sweeps have 5, 6 (8-bit: 7 too) waves
  GROUPS*       planes of one and of two waves, which share a workgroup between four and two frames
"""
from avisynth_sangnom2_amd import synth
from tests import float_cases, ladder_cases

BYTES = {"Y8": 1, "Y16": 2, "Y32": 4}
MAX_WIDTH = {"Y8": 7680, "Y16": 3840, "Y32": 3840}  # eight waves
SEED = 71


def strips_for(nl):  # sn_sweep_args.h, restated; test_sweep_geometry_cpu.py holds it against the header
    return 1 if nl <= 64 else 1 + (nl - 62 + 59) // 60


def waves(bytes_per_sample, w):
    s = strips_for(w // 8)
    return (s + 1) // 2 if bytes_per_sample == 1 else s


def strip_bounds(max_width):
    """{strip count: (narrowest, widest)} over the planes a multiple of 32 wide up to max_width."""
    out = {}
    for w in range(32, max_width + 1, 32):
        lo, _ = out.get(strips_for(w // 8), (w, w))
        out[strips_for(w // 8)] = (lo, w)
    return out


STRIP_BOUNDS = {t: strip_bounds(MAX_WIDTH[t]) for t in BYTES}
WAVE_WIDTHS = {t: tuple(w for s in sorted(b) for w in b[s]) for t, b in STRIP_BOUNDS.items()}
NARROWEST = {t: tuple(b[s][0] for s in sorted(b)) for t, b in STRIP_BOUNDS.items()}
WIDEST = {t: tuple(b[s][1] for s in sorted(b)) for t, b in STRIP_BOUNDS.items()}

EDGE_WIDTHS = tuple(range(32, 993, 32))

_PADDED16 = tuple((w, stride) for stride, ws in ((64, (40,)), (512, (488, 496, 504)), (544, (520, 528, 536)), (992, (968, 976, 984)),
                                                 (1472, (1448, 1456, 1464)), (3392, (3368, 3376, 3384))) for w in ws)
_PADDED8 = _PADDED16 + tuple((w, stride) for stride, ws in ((3872, (3848, 3856, 3864)), (7232, (7208, 7216, 7224))) for w in ws)
PADDED = {"Y8": _PADDED8, "Y16": _PADDED16, "Y32": _PADDED16}

HEIGHTS = (2, 4, 6, 8, 10, 12, 14)
SEAM_WIDTHS = {"Y8": (1440, 7680), "Y16": (544, 3840), "Y32": (544, 3840)}

# The coupled sweeps cover the luma width whatever the plane: 2048 columns are 5 strips, 2560 are 6; 8-bit: 4096, 5120 and 6144
# columns are 9, 11 and 13 strips, 5, 6 and 7 waves (the last wave's high half dead each time).
COUPLED16 = tuple((fmt, w, 40) for fmt in ("YUV420P16", "YUV420PS", "YUV422P16") for w in (2048, 2560))
COUPLED8 = tuple(("YUV420P8", w, 40) for w in (4096, 5120, 6144))
# U and V as ONE sweep (sn_fused_u8_uv.hip) put one strip on a wave and take at most eight strips, so the three clips above
# never reach it (their chroma runs as two sweeps under either policy); its instances of 5, 6 and 7 waves take these widths.
UV_ONE_SWEEP = tuple(("YUV420P8", w, 40) for w in (2048, 2560, 3072))
# wave counts of the coupled sweeps that other files of the suite launch (16-bit and float: 128 .. 3840 and 2912 columns;
# 8-bit 4:2:0: up to 3840 columns, and 7680)
COUPLED_ELSEWHERE = {1: {1, 2, 3, 4, 8}, 2: {1, 2, 3, 4, 7, 8}, 4: {1, 2, 3, 4, 7, 8}}

# (type, width, height): one wave (four frames to a workgroup) and two waves (two frames); fresh_pool widths of the same strides
GROUPS = (("Y16", 256, 24), ("Y16", 736, 24), ("Y32", 256, 24), ("Y32", 736, 24), ("Y8", 256, 24), ("Y8", 1440, 24))
GROUPS_PADDED = (("Y16", 248, 24), ("Y16", 728, 24), ("Y32", 248, 24), ("Y32", 728, 24))
GROUP_FRAMES = (1, 2, 3, 5, 9)


def last_lane(w):
    """(strip, lane of that strip) that holds column w - 1: strip 0 has no left ghosts, every later strip two."""
    gl = (w - 1) // 8
    if gl < 62 or w // 8 <= 64:
        return 0, gl
    s = 1 + (gl - 62) // 60
    return s, 2 + (gl - 62) % 60


def pool_stride(w):
    return (w + 31) & ~31


def frames(clip, pattern, n=2, seed0=SEED):
    """n frames of a pattern: synth's own, tests/float_cases.py for float clips, tests/ladder_cases.py for integer ones."""
    if pattern in ("noise", "edges", "sine", "noise01"):
        return [synth.frame(clip, pattern, seed=seed0 + i) for i in range(n)]
    if clip.bytes == 4:
        return float_cases.frames(clip, pattern, n=n, seed0=seed0)
    return ladder_cases.frames(clip, pattern, n=n, seed0=seed0)
