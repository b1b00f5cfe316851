"""Float inputs the generic patterns of avisynth_sangnom2_amd/synth.py never produce (test_float_values_gpu.py runs them on
the device, test_float_values_cpu.py shows what they exercise).  TEST INFRASTRUCTURE ONLY.

Portable like tests/ladder_cases.py: everything is built from synth's splitmix64 noise and exactly rounded float32
arithmetic, nothing from numpy's generators.  `n` is synth's float noise (a multiple of 2^-24 in [0, 1)), `n8` its 8-bit noise
with the same seed.

  signed     n - 0.5                        negative samples: the nominal range of float chroma
  overshoot  n * 1.5 - 0.25                 below 0 and above 1
  k255       n8 / 255                       8-bit material converted to float: roundings in the 5x product and the 7-tap sum
  negzero    -0.0 everywhere                the output must be 0x80000000 everywhere
  denormal   n * 2^-127, sign from n8 & 1   every sample is a denormal, and so is every output sample: a SangNom value reaches
                                            1.25 times the largest sample, which 2^-127 keeps below 2^-126 (with 2^-126 one
                                            output sample of the two 64x24 frames is the normal 0x00804178)
  small      n * 2^-120                     normals whose differences and /16 fall into the denormal range
  eighths    (n8 % 9) / 8 - 0.5             exact arithmetic: the rare genuine ties
  checker2   synth's checker2 - 0.5         ties among buffers 6, 7, 8
  slope      (y // 2) * d + x * d - 20 with d = 6 aa / 256 (frames(..., aa=...)): the smoothed minimum EQUALS the threshold on
             the first interpolated row.  Every cost of a linear plane is constant; with the horizontal slope equal to the
             line step, buffer 5 costs d / 4, buffer 4 costs d and every other buffer more.  Pool row 0 is zero, so the first
             smoothed row is 14 / 16 of the cost: 21 aa / 16 / 256, the threshold, and every value on the way is dyadic.
             The reference's `minbuf > aaf` is strict there; a `>=` changes those samples.  (Chroma planes: `signed`.)
  huge       signed, with pairs (y, x) = 1e38, (y, x + 1) = -3e37 near the top: finite samples whose 4 * p1 overflows on its
             own (the reference rounds the product before it adds 5 * p2; an fma does not)
  nonfinite  signed, with inf, -inf, nan, 3e38, -3e38 scattered: one special per `every` samples
"""
import numpy as np

from avisynth_sangnom2_amd import ClipFormat, synth
from oracle.oracle import Oracle
from tests.util import oracle_cfg

F32 = np.float32

# the patterns every float path runs; `slope`, `huge` and `nonfinite` have cases of their own
PATTERNS = ("signed", "overshoot", "k255", "negzero", "denormal", "small", "eighths", "checker2")
AA = (0, 48, 128)
SLOPE_AA = (1, 48, 128)
NFRAMES = 2  # parities 0 and 1

HUGE_SHAPE = ("Y32", 256, 400)
# Lines of both fields.  What an fma changes is column x + 1 of the cost cone's right edge, some 60 rows further down, where the
# finite cost it leaves has decayed to the size of the others: nothing infinite may lie to the right of the first pair.
HUGE_PAIRS = ((2, 40), (3, 40), (6, 20))
SPECIALS = (np.inf, -np.inf, np.nan, 3.0e38, -3.0e38)

# (format, width, height, one special per ... samples): the shapes of the non-finite GPU test.  A NaN cost spreads three
# columns per row down the plane, so the taller shapes carry fewer specials: on each of them the reference must still write
# more than 0.7 of the samples, and not all (test_float_values_cpu.py).
NONFINITE_PLAIN = ("Y32", 256, 64, 400)
NONFINITE_PADDED = ("Y32", 200, 64, 400)
NONFINITE_COUPLED = ("YUV420PS", 128, 64, 400)
NONFINITE_BANDS = ("Y32", 480, 200, 4000)


def _n8(clip, seed):
    return synth.frame(ClipFormat(width=clip.width, height=clip.height, bytes=1, bits=8, planes=clip.planes, subw=clip.subw, subh=clip.subh),
                       "noise", seed=seed)


def _specials(plane, seed, every):
    h, w = plane.shape
    r = synth.splitmix64(np.arange(h * w, dtype=np.uint64).reshape(h, w), seed * 0x2545F491 + 0x9E3779B1)
    hit = (r % np.uint64(every)) == 0
    which = ((r >> np.uint64(32)) % np.uint64(len(SPECIALS))).astype(np.int64)
    return np.where(hit, np.array(SPECIALS, dtype=F32)[which], plane).astype(F32)


def frames(clip, pattern, n=NFRAMES, seed0=71, aa=None, every=400):
    assert clip.bytes == 4
    out = []
    for i in range(n):
        noise = synth.frame(clip, "noise", seed=seed0 + i)
        n8 = [p.astype(F32) for p in _n8(clip, seed0 + i)]
        signed = [p - F32(0.5) for p in noise]
        if pattern == "signed":
            planes = signed
        elif pattern == "overshoot":
            planes = [p * F32(1.5) - F32(0.25) for p in noise]
        elif pattern == "k255":
            planes = [q / F32(255) for q in n8]
        elif pattern == "negzero":
            planes = [np.full_like(p, -0.0) for p in noise]
        elif pattern == "denormal":
            planes = [np.where(q.astype(np.int64) & 1, -(p * F32(2.0 ** -127)), p * F32(2.0 ** -127)) for p, q in zip(noise, n8)]
        elif pattern == "small":
            planes = [p * F32(2.0 ** -120) for p in noise]
        elif pattern == "eighths":
            planes = [(q.astype(np.int64) % 9).astype(F32) / F32(8) - F32(0.5) for q in n8]
        elif pattern == "checker2":
            planes = [p - F32(0.5) for p in synth.frame(clip, "checker2", seed=seed0 + i)]
        elif pattern == "slope":
            d = 6.0 * aa / 256.0
            y, x = np.mgrid[0:clip.height, 0:clip.width]
            planes = [((y // 2) * d + x * d - 20.0)] + signed[1:]
        elif pattern == "huge":
            planes = [p.copy() for p in signed]
            for y, x in HUGE_PAIRS:
                planes[0][y, x], planes[0][y, x + 1] = F32(1e38), F32(-3e37)
        elif pattern == "nonfinite":
            planes = [_specials(p, (seed0 + i) * 3 + k, every) for k, p in enumerate(signed)]
        else:
            raise ValueError(pattern)
        out.append([np.ascontiguousarray(p, dtype=F32) for p in planes])
    return out


def written_by_reference(clip, src, parity=1, **kw):
    """(the oracle's planes, masks of the samples the reference writes): where a NaN reaches the minimum of the nine buffers
    the reference takes no arm of its ladder and leaves the sample of the new frame as it was -- undefined content.  A
    written sample is the same whatever the new frame held before."""
    shapes = [p.shape for p in src]
    a = Oracle(oracle_cfg(clip, **kw)).process(src, parity=parity, dst=[np.zeros(s, F32) for s in shapes])
    b = Oracle(oracle_cfg(clip, **kw)).process(src, parity=parity, dst=[np.full(s, 7.0, F32) for s in shapes])
    return a, [(x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y)) for x, y in zip(a, b)]


def assert_defined_samples_match(want, written, got, what=""):
    """Bit patterns for numbers, NaN for NaN (x86 and gfx950 give the default NaN different signs), wherever the reference writes."""
    assert written.mean() > 0.7 and not written.all(), (what, float(written.mean()))
    ok = (want.view(np.uint32) == got.view(np.uint32)) | (np.isnan(want) & np.isnan(got))
    bad = np.argwhere(written & ~ok)
    assert len(bad) == 0, f"{what}: {len(bad)} defined samples differ, first {bad[:4].tolist()}: {want[written & ~ok][:4]} vs {got[written & ~ok][:4]}"
