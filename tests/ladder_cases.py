"""Inputs of the ladder-minimum tests (test_ladder_min3_gpu.py runs them on the device, test_ladder_min3_cpu.py shows what
they exercise).  TEST INFRASTRUCTURE ONLY.

The 8-bit sweeps fold the ladder's keys -- (smoothed cost << 4) | rank -- two at a time with a three-input f16 minimum
(sn_fused_v3_common.h, pk_min3_keys), which is the integer minimum only while every key is a non-negative finite f16
pattern and denormal patterns (keys below 0x0400: costs below 64) pass through untouched.  The patterns put keys on both
sides of that line, on ties inside the pairs that are folded together, and near the top of the range.
"""
import numpy as np

from avisynth_sangnom2_amd import synth

PATTERNS = ("flat", "near-flat", "noise", "checker2", "ramp")
AA = (0, 48, 128)  # threshold keys 0x0010 (a denormal pattern), 0x0400 (the smallest normal), 0x0a90 (the top of the range)
NFRAMES = 2        # parities 0 and 1

# (format, width, height, bands): one wave and one strip; two strips with real ghosts; nine strips (the five-wave
# workgroup); 4:2:0 for the coupled luma sweep, the chroma sweeps and the one-sweep chroma kernel; row bands
# -- (6, 0): six bands with the default run-up, whose own check may hand flat or periodic frames to the pool kernels; (6, 100):
# a run-up of all 100 rows, so every band starts at the top of the plane with the exact state, passes its check on every
# pattern, and what is compared is always the band instances' own output
Y8_SHAPES = (("Y8", 64, 24, None), ("Y8", 992, 24, None), ("Y8", 4096, 16, None), ("Y8", 480, 200, (6, 0)), ("Y8", 480, 200, (6, 100)))
YUV_SHAPES = (("YUV420P8", 64, 40, None), ("YUV420P8", 992, 40, None))


# The same inputs at 9 .. 16 bits (test_u16_ladder_gpu.py): the constants scale with the threshold, 1 << (bits - 8), noise and
# checker cover the depth's range, and the ramp wraps at the depth's modulus inside the plane.  "noise16" fills the 16-bit
# container whatever the depth: samples above the depth's maximum, which the reference wraps modulo 65536 like any other.
U16_PATTERNS = PATTERNS
Y16_SHAPES = (("Y16", 64, 24, None), ("Y16", 544, 24, None), ("Y16", 1920, 16, None), ("Y16", 480, 200, (6, 0)), ("Y16", 480, 200, (6, 100)))
YUV16_SHAPES = (("YUV420P16", 64, 40, None), ("YUV420P16", 1024, 40, None))
ODD_DEPTHS = (9, 14, 15)
ODD_DEPTH_SHAPES = ((64, 24), (544, 24))


def frames(clip, pattern, n=NFRAMES, seed0=71):
    scale = 1 << (clip.bits - 8)
    top = (1 << clip.bits) - 1
    out = []
    for i in range(n):
        planes = synth.frame(clip, "noise", seed=seed0 + i)
        if pattern == "flat":  # every cost zero: all nine buffers tie at key = rank
            planes = [np.full_like(p, (117 + 3 * i) * scale) for p in planes]
        elif pattern == "near-flat":  # costs of 0 .. 2: keys far below 0x0400
            planes = [(96 * scale + p % 3).astype(p.dtype) for p in planes]
        elif pattern == "checker2":  # two-pixel checker of 0 and the maximum: large sums, keys near the top of the range
            planes = synth.frame(clip, "checker2", seed=seed0 + i)
        elif pattern == "ramp":  # slope 1 along a row (wrapping at 256, or at the depth's modulus a few columns in), one column
            # further right per line: the diagonal buffers on either side of the matching one tie
            start = 0 if clip.bits == 8 else top - 39
            planes = [((np.add.outer(np.arange(p.shape[0]), np.arange(p.shape[1])) + 5 * i + start) & top).astype(p.dtype) for p in planes]
        elif pattern == "noise16":
            planes = [synth.plane(p.shape[0], p.shape[1], 2, 16, "noise", (seed0 + i) * 3 + k) for k, p in enumerate(planes)]
        elif pattern != "noise":
            raise ValueError(pattern)
        out.append(planes)
    return out
