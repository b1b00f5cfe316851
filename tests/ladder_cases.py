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


def frames(clip, pattern, n=NFRAMES, seed0=71):
    out = []
    for i in range(n):
        planes = synth.frame(clip, "noise", seed=seed0 + i)
        if pattern == "flat":  # every cost zero: all nine buffers tie at key = rank
            planes = [np.full_like(p, 117 + 3 * i) for p in planes]
        elif pattern == "near-flat":  # costs of 0 .. 2: keys far below 0x0400
            planes = [(96 + p % 3).astype(p.dtype) for p in planes]
        elif pattern == "checker2":  # two-pixel checker of 0 and 255: large sums, keys near 0x0ff0
            planes = synth.frame(clip, "checker2", seed=seed0 + i)
        elif pattern == "ramp":  # slope 1 along a row (wrapping at 256), one column further right per line: the diagonal
            # buffers on either side of the matching one tie
            planes = [((np.add.outer(np.arange(p.shape[0]), np.arange(p.shape[1])) + 5 * i) & 255).astype(p.dtype) for p in planes]
        elif pattern != "noise":
            raise ValueError(pattern)
        out.append(planes)
    return out
