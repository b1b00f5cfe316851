"""The reduction of the anti-aliasing call with dh (include/sangnom_hip.h, "Anti-aliasing at source size") in numpy: the
2W x 2H plane E back to W x H, by a symmetric odd filter centred on E[2y + oy][2x + ox] -- where the source sample (x, y)
lies in E -- with coordinates clamped to E's edge.  Integer samples in int64 (the library's 32-bit sums cannot overflow:
|v| <= 36 * 36 * 65535), float samples as explicit np.float32 operations in the written order.  `point` (taps [1]) is no
kernel of the library: it returns E[2y + oy][2x + ox] itself and pins the ox / oy mapping in the CPU test."""
import numpy as np

from tests.aa_dh_script import kept_offset

TAPS = {"point": ([1], 0), "tent": ([1, 2, 1], 2), "halfband": ([-1, 0, 9, 16, 9, 0, -1], 5)}
KERNEL_ID = {"tent": 1, "halfband": 2}


def _taps_at(E, axis, centre, r):
    """E sampled along `axis` at clamp(centre + i - r) for i = 0 .. 2r: a list of 2r + 1 arrays."""
    n = E.shape[axis]
    return [np.take(E, np.clip(centre + i - r, 0, n - 1), axis=axis) for i in range(2 * r + 1)]


def _sum_float(kernel, a):
    f = np.float32
    if kernel == "point":
        return a[0]
    if kernel == "tent":
        return ((a[0] + a[2]).astype(f) + (a[1] + a[1]).astype(f)).astype(f)
    side = ((a[2] + a[4]).astype(f) * f(9.0)).astype(f)
    mid = (a[3] * f(16.0)).astype(f)
    return ((side + mid).astype(f) - (a[0] + a[6]).astype(f)).astype(f)


def reduce_unclamped(E, kernel, ox, oy):
    """Integer planes: v of the contract before rounding, shift and clamp (int64).  Float planes: v (float32)."""
    k, _ = TAPS[kernel]
    r = len(k) // 2
    H2, W2 = E.shape
    X = 2 * np.arange(W2 // 2) + ox
    Y = 2 * np.arange(H2 // 2) + oy
    if E.dtype == np.float32:
        h = _sum_float(kernel, _taps_at(E, 1, X, r))
        return _sum_float(kernel, _taps_at(h, 0, Y, r))
    E = E.astype(np.int64)
    h = sum(int(c) * a for c, a in zip(k, _taps_at(E, 1, X, r)))
    return sum(int(c) * a for c, a in zip(k, _taps_at(h, 0, Y, r)))


def reduce_plane(E, kernel, ox, oy, bits):
    """One plane E [2H, 2W] -> [H, W] of E's dtype; `bits` is the clip's bit depth (the integer clamp)."""
    _, s = TAPS[kernel]
    v = reduce_unclamped(E, kernel, ox, oy)
    if E.dtype == np.float32:
        return (v * np.float32(0.5 ** (2 * s))).astype(np.float32)
    if s:
        v = (v + (1 << (2 * s - 1))) >> (2 * s)
    return np.clip(v, 0, (1 << bits) - 1).astype(E.dtype)


def reduce_model(planes, kernel, order=1, parity=1, bits=8):
    """A frame of the dh script (tests/aa_dh_script.Script.frame) at source size."""
    off = kept_offset(order, parity)
    return [reduce_plane(E, kernel, 1 - off, off, bits) for E in planes]
