"""The contra-sharpening of the anti-aliasing call (include/sangnom_hip.h, "Contra-sharpening") in numpy: the call's result R
is sharpened by an unsharp mask of [1 2 1] x [1 2 1], limited per sample by what S - R allows over the 3 x 3 neighbourhood.
Coordinates outside the plane are clamped to its edge.  Integer samples in int64 (the library's 32-bit values cannot
overflow: |d| * 255 < 2^24 and the sums stay below 2^21), float samples as explicit np.float32 operations in the written
order."""
import numpy as np

f32 = np.float32


def _at(P, dy, dx):
    """P(y + dy, x + dx) for every (y, x), coordinates clamped."""
    H, W = P.shape
    return P[np.clip(np.arange(H) + dy, 0, H - 1)][:, np.clip(np.arange(W) + dx, 0, W - 1)]


def sharpen_terms(S, R, amount, bits=8):
    """(d1, mn, mx, c) of the contract: int64 for integer planes, float32 for float planes."""
    if R.dtype == np.float32:
        with np.errstate(invalid="ignore", over="ignore"):
            h = ((_at(R, 0, -1) + _at(R, 0, 1)).astype(f32) + (R + R).astype(f32)).astype(f32)
            v = ((_at(h, -1, 0) + _at(h, 1, 0)).astype(f32) + (h + h).astype(f32)).astype(f32)
            B = (v * f32(0.0625)).astype(f32)
            d = (R - B).astype(f32)
            k = f32(amount) * f32(0.015625)
            d1 = (d * k).astype(f32)
            D = (S - R).astype(f32)
            mn = np.zeros(R.shape, f32)
            mx = np.zeros(R.shape, f32)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    t = _at(D, dy, dx)
                    mn = np.where(t < mn, t, mn)  # a NaN t: the comparison is false
                    mx = np.where(t > mx, t, mx)
            c = d1.copy()
            c = np.where(c < mn, mn, c)
            c = np.where(c > mx, mx, c)
        return d1, mn, mx, c
    S = S.astype(np.int64)
    R = R.astype(np.int64)
    h = _at(R, 0, -1) + 2 * R + _at(R, 0, 1)
    B = (_at(h, -1, 0) + 2 * h + _at(h, 1, 0) + 8) >> 4
    d = R - B
    d1 = np.sign(d) * ((np.abs(d) * amount) >> 6)
    D = S - R
    nb = np.stack([_at(D, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    mn = np.minimum(0, nb.min(axis=0))
    mx = np.maximum(0, nb.max(axis=0))
    return d1, mn, mx, np.minimum(np.maximum(d1, mn), mx)


def sharpen_plane(S, R, amount, bits=8):
    """out of the contract, R's dtype."""
    d1, mn, mx, c = sharpen_terms(S, R, amount, bits)
    if R.dtype == np.float32:
        with np.errstate(invalid="ignore", over="ignore"):
            return np.where(np.isnan(d1) | (c == 0), R, (R + c).astype(f32)).astype(f32)
    return np.clip(R.astype(np.int64) + c, 0, (1 << bits) - 1).astype(R.dtype)


def sharpen_model(frame, result, amount, chroma, bits=8, processed=None):
    """A frame: plane 0, and with chroma every plane, sharpened where it is processed; every other plane keeps the result."""
    return [sharpen_plane(S, R, amount, bits) if (p == 0 or chroma) and (processed is None or processed[p]) else R
            for p, (S, R) in enumerate(zip(frame, result))]
