"""The edge mask of the anti-aliasing call (include/sangnom_hip.h, "Edge mask") in numpy: a Sobel mask of the source plane
S with two thresholds and one optional 3 x 3 expansion, and the merge of the call's result R into S through it.  Coordinates
outside S are clamped to its edge.  Integer samples in int64 (the library's 32-bit values cannot overflow: |gx| + |gy| <=
8 * 65535 and S * 256 + 128 < 2^31), float samples as explicit np.float32 operations in the written order, Tlo, Thi and k
included."""
import numpy as np

f32 = np.float32


def _at(S, dy, dx):
    """S(y + dy, x + dx) for every (y, x), coordinates clamped."""
    H, W = S.shape
    return S[np.clip(np.arange(H) + dy, 0, H - 1)][:, np.clip(np.arange(W) + dx, 0, W - 1)]


def sobel_e(S, bits=8):
    """e of the contract: int64 for integer planes, float32 for float planes."""
    if S.dtype == np.float32:
        def col(dx):
            return ((_at(S, -1, dx) + _at(S, 1, dx)).astype(f32) + (_at(S, 0, dx) + _at(S, 0, dx)).astype(f32)).astype(f32)

        def row(dy):
            return ((_at(S, dy, -1) + _at(S, dy, 1)).astype(f32) + (_at(S, dy, 0) + _at(S, dy, 0)).astype(f32)).astype(f32)
        with np.errstate(invalid="ignore", over="ignore"):
            gx = (col(1) - col(-1)).astype(f32)
            gy = (row(1) - row(-1)).astype(f32)
            return ((np.abs(gx) + np.abs(gy)).astype(f32) * f32(0.25)).astype(f32)
    S = S.astype(np.int64)
    gx = (_at(S, -1, 1) + 2 * _at(S, 0, 1) + _at(S, 1, 1)) - (_at(S, -1, -1) + 2 * _at(S, 0, -1) + _at(S, 1, -1))
    gy = (_at(S, 1, -1) + 2 * _at(S, 1, 0) + _at(S, 1, 1)) - (_at(S, -1, -1) + 2 * _at(S, -1, 0) + _at(S, -1, 1))
    return (np.abs(gx) + np.abs(gy)) >> 2


def edge_mask(S, lo, hi, expand, bits=8):
    """m of the contract: int64 in 0..256, S's shape."""
    e = sobel_e(S, bits)
    if S.dtype == np.float32:
        tlo = (f32(lo) / f32(255.0)).astype(f32)
        thi = (f32(hi) / f32(255.0)).astype(f32)
        with np.errstate(invalid="ignore", over="ignore"):
            above = e > tlo  # False for a NaN
            full = above & (e >= thi)
            m0 = np.zeros(e.shape, np.int64)
            ramp = above & ~full
            if hi > lo and ramp.any():
                k = (f32(256.0) / (thi - tlo).astype(f32)).astype(f32)
                v = ((e[ramp] - tlo).astype(f32) * k).astype(f32)
                m0[ramp] = np.minimum(256, v.astype(np.int64))  # truncation: v >= 0
            m0[full] = 256
    else:
        tlo, thi = lo << (bits - 8), hi << (bits - 8)
        m0 = np.where(e <= tlo, 0, np.where(e >= thi, 256, ((e - tlo) * 256) // max(thi - tlo, 1)))
    if not expand:
        return m0
    return np.max(np.stack([_at(m0, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]), axis=0)


def merge_plane(S, R, lo, hi, expand, bits=8):
    """out of the contract, S's dtype."""
    m = edge_mask(S, lo, hi, expand, bits)
    if S.dtype == np.float32:
        with np.errstate(invalid="ignore", over="ignore"):
            a = (m.astype(f32) * f32(0.00390625)).astype(f32)
            mid = (S + ((R - S).astype(f32) * a).astype(f32)).astype(f32)
        return np.where(m == 0, S, np.where(m == 256, R, mid)).astype(f32)
    return ((S.astype(np.int64) * (256 - m) + R.astype(np.int64) * m + 128) >> 8).astype(S.dtype)


def mask_plane(S, lo, hi, expand, bits=8):
    """What the kernel writes without a result to merge: the mask in S's sample type."""
    m = edge_mask(S, lo, hi, expand, bits)
    if S.dtype == np.float32:
        return (m.astype(f32) * f32(0.00390625)).astype(f32)
    return ((m * ((1 << bits) - 1) + 128) >> 8).astype(S.dtype)


def merge_model(frame, result, lo, hi, expand, bits=8, processed=None):
    """A frame: every processed plane's result merged into that plane's source through that plane's own mask; a plane that
    is not processed keeps the result as it is (a copy of the source)."""
    return [merge_plane(S, R, lo, hi, expand, bits) if processed is None or processed[p] else R for p, (S, R) in enumerate(zip(frame, result))]
