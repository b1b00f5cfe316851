"""Chroma merged through the luma plane's mask (include/sangnom_hip.h, "Edge mask", the paragraph on mc) in numpy: m_L is
tests/mask_model.edge_mask of the SOURCE luma plane, mc its block mean over 2^sw x 2^sh luma samples with rounding, and the
merge and the written mask are the existing formulas with m = mc.  Integers in int64 (the library's 32-bit sums are at most
16 * 256), floats as explicit np.float32 operations in the written order."""
import numpy as np

from tests.mask_model import edge_mask, merge_plane

f32 = np.float32


def reduce_mask(m, sw, sh):
    """mc of the contract: m is m_L [H << sh, W << sw], the result [H, W] in int64."""
    n = sw + sh
    if n == 0:
        return m.astype(np.int64)
    Hl, Wl = m.shape
    assert Hl % (1 << sh) == 0 and Wl % (1 << sw) == 0
    s = m.astype(np.int64).reshape(Hl >> sh, 1 << sh, Wl >> sw, 1 << sw).sum(axis=(1, 3))
    return (s + ((1 << n) >> 1)) >> n


def chroma_mask(L, lo, hi, expand, bits=8, sw=1, sh=1):
    return reduce_mask(edge_mask(L, lo, hi, expand, bits), sw, sh)


def _merge(S, R, m):
    if S.dtype == np.float32:
        with np.errstate(invalid="ignore", over="ignore"):
            a = (m.astype(f32) * f32(0.00390625)).astype(f32)
            mid = (S + ((R - S).astype(f32) * a).astype(f32)).astype(f32)
        return np.where(m == 0, S, np.where(m == 256, R, mid)).astype(f32)
    return ((S.astype(np.int64) * (256 - m) + R.astype(np.int64) * m + 128) >> 8).astype(S.dtype)


def merge_plane_luma(L, S, R, lo, hi, expand, bits=8, sw=1, sh=1):
    """out of the contract for one chroma plane: S and R [H, W], L [H << sh, W << sw]; S's dtype."""
    m = chroma_mask(L, lo, hi, expand, bits, sw, sh)
    assert m.shape == S.shape == R.shape
    return _merge(S, R, m)


def mask_plane_luma(L, lo, hi, expand, bits=8, sw=1, sh=1):
    """What the kernel writes without a result to merge: mc in L's sample type."""
    m = chroma_mask(L, lo, hi, expand, bits, sw, sh)
    if L.dtype == np.float32:
        return (m.astype(f32) * f32(0.00390625)).astype(f32)
    return ((m * ((1 << bits) - 1) + 128) >> 8).astype(L.dtype)


def merge_model_luma(frame, result, lo, hi, expand, bits=8, sw=1, sh=1, processed=None):
    """A frame: plane 0 through its own mask, planes 1 and 2 through mc of the source luma plane; a plane that is not processed
    keeps the result as it is (a copy of the source)."""
    out = []
    for p, (S, R) in enumerate(zip(frame, result)):
        if processed is not None and not processed[p]:
            out.append(R)
        elif p == 0:
            out.append(merge_plane(S, R, lo, hi, expand, bits))
        else:
            out.append(merge_plane_luma(frame[0], S, R, lo, hi, expand, bits, sw, sh))
    return out
