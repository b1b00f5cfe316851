"""The rank repair of the anti-aliasing call (include/sangnom_hip.h, "Rank repair") in numpy: each sample of the call's result
R is clamped into [a[rank], a[10 - rank]] of the nine source samples around it, a[1] <= ... <= a[9].  Coordinates outside the
plane are clamped to its edge.  Integer samples: np.sort over the nine and the clamp.  Float samples on bit patterns: R comes
back bit for bit wherever it or one of the nine is a NaN and wherever lo <= R <= hi; a bound that is a zero is +0.0."""
import numpy as np

f32 = np.float32


def _at(P, dy, dx):
    """P(y + dy, x + dx) for every (y, x), coordinates clamped."""
    H, W = P.shape
    return P[np.clip(np.arange(H) + dy, 0, H - 1)][:, np.clip(np.arange(W) + dx, 0, W - 1)]


def repair_bounds(S, rank):
    """(lo, hi) = (a[rank], a[10 - rank]) per sample, in S's dtype.  Float: where one of the nine is a NaN the pair means nothing
    (np.sort puts NaNs last); -0.0 and +0.0 compare equal, as `<` has it."""
    nine = np.sort(np.stack([_at(S, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]), axis=0)
    return nine[rank - 1], nine[9 - rank]


def repair_plane(S, R, rank, bits=8):
    """out of the contract, R's dtype."""
    assert 1 <= rank <= 4 and S.shape == R.shape
    lo, hi = repair_bounds(S, rank)
    if R.dtype != np.float32:
        return np.minimum(np.maximum(R, lo.astype(R.dtype)), hi.astype(R.dtype)).astype(R.dtype)
    S = S.astype(f32)
    nan = np.isnan(R)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            nan = nan | np.isnan(_at(S, dy, dx))
    with np.errstate(invalid="ignore"):
        below, above = R < lo, R > hi  # (a -0.0 R against a +0.0 bound: neither)
    plus = lambda b: np.where(b == 0, f32(0.0), b).astype(f32)  # a zero bound: +0.0
    out = R.view(np.uint32).copy()
    out = np.where(~nan & below, plus(lo).view(np.uint32), out)
    out = np.where(~nan & above, plus(hi).view(np.uint32), out)
    return out.astype(np.uint32).view(f32)


def repair_model(frame, result, rank, chroma, bits=8, processed=None):
    """A frame: plane 0, and with chroma every plane, repaired where it is processed; every other plane keeps the result."""
    return [repair_plane(S, R, rank, bits) if (p == 0 or chroma) and (processed is None or processed[p]) else R
            for p, (S, R) in enumerate(zip(frame, result))]
