"""The rows, frames and patterns of the rank-repair tests.  The call's rows are tests/mask_cases.py's (through
tests/sharpen_cases.py), whose unmasked model frames are computed once there; the expectation is the stages in the library's
order: last step, sharpen, repair, mask.  The kernel's patterns are here too, because tests/test_aa_repair_cpu.py asserts on
the CPU that neither the rows nor the patterns let a GPU test pass trivially."""
import numpy as np

from avisynth_sangnom2_amd import clip_format, synth
from tests import fields_cases as fc
from tests import mask_cases as mc
from tests.fields_model import BothScript, processed_planes
from tests.mask_luma_model import merge_model_luma
from tests.mask_model import merge_model
from tests.repair_model import repair_bounds, repair_model
from tests.sharpen_cases import AMOUNT, BATCH, CHUNK, HOST, LUMA_OFF, MASK, P010, unmasked  # noqa: F401  (the rows, shared by import)
from tests.sharpen_model import sharpen_model

RANKS = (1, 3)  # of the call's tests; the kernel's run all four
FORMS = (None, "tent", "halfband")  # without dh; dh + reduce
ROWS = list(BATCH) + [LUMA_OFF, CHUNK, P010]

# A row whose frame 0 fails a condition of tests/test_aa_repair_cpu.py gets another first seed here (none has needed one).
FIRST = {}


def first_of(case):
    return FIRST.get(repr(case[:4]), 301)


def forms_of(case):
    """Row 0 with the tent too; LUMA_OFF is a row of the form without dh only (dh processes every plane)."""
    if case is LUMA_OFF:
        return [None]
    return list(FORMS) if case is BATCH[0] else [None, "halfband"]


def chromas_of(case):
    """sn_aa_repair.chroma of the runs of a row: 0, and 1 too on the subsampled rows (the 4:4:4 row's chroma is not filtered
    -- aac = 0 --, and an average of the lines above and below never leaves the source's 3 x 3 range)."""
    clip = clip_format(case[0], case[1], case[2])
    return [False, True] if clip.planes == 3 and (clip.subw or clip.subh) else [False]


BOTH_ROWS = (12, 13, fc.STAGES_YUV)  # of tests/fields_cases.CASES: the rows with edges (sharpened; masked; every stage on 4:2:0)


def repaired_planes(case, form, chroma):
    proc = mc.processed_of(case) if form is None else [True] * len(mc.processed_of(case))
    return [proc[p] and (p == 0 or bool(chroma)) for p in range(len(proc))]


def behind(clip, proc, frame, result, rank=0, chroma=False, sharpen=None, mask=None, mask_chroma="own"):
    """The stages behind the last step, in the library's order.  sharpen: (amount, chroma) or None; mask: (lo, hi, expand) or None."""
    r = result
    if sharpen:
        r = sharpen_model(frame, r, sharpen[0], sharpen[1], clip.bits, proc)
    if rank:
        r = repair_model(frame, r, rank, chroma, clip.bits, proc)
    if mask:
        lo, hi, expand = mask
        if mask_chroma == "luma":
            r = merge_model_luma(frame, r, lo, hi, expand, clip.bits, clip.subw, clip.subh, proc)
        else:
            r = merge_model(frame, r, lo, hi, expand, clip.bits, proc)
    return r


def expected(case, form, rank, chroma, sharpen=None, mask=None, count=mc.NFRAMES, mask_chroma="own"):
    """(frames, parities, plain, want): `want` is merge_model(source, repair_model(source, sharpen_model(source, unmasked)));
    `plain` is the same without the repair (what the call gives today).  form: "tent" | "halfband" (dh + reduce) or None."""
    frames, parities, res = unmasked(case, form, count, first_of(case))
    clip = clip_format(case[0], case[1], case[2])
    proc = mc.processed_of(case) if form is None else None
    want = [behind(clip, proc, fr, r, rank, chroma, sharpen, mask, mask_chroma) for fr, r in zip(frames, res)]
    plain = [behind(clip, proc, fr, r, 0, False, sharpen, mask, mask_chroma) for fr, r in zip(frames, res)]
    return frames, parities, plain, want


_BOTH = {}


def both_unmasked(i, count=None):
    """(frames, the averaged results of tests/fields_model.BothScript) of row i of tests/fields_cases.CASES, computed once."""
    if (i, count) not in _BOTH:
        case = fc.CASES[i]
        clip = clip_format(case.fmt, case.w, case.h)
        frames = fc.frames_of(case, count)
        script = BothScript(clip, **case.kw, **case.skw)
        _BOTH[(i, count)] = (frames, [script.frame(fr, parity=1) for fr in frames])
    return _BOTH[(i, count)]


def expected_both(i, rank, chroma, count=None):
    """(frames, plain, want) of row i of tests/fields_cases.CASES with its own sharpening and mask and the repair between them."""
    case = fc.CASES[i]
    clip = clip_format(case.fmt, case.w, case.h)
    proc = processed_planes(clip.planes, case.kw)
    frames, res = both_unmasked(i, count)
    mask, mchroma = (case.mask[:3], case.mask[3]) if case.mask else (None, "own")
    want = [behind(clip, proc, fr, r, rank, chroma, case.sharpen, mask, mchroma) for fr, r in zip(frames, res)]
    plain = [behind(clip, proc, fr, r, 0, False, case.sharpen, mask, mchroma) for fr, r in zip(frames, res)]
    return frames, plain, want


def classes(S, R, rank):
    """The shares of samples of R below a[rank], above a[10 - rank] and within, over the samples whose nine hold no NaN."""
    lo, hi = repair_bounds(S, rank)
    with np.errstate(invalid="ignore"):
        below, above = R < lo, R > hi
    return below.mean(), above.mean(), (~below & ~above).mean()


# ---- the kernel's shapes and patterns ------------------------------------------------------------------------------------------

def kernel_shapes(B, tile_bytes, th):
    """(W, H): planes narrower than the window (every tap clamped); one less than the tile, the tile and one more in each
    direction; three tiles each way with ragged edges."""
    TW = tile_bytes // B
    return [(1, 1), (2, 3), (3, 2), (TW - 1, th), (TW, th), (TW + 1, th), (TW, th - 1), (TW, th + 1), (2 * TW + 22, 2 * th + 5)]


def special(W, H):
    """0.5 with NaN (one with a payload), infinities of both signs and -0.0 in it, alone, side by side and on the plane's edges."""
    sp = np.full((H, W), 0.5, np.float32)
    for k, v in enumerate([np.nan, np.inf, -np.inf, -0.0, np.inf, np.inf, -np.inf, -0.0, 0.0]):
        sp[(k * 7) % H, (k * 29 + (k > 4)) % W] = v
    sp[H - 1, W - 1] = np.inf
    sp[0, W // 2] = np.nan
    sp.view(np.uint32)[H // 2, 0] = 0xFFC01234  # a negative NaN with a payload
    return sp


def kernel_patterns(clip, W, H, seed):
    """(S, R) per frame of one launch [H, W]: edges against a noisy copy of them, full-range noise against noise, a one-pixel
    checker against its inverse (ties: five equal values among the nine, and R beyond either bound), a constant S against noise,
    and for float the NaN / infinity / -0.0 plane as S and as R in turn, and zeros of both signs against each other."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    if clip.bytes == 4:
        f = np.float32
        noise = lambda: (rng.random((H, W), dtype=f) * f(2) - f(1)).astype(f)
        edges = synth.plane(H, W, 4, 32, "edges", seed)
        chk = ((x + y) & 1).astype(f)
        soft = (edges + noise() * f(0.125)).astype(f)
        zeros = np.where((x + 2 * y) % 3 == 0, f(-0.0), f(0.0)).astype(f)
        tiny = (noise() * f(1e-3)).astype(f)
        return [(edges, soft), (noise(), noise()), ((f(1) - chk).astype(f), chk), (np.full((H, W), 0.3, f), noise()), (special(W, H), noise()),
                (noise(), special(W, H)), (zeros, np.where(x % 2 == 0, zeros, tiny).astype(f)), (np.where(y % 2 == 0, zeros, -tiny).astype(f), (-zeros).astype(f))]
    mx = (1 << clip.bits) - 1
    noise = lambda: rng.integers(0, mx + 1, (H, W)).astype(clip.dtype)
    edges = synth.plane(H, W, clip.bytes, clip.bits, "edges", seed)
    soft = np.clip(edges.astype(np.int64) + rng.integers(-(mx >> 3), (mx >> 3) + 1, (H, W)), 0, mx).astype(clip.dtype)
    chk = (((x + y) & 1) * mx).astype(clip.dtype)
    return [(edges, soft), (noise(), noise()), ((mx - chk).astype(clip.dtype), chk), (np.full((H, W), mx // 3, clip.dtype), noise())]
