"""The rows and frames of the contra-sharpening tests of the anti-aliasing call: tests/mask_cases.py's, whose unmasked model
frames (aa_script's without dh, the dh script plus reduce_model with dh and a reduction) are computed once there.  The
expectation is the stages in the library's order: last step, sharpen, mask."""
from avisynth_sangnom2_amd import clip_format
from tests import mask_cases as mc
from tests.mask_cases import BATCH, CHUNK, HOST, LUMA_OFF, P010, unmasked  # noqa: F401  (the rows, shared by import)
from tests.mask_luma_model import merge_model_luma
from tests.mask_model import merge_model
from tests.sharpen_model import sharpen_model

AMOUNT = 64
MASK = (mc.LO, mc.HI, 1)  # lo, hi, expand of the masked runs


def expected(case, form, amount, chroma, mask, count=mc.NFRAMES, first=301, mask_chroma="own"):
    """(frames, parities, unsharpened, want): `want` is merge_model(source, sharpen_model(source, unmasked result)) with
    mask = (lo, hi, expand), the sharpened frame itself with mask = None; `unsharpened` is the same without the sharpening
    (what the call gives today).  form: "tent" | "halfband" (dh + reduce) or None (without dh)."""
    frames, parities, res = unmasked(case, form, count, first)
    clip = clip_format(case[0], case[1], case[2])
    proc = mc.processed_of(case) if form is None else None

    def masked(fr, r):
        if mask is None:
            return r
        lo, hi, expand = mask
        if mask_chroma == "luma":
            return merge_model_luma(fr, r, lo, hi, expand, clip.bits, clip.subw, clip.subh, proc)
        return merge_model(fr, r, lo, hi, expand, clip.bits, proc)
    want = [masked(fr, sharpen_model(fr, r, amount, chroma, clip.bits, proc)) for fr, r in zip(frames, res)]
    plain = [masked(fr, r) for fr, r in zip(frames, res)]
    return frames, parities, plain, want
