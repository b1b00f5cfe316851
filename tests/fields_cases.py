"""The rows and frames of the both-fields tests of the anti-aliasing call (tests/test_aa_fields_cpu.py asserts that they are
not trivial, tests/test_aa_fields_gpu.py runs them): the expectation is tests/fields_model.BothScript followed by the
sharpening and mask models in the library's order.  Every expectation is computed once and left unchanged."""
from collections import namedtuple

from avisynth_sangnom2_amd import clip_format, synth
from tests.aa_script import Script
from tests.fields_model import BothScript, processed_planes
from tests.mask_luma_model import merge_model_luma
from tests.mask_model import merge_model
from tests.sharpen_model import sharpen_model

# kw: filter keywords of library and script; ckw: the library's only; skw: the script's only; sharpen: (amount, chroma) or None;
# mask: (lo, hi, expand, "own" | "luma") or None
Case = namedtuple("Case", "fmt w h frames pattern kw ckw skw sharpen mask")


def C(fmt, w, h, frames=2, pattern="noise", kw=None, ckw=None, skw=None, sharpen=None, mask=None):
    return Case(fmt, w, h, frames, pattern, kw or {}, ckw or {}, skw or {}, sharpen, mask)


CASES = [
    C("Y8", 64, 32),
    C("Y8", 72, 40, frames=3),                       # neither width is a multiple of 32: each of the four instances carries its own history
    C("YUV420P8", 128, 64, kw=dict(aac=48)),
    C("YUV420P8", 104, 48, kw=dict(aac=48)),         # chroma 52 x 24: history, and Y, U and V share each instance's pool
    C("YUV422P8", 64, 32, kw=dict(aac=48)),
    C("Y10", 96, 32),
    C("Y16", 64, 32),
    C("Y32", 64, 32),
    C("YUV420P8", 128, 64, kw=dict(luma=False, aac=48)),
    C("YUV420P8", 104, 48, frames=3, kw=dict(aac=48), ckw=dict(isolated_planes=True), skw=dict(isolated=True)),
    C("Y8", 72, 40, frames=3, ckw=dict(fresh_pool=True), skw=dict(fresh=True)),
    C("Y8", 72, 40, ckw=dict(opt=1), skw=dict(opt=1)),
    C("Y8", 72, 40, pattern="edges", sharpen=(64, False)),
    C("Y8", 72, 40, pattern="edges", mask=(16, 96, 1, "own")),
    C("YUV420P8", 128, 64, pattern="edges", kw=dict(aac=48), sharpen=(64, True), mask=(16, 96, 1, "luma")),
]
IDS = [f"{i}-{c.fmt}-{c.w}x{c.h}" for i, c in enumerate(CASES)]
PLAIN_Y8, HISTORY_Y8, YUV420, STAGES_YUV = 0, 1, 2, 14


def frames_of(case, count=None):
    clip = clip_format(case.fmt, case.w, case.h)
    seeds = range(401, 401 + (count or case.frames))
    if case.pattern == "edges":  # slanted stripes on every plane (tests/mask_cases.py)
        from tests.mask_cases import good_seeds
        seeds = good_seeds(401, count or case.frames)
    return [synth.frame(clip, case.pattern, seed=s) for s in seeds]


def lib_kw(case):
    """The keywords of SangNomAA / SangNomAAHost for the case, fields="both" included."""
    kw = dict(case.kw, **case.ckw, fields="both")
    if case.sharpen:
        kw.update(sharpen=case.sharpen[0], sharpen_chroma=case.sharpen[1])
    if case.mask:
        kw.update(mask=case.mask[:2], mask_expand=case.mask[2], mask_chroma=case.mask[3])
    return kw


def stages(case, frame, result):
    """The sharpening and the mask behind the averaged result, as the library orders them."""
    clip = clip_format(case.fmt, case.w, case.h)
    proc = processed_planes(clip.planes, case.kw)
    r = result
    if case.sharpen:
        r = sharpen_model(frame, r, case.sharpen[0], case.sharpen[1], clip.bits, proc)
    if case.mask:
        lo, hi, expand, chroma = case.mask
        if chroma == "luma":
            r = merge_model_luma(frame, r, lo, hi, expand, clip.bits, clip.subw, clip.subh, proc)
        else:
            r = merge_model(frame, r, lo, hi, expand, clip.bits, proc)
    return r


_EXPECTED = {}


def expected(i, count=None, order=1, parities=None):
    """(frames, want, last): want[f] the planes of frame f; last = the two results the final average of frame 0 sees.  order and
    parities go to the model, which ignores them."""
    key = (i, count, order, repr(parities))
    if key not in _EXPECTED:
        case = CASES[i]
        clip = clip_format(case.fmt, case.w, case.h)
        frames = frames_of(case, count)
        script = BothScript(clip, order=order, **case.kw, **case.skw)
        want, last = [], None
        for f, fr in enumerate(frames):
            r = script.frame(fr, parity=parities[f] if parities else 1)
            if f == 0:
                last = script.last
            want.append(stages(case, fr, r))
        _EXPECTED[key] = (frames, want, last)
    return _EXPECTED[key]


_ONE = {}


def one_field(i, order):
    """Frame 0 of the case through the one-field script of that order, and the same stages."""
    if (i, order) not in _ONE:
        case = CASES[i]
        clip = clip_format(case.fmt, case.w, case.h)
        fr = frames_of(case)[0]
        _ONE[(i, order)] = stages(case, fr, Script(clip, order=order, **case.kw, **case.skw).frame(fr))
    return _ONE[(i, order)]
