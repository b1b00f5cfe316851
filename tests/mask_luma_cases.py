"""The frames of the tests of the luma-derived chroma mask, shared by the CPU test (which asserts the class condition) and
the GPU tests.  Pattern "edges" with thresholds (40, 96) and frame seeds s with s % 7 == 6: their luma plane (seed 3 s) has
stripes of slope 1, their chroma planes slopes 2 and 3, none vertical.  With tests/mask_cases.py's thresholds (16, 96) the
block mean of the luma mask leaves one class of mc nearly empty; with these every chroma plane holds at least 5 % of each
of mc = 0, 0 < mc < 256 and mc = 256, and mc differs from the plane's own mask on about half of it."""
from avisynth_sangnom2_amd import clip_format, synth
from tests.aa_dh_script import Script as DhScript
from tests.aa_script import Script
from tests.mask_luma_model import merge_model_luma
from tests.mask_model import merge_model
from tests.reduce_model import reduce_model

LO, HI = 40, 96
EXPANDS = (0, 1)
SEEDS = (307, 314, 321, 328)
NFRAMES = len(SEEDS)

# (format, width, height, filter kwargs, context kwargs, script kwargs, parities)
BATCH = [
    ("YUV420P8", 128, 64, dict(aac=48), {}, {}, None),
    ("YUV420P8", 96, 80, {}, {}, {}, None),                      # history in the turned pass
    ("YUV422P8", 128, 64, {}, {}, {}, None),
    ("YUV444PS", 64, 32, {}, {}, {}, None),
    ("YUV420P10", 128, 64, {}, {}, {}, None),
    ("YUV420P16", 96, 64, dict(order=2), {}, {}, None),
    ("YUV420P8", 128, 64, dict(order=0), {}, {}, [1, 0, 0, 1]),
    ("YUV420P8", 128, 64, {}, dict(opt=1), dict(opt=1), None),
]
CHROMA_OFF = ("YUV420P8", 128, 64, dict(chroma=False), {}, {}, None)  # without dh only: luma by its own mask, chroma copied
Y8 = ("Y8", 128, 64, {}, {}, {}, None)                                 # the option has no effect
CHUNK = ("YUV420P8", 512, 256, {}, {}, {}, None)                      # a batch walked in chunks under a small scratch budget
HOST = BATCH[0]
NV12 = BATCH[0]
P010 = BATCH[4]
YUY2 = BATCH[2]
# the sizes the class condition was measured on beyond the cases above
EXTRA_SIZES = [("YUV420P8", 40, 96), ("YUV420P8", 200, 136), ("YUV422P10", 128, 64), ("YUV420PS", 64, 48)]


def frames_of(fmt, w, h, count=NFRAMES):
    clip = clip_format(fmt, w, h)
    return [synth.frame(clip, "edges", seed=s) for s in SEEDS[:count]]


def kernel_of(i):
    """The first row runs both reduce kernels, the others the half-band one."""
    return ["tent", "halfband"] if i == 0 else ["halfband"]


_UNMASKED = {}  # (case, form, count) -> (frames, parities, the unmasked model's frames): computed once, left unchanged


def unmasked(case, form, count=NFRAMES):
    """form: "tent" | "halfband" (dh + reduce) or None (without dh).  Returns (frames, parities, unmasked result per frame)."""
    key = (repr(case), form, count)
    if key not in _UNMASKED:
        fmt, w, h, kw, ckw, skw, par = case[:7]
        clip = clip_format(fmt, w, h)
        frames = frames_of(fmt, w, h, count)
        parities = (par or [1] * NFRAMES)[:count]
        if form is None:
            script = Script(clip, **kw, **skw)
            res = [script.frame(fr, parity=parities[f]) for f, fr in enumerate(frames)]
        else:
            dkw = {k: v for k, v in kw.items() if k not in ("luma", "chroma")}
            script = DhScript(clip, **dkw, **skw)
            res = [reduce_model(script.frame(fr, parity=parities[f]), form, order=kw.get("order", 1), parity=parities[f], bits=clip.bits)
                   for f, fr in enumerate(frames)]
        _UNMASKED[key] = (frames, parities, res)
    return _UNMASKED[key]


def processed_of(case):
    fmt, kw = case[0], case[3]
    planes = clip_format(fmt, case[1], case[2]).planes
    return [bool(kw.get("luma", True))] + [bool(kw.get("chroma", True))] * (planes - 1)


def expected(case, form, expand, count=NFRAMES):
    """(frames, parities, unmasked, merged through luma's mask, merged through every plane's own mask) of a case."""
    frames, parities, res = unmasked(case, form, count)
    clip = clip_format(case[0], case[1], case[2])
    proc = processed_of(case) if form is None else None
    want = [merge_model_luma(fr, r, LO, HI, expand, clip.bits, clip.subw, clip.subh, proc) for fr, r in zip(frames, res)]
    own = [merge_model(fr, r, LO, HI, expand, clip.bits, proc) for fr, r in zip(frames, res)]
    return frames, parities, res, want, own
