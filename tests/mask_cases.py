"""The frames of the edge-mask tests of the anti-aliasing call, shared by the CPU test (which asserts that every plane of
every one of them holds all three classes of the mask: m = 0, 0 < m < 256, m = 256) and the GPU tests.  Pattern "edges" of
synth: slanted stripes with jitter ("noise" and "checker" saturate the mask, "sine" never reaches 256).  The seeds are
chosen so that no plane has vertical stripes (a plane seed that is 3 modulo 7), which have no ramp class."""
from avisynth_sangnom2_amd import clip_format, synth
from tests.aa_dh_script import Script as DhScript
from tests.aa_script import Script
from tests.mask_model import merge_model
from tests.reduce_model import reduce_model

LO, HI = 16, 96
EXPANDS = (0, 1)

# (format, width, height, filter kwargs, context kwargs, script kwargs, parities of the first call)
BATCH = [
    ("Y8", 128, 64, {}, {}, {}, None),
    ("Y8", 96, 80, {}, {}, {}, None),                      # history in the turned pass
    ("Y8", 40, 96, {}, {}, {}, None),                      # history in the second pass
    ("Y8", 200, 136, {}, {}, {}, None),                    # ragged tiles
    ("Y32", 132, 66, {}, {}, {}, None),
    ("Y16", 96, 64, dict(order=2), {}, {}, None),
    ("Y10", 64, 48, {}, {}, {}, None),
    ("YUV420P8", 128, 64, dict(aac=48), {}, {}, None),
    ("YUV422P8", 128, 64, dict(aac=48), {}, {}, None),
    ("YUV444PS", 64, 32, {}, {}, {}, None),
    ("Y8", 128, 64, dict(order=0), {}, {}, [1, 0, 0, 1, 1]),
    ("Y8", 128, 64, {}, dict(opt=1), dict(opt=1), None),
]
LUMA_OFF = ("YUV420P8", 128, 64, dict(luma=False, aac=48), {}, {}, None)  # without dh only: luma is copied, chroma merged
HOST = [("Y8", 128, 64, {}), ("YUV420P8", 128, 64, dict(aac=48)), ("Y16", 96, 64, {})]
CHUNK = ("Y8", 512, 256, {}, {}, {}, None)                       # a batch walked in chunks under a small scratch budget
P010 = ("YUV420P10", 128, 64, dict(aac=48), {}, {}, None)        # a SEMIPLANAR_MSB source

NFRAMES = 8


def good_seeds(first, count, planes=3):
    """`count` frame seeds from `first` on whose planes (plane seed 3 s + p) all have slanted stripes."""
    out, s = [], first
    while len(out) < count:
        if all((3 * s + p) % 7 != 3 for p in range(planes)):
            out.append(s)
        s += 1
    return out


def frames_of(fmt, w, h, first=301, count=NFRAMES):
    clip = clip_format(fmt, w, h)
    return [synth.frame(clip, "edges", seed=s) for s in good_seeds(first, count)]


def kernel_of(i):
    """The first row runs both reduce kernels, the others the half-band one."""
    return ["tent", "halfband"] if i == 0 else ["halfband"]


_UNMASKED = {}  # (case, form) -> (frames, parities, the unmasked model's frames): computed once, left unchanged


def unmasked(case, form, count=NFRAMES, first=301):
    """form: "tent" | "halfband" (dh + reduce) or None (without dh).  Returns (frames, parities, unmasked result per frame)."""
    key = (repr(case), form, count, first)
    if key not in _UNMASKED:
        fmt, w, h, kw, ckw, skw, par = case[:7]
        clip = clip_format(fmt, w, h)
        frames = frames_of(fmt, w, h, first, count)
        parities = ((par or [1] * 5) + [1, 1, 1])[:count]
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


def expected(case, form, expand, count=NFRAMES, first=301):
    """(frames, parities, unmasked, merged) of a case."""
    frames, parities, res = unmasked(case, form, count, first)
    bits = clip_format(case[0], case[1], case[2]).bits
    proc = processed_of(case) if form is None else None
    return frames, parities, res, [merge_model(fr, r, LO, HI, expand, bits, proc) for fr, r in zip(frames, res)]
