"""Case tables of the fused sweeps in the SSE2 arithmetic (sn_policy.sse2_sweeps = 1), shared by tests/test_sse2_sweeps_gpu.py
and the self-check in tests/test_sse2_sweeps_cpu.py.  TEST INFRASTRUCTURE ONLY.

A case is (format, width, height, filter kwargs, context kwargs, frames, pattern).  The patterns noise01 and checker2 (0 / MAXT
samples) saturate both the SangNom value and the box, so on every 8-bit and 16-bit case the SSE2 model's output differs from
the opt=0 oracle's -- the self-check asserts it for each table entry, and each GPU test asserts it again on its own input
before it looks at the library.  Shapes are the smallest that reach each code path: a 16-bit wave covers 512 columns (480
new ones from the second wave on), seams are exchanged every five rows.
"""
import numpy as np

from avisynth_sangnom2_amd import clip_format, synth
from tests import sse2_model as sm
from tests.util import same

SEED = 1200  # first frame's seed of every case (frame i: SEED + i)

# the reference's own opt=1 outputs on fused-eligible geometry, and the one fixture that is not (72 wide, history-carrying)
FIXTURES = ["sse2_y16", "sse2_y10", "sse2_yuv420p8", "sse2_yuv420p16"]
FIXTURE_NOT_ELIGIBLE = "sse2_y16_noise01"

# the five configurations tests/test_sse2_mode_gpu.py reports as "no sweeps" (knob 0)
REPORTING = [("Y16", 256, 64, {}), ("Y10", 256, 64, {}), ("YUV420P8", 256, 64, dict(aac=48)), ("YUV422P8", 256, 64, dict(aac=48)),
             ("YUV420P16", 256, 64, dict(aac=48, isolated_planes=True))]

# 16-bit planes on their own (kPlain, both boxes; the gather stage 3)
PLAIN16 = [
    ("Y16", 64, 24, {}, {}, 1, "noise01"),
    ("Y16", 512, 24, {}, {}, 1, "checker2"),               # one full wave
    ("Y16", 544, 40, {}, {}, 1, "noise01"),                # a second wave that is nearly all dead lanes: one seam
    ("Y16", 1024, 40, dict(order=0), {}, 2, "noise01"),
    ("Y16", 1920, 24, dict(order=2), {}, 1, "noise"),
    ("Y16", 3840, 24, {}, {}, 1, "noise01"),               # eight waves
    ("Y10", 512, 24, {}, {}, 1, "noise01"),                # (exempt from the differs check, like every 9..15-bit case)
    ("Y16", 256, 20, dict(dh=True), {}, 1, "noise01"),
    ("YUV444P16", 64, 16, dict(aac=48, dh=True), {}, 1, "noise01"),
]

# fresh_pool planes a multiple of 8 and not of 32 wide: the padded sweep (kPadded)
PADDED16 = [("Y16", 104, 24, {}, "noise01"), ("Y16", 1000, 32, dict(order=0), "checker2"), ("YUV420P16", 208, 32, dict(aac=48), "noise01")]

# row bands (BAND of kPlain; of kLumaSpill in the single-frame 4:2:0 hybrid)
BANDS = [("Y16", 960, 200, {}), ("YUV420P8", 256, 128, dict(aac=48)), ("YUV420P16", 256, 128, dict(aac=48))]
BANDS_FRAMES, BANDS_PATTERN = 2, "noise01"

# pool-coupled sweeps (kLumaSpill, kChroma, kChromaLast, the stale waves; 8-bit: U and V as one sweep too)
COUPLED = [
    ("YUV420P8", 128, 32, dict(aac=48), {}, 2, "noise01"),
    ("YUV420P8", 1024, 64, dict(aac=48), {}, 1, "noise01"),
    ("YUV422P8", 128, 24, dict(aac=48), {}, 1, "checker2"),
    ("YUV420P16", 128, 32, dict(aac=48), {}, 2, "noise01"),
    ("YUV420P16", 1088, 64, dict(aac=48), {}, 1, "noise01"),   # two luma waves, a chroma region that ends inside a wave
    ("YUV422P16", 128, 24, dict(aac=48), {}, 1, "noise01"),
    ("YUV420P8", 128, 32, dict(aac=48, order=0), {}, 2, "noise01"),   # parities 1, 0
    ("YUV420P8", 128, 32, dict(aac=48), dict(isolated_planes=True), 2, "noise01"),
    ("YUV420P16", 128, 32, dict(aac=48), dict(isolated_planes=True), 2, "noise01"),
]

HANDOFF = [("YUV420P8", 128, 32), ("YUV420P16", 128, 32)]
HANDOFF_PATTERN, HANDOFF_SEED = "noise01", 5

AA = [("YUV420P8", 128, 64, dict(aac=48)), ("Y16", 128, 64, {})]
AA_FRAMES, AA_PATTERN, AA_SEED = 2, "noise01", 40


def case_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}-{c[6]}-" + "-".join(f"{a}{b}" for a, b in {**c[3], **c[4]}.items())


def frames_of(clip, pattern, n, seed0=SEED):
    return [synth.frame(clip, pattern, seed=seed0 + i) for i in range(n)]


def parities_of(n):
    return [(f + 1) & 1 for f in range(n)]  # 1, 0, 1, ...


def model_kw(clip, kw):
    return dict(bytes=clip.bytes, bits=clip.bits, planes=clip.planes, subw=clip.subw, subh=clip.subh,
                order=kw.get("order", 1), aa=kw.get("aa", 48), aac=kw.get("aac", 0), dh=kw.get("dh", False))


def want(clip, kw, frames, parities, arithmetic, isolated=False, fresh=False):
    """Per frame the planes the reference would give (arithmetic 1: its opt=1 path): one instance with the shared pool, or
    (isolated) one instance per plane, or (fresh) a new instance per plane and frame."""
    if not (isolated or fresh):
        m = sm.model_for(arithmetic, clip.width, clip.height, **model_kw(clip, kw))
        return [m.get_frame(fr, parity=par) for fr, par in zip(frames, parities)]
    out, keep = [], {}
    for fr, par in zip(frames, parities):
        planes = []
        for p in range(clip.planes):
            k = model_kw(clip, kw)
            k.update(planes=1, subw=0, subh=0, aa=k["aa"] if p == 0 else k["aac"])
            if fresh or p not in keep:
                keep[p] = sm.model_for(arithmetic, clip.width >> (clip.subw if p else 0), clip.height >> (clip.subh if p else 0), **k)
            planes.append(keep[p].get_frame([fr[p]], parity=par)[0])
        out.append(planes)
    return out


def differs(a_frames, b_frames):
    return any(not same(a, b) for x, y in zip(a_frames, b_frames) for a, b in zip(x, y))


_cache = {}


def expected(fmt, w, h, kw, ckw, n, pattern, parities=None, seed0=SEED):
    """(clip, frames, parities, the SSE2 model's frames) of a case, computed once per session and never modified.  For 8-bit
    and 16-bit clips asserts that the opt=0 oracle gives something else on this input."""
    key = (fmt, w, h, tuple(sorted(kw.items())), tuple(sorted(ckw.items())), n, pattern, tuple(parities or ()), seed0)
    if key not in _cache:
        clip = clip_format(fmt, w, h)
        frames = frames_of(clip, pattern, n, seed0)
        par = list(parities) if parities else parities_of(n)
        isolated, fresh = bool(ckw.get("isolated_planes")), bool(ckw.get("fresh_pool"))
        out1 = want(clip, kw, frames, par, 1, isolated, fresh)
        if clip.bits in (8, 16):  # (9..15 bits: the two paths almost never differ on in-range samples)
            assert differs(out1, want(clip, kw, frames, par, 0, isolated, fresh)), "this case cannot tell the SSE2 arithmetic from the default"
        for fr in out1:
            for pl in fr:
                pl.setflags(write=False)
        _cache[key] = (clip, frames, par, out1)
    return _cache[key]


def every_case():
    """All table entries in the form expected() takes (the self-check walks them)."""
    for c in PLAIN16 + COUPLED:
        yield c + (None,)
    for fmt, w, h, kw, pattern in PADDED16:
        yield (fmt, w, h, kw, dict(fresh_pool=True), 3, pattern, (1, 0, 1))
    for fmt, w, h, kw in BANDS:
        yield (fmt, w, h, kw, {}, BANDS_FRAMES, BANDS_PATTERN, (1, 1))


def to_torch(planes_per_frame, clip, dev):
    """Frames -> per plane a device tensor [N, H, W] (torch has no uint16: same bits as int16)."""
    import torch
    vt = {1: np.uint8, 2: np.int16, 4: np.float32}[clip.bytes]
    return [torch.from_numpy(np.stack([fr[p] for fr in planes_per_frame]).view(vt)).pin_memory().to(dev) for p in range(clip.planes)]
