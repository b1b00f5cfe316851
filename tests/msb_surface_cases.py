"""MSB-aligned device surfaces (SN_LAYOUT_PLANAR_MSB / SN_LAYOUT_SEMIPLANAR_MSB: P010, P012): the case table, the sources and
the expected frames of tests/test_msb_surfaces_gpu.py and tests/test_msb_surfaces_cpu.py.  TEST INFRASTRUCTURE ONLY.

One rule defines the result (include/sangnom_hip.h): with ss and ds the shifts of the two sides, 16 - bits for an _MSB layout
and 0 otherwise, the destination holds what the call gives on src >> ss, every sample shifted left by ds.  So the LSB-aligned
frames are tests/surface_cases.py's (synth.frame), their expected frames the CPU oracle's on them (the SSE2 model for opt=1,
tests/aa_script.py / tests/aa_dh_script.py for the anti-aliasing call), and an MSB source is those frames shifted left with
RANDOM NON-ZERO LOW BITS OR-ed in: an implementation that lets low bits through on kept or copied lines fails."""
import numpy as np

from avisynth_sangnom2_amd import clip_format, synth
from tests import surface_cases as sc
from tests.util import same

C = sc.Case
LOW_SEED = 77

PARITY = [
    C("YUV420P10", 256, 64, dict(aac=48), path="sweep"),               # P010: the coupled 16-bit sweeps
    C("YUV420P12", 256, 64, dict(aac=48), path="sweep"),               # P012: shift 4
    C("YUV420P10", 100, 40, n=4),                                      # history-carrying; rows of 200 bytes: vectors, then a ragged tail
    C("YUV420P10", 96, 32, dict(aac=48), path="pool"),
    C("YUV420P10", 128, 24, dict(dh=True)),
    C("YUV420P10", 128, 32, dict(order=0), parities=(0, 1, 0)),        # two field offsets in one call
    C("YUV420P10", 128, 32, {}, dict(opt=1, sse2_sweeps=1), pattern="noise01"),
]
CHUNKED = PARITY[2]
MIXED = C("YUV420P10", 256, 64, dict(aac=48))
# (source semi-planar, source MSB, destination semi-planar, destination MSB)
MIXED_SIDES = [(True, True, False, False), (False, False, True, True), (False, True, True, False), (True, True, False, True)]
LUMA_ONLY = [C("Y10", 64, 32), C("Y10", 3872, 32, {}, dict(column_parts=1), path="sweep")]
COPIED = [C("YUV420P10", 256, 64, dict(chroma=False)), C("YUV420P10", 256, 64, dict(luma=False, aac=30))]
COPIED_SIDES = [(True, True), (True, False)]  # (source MSB, destination MSB), semi-planar both
LAYOUTS = [C("YUV420P10", 256, 64, dict(aac=48)), C("YUV420P10", 100, 40, n=4)]
AA = [("YUV420P10", False), ("YUV420P10", True)]  # 128 x 64
SIXTEEN = C("YUV420P16", 256, 64, dict(aac=48))   # shift 0: the _MSB layouts are the plain ones
REFUSED = [C("YUV420P8", 64, 32), C("YUV420PS", 64, 32)]
EVERY = PARITY + LUMA_ONLY + COPIED  # every clip and argument set of the GPU tests (MIXED and LAYOUTS are among PARITY's)


def shift_of(clip):
    return 16 - clip.bits if clip.bytes == 2 else 0


def low_bits(shape, s, seed):
    """Random values in 1 .. 2^s - 1 (never zero), uint16; zeros for s == 0."""
    if s == 0:
        return np.zeros(shape, dtype=np.uint16)
    r = synth.splitmix64(np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape), seed * 0x10001 + 0x2545F491)
    return (np.uint64(1) + (r >> np.uint64(20)) % np.uint64((1 << s) - 1)).astype(np.uint16)


def up(frames, s):
    """LSB-aligned frames shifted left by s: what an MSB destination has to hold."""
    return [[(pl.astype(np.uint16) << np.uint16(s)).astype(np.uint16) for pl in fr] for fr in frames]


def msb_source(frames, s, seed=LOW_SEED):
    """... and with random non-zero low bits: what an MSB source may hold.  (words >> s) is the frame again."""
    out = []
    for f, fr in enumerate(frames):
        planes = []
        for p, pl in enumerate(fr):
            w = (pl.astype(np.uint16) << np.uint16(s)) | low_bits(pl.shape, s, seed + 16 * f + p)
            assert same(w >> np.uint16(s), pl) and (s == 0 or np.all(w & np.uint16((1 << s) - 1)))
            w.setflags(write=False)
            planes.append(w)
        out.append(planes)
    return out


_cache = {}


def _frozen(frames):
    for fr in frames:
        for pl in fr:
            pl.setflags(write=False)
    return frames


def expected(case):
    """(clip, LSB-aligned frames, parities, the expected LSB-aligned frames): surface_cases.expected, except that for opt=1 the
    SSE2 model's frames are taken as they are (on 9..15-bit samples its two arithmetics rarely differ, which that helper insists on)."""
    if case.ckw.get("opt") != 1:
        return sc.expected(case)
    if case.id not in _cache:
        from tests import sse2_sweep_cases as ssc
        clip, frames = sc.frames_of(case)
        _cache[case.id] = (clip, _frozen(frames), case.par, _frozen(ssc.want(clip, case.kw, frames, case.par, 1)))
    return _cache[case.id]


def as_sixteen(case):
    """The same case on a 16-bit clip: what a caller gets who creates a 16-bit context for MSB-aligned words."""
    return clip_format(case.fmt.replace("P10", "P16").replace("P12", "P16").replace("Y10", "Y16"), case.w, case.h)


def sixteen_bit_result(case, words):
    """What a 16-bit context gives on `words` (frames of 16-bit words), from the same oracle / model."""
    clip16 = as_sixteen(case)
    if case.ckw.get("opt") == 1:
        from tests import sse2_sweep_cases as ssc
        return ssc.want(clip16, case.kw, words, case.par, 1)
    from oracle.oracle import Oracle
    from tests.util import oracle_cfg
    ora = Oracle(oracle_cfg(clip16, **case.kw))
    return [ora.process(fr, parity=par) for fr, par in zip(words, case.par)]


def expected_aa(fmt, dh):
    return sc.expected_aa(fmt, dh)


def sixteen_bit_result_aa(fmt, dh, words):
    from tests import aa_dh_script, aa_script
    clip16 = clip_format(fmt.replace("P10", "P16"), 128, 64)
    script = (aa_dh_script if dh else aa_script).Script(clip16, aac=48)
    return [script.frame(fr) for fr in words]


def roundup256(x):
    return (x + 255) // 256 * 256


def scratch_frame_bytes(clip, src_semi, src_msb, dst_semi, luma=True, chroma=True, dh=False):
    """Scratch per frame as include/sangnom_hip.h documents it: the chroma planes (U and V in the source's and in the
    destination's geometry) when processed chroma passes a semi-planar side or comes from an MSB source, plus one luma plane
    when processed luma comes from an MSB source; pitches rounded up to 256 bytes."""
    s = shift_of(clip) if src_msb else 0
    total = 0
    if clip.planes >= 3 and (chroma or dh) and (src_semi or dst_semi or s):
        total += sc.scratch_frame_bytes(clip, dh)
    if (luma or dh) and s:
        total += roundup256(clip.width * clip.bytes) * clip.height
    return total


def scratch_frames(per_frame, max_batch, budget_mb):
    return max(1, min(max_batch, (budget_mb << 20) // 16 // per_frame))
