"""sn_aa_process_device_surfaces through every ordered pair of side classes: the clips, forms, contexts, expected frames and the
scratch / counter model of tests/test_aa_surface_pairs_cpu.py and tests/test_aa_surface_pairs_gpu.py.  TEST INFRASTRUCTURE ONLY.

Three clips of 100 x 16 -- no multiple of 32, so both passes carry history from call to call; 100 mod 6 = 4 leaves v210 a partial
group and the 200 of a dh destination another (200 mod 6 = 2):
    YUV422P10  the seven SIDES of tests/test_surface_pairs_gpu.py, 49 pairs
    YUV422P8   planar, nv16, yuyv, uyvy: 16 pairs (8-bit: copy|shift16 is 2-D copies; the second byte order)
    YUV420P8   planar, nv12: 4 pairs
Three frames per call, order=0 with parities (0, 1, 0): two field offsets inside a call, so the turns and the reduction are cut
into runs.  The frames are pattern "edges" of synth with tests/mask_cases.good_seeds(301, 3): every plane's edge mask holds all
three classes (the CPU test asserts it).  ONE model instance per walk is fed the same three frames once per call: call k has to
give the model's frames 3 k .. 3 k + 2.

The scratch and counter model (side_class, surface_call, ScratchModel) is written from the table and the text of
include/sangnom_hip.h ("Decoder and encoder surfaces", "Packed 4:2:2") and the comment block of csrc/sn_surface_plan.h, not from
running the library; the CPU test holds it against the 147 recorded entries of tests/test_surface_pairs_gpu.py before anything
else relies on it."""
from dataclasses import dataclass

import numpy as np

from avisynth_sangnom2_amd import clip_format, synth
from tests import mask_cases as kc
from tests import msb_surface_cases as mc
from tests import packed_surface_cases as pc
from tests import test_surface_pairs_gpu as sp  # SIDES, RECORDED and the helpers that lay a side out
from tests.aa_dh_script import Script as DhScript
from tests.aa_script import Script
from tests.mask_model import edge_mask, merge_model
from tests.reduce_model import reduce_model

W, H, N = 100, 16, 3
ORDER, PARITIES = 0, (0, 1, 0)
LO, HI = kc.LO, kc.HI
CLIPS = {"YUV422P10": sp.SIDES, "YUV422P8": ("planar", "nv16", "yuyv", "uyvy"), "YUV420P8": ("planar", "nv12")}
MASK = dict(mask=(LO, HI))
# the library's keywords of a form; "plain" is the call as it is
FORMS = {
    "plain": {},
    "dh": dict(dh=True),
    "reduce": dict(dh=True, reduce="halfband"),
    "plain+mask": dict(mask_expand=1, **MASK),
    "reduce+mask": dict(dh=True, reduce="halfband", mask_expand=0, **MASK),
}
CONTEXTS = {"all": dict(aac=48), "chroma_off": dict(aac=48, chroma=False), "luma_off": dict(luma=False, aac=30)}
# dh forces every plane, so only the forms without it tell the three contexts apart
WALKS = [(clip, context, form) for clip in CLIPS for context in CONTEXTS for form in FORMS
         if context == "all" or form in ("plain", "plain+mask")]


def pairs_of(clip_name):
    sides = CLIPS[clip_name]
    return [(s, d) for s in sides for d in sides]


def clip_of(clip_name):
    return clip_format(clip_name, W, H)


def frames_of(clip_name, count=N):
    clip = clip_of(clip_name)
    frames = [synth.frame(clip, "edges", seed=s) for s in kc.good_seeds(301, count)]
    for fr in frames:
        for pl in fr:
            pl.setflags(write=False)
    return frames


def processed_of(context, form):
    """Per plane: the passes work on it (dh forces every plane)."""
    kw = CONTEXTS[context]
    dh = bool(FORMS[form].get("dh"))
    return [dh or kw.get("luma", True)] + [dh or kw.get("chroma", True)] * 2


def destination_size(form):
    """(width, height) of the destination's luma."""
    kw = FORMS[form]
    return (2 * W, 2 * H) if kw.get("dh") and not kw.get("reduce") else (W, H)


# ---- the expected frames -------------------------------------------------------------------------------------------------------

def model_walk(clip_name, context, form, frames, parities, calls):
    """`calls` calls of one context, each on the same `frames`: per call and frame (the unmasked result, the expected frame),
    planar and LSB-aligned, from ONE instance of the script."""
    clip, kw, fkw = clip_of(clip_name), CONTEXTS[context], FORMS[form]
    dh, reduce, mask = bool(fkw.get("dh")), fkw.get("reduce"), "mask" in fkw
    script = DhScript(clip, order=ORDER, aac=kw["aac"]) if dh else Script(clip, order=ORDER, **kw)
    proc = None if dh else processed_of(context, form)
    out = []
    for _ in range(calls):
        call = []
        for fr, q in zip(frames, parities):
            r = script.frame(fr, parity=q)
            if reduce:
                r = reduce_model(r, reduce, order=ORDER, parity=q, bits=clip.bits)
            want = merge_model(fr, r, LO, HI, fkw["mask_expand"], clip.bits, proc) if mask else r
            for pl in list(r) + list(want):
                pl.setflags(write=False)
            call.append((r, want))
        out.append(call)
    return out


_cache = {}


def expected(clip_name, context, form, parities=PARITIES):
    """model_walk over that clip's pairs on its three frames, once per session and left unchanged."""
    key = (clip_name, context, form, tuple(parities))
    if key not in _cache:
        _cache[key] = model_walk(clip_name, context, form, frames_of(clip_name), parities, len(pairs_of(clip_name)))
    return _cache[key]


def mask_classes(plane, expand, bits):
    """(some m = 0, some 0 < m < 256, some m = 256) of a source plane's edge mask."""
    m = edge_mask(plane, LO, HI, expand, bits)
    return bool((m == 0).any()), bool(((m > 0) & (m < 256)).any()), bool((m == 256).any())


# ---- laying out the sides ------------------------------------------------------------------------------------------------------

def planar_again(clip, side, arrays):
    """What tests/test_surface_pairs_gpu._rows laid out, unpacked with the numpy unpackers of the layout modules: per frame the
    LSB-aligned planar planes."""
    n = arrays[0].shape[0]
    if sp._packed(side):
        return pc.unpack_frames(side, clip, [arrays[0][f] for f in range(n)])
    s = mc.shift_of(clip) if side.endswith("_msb") else 0
    planes = [arrays[0], arrays[1][..., 0::2], arrays[1][..., 1::2]] if side.startswith("nv") else list(arrays)
    return [[np.ascontiguousarray(pl[f] >> s if s else pl[f]) for pl in planes] for f in range(n)]


# ---- scratch and counters, from the documents ------------------------------------------------------------------------------------

@dataclass(frozen=True)
class SideClass:
    packed: bool  # SN_LAYOUT_PACKED_*: one plane holds Y, U and V
    semi: bool    # SN_LAYOUT_SEMIPLANAR*: one UV plane
    shift: int    # an _MSB layout: 16 - bits_per_sample zero bits below every sample; 0 on a 16-bit clip and without _MSB


def side_class(side, clip):
    msb = side.endswith("_msb")
    return SideClass(sp._packed(side), side.startswith("nv"), mc.shift_of(clip) if msb else 0)


@dataclass(frozen=True)
class SurfaceCall:
    split: bool   # the call's frames count in split_frames
    merged: bool  # ... in merged_frames
    copied: bool  # ... in copied_frames
    parts: frozenset  # of "in" (U and V, source geometry), "out" (U and V, destination geometry), "y", "yo": the scratch it needs


def surface_call(src, dst, luma, chroma, planes=3):
    """One surface call of a context that processes luma / chroma (dh: both), by the header's rules.
    Both sides SN_LAYOUT_PLANAR: the call IS the strided call, no scratch and no counter.
    With a packed side every plane goes through its planar form, the table of "Packed 4:2:2":
        source packed, MSB-aligned or semi-planar: U and V in;  source packed or MSB-aligned: Y in;
        destination packed or semi-planar: U and V out;         destination packed: Y out;
        a packed or semi-planar source frame is split once, a packed or semi-planar destination frame merged once.
    Without one: both chroma geometries when processed chroma passes a semi-planar side or comes from an MSB-aligned source, one
    luma plane when processed luma comes from an MSB-aligned source; chroma that is not processed never reaches scratch or a pass
    (a UV plane is split / merged for the passes only).
    copied_frames: the call's frames whenever the clip has chroma that is not processed."""
    has_chroma = planes >= 3
    if not (src.packed or src.semi or src.shift or dst.packed or dst.semi or dst.shift):
        return SurfaceCall(False, False, False, frozenset())
    parts = set()
    if src.packed or dst.packed:
        if src.packed or src.semi or src.shift:
            parts.add("in")
        if src.packed or src.shift:
            parts.add("y")
        if dst.packed or dst.semi:
            parts.add("out")
        if dst.packed:
            parts.add("yo")
        split, merged = src.packed or src.semi, dst.packed or dst.semi
    else:
        if has_chroma and chroma and (src.semi or dst.semi or src.shift):
            parts |= {"in", "out"}
        if luma and src.shift:
            parts.add("y")
        split, merged = has_chroma and chroma and src.semi, has_chroma and chroma and dst.semi
    return SurfaceCall(bool(split), bool(merged), has_chroma and not chroma, frozenset(parts))


def part_bytes(clip, dst_size):
    """Bytes per frame of each scratch part: pitches rounded up to 256; "in" and "out" are two planes."""
    B = clip.bytes
    R = mc.roundup256
    (w, h), (ow, oh) = (clip.width, clip.height), dst_size
    return {"in": 2 * R((w >> clip.subw) * B) * (h >> clip.subh), "y": R(w * B) * h,
            "out": 2 * R((ow >> clip.subw) * B) * (oh >> clip.subh), "yo": R(ow * B) * oh}


DEFAULT_BUDGET = 24 << 30  # sn_policy.scratch_budget_mb = 0: a sixteenth of it is the header's 1.5 GiB


class ScratchModel:
    """What a context holds across its calls: a call whose need grows gives back what the context holds and takes the union of
    what it held and what the call needs, for min(max_batch, what a sixteenth of the budget holds, at least 1) frames."""

    def __init__(self, clip, dst_size, max_batch, budget=DEFAULT_BUDGET):
        self.bytes_of = part_bytes(clip, dst_size)
        self.max_batch, self.budget = max_batch, budget
        self.held, self.cap = frozenset(), 0

    def per_frame(self, parts=None):
        return sum(self.bytes_of[p] for p in (self.held if parts is None else parts))

    def call(self, call, n):
        """-> ((split, merged, copied) frames the call adds, scratch_bytes after it, frames the scratch holds)."""
        if not call.parts <= self.held:
            self.held = self.held | call.parts
            self.cap = max(1, min(self.max_batch, self.budget // 16 // self.per_frame()))
        return (n * call.split, n * call.merged, n * call.copied), self.per_frame() * self.cap, self.cap


def model_counters(clip_name, context, form, pairs=None, n=N, max_batch=N, budget=DEFAULT_BUDGET):
    """Per pair of a walk: (counters added, scratch_bytes after the call, frames the scratch holds, the plan's inputs)."""
    clip = clip_of(clip_name)
    proc = processed_of(context, form)
    model = ScratchModel(clip, destination_size(form), max_batch, budget)
    out = []
    for s, d in (pairs_of(clip_name) if pairs is None else pairs):
        sc_, dc = side_class(s, clip), side_class(d, clip)
        out.append(model.call(surface_call(sc_, dc, proc[0], proc[1], clip.planes), n) + ((sc_, dc, proc[0], proc[1]),))
    return out


# ---- the chunked walk ----------------------------------------------------------------------------------------------------------
# Seven pairs, every class once a source and once a destination, on a budget of 1 MB: a sixteenth of it is 65 536 bytes.  A part
# of this clip is 4 096 bytes per plane and frame, so the first call (planar -> nv16_msb: U and V in and out, 16 384) holds four of
# the five frames and every later one (all six planes, 24 576) two.  Parities (0, 1, 1, 0, 1): chunks of four (0 1 1 0 | 1) and of
# two (0 1 | 1 0 | 1) both have a change of field offset inside a chunk.
CHUNK_CLIP = "YUV422P10"
CHUNK_N, CHUNK_PARITIES, CHUNK_BUDGET_MB = 5, (0, 1, 1, 0, 1), 1
CHUNK_PAIRS = [(sp.SIDES[i], sp.SIDES[(i + 3) % 7]) for i in range(7)]
CHUNK_FORMS = ("reduce+mask", "plain")


def chunk_frames():
    """Five frames: the clip's three and the first two of them again (their parities and the history before them differ).  The
    next two "edges" frames tell the parities apart less well: the fourth's half-band-reduced luma differs in 48 samples between
    its two parities, and the mask keeps all but five of them from the result."""
    frames = frames_of(CHUNK_CLIP)
    return [frames[f % N] for f in range(CHUNK_N)]


def chunk_expected(form, parities=CHUNK_PARITIES):
    key = ("chunks", form, tuple(parities))
    if key not in _cache:
        _cache[key] = model_walk(CHUNK_CLIP, "all", form, chunk_frames(), parities, len(CHUNK_PAIRS))
    return _cache[key]


def chunk_counters(form):
    return model_counters(CHUNK_CLIP, "all", form, CHUNK_PAIRS, CHUNK_N, CHUNK_N, CHUNK_BUDGET_MB << 20)
