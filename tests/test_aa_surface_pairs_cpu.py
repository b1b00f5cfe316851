"""What tests/test_aa_surface_pairs_gpu.py relies on, checked without a GPU (tests/aa_surface_pair_cases.py):
  - the edge mask of every source plane holds all three classes, so a masked form exercises keep, ramp and replace;
  - the expected frames of the forms, contexts and parities differ from one another plane by plane, so a call that took another
    route cannot pass (the idiom of tests/sse2_sweep_cases.differs);
  - the scratch and counter model written from the documents gives the 147 entries recorded from the library that still had its
    hand-written walks, and only then speaks for the dh geometry, the 8-bit clips and the chunked walk;
  - a laid-out source, unpacked again by the numpy unpackers, is the planar frame it was made from.

Two figures about the expected frames, as they come from the models:
  - parities (0, 1, 0) against (1, 1, 1) differ in every processed plane of frames 0 and 2.  Frame 1 has parity 1 in both and can
    differ through the passes' history only, which on this clip does not reach every plane (10-bit plain: 46 of the 147 planes
    of the walk's frames 1 are the same); so every frame is also held against (1, 0, 1), where each frame's own parity differs.
  - chroma_off against all differ in every chroma plane.  Luma is processed alike in both, and differs only through the history
    the planes share (the first frame's luma is the same), so it is not asserted."""
import pytest

from tests import aa_surface_pair_cases as ac
from tests import test_surface_pairs_gpu as sp
from tests.util import same

ALL_WALKS = [pytest.param(*w, id="-".join(w)) for w in ac.WALKS]


def _planes(context, form, processed=True):
    return [p for p, on in enumerate(ac.processed_of(context, form)) if on == processed]


def _equal_planes(a, b, frames, planes, which=1):
    """(call, frame, plane) where two walks' frames are the same; which: 0 the unmasked result, 1 the expected frame."""
    return [(k, f, p) for k, (ca, cb) in enumerate(zip(a, b)) for f in frames for p in planes if same(ca[f][which][p], cb[f][which][p])]


@pytest.mark.parametrize("clip_name", list(ac.CLIPS))
def test_every_source_plane_has_the_three_mask_classes(clip_name):
    clip = ac.clip_of(clip_name)
    for f, fr in enumerate(ac.frames_of(clip_name)):
        for p, pl in enumerate(fr):
            for expand in (0, 1):
                assert ac.mask_classes(pl, expand, clip.bits) == (True, True, True), f"{clip_name} frame {f} plane {p} expand {expand}"


@pytest.mark.parametrize("clip_name,context,form", ALL_WALKS)
def test_the_parities_are_told_apart(clip_name, context, form):
    want, planes = ac.expected(clip_name, context, form), _planes(context, form)
    assert len(want) == len(ac.pairs_of(clip_name)) and all(len(call) == ac.N for call in want) and planes
    assert not _equal_planes(want, ac.expected(clip_name, context, form, (1, 1, 1)), (0, 2), planes)
    assert not _equal_planes(want, ac.expected(clip_name, context, form, (1, 0, 1)), (0, 1, 2), planes)


@pytest.mark.parametrize("clip_name,context,form", [w for w in ALL_WALKS if "mask" in w.values[2]])
def test_a_masked_frame_is_neither_the_result_nor_the_source(clip_name, context, form):
    frames = ac.frames_of(clip_name)
    for k, call in enumerate(ac.expected(clip_name, context, form)):
        for f, (unmasked, want) in enumerate(call):
            for p in _planes(context, form):
                assert not same(want[p], unmasked[p]) and not same(want[p], frames[f][p]), f"call {k} frame {f} plane {p}"
            for p in _planes(context, form, processed=False):  # not merged: the source as it is
                assert same(want[p], frames[f][p]) and same(unmasked[p], frames[f][p]), f"call {k} frame {f} plane {p}"


@pytest.mark.parametrize("clip_name", list(ac.CLIPS))
@pytest.mark.parametrize("form", ["plain", "plain+mask"])
def test_the_contexts_are_told_apart(clip_name, form):
    every = ac.expected(clip_name, "all", form)
    frames = range(ac.N)
    for context in ("chroma_off", "luma_off"):
        off = _planes(context, form, processed=False)
        assert off and not _equal_planes(ac.expected(clip_name, context, form), every, frames, off), context
    # luma_off has another aac as well: its chroma is not the chroma of `all`
    assert not _equal_planes(ac.expected(clip_name, "luma_off", form), every, frames, (1, 2))


@pytest.mark.parametrize("clip_name", list(ac.CLIPS))
def test_the_forms_are_told_apart(clip_name):
    frames, planes = range(ac.N), (0, 1, 2)
    assert not _equal_planes(ac.expected(clip_name, "all", "reduce"), ac.expected(clip_name, "all", "plain"), frames, planes)
    assert not _equal_planes(ac.expected(clip_name, "all", "reduce+mask"), ac.expected(clip_name, "all", "plain+mask"), frames, planes)
    assert not _equal_planes(ac.expected(clip_name, "all", "reduce+mask"), ac.expected(clip_name, "all", "reduce"), frames, planes)
    # dh has another size altogether
    dw, dh = ac.destination_size("dh")
    assert all(fr[1][0].shape == (dh, dw) == (2 * ac.H, 2 * ac.W) for call in ac.expected(clip_name, "all", "dh") for fr in call)


def test_the_scratch_model_gives_the_recorded_entries():
    """All 147: three contexts, 49 pairs each, counters and scratch_bytes.  The plan's counters and parts do not depend on
    all_lines, so the plain call's record speaks for the anti-aliasing call at source size."""
    seen = 0
    for context, recorded in sp.RECORDED.items():
        got = ac.model_counters("YUV422P10", context, "plain")
        assert ac.pairs_of("YUV422P10") == sp.PAIRS and len(got) == len(recorded) == 49
        for (src, dst), (counters, scratch, cap, _), entry in zip(sp.PAIRS, got, recorded):
            assert (counters, scratch) == entry, f"{context} {src} -> {dst}: the model gives {(counters, scratch)}, recorded {entry}"
            assert cap in (0, ac.N)
            seen += 1
    assert seen == 147


def test_the_scratch_model_on_the_other_geometries():
    """Spot values worked out by hand from the header's table, pitches rounded up to 256."""
    # dh: source 100 x 16, destination 200 x 32, 2 bytes: in 2 * 256 * 16, y 256 * 16, out 2 * 256 * 32, yo 512 * 32
    assert ac.part_bytes(ac.clip_of("YUV422P10"), ac.destination_size("dh")) == {"in": 8192, "y": 4096, "out": 16384, "yo": 16384}
    assert ac.part_bytes(ac.clip_of("YUV422P10"), ac.destination_size("reduce")) == {"in": 8192, "y": 4096, "out": 8192, "yo": 4096}
    assert ac.part_bytes(ac.clip_of("YUV420P8"), ac.destination_size("plain")) == {"in": 4096, "y": 4096, "out": 4096, "yo": 4096}
    assert ac.part_bytes(ac.clip_of("YUV420P8"), ac.destination_size("dh")) == {"in": 4096, "y": 4096, "out": 8192, "yo": 8192}
    dh = ac.model_counters("YUV422P10", "all", "dh")
    assert [c[:2] for c in dh[:5]] == [((0, 0, 0), 0), ((0, 0, 0), 0), ((0, 3, 0), 3 * 24576), ((0, 3, 0), 3 * 24576), ((0, 3, 0), 3 * 40960)]
    assert dh[-1][:2] == ((3, 3, 0), 3 * 45056)
    # 8-bit: no _MSB side, so luma never comes in through scratch unless the source is packed
    p8 = dict(zip(ac.pairs_of("YUV422P8"), ac.model_counters("YUV422P8", "chroma_off", "plain")))
    assert p8[("planar", "planar")][:2] == ((0, 0, 0), 0) and p8[("planar", "nv16")][:2] == ((0, 0, 3), 0)
    assert p8[("planar", "yuyv")][:2] == ((0, 3, 3), 3 * 12288) and p8[("uyvy", "uyvy")][:2] == ((3, 3, 3), 3 * 24576)
    nv12 = ac.model_counters("YUV420P8", "all", "plain")
    assert [c[:2] for c in nv12] == [((0, 0, 0), 0), ((0, 3, 0), 3 * 8192), ((3, 0, 0), 3 * 8192), ((3, 3, 0), 3 * 8192)]


def test_the_walks_reach_many_plans():
    """Calls and distinct inputs of surface_plan() (side classes, processed planes) over all the walks, planar -> planar apart."""
    calls, plans = 0, set()
    for clip_name, context, form in ac.WALKS:
        for counters, scratch, cap, key in ac.model_counters(clip_name, context, form):
            calls += 1
            if key[0] != key[1] or key[0].packed or key[0].semi or key[0].shift:
                plans.add(key)
    print(f"{calls} calls, {len(plans)} distinct plan inputs")
    assert calls == (49 + 16 + 4) * 9 == 621 and len(plans) == 105


@pytest.mark.parametrize("form", ac.CHUNK_FORMS)
def test_the_chunked_walk_never_fits_whole(form):
    """Every one of the seven calls holds fewer frames than the batch, at least one holds two or more, and wherever two or more
    are held a chunk has a change of field offset inside it."""
    caps = [c[2] for c in ac.chunk_counters(form)]
    assert len(caps) == 7 and sorted(s for s, _ in ac.CHUNK_PAIRS) == sorted(d for _, d in ac.CHUNK_PAIRS) == sorted(sp.SIDES)
    assert all(1 <= cap < ac.CHUNK_N for cap in caps) and any(cap >= 2 for cap in caps), caps
    for cap in set(caps):
        chunks = [ac.CHUNK_PARITIES[i:i + cap] for i in range(0, ac.CHUNK_N, cap)]
        assert cap < 2 or any(len(set(c)) == 2 for c in chunks), (cap, chunks)
    other = ac.chunk_expected(form, tuple(1 - q for q in ac.CHUNK_PARITIES))
    assert not _equal_planes(ac.chunk_expected(form), other, range(ac.CHUNK_N), (0, 1, 2))


@pytest.mark.parametrize("clip_name", list(ac.CLIPS))
def test_a_laid_out_source_unpacks_to_the_planar_frames(clip_name):
    """Sources (with their junk) and destinations of every side class of the clip, the uyvy and nv12 helpers included."""
    clip, frames = ac.clip_of(clip_name), ac.frames_of(clip_name)
    for side in ac.CLIPS[clip_name]:
        for source in (True, False):
            arrays = sp._rows(clip, frames, side, source)
            assert all(a.shape[:2] == (ac.N, ac.H >> (clip.subh if i else 0)) for i, a in enumerate(arrays)), side
            back = ac.planar_again(clip, side, arrays)
            for f, fr in enumerate(frames):
                for p in range(3):
                    assert back[f][p].shape == fr[p].shape and same(back[f][p], fr[p]), f"{clip_name} {side} source={source} frame {f} plane {p}"
    if clip_name == "YUV422P8":  # the byte orders really are two
        assert not same(sp._rows(clip, frames, "yuyv", True)[0], sp._rows(clip, frames, "uyvy", True)[0])
    if clip.bits == 10:  # the junk is there: an MSB source is not the destination's words, a v210 source has bits 30-31 set
        for side in ("planar_msb", "nv16_msb", "yuyv_msb", "v210"):
            assert not same(sp._rows(clip, frames, side, True)[0], sp._rows(clip, frames, side, False)[0]), side
