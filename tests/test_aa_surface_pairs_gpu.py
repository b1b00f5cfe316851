"""Every ordered pair of surface side classes through sn_aa_process_device_surfaces (tests/aa_surface_pair_cases.py): three clips
of 100 x 16 -- YUV422P10 with the seven side classes of tests/test_surface_pairs_gpu.py, YUV422P8 with planar, NV16, YUY2 and
UYVY, YUV420P8 with planar and NV12 -- in five forms (the call as it is, dh, dh reduced by the half-band kernel, and the first and
the last of them merged through the edge mask) on a context that processes every plane, and without dh on one with chroma=False
and one with luma=False.  Each parameter is ONE context that serves its clip's pairs one after the other, three frames a call
with order=0 and parities (0, 1, 0), against ONE instance of the numpy script: the clip carries history, so call k has to give the
script's frames 3 k .. 3 k + 2 whichever route the frames before them took.  Tolerance zero.

Every source carries junk where it must be ignored, and is compared with what was uploaded when the walk is over: nothing of the
call may write a source (the merge runs in place on the destination).  Every destination row is followed by guard bytes that must
stay.  The counters a call adds and scratch_bytes after it are those recorded in tests/test_surface_pairs_gpu.py wherever the
destination has the source's size on the 10-bit clip (the plan's counters and parts do not depend on all_lines), and the Python
model's (which the CPU test holds against that record) for the dh geometry and the 8-bit clips.

The second test walks seven pairs under a scratch budget that holds four or two of a call's five frames, with parities that
change inside a chunk, and expects the bytes of the unchunked script."""
import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNomAA
from tests import aa_surface_pair_cases as ac
from tests import test_surface_pairs_gpu as sp
from tests.util import describe_diff, same, to_host

pytestmark = pytest.mark.gpu


def walk(clip_name, context, form, pairs, frames, parities, want, **policy):
    """The calls of one context, each checked byte for byte; yields (src, dst, counters the call added, scratch_bytes)."""
    import torch
    clip, n = ac.clip_of(clip_name), len(frames)
    what = f"{clip_name} {context} {form}"
    sides = sorted({s for pair in pairs for s in pair})
    uploaded = {side: sp._rows(clip, frames, side, True) for side in sides}
    raw = {side: [sp._up(a) for a in uploaded[side]] for side in sides}
    sources = {side: sp._tensors(side, raw[side]) for side in sides}
    with SangNomAA(clip, max_batch=n, order=ac.ORDER, **ac.CONTEXTS[context], **ac.FORMS[form], **policy) as aa:
        before = (0, 0, 0)
        for (src, dst), call in zip(pairs, want):
            expect = sp._rows(clip, [fr for _, fr in call], dst, False)
            full, views = sp._guarded(expect)
            s, d = sp._keywords(src), sp._keywords(dst)
            torch.cuda.synchronize()
            aa.process_surfaces(sources[src], sp._tensors(dst, views), parities, src_msb=s["msb"], dst_msb=d["msb"], src_packed=s["packed"],
                                dst_packed=d["packed"])
            aa.synchronize()
            for k, (a, t) in enumerate(zip(expect, full)):
                got = to_host(t).view(a.dtype)
                r = a.shape[2]
                assert same(a, got[:, :, :r]), f"{what} {src} -> {dst} tensor {k}: " + describe_diff(a, np.ascontiguousarray(got[:, :, :r]))
                guard = np.ascontiguousarray(got[:, :, r:]).view(np.uint8)
                assert guard.shape[2] == sp.GUARD_BYTES and np.all(guard == sp.GUARD), f"{what} {src} -> {dst} tensor {k}: bytes between rows written"
            i = aa.surface_info()
            now = (i.split_frames, i.merged_frames, i.copied_frames)
            yield src, dst, tuple(b - a for a, b in zip(before, now)), i.scratch_bytes
            before = now
        for side in sides:
            for k, (a, t) in enumerate(zip(uploaded[side], raw[side])):
                assert same(a, to_host(t).view(a.dtype)), f"{what}: source {side} tensor {k} was written"
        assert aa.info(0).frames == aa.info(1).frames == len(pairs) * n


@pytest.mark.parametrize("clip_name,context,form", [pytest.param(*w, id="-".join(w)) for w in ac.WALKS])
def test_every_pair_of_side_classes(hip_lib, clip_name, context, form):
    pairs = ac.pairs_of(clip_name)
    done = list(walk(clip_name, context, form, pairs, ac.frames_of(clip_name), ac.PARITIES, ac.expected(clip_name, context, form)))
    assert [(s, d) for s, d, _, _ in done] == pairs
    model = [(counters, scratch) for counters, scratch, _, _ in ac.model_counters(clip_name, context, form)]
    if clip_name == "YUV422P10":
        # counters: the record (dh forces every plane: that of "all"); scratch_bytes: the record where the destination has the
        # source's size, the model for dh
        recorded = sp.RECORDED[context]
        assert pairs == sp.PAIRS and len(recorded) == len(pairs)
        want = [(rec[0], mod[1] if form == "dh" else rec[1]) for rec, mod in zip(recorded, model)]
    else:
        want = model
    for (src, dst, counters, scratch), expected in zip(done, want):
        print(f"{clip_name} {context} {form} {src} -> {dst}: {counters} {scratch}")
        assert (counters, scratch) == expected, f"{clip_name} {context} {form} {src} -> {dst}: {(counters, scratch)}, expected {expected}"


@pytest.mark.parametrize("form", ac.CHUNK_FORMS)
def test_chunks_with_a_change_of_parity_inside(hip_lib, form):
    """A budget of 1 MB: no call holds its five frames (a call that fits whole fails the test), the calls behind the first hold
    two, and the chunks run in order: the bytes are the unchunked script's."""
    done = list(walk(ac.CHUNK_CLIP, "all", form, ac.CHUNK_PAIRS, ac.chunk_frames(), ac.CHUNK_PARITIES, ac.chunk_expected(form),
                     scratch_budget_mb=ac.CHUNK_BUDGET_MB))
    model = ac.chunk_counters(form)
    per_frame = ac.ScratchModel(ac.clip_of(ac.CHUNK_CLIP), ac.destination_size(form), ac.CHUNK_N)
    held, caps = frozenset(), []
    for (src, dst, counters, scratch), (want_counters, want_scratch, want_cap, key) in zip(done, model):
        held = held | ac.surface_call(key[0], key[1], key[2], key[3]).parts
        frame = per_frame.per_frame(held)
        assert scratch % frame == 0, f"{src} -> {dst}: scratch_bytes {scratch} is no multiple of a frame's {frame}"
        caps.append(scratch // frame)
        print(f"{form} {src} -> {dst}: {counters} {scratch} = {caps[-1]} frames of {frame}")
        assert 1 <= caps[-1] < ac.CHUNK_N, f"{src} -> {dst}: the scratch holds {caps[-1]} of {ac.CHUNK_N} frames: the call was not chunked"
        assert (counters, scratch) == (want_counters, want_scratch), f"{src} -> {dst}: {(counters, scratch)}, expected {(want_counters, want_scratch)}"
    assert len(caps) == 7 and max(caps) >= 2
