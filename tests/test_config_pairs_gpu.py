"""Every row of the covering table of tests/config_space.py on the device: bit-exact against the reference, and on the route
the table predicts.

The other device tests walk one dimension of the library each; the rows here put every feasible pair of option values together
at least once (tests/test_config_pairs_cpu.py proves that from the table).  A row creates its context, sets the row bands where
it says so, runs its frames its way -- twice on the same context where the clip carries history, so that pool state crosses a
call boundary -- compares every plane of every frame with config_space.expected(row), and holds the counters of sn_info,
sn_parts_info and sn_surface_info against config_space.predicted(row).  Device destinations are views into padded allocations
that start from a fill value (tests/layout_cases.py); nothing outside the planes may change.
"""
import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2
from tests import config_space as cs
from tests import layout_cases as lc
from tests import small_plane_cases as sp
from tests.util import describe_diff, same, to_host

pytestmark = pytest.mark.gpu

DST_LAYOUT = "lines"  # base 64, pitch roundup(row, 64) + 64 (1 + p), two pitches between frames: larger than the plane everywhere


def _upload(alloc):
    import torch
    return torch.from_numpy(alloc).pin_memory().to(torch.device("cuda:0"))


def _tview(t, L):
    """The [n, rows, w] view of a plane inside its device allocation."""
    import torch
    flat = t if L.B == 1 else t.view({2: torch.int16, 4: torch.float32}[L.B])
    return flat.as_strided((L.n, L.rows, L.w), (L.stride // L.B, L.pitch // L.B, 1), L.base // L.B)


def _source(row, clip, words, dev):
    """The call's source: planar tensors, or [Y, UV] for a semi-planar source."""
    src = sp.to_torch(words, clip, dev)
    if row["way"] == "semi_in":
        import torch
        src = [src[0], torch.stack([src[1], src[2]], dim=-1).contiguous()]
    return src


def _destination(row, flt, clip, n):
    """(layouts, host allocations, device allocations, the tensors the call takes) of a destination in DST_LAYOUT."""
    shapes = [flt.plane_shape_out(p) for p in range(clip.planes)]
    semi = row["way"] == "semi_out"
    if semi:
        shapes = [shapes[0], (shapes[1][0], 2 * shapes[1][1])]  # a UV plane: rows of U V U V ...
    layouts = lc.batch_layout(DST_LAYOUT, shapes, clip.bytes, n)
    allocs = lc.destination_batch(layouts)
    dev = [_upload(a) for a in allocs]
    views = [_tview(t, L) for t, L in zip(dev, layouts)]
    if semi:
        views[1] = views[1].unflatten(2, (shapes[1][1] // 2, 2))
    return layouts, dev, views, semi


def _as_destination(want, semi):
    """The expected frames in the destination's plane structure."""
    if not semi:
        return want
    return [[fr[0], np.ascontiguousarray(np.stack([fr[1], fr[2]], axis=-1).reshape(fr[1].shape[0], -1))] for fr in want]


def _ring(flt, frames, par, depth):
    """As tools/fuzz.py drives the ring: submit until every slot is in flight, collect the oldest; the rest at the end."""
    assert flt.host_slots() == depth
    got, inflight = [], []
    for fr, pa in zip(frames, par):
        if len(inflight) == depth:
            got.append(flt.collect(inflight.pop(0)))
        inflight.append(flt.submit(fr, parity=pa))
    while inflight:
        got.append(flt.collect(inflight.pop(0)))
    return got


def _call(row, flt, clip, frames, words, par, want):
    """One call of the row's way on n frames; asserts the frames (and, for device ways, the destination's padding)."""
    what, n = row.id, len(frames)
    if row["way"] in ("host", "ring"):
        got = [flt.get_frame(fr, parity=pa) for fr, pa in zip(frames, par)] if row["way"] == "host" else _ring(flt, frames, par, cs.ring_depth(row))
        assert len(got) == n
        for f in range(n):
            for p in range(clip.planes):
                assert got[f][p].shape == want[f][p].shape and same(want[f][p], got[f][p]), f"{what} frame {f} plane {p}: " + describe_diff(want[f][p], got[f][p])
        return
    import torch
    dev = torch.device("cuda:0")
    src = _source(row, clip, words, dev)
    layouts, allocs, dst, semi = _destination(row, flt, clip, n)
    torch.cuda.synchronize()
    if row["way"] == "batch":
        flt.process_batch(src, dst, parity=par)
    else:
        flt.process_surfaces(src, dst, parity=par, src_msb=row["align"] == "msb_in", dst_msb=row["align"] == "msb_out")
    flt.synchronize()
    lc.assert_clean(what, [to_host(t) for t in allocs], layouts, _as_destination(want, semi), clip.dtype)


@pytest.mark.parametrize("row", cs.ALL_ROWS, ids=[r.id for r in cs.ALL_ROWS])
def test_row_is_bit_exact_and_on_its_predicted_route(hip_lib, row):
    clip, frames, par, want = cs.expected(row)
    words = cs.source_words(row)
    n, calls = row["nframes"], cs.calls_of(row)
    assert len(frames) == n * calls
    with SangNom2(clip, **cs.context_kw(row)) as flt:
        if cs.bands_of(row):
            flt.set_bands(*cs.bands_of(row))
        for c in range(calls):
            s = slice(c * n, (c + 1) * n)
            _call(row, flt, clip, frames[s], words[s], par[s], want[s])
        i, pi, si = flt.info(), flt.parts_info(), flt.surface_info()
    got = dict(history_free=i.history_free, fused_eligible=i.fused_eligible, fused_frames=i.fused_frames, banded_frames=i.banded_frames,
               band_fallbacks=i.band_fallbacks, chained_frames=i.chained_frames, uv_sweeps=i.uv_sweeps, part_frames=pi.part_frames,
               split_frames=si.split_frames, merged_frames=si.merged_frames)
    allowed = cs.predicted(row)
    off = {k: (v, sorted(allowed[k])) for k, v in got.items() if v not in allowed[k]}
    assert not off, f"{row.id}: counters outside the prediction (got, allowed): {off}"
    assert i.banded_frames <= i.fused_frames
