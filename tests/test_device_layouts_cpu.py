"""The layout helpers of tests/test_device_layouts_gpu.py, checked on numpy arrays (no library call): that the two layouts
are in the alignment classes tests/layout_cases.py claims for every case of the matrix, that its mask is the complement of
the planes, and that its checker sees a byte flipped right of a row, between two frames and before the base.
"""
import numpy as np
import pytest

from avisynth_sangnom2_amd import clip_format
from tests import layout_cases as lc

ARR_IDS = [f"{s}-to-{d}" for s, d in lc.ARRANGEMENTS]


def _all_layouts():
    """(what, source layouts, destination layouts, fused) of every launch of the GPU file."""
    for case in lc.ALL:
        for arr in lc.ARRANGEMENTS:
            yield (f"{case.id} {arr[0]}->{arr[1]}",) + lc.layouts_of(case, arr) + (case.fused,)
    for fmt, w, h in lc.TURNS:
        B = clip_format(fmt, w, h).bytes
        for arr in lc.ARRANGEMENTS:
            yield f"turn {fmt} {w}x{h}", lc.batch_layout(arr[0], [(h, w)], B, lc.NFRAMES), lc.batch_layout(arr[1], [(w, h)], B, lc.NFRAMES), False


def test_the_matrix_has_every_case_once():
    ids = [c.id for c in lc.ALL]
    assert len(set(ids)) == len(ids) == 37
    assert all(c.n == 3 and c.parities == (1, 0, 1) for c in lc.SWEEPS)
    assert all(c.n == 2 for c in lc.BANDS)


def test_alignment_classes():
    for what, sl, dl, fused in _all_layouts():
        for p, (s, d) in enumerate(zip(sl, dl)):
            for L in (s, d):
                # the library's own requirement: alignment to the sample size
                assert L.base % L.B == 0 and L.pitch % L.B == 0 and L.stride % L.B == 0, what
                assert L.pitch >= L.row + 8 and L.stride >= (L.rows + 2) * L.pitch and L.base >= 8, what
                if L.name == "lines":
                    assert L.base % 64 == 0 and L.pitch % 64 == 0 and L.stride % 64 == 0, what
                    assert L.pitch - L.row >= 64 * (1 + p), what
                elif fused:
                    assert L.base % 16 == 8 and L.pitch % 8 == 0 and L.stride % 8 == 0, what
                    # 8 mod 16 wherever the row is a multiple of 16 bytes: every fused width but the 8-bit planes 104 wide
                    assert (L.pitch % 16 == 8 and L.stride % 16 == 8) == (L.row % 16 == 0), what
                    assert L.row % 16 == 0 or (L.B == 1 and L.w == 104), what
            assert s.name != d.name and s.pitch != d.pitch and s.stride != d.stride, what
            if s.name == "odd8" and s.row == d.row:
                assert s.pitch < d.pitch, what  # the first arrangement: a row addressed with the other side's pitch leaves its plane
            if fused:
                assert lc.fused_layout_ok(s, d), what
        if len(sl) == 3:
            assert sl[1].pitch != sl[2].pitch and dl[1].pitch != dl[2].pitch, what
            assert sl[1].stride != sl[2].stride and dl[1].stride != dl[2].stride, what


def test_some_case_is_8_mod_16_on_every_sweep():
    """The 16-bit and float sweeps move 128 bits at base + 16 k - 8 and base + 16 k: each of their cases has the odd8 side."""
    for case in lc.U16 + lc.F32 + lc.PARTS:
        for arr in lc.ARRANGEMENTS:
            sl, dl = lc.layouts_of(case, arr)
            odd = sl if arr[0] == "odd8" else dl
            assert all(L.base % 16 == 8 and L.pitch % 16 == 8 and L.stride % 16 == 8 for L in odd), case.id


@pytest.mark.parametrize("name", lc.LAYOUTS)
def test_outside_mask_is_the_complement_of_the_planes(name):
    for p, (rows, w, B) in enumerate(((6, 24, 1), (4, 16, 2), (2, 8, 4))):
        L = lc.plane_layout(name, p, w, rows, B, 3)
        inside = np.zeros(L.nbytes, dtype=bool)
        for f in range(L.n):
            for y in range(L.rows):
                o = L.base + f * L.stride + y * L.pitch
                assert not inside[o:o + L.row].any()  # rows do not overlap
                inside[o:o + L.row] = True
        m = lc.outside_mask(L)
        assert np.array_equal(m, ~inside)
        assert int((~m).sum()) == L.n * L.rows * L.row
        # and the view addresses exactly those bytes
        a = np.zeros(L.nbytes, dtype=np.uint8)
        lc.view(a, L, lc.VIEW_DTYPE[B]).view({1: np.uint8, 2: np.uint16, 4: np.uint32}[B])[...] = (1 << 8 * B) - 1
        assert np.array_equal(a != 0, inside)


def _finished_launch(name, B):
    """A destination and source as a correct launch would leave them: (dst, dst layouts, want, dtype, src after, src uploaded)."""
    dtype = {1: np.uint8, 2: np.uint16, 4: np.float32}[B]
    rng = np.random.RandomState(B)
    shapes = [(6, 16), (4, 8), (4, 8)]
    n = 3
    want = [[(rng.randint(0, 200, size=s).astype(dtype)) for s in shapes] for _ in range(n)]
    dl = lc.batch_layout(name, shapes, B, n)
    dst = lc.destination_batch(dl)
    for p, L in enumerate(dl):
        v = lc.view(dst[p], L, lc.VIEW_DTYPE[B]).view(dtype)
        for f in range(n):
            v[f] = want[f][p]
    sl = lc.batch_layout("lines" if name == "odd8" else "odd8", shapes, B, n)
    up = lc.source_batch(sl, want, dtype)
    return dst, dl, want, dtype, [a.copy() for a in up], up


@pytest.mark.parametrize("B", (1, 2, 4))
@pytest.mark.parametrize("name", lc.LAYOUTS)
def test_the_checker_reports_what_it_is_there_for(name, B):
    dst, dl, want, dtype, after, up = _finished_launch(name, B)
    assert lc.problems(dst, dl, want, dtype, after, up) == []
    assert all((a[lc.outside_mask(L)] == lc.FILL_DST).all() for a, L in zip(dst, dl))
    assert all((a[lc.outside_mask(L)] == lc.FILL_SRC).all() for a, L in zip(up, lc.batch_layout("lines" if name == "odd8" else "odd8", [(6, 16), (4, 8), (4, 8)], B, 3)))
    L = dl[1]
    right_of_row = L.base + 1 * L.stride + 2 * L.pitch + L.row        # the byte just right of row 2 of frame 1
    between = L.base + 0 * L.stride + L.rows * L.pitch + 3            # behind frame 0's last row, before frame 1
    before = L.base - 1
    for off in (right_of_row, between, before):
        dst[1][off] ^= 0x01
    found = lc.problems(dst, dl, want, dtype, after, up)
    assert len(found) == 3 and all(f.startswith("plane 1 destination padding written") for f in found), found
    assert any(f"byte {right_of_row}: 0 right of row 2 of frame 1" in f for f in found), found
    assert any(f"byte {between}: between frames 0 and 1" in f for f in found), found
    assert any(f"byte {before}: 1 before the base" in f for f in found), found
    for off in (right_of_row, between, before):
        dst[1][off] ^= 0x01
    assert lc.problems(dst, dl, want, dtype, after, up) == []
    # a wrong sample inside a plane, and a source that was written to
    lc.view(dst[2], dl[2], lc.VIEW_DTYPE[B]).view(dtype)[2, 3, 7] += 1
    after[0][5] ^= 0x80
    found = lc.problems(dst, dl, want, dtype, after, up)
    assert len(found) == 2 and found[0].startswith("frame 2 plane 2: 1 differing samples, first at [[3, 7]]") and \
        found[1] == "plane 0 source allocation changed in 1 bytes, first at 5", found
    with pytest.raises(AssertionError, match="frame 2 plane 2"):
        lc.assert_clean("case", dst, dl, want, dtype, after, up)
