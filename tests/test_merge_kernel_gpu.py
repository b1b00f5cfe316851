"""sn_merge_device and sn_turn_merge_device (csrc/sn_merge.hip, the second source of csrc/sn_turn.hip) against
tests/fields_model.merge_plane, bit for bit.  Planes of a few hundred samples in byte buffers with guard bytes around and
between the rows: every width around the 16-byte piece, heights 1, 2 and 5, three frames with a frame stride, rows that start on
multiples of 16 bytes (16 bytes per lane), pitches that are no multiple of 16 and a base one sample off (sample by sample), in
place on either input, and the refusal of any other overlap."""
import ctypes

import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2, capi, clip_format
from tests.fields_model import merge_plane
from tests.util import same, to_host

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 15, 16, 17, 63, 64, 65, 130)
HEIGHTS = (1, 2, 5)
TYPES = {"Y8": (np.uint8, 8), "Y10": (np.uint16, 10), "Y16": (np.uint16, 16), "Y32": (np.float32, 32)}
GUARD = 0x5C
N = 3
SPECIAL = [0x7F800000, 0xFF800000, 0xFFC12345, 0x7F812345, 0x80000000, 0x00000000, 0x00000001, 0x80000003, 0x7F7FFFFF, 0xFF7FFFFF, 0x3E800000,
           0x3F000000]  # +-inf, NaNs with payloads, +-0, denormals, +-the largest finite, 0.25, 0.5


def _planes(fmt, w, h, seed):
    """Two stacks [N, h, w]; the float ones hold every pair of SPECIAL somewhere when there is room."""
    dtype, bits = TYPES[fmt]
    rng = np.random.default_rng(seed)
    if dtype == np.float32:
        a, b = (rng.random((N, h, w), dtype=np.float32) * 2 - 0.5 for _ in range(2))
        fa, fb = a.reshape(-1).view(np.uint32), b.reshape(-1).view(np.uint32)
        k = 0
        for x in SPECIAL:
            for y in SPECIAL:
                if k < fa.size:
                    fa[k], fb[k] = x, y
                    k += 1
        return a, b
    hi = (1 << bits) - 1
    a, b = (rng.integers(0, hi + 1, (N, h, w)).astype(dtype) for _ in range(2))
    a.reshape(-1)[:4], b.reshape(-1)[:4] = [0, hi, hi, hi - 1][:a.size], [1, hi, hi - 1, hi][:a.size]
    return a, b


class Buf:
    """`data` [N, h, w] laid out in a byte buffer: base at `off`, rows `pitch` apart, frames `fs` apart, GUARD everywhere else."""

    def __init__(self, shape, dtype, off, pitch, fs, data=None):
        import torch
        n, h, w = shape
        self.shape, self.dtype, self.off, self.pitch, self.fs = shape, np.dtype(dtype), off, pitch, fs
        size = off + (n - 1) * fs + (h - 1) * pitch + w * self.dtype.itemsize + 64
        self.host = np.full(size, GUARD, np.uint8)
        if data is not None:
            self.put(data)
        self.dev = torch.from_numpy(self.host.copy()).pin_memory().to("cuda:0")
        assert self.dev.data_ptr() % 256 == 0
        self.ptr = self.dev.data_ptr() + off

    def put(self, data):
        n, h, w = self.shape
        rb = w * self.dtype.itemsize
        for f in range(n):
            for y in range(h):
                at = self.off + f * self.fs + y * self.pitch
                self.host[at:at + rb] = np.ascontiguousarray(data[f, y]).view(np.uint8)

    def args(self):
        return self.ptr, self.fs, self.pitch


def _layouts(w, h, B):
    """(name, off, pitch, frame stride) per plane kind: aligned rows; a pitch that is no multiple of 16; a base one sample off."""
    row = w * B
    p16 = (row + 15) // 16 * 16
    odd = row + 3 * B
    while odd % 16 == 0:
        odd += B
    return [("aligned", 0, p16, p16 * h + 48), ("pitch", 0, odd, odd * h + 5 * B), ("base", 16 + B, p16 + 16, (p16 + 16) * h + 16)]


def _merge(flt, a, b, d, w, h):
    rc = flt._lib.sn_merge_device(flt._h, N, *a.args(), *b.args(), w, h, *d.args())
    assert rc == capi.SN_OK, flt._lib.sn_last_error(flt._h)
    flt.synchronize()


@pytest.mark.parametrize("fmt", list(TYPES))
def test_merge_matches_the_model_at_every_width_height_and_alignment(hip_lib, fmt):
    dtype, _ = TYPES[fmt]
    B = np.dtype(dtype).itemsize
    with SangNom2(clip_format(fmt, 64, 32), device=0) as flt:
        for w in WIDTHS:
            for h in HEIGHTS:
                a, b = _planes(fmt, w, h, seed=w * 8 + h)
                want = np.stack([merge_plane(a[f], b[f]) for f in range(N)])
                for name, off, pitch, fs in _layouts(w, h, B):
                    what = f"{fmt} {w}x{h} {name}"
                    A, Bb = Buf(a.shape, dtype, off, pitch, fs, a), Buf(a.shape, dtype, off, pitch, fs, b)
                    D = Buf(a.shape, dtype, off, pitch, fs)
                    _merge(flt, A, Bb, D, w, h)
                    D.put(want)  # the expectation: the guard pattern with the averaged rows in it
                    assert np.array_equal(to_host(D.dev), D.host), f"{what}: dst differs, or bytes outside the rows were written"
                    assert np.array_equal(to_host(A.dev), A.host) and np.array_equal(to_host(Bb.dev), Bb.host), f"{what}: an input was written"
                    # in place on a, then on b
                    _merge(flt, A, Bb, A, w, h)
                    A.put(want)
                    assert np.array_equal(to_host(A.dev), A.host), f"{what}: in place on a"
                    A2 = Buf(a.shape, dtype, off, pitch, fs, a)
                    _merge(flt, A2, Bb, Bb, w, h)
                    Bb.put(want)
                    assert np.array_equal(to_host(Bb.dev), Bb.host), f"{what}: in place on b"


def test_mixed_alignments_take_the_sample_path_and_give_the_same(hip_lib):
    """One plane off the 16-byte grid is enough to leave the vector path: a aligned, b one sample off, dst with an odd pitch."""
    fmt, w, h = "Y16", 65, 5
    a, b = _planes(fmt, w, h, seed=5)
    want = np.stack([merge_plane(a[f], b[f]) for f in range(N)])
    with SangNom2(clip_format(fmt, 64, 32), device=0) as flt:
        lay = _layouts(w, h, 2)
        A, Bb, D = Buf(a.shape, np.uint16, *lay[0][1:], a), Buf(a.shape, np.uint16, *lay[2][1:], b), Buf(a.shape, np.uint16, *lay[1][1:])
        _merge(flt, A, Bb, D, w, h)
        D.put(want)
        assert np.array_equal(to_host(D.dev), D.host)


def test_the_tensor_method_and_the_refusals(hip_lib):
    import torch
    clip = clip_format("Y8", 64, 32)
    a, b = _planes("Y8", 100, 7, seed=9)
    want = np.stack([merge_plane(a[f], b[f]) for f in range(N)])
    with SangNom2(clip, device=0) as flt:
        ta, tb = (torch.from_numpy(x).pin_memory().to("cuda:0") for x in (a, b))
        td = torch.zeros_like(ta)
        flt.merge(ta, tb, td)
        flt.synchronize()
        assert np.array_equal(to_host(td), want)
        L, h_ = flt._lib, flt._h
        pa, pb, pd = ta.data_ptr(), tb.data_ptr(), td.data_ptr()
        ok = lambda *x: L.sn_merge_device(h_, *x)
        # any overlap other than the very plane: one sample on, one row on, the same base with another pitch or frame stride
        for dst, dfs, dp in ((pa + 1, 700, 100), (pa + 100, 700, 100), (pa, 700, 101), (pa, 701, 100), (pb + 699, 700, 100), (pb - 50, 700, 100)):
            assert ok(N, pa, 700, 100, pb, 700, 100, 100, 7, dst, dfs, dp) == capi.SN_ERR_INVALID_ARG
            assert b"overlaps" in L.sn_last_error(h_)
        assert ok(N, pa, 700, 100, pb, 700, 100, 100, 7, pa, 700, 100) == capi.SN_OK  # a itself
        assert ok(N, pa, 700, 100, pb, 700, 100, 100, 7, pb, 700, 100) == capi.SN_OK  # b itself
        assert ok(0, pa, 700, 100, pb, 700, 100, 100, 7, pa + 1, 700, 100) == capi.SN_OK  # no frames: nothing to overlap, nothing queued
        assert ok(N, pa, 700, 99, pb, 700, 100, 100, 7, pd, 700, 100) == capi.SN_ERR_INVALID_ARG  # a pitch below the row
        assert ok(N, None, 700, 100, pb, 700, 100, 100, 7, pd, 700, 100) == capi.SN_ERR_INVALID_ARG
        assert ok(N, pa, 700, 100, pb, 700, 100, 0, 7, pd, 700, 100) == capi.SN_ERR_INVALID_ARG
        flt.synchronize()
        assert np.array_equal(to_host(td), want)  # the refused calls queued nothing
        # turn-merge: dst overlaps neither input
        tt = torch.zeros((N, 100, 7), dtype=torch.uint8, device="cuda:0")
        turn = lambda *x: L.sn_turn_merge_device(h_, *x)
        assert turn(1, N, pa, 700, 100, pb, 700, 100, 100, 7, pa, 700, 7) == capi.SN_ERR_INVALID_ARG
        assert turn(1, N, pa, 700, 100, pb, 700, 100, 100, 7, pb + 8, 700, 7) == capi.SN_ERR_INVALID_ARG
        assert turn(0, N, pa, 700, 100, pb, 700, 100, 100, 7, tt.data_ptr(), 700, 7) == capi.SN_ERR_INVALID_ARG  # no direction
        assert turn(1, N, pa, 700, 100, pb, 700, 100, 100, 7, tt.data_ptr(), 700, 6) == capi.SN_ERR_INVALID_ARG  # dst rows are 7 samples
        with pytest.raises(ValueError):
            flt.merge(ta, tb[:, :, :50], td)
        with pytest.raises(ValueError):
            flt.turn_merge(ta, tb, td, 1)


# ---- the turn with a second source ---------------------------------------------------------------------------------------------

VT = {1: "uint8", 2: "int16", 4: "float32"}  # torch has no uint16: same bits


@pytest.mark.parametrize("fmt", ["Y8", "Y16", "Y32"])
@pytest.mark.parametrize("w,h", [(64, 64), (128, 64), (65, 67), (30, 20)])
def test_turn_merge_is_the_turn_of_the_average(hip_lib, fmt, w, h):
    """Whole 64 x 64 tiles move as dwords, ragged ones sample by sample; a pitch that is no multiple of 4 sends every tile down
    the sample path (not for float, whose samples are dwords).  Both directions; the columns beyond the rows keep their bytes."""
    import torch
    dtype, _ = TYPES[fmt]
    B = np.dtype(dtype).itemsize
    a, b = _planes(fmt, w, h, seed=w + h)
    a, b = a[:2], b[:2]
    avg = [merge_plane(a[f], b[f]) for f in range(2)]

    def dev(x, extra):  # [2, h, w] as a view of a tensor `extra` samples wider
        full = np.zeros((2, x.shape[1], x.shape[2] + extra), x.dtype)
        full[:, :, :x.shape[2]] = x
        t = torch.from_numpy(full.view(VT[B])).pin_memory().to("cuda:0")
        return t[:, :, :x.shape[2]]

    def odd_extra(width):
        e = 1
        while ((width + e) * B) % 4 == 0 and B < 4:
            e += 1
        return e

    with SangNom2(clip_format(fmt, 64, 32), device=0) as flt:
        for pitches in ("even", "odd"):
            if pitches == "odd" and B == 4:
                continue
            ea, ed = (4, 4) if pitches == "even" else (odd_extra(w), odd_extra(h))
            assert pitches == "even" or (((w + ea) * B) % 4 and ((h + ed) * B) % 4)
            ta, tb = dev(a, ea), dev(b, ea)
            for direction, k in ((1, -1), (-1, 1)):  # TurnRight is rot90 clockwise
                full = torch.from_numpy(np.full((2, w, h + ed), (GUARD * 0x01010101) & ((1 << 8 * B) - 1), {1: np.uint8, 2: np.uint16, 4: np.uint32}[B])
                                        .view(VT[B])).pin_memory().to("cuda:0")
                guard = to_host(full).copy()
                flt.turn_merge(ta, tb, full[:, :, :h], direction)
                flt.synchronize()
                got = to_host(full)
                for f in range(2):
                    want = np.rot90(avg[f], k=k)
                    assert same(want, np.ascontiguousarray(got[f, :, :h]).view(dtype)), f"{fmt} {w}x{h} {pitches} direction {direction} frame {f}"
                beyond = lambda x: np.ascontiguousarray(x[:, :, h:]).view(np.uint8)
                assert np.array_equal(beyond(got), beyond(guard)), "columns beyond the rows were written"
