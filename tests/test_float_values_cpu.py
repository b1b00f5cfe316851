"""What the inputs of test_float_values_gpu.py exercise, worked out on the CPU with the two restatements of the reference.

The bit-exact GPU test means something only if its inputs reach what they are named for: every arm of the ladder on
negative, out-of-range, non-dyadic and denormal samples; outputs that ARE denormals; a minimum that equals the threshold
(where `>` and `>=` part); ties at the minimum; huge finite samples on which an fma and the reference's multiply-then-add
part, with every output finite (nothing masked); and non-finite samples that leave most of the frame defined.
Shape: Y32 64x24, two frames, unless said otherwise.
"""
import numpy as np
import pytest

from avisynth_sangnom2_amd import clip_format
from oracle.oracle import Oracle
from oracle.sangnom_numpy import NumpySangNom
from tests import float_cases as fc
from tests.util import oracle_cfg, same

F32 = np.float32
RANK = (12, 6, 4, 2, 0, 1, 3, 5, 7)  # of buffer 0 .. 8 in the reference's ladder: smaller wins a tie
THRESHOLD_ARM = 9
W, H = 64, 24


class _Recording(NumpySangNom):
    """Keeps the smoothed costs of every plane it filters: [(plane, costs[9][rows][w])]."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.seen = []

    def _plane(self, dst, offset, plane):
        super()._plane(dst, offset, plane)
        h, w = dst.shape
        self.seen.append((plane, self.pool[:, 1:h // 2, :w].copy()))


class _Fma(NumpySangNom):
    """The restatement with the SangNom value's 4 * p1 + 5 * p2 as one fused multiply-add (p1 * 4 unrounded)."""

    def _sg(self, p1, p2, p3):
        with np.errstate(all="ignore"):
            q5 = (p2 * F32(5)).astype(np.float64)
            s = (p1.astype(np.float64) * 4.0 + q5).astype(F32) - p3
            return s * F32(0.125)


def _model(cls, clip, **kw):
    return cls(clip.width, clip.height, bytes=clip.bytes, bits=clip.bits, planes=clip.planes, subw=clip.subw, subh=clip.subh, order=1, **kw)


def _costs(clip, pattern, **frames_kw):
    m = _model(_Recording, clip, aa=48, aac=48)
    with np.errstate(all="ignore"):
        for f, src in enumerate(fc.frames(clip, pattern, **frames_kw)):
            m.get_frame(src, parity=f & 1)
    return [v for _plane, v in m.seen]  # the smoothed costs do not depend on the threshold


def _thr(aa):
    return F32(F32(F32(aa) * F32(21.0) / F32(16.0)) / F32(256.0))


def _arms(v, aa):
    lo = v.min(axis=0)
    winner = np.where(v == lo, np.array(RANK)[:, None, None], 99).argmin(axis=0)  # the best-ranked buffer among those at the minimum
    by_thr = (lo > _thr(aa)) & (v[4] != lo)
    return lo, winner, by_thr


@pytest.mark.parametrize("pattern", ("signed", "overshoot", "k255", "denormal", "small"))
def test_every_arm_of_the_ladder_wins_somewhere(pattern):
    arms = set()
    for v in _costs(clip_format("Y32", W, H), pattern):
        for aa in fc.AA:
            _lo, winner, by_thr = _arms(v, aa)
            arms.update(np.unique(np.where(by_thr, THRESHOLD_ARM, winner)).tolist())
    print(f"{pattern}: arms {sorted(arms)}")
    assert arms == set(range(10)), f"{pattern}: arms that never win: {sorted(set(range(10)) - arms)}"


def _is_denormal(a):
    b = a.view(np.uint32)
    return ((b & 0x7F800000) == 0) & ((b & 0x007FFFFF) != 0)


def test_denormal_inputs_give_denormal_outputs_and_both_restatements_keep_them():
    clip = clip_format("Y32", W, H)
    ora, m = Oracle(oracle_cfg(clip)), _model(NumpySangNom, clip)
    count = 0
    for f, src in enumerate(fc.frames(clip, "denormal")):
        want = ora.process(src, parity=f & 1)[0]
        assert same(want, m.get_frame(src, parity=f & 1)[0]), "a restatement flushes denormals on this host"
        count += int(_is_denormal(want).sum())
    print(f"denormal: {count} of {fc.NFRAMES * W * H} output samples are nonzero denormals")
    assert count == fc.NFRAMES * W * H
    ora = Oracle(oracle_cfg(clip))
    count = sum(int(_is_denormal(ora.process(src, parity=f & 1)[0]).sum()) for f, src in enumerate(fc.frames(clip, "small")))
    print(f"small: {count} output samples are nonzero denormals")
    assert count >= 1


def test_negative_zero_stays_negative_zero():
    clip = clip_format("Y32", W, H)
    for aa in fc.AA:
        ora = Oracle(oracle_cfg(clip, aa=aa))
        for f, src in enumerate(fc.frames(clip, "negzero")):
            assert (ora.process(src, parity=f & 1)[0].view(np.uint32) == 0x80000000).all()


@pytest.mark.parametrize("aa", fc.SLOPE_AA)
def test_slope_puts_the_minimum_on_the_threshold(aa):
    """min == thr with buffer 4 above the minimum and another buffer winning: `>` interpolates along that buffer, `>=` would
    take the threshold arm."""
    at, above = 0, 0
    for v in _costs(clip_format("Y32", W, H), "slope", aa=aa):
        lo, winner, _ = _arms(v, aa)
        at += int(((lo == _thr(aa)) & (v[4] != lo) & (winner != 4)).sum())
        above += int(((lo > _thr(aa)) & (v[4] != lo)).sum())
    print(f"slope aa={aa}: {at} samples with min == thr that a buffer other than 4 wins, {above} above the threshold")
    assert at >= 40
    assert above > 0


def test_checker2_and_eighths_tie_at_the_minimum():
    ties = 0
    for pattern in ("checker2", "eighths"):
        for v in _costs(clip_format("Y32", W, H), pattern):
            for aa in fc.AA:
                lo, winner, by_thr = _arms(v, aa)
                ties += int((((v == lo).sum(axis=0) >= 2) & (winner != 4) & ~by_thr).sum())
    print(f"checker2 + eighths: {ties} ties at the minimum won by a buffer other than 4")
    assert ties > 0


def test_huge_finite_samples_part_an_fma_from_the_reference_and_nothing_is_masked():
    fmt, w, h = fc.HUGE_SHAPE
    clip = clip_format(fmt, w, h)
    ora, plain, fma = Oracle(oracle_cfg(clip, aa=128)), _model(NumpySangNom, clip, aa=128), _model(_Fma, clip, aa=128)
    differ = 0
    with np.errstate(all="ignore"):
        for f, src in enumerate(fc.frames(clip, "huge")):
            assert np.isfinite(src[0]).all()
            want = ora.process(src, parity=f & 1)[0]
            assert np.isfinite(want).all(), "an undefined or infinite output sample: the comparison would have to mask it"
            assert same(want, plain.get_frame(src, parity=f & 1)[0])
            differ += int((want.view(np.uint32) != fma.get_frame(src, parity=f & 1)[0].view(np.uint32)).sum())
        # on ordinary input the emulation is the restatement
        a, b = _model(NumpySangNom, clip, aa=128), _model(_Fma, clip, aa=128)
        for f, src in enumerate(fc.frames(clip, "overshoot")):
            assert same(a.get_frame(src, parity=f & 1)[0], b.get_frame(src, parity=f & 1)[0])
    print(f"huge: {differ} of {fc.NFRAMES * w * h} samples differ between the reference and an fma")
    assert differ >= 1


@pytest.mark.parametrize("shape", (fc.NONFINITE_PLAIN, fc.NONFINITE_PADDED, fc.NONFINITE_COUPLED, fc.NONFINITE_BANDS), ids=lambda s: f"{s[0]}-{s[1]}x{s[2]}")
def test_non_finite_inputs_leave_most_of_the_frame_defined(shape):
    fmt, w, h, every = shape
    clip = clip_format(fmt, w, h)
    kw = dict(aac=48) if clip.planes > 1 else {}
    for f, src in enumerate(fc.frames(clip, "nonfinite", every=every)):
        assert not np.isfinite(src[0]).all()
        _want, written = fc.written_by_reference(clip, src, parity=f & 1, **kw)
        for p, m in enumerate(written):
            print(f"nonfinite {fmt} {w}x{h} frame {f} plane {p}: the reference writes {m.mean():.3f} of the samples")
            assert 0.7 < m.mean() < 1.0
