"""What the inputs of test_ladder_min3_gpu.py exercise, worked out on the CPU with the numpy restatement.

The device folds the ladder's keys in pairs -- buffers (0, 1), (2, 3), (4, 5), (6, 7), then buffer 8, starting from the
threshold key -- with a three-input f16 minimum (sn_fused_v3_common.h, fold_key).  The bit-exact GPU test means something
only if its inputs make every arm of the ladder win somewhere, put winning costs on both sides of 64 (key 0x0400: below it
a key is an f16 denormal pattern), and produce ties inside the folded pairs, where only the rank in the key's low nibble
decides -- in pairs whose even buffer has the better rank, (4, 5) and (6, 7), and in pairs whose odd one has, (0, 1) and
(2, 3).
"""
import numpy as np

from avisynth_sangnom2_amd import clip_format
from oracle.sangnom_numpy import NumpySangNom
from tests import ladder_cases as lc

RANK = (12, 6, 4, 2, 0, 1, 3, 5, 7)  # of buffer 0 .. 8 in the ladder (rank_of, sn_fused_u8_parts.h): smaller wins a tie
THRESHOLD_ARM = 9


class _Recording(NumpySangNom):
    """Keeps the smoothed costs of every plane it filters: [(plane, costs[9][rows][w])]."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.seen = []

    def _plane(self, dst, offset, plane):
        super()._plane(dst, offset, plane)
        h, w = dst.shape
        self.seen.append((plane, self.pool[:, 1:h // 2, :w].copy()))


def _ladder_facts():
    arms = set()              # arms that win somewhere: buffers 0 .. 8 and the threshold
    below, above = 0, 0       # winning smoothed costs < 64 / >= 64
    even_first, odd_first = 0, 0  # ties at the minimum inside a folded pair that the pair's even / odd buffer wins
    rank = np.array(RANK)[:, None, None]
    for fmt, w, h, _bands in lc.Y8_SHAPES + lc.YUV_SHAPES:
        clip = clip_format(fmt, w, h)
        for pattern in lc.PATTERNS:
            # the smoothed costs do not depend on the threshold: one pass per input, every threshold read off it
            m = _Recording(w, h, bytes=clip.bytes, bits=clip.bits, planes=clip.planes, subw=clip.subw, subh=clip.subh, order=1, aa=48, aac=48)
            for f, src in enumerate(lc.frames(clip, pattern)):
                m.get_frame(src, parity=f & 1)
            for _plane, v in m.seen:
                lo = v.min(axis=0)
                winner = np.where(v == lo, rank, 99).argmin(axis=0)  # the best-ranked buffer among those at the minimum
                for aa in lc.AA:
                    thr = int(np.float32(aa) * np.float32(21.0) / np.float32(16.0))
                    by_thr = (lo > thr) & (v[4] != lo)
                    arm = np.where(by_thr, THRESHOLD_ARM, winner)
                    arms.update(np.unique(arm).tolist())
                    cost = np.where(by_thr, thr + 1, lo)  # the threshold arm's key is (thr + 1) << 4
                    below += int((cost < 64).sum())
                    above += int((cost >= 64).sum())
                    for e in (0, 2, 4, 6):
                        tie = (v[e] == lo) & (v[e + 1] == lo) & ~by_thr
                        if RANK[e] < RANK[e + 1]:
                            even_first += int((tie & (winner == e)).sum())
                        else:
                            odd_first += int((tie & (winner == e + 1)).sum())
    return arms, below, above, even_first, odd_first


def test_inputs_reach_every_arm_both_key_ranges_and_pair_ties():
    arms, below, above, even_first, odd_first = _ladder_facts()
    print(f"arms {sorted(arms)}, winning costs below 64: {below}, at or above: {above}, pair ties won by the even buffer: {even_first}, by the odd one: {odd_first}")
    assert arms == set(range(10)), f"arms that never win: {sorted(set(range(10)) - arms)}"
    assert below > 0 and above > 0, (below, above)
    assert even_first > 0 and odd_first > 0, (even_first, odd_first)
