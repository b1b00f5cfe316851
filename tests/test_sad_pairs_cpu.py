"""The vertical pairs of the plain 8-bit sweep and its two byte SADs, as a numpy model (sn_fused_u8_parts.h: PairLine,
pair_down, sad_pairs_sum, last_pairs).  Fixes the byte order on paper: what v_perm_b32, v_sad_u8 and v_sad_hi_u8 do is
written out from the ISA's definitions, and the packed result is checked against O + |a - b| + |c - d| per strip.

  pair    byte 0 = the column's pixel in the upper line, byte 1 = in the lower line, bytes 2 and 3 = zero
  perm    D.byte[i] = {S0, S1}.byte[sel.byte[i]] with S1 = bytes 0..3, S0 = bytes 4..7, selector 12 = 0x00
  sad     D = accumulator + sum of |S0.byte[i] - S1.byte[i]| over the four bytes;  sad_hi adds the sum << 16
"""
import itertools

import numpy as np

U32 = np.uint32


def v_perm_b32(s0, s1, sel):
    s0, s1 = np.asarray(s0, U32), np.asarray(s1, U32)
    both = (s0.astype(np.uint64) << np.uint64(32)) | s1.astype(np.uint64)
    out = np.zeros(both.shape, np.uint64)
    for i in range(4):
        k = (sel >> (8 * i)) & 0xff
        if k == 0x0c:
            continue
        assert k < 8
        out |= ((both >> np.uint64(8 * k)) & np.uint64(0xff)) << np.uint64(8 * i)
    return out.astype(U32)


def _byte_sad(s0, s1):
    s0, s1 = np.asarray(s0, U32).astype(np.int64), np.asarray(s1, U32).astype(np.int64)
    return sum(np.abs(((s0 >> (8 * i)) & 0xff) - ((s1 >> (8 * i)) & 0xff)) for i in range(4))


def v_sad_u8(s0, s1, acc):
    return ((_byte_sad(s0, s1) + np.asarray(acc, U32).astype(np.int64)) & 0xffffffff).astype(U32)


def v_sad_hi_u8(s0, s1, acc):
    return (((_byte_sad(s0, s1) << 16) + np.asarray(acc, U32).astype(np.int64)) & 0xffffffff).astype(U32)


def pair_down(old, raw, k):
    """sn_fused_u8_parts.h: __builtin_amdgcn_perm(raw, old, 0x0c0c0401 + (k << 8))"""
    return v_perm_b32(raw, old, 0x0c0c0401 + (k << 8))


def pair_of(upper, lower):
    return (np.asarray(upper, U32) | (np.asarray(lower, U32) << U32(8))).astype(U32)


def sad_pairs_sum(za_lo, zb_lo, za_hi, zb_hi, o):
    return v_sad_hi_u8(za_hi, zb_hi, v_sad_u8(za_lo, zb_lo, o))


EXTREMES = (0, 1, 127, 128, 254, 255)


def test_pair_down_moves_the_lower_pixel_up_and_takes_byte_k():
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(U32)
    up, low = rng.integers(0, 256, 4096).astype(U32), rng.integers(0, 256, 4096).astype(U32)
    for k in range(4):
        new = pair_down(pair_of(up, low), raw, k)
        assert np.array_equal(new, pair_of(low, (raw >> U32(8 * k)) & U32(0xff)))
    # from no pairs at all (the sweep's first line): the pixel in byte 1, nothing else
    assert np.array_equal(pair_down(np.zeros(4096, U32), raw, 2), ((raw >> U32(16)) & U32(0xff)) << U32(8))


def test_two_sads_on_all_byte_extremes():
    """every combination of extreme bytes in the four samples of each strip, O at 0 and 255 in both halves"""
    combos = np.array(list(itertools.product(EXTREMES, repeat=4)), dtype=np.int64)  # a, b, c, d
    a, b, c, d = (combos[:, i] for i in range(4))
    want_half = np.abs(a - b) + np.abs(c - d)
    za, zb = pair_of(a, c), pair_of(b, d)  # column x + k: lines (r, r + 1);  column x - k: lines (r + 1, r + 2)
    n = len(combos)
    for o_lo, o_hi in itertools.product((0, 255), repeat=2):
        o = np.full(n, o_lo | (o_hi << 16), U32)
        # the low strip runs through the combinations, the high strip through them in reverse: the halves are independent
        got = sad_pairs_sum(za, zb, za[::-1], zb[::-1], o)
        assert np.array_equal(got & U32(0xffff), (o_lo + want_half).astype(U32))
        assert np.array_equal(got >> U32(16), (o_hi + want_half[::-1]).astype(U32))
    assert int(want_half.max()) == 510  # 255 + 510 = 765 per half: no carry into the other half, none out of the word


def test_two_sads_on_random_bytes():
    rng = np.random.default_rng(9)
    n = 1 << 16
    px = rng.integers(0, 256, (2, 4, n)).astype(np.int64)  # [strip][a, b, c, d]
    o = rng.integers(0, 256, (2, n)).astype(np.int64)
    got = sad_pairs_sum(pair_of(px[0, 0], px[0, 2]), pair_of(px[0, 1], px[0, 3]), pair_of(px[1, 0], px[1, 2]), pair_of(px[1, 1], px[1, 3]),
                        (o[0] | (o[1] << 16)).astype(U32))
    for h in range(2):
        want = o[h] + np.abs(px[h, 0] - px[h, 1]) + np.abs(px[h, 2] - px[h, 3])
        assert np.array_equal((got >> U32(16 * h)) & U32(0xffff), want.astype(U32))


def test_rows_of_a_plane_through_the_pair_update():
    """A column pair of a small plane swept row by row as the kernel does it: the pairs of line k from those of line k - 1
    and line k's dword, the two sets swapping roles, the last row on pairs without lower pixels (last_pairs)."""
    rng = np.random.default_rng(11)
    nlines, n = 7, 512
    raw = rng.integers(0, 1 << 32, (2, nlines, n), dtype=np.uint64).astype(U32)  # [column x + k / x - k][line][lane]
    ka, kb = 1, 3  # the byte of the dword that holds column x + k / column x - k
    pix = lambda s, line, k: ((raw[s, line] >> U32(8 * k)) & U32(0xff)).astype(np.int64)
    # pairs[line] = (line - 1, line) of both columns; line 0 from nothing
    za = [pair_down(np.zeros(n, U32), raw[0, 0], ka)]
    zb = [pair_down(np.zeros(n, U32), raw[1, 0], kb)]
    for line in range(1, nlines):
        za.append(pair_down(za[-1], raw[0, line], ka))
        zb.append(pair_down(zb[-1], raw[1, line], kb))
    o = rng.integers(0, 256, n).astype(np.int64)
    zero = np.zeros(n, U32)
    for r in range(1, nlines - 1):  # row r: n = line r with the pairs (r - 1, r), nn = line r + 1 with (r, r + 1)
        got = v_sad_u8(za[r], zb[r + 1], o.astype(U32))
        want = o + np.abs(pix(0, r - 1, ka) - pix(1, r, kb)) + np.abs(pix(0, r, ka) - pix(1, r + 1, kb))
        assert np.array_equal(got, want.astype(U32)), r
        assert np.array_equal(v_sad_hi_u8(za[r], zb[r + 1], zero), (want.astype(U32) - o.astype(U32)) << U32(16)), r
    # the last row r = nlines - 1: one term, n keeps byte 0, nn = n's byte 1 in byte 0
    r = nlines - 1
    got = v_sad_u8(za[r] & U32(0xff), zb[r] >> U32(8), o.astype(U32))
    assert np.array_equal(got, (o + np.abs(pix(0, r - 1, ka) - pix(1, r, kb))).astype(U32))


def test_a_swapped_pair_or_operand_is_not_the_same_sum():
    """the checks above can tell the layouts apart: bytes in the wrong order, or +k / -k swapped between the lines, differ"""
    a, b, c, d = (np.array([v], np.int64) for v in (10, 200, 220, 90))
    right = v_sad_u8(pair_of(a, c), pair_of(b, d), np.zeros(1, U32))[0]
    assert right == abs(10 - 200) + abs(220 - 90)
    assert v_sad_u8(pair_of(c, a), pair_of(b, d), np.zeros(1, U32))[0] != right  # a pair upside down
    assert v_sad_u8(pair_of(a, c), pair_of(d, b), np.zeros(1, U32))[0] != right  # the other column's lines one row off
