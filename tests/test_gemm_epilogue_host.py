"""Host model of the lane-private forward epilogue's mask-bit extraction
(csrc/include/gemm_tile.h): bf_pos01_pair - a signed 16-bit max with 0, then a signed 16-bit min
with 1, on both halves of a packed bf16 word - must mark exactly the halves bf_pos_pair marks,
and the dword assembled from it must be the dword the bf_pos_pair form assembled. Bit equality
throughout; both halves are swept over all 2^16 values against partner halves of every class
(zeros, smallest / largest positive and negative, infinities, NaNs of both signs).
"""
import numpy as np
import pytest

ALL = np.arange(1 << 16, dtype=np.uint32)
PARTNERS = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x3f80, 0xbf80, 0x7f7f, 0xff7f, 0x7f80,
                     0xff80, 0x7fc0, 0xffc0, 0x7fff, 0xffff, 0x1234, 0xfedc], dtype=np.uint32)


def bf_pos_pair(w):
    """gemm_tile.h bf_pos_pair: bit 15 / 31 set iff that bf16 half is > 0."""
    w = w.astype(np.uint32)
    return ((w & 0x7fff7fff) + 0x7fff7fff) & ~w & 0x80008000


def bf_pos01_pair(w):
    """gemm_tile.h bf_pos01_pair: v_pk_max_i16 w, 0 then v_pk_min_i16 ., 1 (per 16-bit half)."""
    h = w.astype(np.uint32).view(np.int16)
    return np.minimum(np.maximum(h, np.int16(0)), np.int16(1)).view(np.uint32)


def words():
    """Every half value in each position against every partner."""
    lo = (PARTNERS[:, None] << 16) | ALL[None, :]
    hi = (ALL[None, :] << 16) | PARTNERS[:, None]
    return np.ascontiguousarray(np.concatenate([lo.reshape(-1), hi.reshape(-1)]))


def test_pos01_marks_what_pos_pair_marks():
    w = words()
    assert np.array_equal(bf_pos01_pair(w), bf_pos_pair(w) >> 15)


def test_relu_outputs_are_covered():
    """The halves a ReLU can store (sign clear: +0, positive, +inf) are all in the sweep, and so
    are the ones it cannot (the extraction keeps the sign guard, so it does not rely on that)."""
    w = words()
    assert set(np.unique(w & 0xffff).tolist()) == set(range(1 << 16))
    assert set(np.unique(w >> 16).tolist()) == set(range(1 << 16))


@pytest.mark.parametrize("s", range(8))
def test_mask_dword_contribution(s):
    """One (i, j) pair's contribution to its mask dword, s = (i & 1) * 4 + (j & 3): lo -> bits
    15 - s / 31 - s, hi -> bits 7 - s / 23 - s."""
    lo = words()
    hi = lo[::-1].copy()
    old = (bf_pos_pair(lo) >> s) | (bf_pos_pair(hi) >> (8 + s))
    new = ((bf_pos01_pair(lo) << 8) | bf_pos01_pair(hi)) << (7 - s)
    assert np.array_equal(old, new.astype(np.uint32))
