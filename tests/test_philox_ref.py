"""The NumPy noise reference (tests/philox_ref.py) is itself pinned: the published Philox4x32-10
known-answer vectors bit for bit, and every field of the three counter layouts reaches the
output. CPU only; tests/test_sampling_noise_gpu.py holds the HIP kernels to this reference."""
import numpy as np
import pytest

import philox_ref as pr

# Random123 kat_vectors, philox4x32 10 rounds: (counter, key, expected)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_known_answer_vectors(ctr, key, want):
    got = pr.philox4x32_10(*ctr, *key)
    assert all(w.dtype == np.uint32 for w in got)
    assert tuple(int(w) for w in got) == want


def test_philox_is_vectorised():
    """All three vectors in one call, and broadcasting a scalar key over a counter grid."""
    cols = [np.array([k[0][i] for k in KAT], dtype=np.uint64) for i in range(4)]
    keys = [np.array([k[1][i] for k in KAT], dtype=np.uint64) for i in range(2)]
    got = np.stack(pr.philox4x32_10(*cols, *keys), axis=1)
    assert got.tolist() == [list(k[2]) for k in KAT]
    grid = pr.philox4x32_10(np.arange(3)[:, None], np.arange(5)[None, :], 1, 2, 3, 4)
    assert grid[0].shape == (3, 5)
    one = pr.philox4x32_10(2, 4, 1, 2, 3, 4)
    assert [int(w[2, 4]) for w in grid] == [int(w) for w in one]


def test_box_muller_definition():
    """u1 = ((a >> 8) + 1) / 2^24 in (0, 1], u2 = (b >> 8) / 2^24 in [0, 1); the low 8 bits of
    either word are unused; the float32 twin agrees to float32 rounding."""
    a = np.array([0, 0xFF, 0x100, 0xFFFFFFFF, 0x80000000], dtype=np.uint32)
    b = np.array([0, 0x40000000, 0x80000000, 0xC0000000, 0xFFFFFFFF], dtype=np.uint32)
    u1, u2 = pr.uniforms(a, b)
    assert u1.tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -23, 1.0, 0.5 + 2.0 ** -24]
    assert u2.tolist() == [0.0, 0.25, 0.5, 0.75, 1.0 - 2.0 ** -24]
    n0, n1 = pr.box_muller64(a, b)
    r = np.sqrt(-2.0 * np.log(u1))
    assert n0.dtype == np.float64
    assert np.allclose(n0, r * np.cos(2 * np.pi * u2), rtol=0, atol=1e-15)
    assert np.allclose(n1, r * np.sin(2 * np.pi * u2), rtol=0, atol=1e-15)
    assert n0[3] == 0.0 and n1[3] == 0.0            # u1 = 1: r = 0, log never sees 0
    assert np.isfinite(n0).all() and np.isfinite(n1).all()
    assert abs(n0[0] - np.sqrt(48 * np.log(2.0))) < 1e-12      # largest radius, angle 0
    f0, f1 = pr.box_muller32(a, b)
    assert f0.dtype == np.float32
    assert np.abs(f0 - n0).max() < 1e-5 and np.abs(f1 - n1).max() < 1e-5


def test_rounding_floor_is_float32_sized():
    F = pr.rounding_floor(pr.reparam_eps, 64, 260, 7, 0, 0)
    assert 1e-8 < F < 6.25e-6


SEED, OFF = (3 << 32) | 5, (1 << 32) + 2


def test_layouts_are_deterministic_and_float64():
    for fn, args in ((pr.reparam_eps, (5, 260, SEED, OFF, 1)), (pr.normal_fill_ref, (1027, SEED, OFF, 1)),
                     (pr.vae_eps, (9, 40, SEED, OFF))):
        a, b = fn(*args), fn(*args)
        assert a.dtype == np.float64 and np.isfinite(a).all()
        assert np.array_equal(a, b)
    assert pr.reparam_eps(5, 260, SEED, OFF, 1).shape == (5, 260)
    assert pr.normal_fill_ref(1027, SEED, OFF, 1).shape == (1027,)
    assert pr.vae_eps(9, 40, SEED, OFF).shape == (9, 40)


def _all_differ(a, b):
    """Two draws of continuous noise: every element differs unless the counters coincide."""
    return a.shape == b.shape and bool((a != b).all())


def test_reparam_every_counter_field_matters():
    base = pr.reparam_eps(6, 24, SEED, OFF, 1)
    assert _all_differ(base, pr.reparam_eps(6, 24, SEED + 1, OFF, 1))            # seed lo
    assert _all_differ(base, pr.reparam_eps(6, 24, SEED + (1 << 32), OFF, 1))    # seed hi
    assert _all_differ(base, pr.reparam_eps(6, 24, SEED, OFF + 1, 1))            # offset lo
    assert _all_differ(base, pr.reparam_eps(6, 24, SEED, OFF + (1 << 32), 1))    # offset hi
    assert _all_differ(base, pr.reparam_eps(6, 24, SEED, OFF, 2))                # stream
    flat = base.reshape(-1)
    assert len(np.unique(flat)) == flat.size         # rows, column groups and the 4 picks
    assert _all_differ(base[:-1], base[1:])          # row
    assert _all_differ(base[:, :-4], base[:, 4:])    # column group
    wide = pr.reparam_eps(2, 260, SEED, OFF, 1)      # 65 groups: the group index is not folded
    assert len(np.unique(wide)) == wide.size
    # a narrower or shorter tensor is a prefix: element (row, col) does not depend on (B, D)
    assert np.array_equal(pr.reparam_eps(3, 7, SEED, OFF, 1), base[:3, :7])


def test_normal_fill_every_counter_field_matters():
    n = 1027
    base = pr.normal_fill_ref(n, SEED, OFF, 1)
    assert _all_differ(base, pr.normal_fill_ref(n, SEED + 1, OFF, 1))
    assert _all_differ(base, pr.normal_fill_ref(n, SEED + (1 << 32), OFF, 1))
    assert _all_differ(base, pr.normal_fill_ref(n, SEED, OFF + 1, 1))
    assert _all_differ(base, pr.normal_fill_ref(n, SEED, OFF + (1 << 32), 1))
    assert _all_differ(base, pr.normal_fill_ref(n, SEED, OFF, 2))
    assert len(np.unique(base)) == n
    assert np.array_equal(pr.normal_fill_ref(6, SEED, OFF, 1), base[:6])
    # not reparam_sample's row 0: the group's high word is XORed with a constant
    assert _all_differ(base[:24], pr.reparam_eps(1, 24, SEED, OFF, 1)[0])


def test_vae_every_counter_field_matters():
    base = pr.vae_eps(9, 40, SEED, OFF)
    assert _all_differ(base, pr.vae_eps(9, 40, SEED + 1, OFF))
    assert _all_differ(base, pr.vae_eps(9, 40, SEED, OFF + 1))
    assert _all_differ(base, pr.vae_eps(9, 40, SEED, OFF + (1 << 32)))
    # vae_step keeps 32 bits of the seed
    assert np.array_equal(base, pr.vae_eps(9, 40, SEED & 0xFFFFFFFF, OFF))
    flat = base.reshape(-1)
    assert len(np.unique(flat)) == flat.size         # rows, lane pairs, n0 / n1
    assert _all_differ(base[:-1], base[1:])
    assert _all_differ(base[:, :-2], base[:, 2:])
    # a lane pair is the cosine and the sine of ONE radius and angle
    a, b, odd = pr.vae_words(9, 40, SEED, OFF)
    assert np.array_equal(a[:, 0::2], a[:, 1::2]) and np.array_equal(b[:, 0::2], b[:, 1::2])
    assert not odd[:, 0::2].any() and odd[:, 1::2].all()
    u1, _ = pr.uniforms(a, b)
    assert np.allclose(base[:, 0::2] ** 2 + base[:, 1::2] ** 2, -2.0 * np.log(u1[:, 0::2]), rtol=1e-12)


def test_streams_are_pairwise_different_at_offset_zero():
    draws = [pr.reparam_eps(4, 16, 7, 0, s) for s in range(8)]
    for i in range(8):
        for j in range(i + 1, 8):
            assert _all_differ(draws[i], draws[j]), (i, j)
    fills = [pr.normal_fill_ref(64, 7, 0, s) for s in range(8)]
    for i in range(8):
        for j in range(i + 1, 8):
            assert _all_differ(fills[i], fills[j]), (i, j)
