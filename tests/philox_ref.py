"""Bit-exact NumPy reference of the in-kernel Gaussian noise (a test helper, not a conftest).

Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) in uint64
arithmetic, so every 32 x 32 -> 64-bit product is exact, followed by Box-Muller in float64.
Nothing here is taken from the kernels except the documented counter layouts
(docs/ARCHITECTURE.md, "Noise: counter layouts"):

    reparam_sample  counter (col // 4, row, off_lo, off_hi ^ stream * 0x9E3779B9)
                    key     (seed_lo, seed_hi); element col takes normal col % 4 of
                    box_muller(x, y), box_muller(z, w)
    normal_fill     counter (g_lo, g_hi ^ 0x5bd1e995, off_lo, off_hi ^ stream * 0x9E3779B9),
                    g = i // 4; key and normals as above
    vae_step        counter (row, lane >> 1, off_lo, off_hi ^ 0x5EA), key (seed_lo, 0xA5A5);
                    box_muller(x, y): even lane takes n0, odd lane n1

tests/test_philox_ref.py pins the round function to the published known-answer vectors.
"""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_PHILOX_M0 = np.uint64(0xD2511F53)
_PHILOX_M1 = np.uint64(0xCD9E8D57)
_WEYL_0 = 0x9E3779B9    # golden ratio
_WEYL_1 = 0xBB67AE85    # sqrt(3) - 1
_STREAM_MULT = 0x9E3779B9
_FILL_HI_XOR = 0x5BD1E995
_VAE_C3_XOR = 0x5EA
_VAE_K1 = 0xA5A5
_TWO_PI = 6.283185307179586


def _u64(v):
    return np.asarray(v, dtype=np.uint64) & _M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten Philox-4x32 rounds over broadcastable arrays of 32-bit words; four uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u64(v) for v in (c0, c1, c2, c3, k0, k1)))
    for r in range(10):
        kr0 = (k0 + np.uint64((r * _WEYL_0) & 0xFFFFFFFF)) & _M32
        kr1 = (k1 + np.uint64((r * _WEYL_1) & 0xFFFFFFFF)) & _M32
        p0 = _PHILOX_M0 * c0          # < 2^64: exact
        p1 = _PHILOX_M1 * c2
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ kr0, p1 & _M32, (p0 >> _S32) ^ c3 ^ kr1, p0 & _M32)
    return tuple(w.astype(np.uint32) for w in (c0, c1, c2, c3))


def uniforms(a, b):
    """(u1, u2) of a Box-Muller pair as exact float64: u1 in (0, 1], u2 in [0, 1)."""
    a, b = np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32)
    u1 = ((a >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = (b >> np.uint32(8)).astype(np.float64) / 16777216.0
    return u1, u2


def box_muller64(a, b):
    u1, u2 = uniforms(a, b)
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(_TWO_PI * u2), r * np.sin(_TWO_PI * u2)


def box_muller32(a, b):
    """The same map with every operation rounded to float32 (NumPy's float32 log / sqrt / cos /
    sin). Only used to measure the float32 rounding floor of a draw, :func:`rounding_floor`."""
    u1, u2 = uniforms(a, b)
    u1, u2 = u1.astype(np.float32), u2.astype(np.float32)   # 24-bit values: exact
    r = np.sqrt(np.float32(-2.0) * np.log(u1))
    t = np.float32(_TWO_PI) * u2
    n0, n1 = r * np.cos(t), r * np.sin(t)
    assert n0.dtype == np.float32 and n1.dtype == np.float32
    return n0, n1


def _split(v):
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v & 0xFFFFFFFF, v >> 32


def _stream_c3(off_hi, stream_id):
    return off_hi ^ ((int(stream_id) * _STREAM_MULT) & 0xFFFFFFFF)


def _group_words(x, y, z, w):
    """Per-group Philox words -> per-element (a, b, odd): element q of a group draws from
    box_muller(x, y) for q < 2 and box_muller(z, w) otherwise, taking n0 (q even) or n1."""
    a = np.stack([x, x, z, z], axis=-1)
    b = np.stack([y, y, w, w], axis=-1)
    odd = np.broadcast_to(np.array([False, True, False, True]), a.shape)
    flat = a.shape[:-2] + (a.shape[-2] * 4,)
    return a.reshape(flat), b.reshape(flat), odd.reshape(flat)


def reparam_words(B, D, seed, offset, stream_id):
    """(a, b, odd), each [B, D]: the two Philox words behind every element of reparam_sample's
    eps and whether it takes the sine (odd) or cosine normal of that pair."""
    k0, k1 = _split(seed)
    off_lo, off_hi = _split(offset)
    g = np.arange((D + 3) // 4, dtype=np.uint64)[None, :]
    row = np.arange(B, dtype=np.uint64)[:, None]
    a, b, odd = _group_words(*philox4x32_10(g, row, off_lo, _stream_c3(off_hi, stream_id), k0, k1))
    return a[:, :D], b[:, :D], odd[:, :D]


def normal_fill_words(n, seed, offset, stream_id):
    k0, k1 = _split(seed)
    off_lo, off_hi = _split(offset)
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    a, b, odd = _group_words(*philox4x32_10(g & _M32, (g >> _S32) ^ np.uint64(_FILL_HI_XOR), off_lo,
                                            _stream_c3(off_hi, stream_id), k0, k1))
    return a[:n], b[:n], odd[:n]


def vae_words(B, dz, seed, offset):
    """vae_step keeps only the low 32 bits of the seed; lanes 2p and 2p + 1 share one pair."""
    k0, _ = _split(seed)
    off_lo, off_hi = _split(offset)
    row = np.arange(B, dtype=np.uint64)[:, None]
    lane = np.arange(dz, dtype=np.uint64)[None, :]
    x, y, _, _ = philox4x32_10(row, lane >> np.uint64(1), off_lo, off_hi ^ _VAE_C3_XOR, k0, _VAE_K1)
    return x, y, np.broadcast_to((lane & np.uint64(1)).astype(bool), x.shape)


def _normals(words, bm):
    a, b, odd = words
    n0, n1 = bm(a, b)
    return np.where(odd, n1, n0)


def reparam_eps(B, D, seed, offset, stream_id, bm=box_muller64):
    """eps [B, D] of vinf::reparam_sample (float64)."""
    return _normals(reparam_words(B, D, seed, offset, stream_id), bm)


def normal_fill_ref(n, seed, offset, stream_id, bm=box_muller64):
    """The n values of vinf::normal_fill (float64)."""
    return _normals(normal_fill_words(n, seed, offset, stream_id), bm)


def vae_eps(B, dz, seed, offset, bm=box_muller64):
    """eps [B, dz] of the Philox branch of vinf::vae_step (float64)."""
    return _normals(vae_words(B, dz, seed, offset), bm)


def rounding_floor(layout_fn, *args):
    """F = max |box_muller32 - box_muller64| over the very draws of one case: what evaluating
    the same formula in float32 costs, from the reference alone."""
    lo = layout_fn(*args, bm=box_muller32).astype(np.float64)
    return float(np.max(np.abs(lo - layout_fn(*args, bm=box_muller64))))
