"""The exact-operand GEMM oracle (tests/gemm_exact.py) checked on the CPU: its generators keep
fp32 accumulation exact, and its comparisons reject the corruptions a subtly wrong kernel
produces - including two that the max-normalised `_check` of tests/test_gemm_gpu.py accepts."""
import pytest
import torch

import gemm_exact as gx


# ------------------------------------------------------------------------------ generators
@pytest.mark.parametrize("gen,bound,dtype", [(gx.gen_bf16, 7, torch.bfloat16),
                                             (gx.gen_e4m3, 8, torch.float8_e4m3fn)])
@pytest.mark.parametrize("shift", [0, 3, 6])
def test_generators_round_trip(gen, bound, dtype, shift):
    a = gen((37, 96), seed=1, shift=shift)
    assert a.t.dtype == dtype
    assert int(a.i.abs().max()) == bound
    assert torch.equal(a.t.double(), a.i.double() * 2.0 ** -shift)      # stored exactly
    assert torch.equal(a.t.float().to(dtype).view(torch.uint8), a.t.view(torch.uint8))
    share = (a.i == 0).double().mean().item()
    assert 0.2 < share < 0.45                                           # ReLU masks non-trivial


def test_e4m3_integers_to_16_are_exact():
    i = torch.arange(-16, 17, dtype=torch.float32)
    assert torch.equal(i.to(torch.float8_e4m3fn).float(), i)


def test_bf16_conversion_is_nearest_even():
    x = torch.tensor([257.0, 259.0, 261.0, 263.0])
    assert x.to(torch.bfloat16).float().tolist() == [256.0, 260.0, 260.0, 264.0]


def test_bound_is_asserted():
    a = gx.gen_bf16((8, 64), seed=2)
    b = gx.gen_bf16((64, 8), seed=3)
    worst = gx.assert_exact_bound(a, b)
    assert worst == int((a.i.abs() @ b.i.abs()).max())
    big = gx.Exact(torch.full((8, 8), gx.EXACT - 1), 0, torch.float32)
    with pytest.raises(AssertionError, match="2\\^24"):
        gx.assert_exact_bound(a, b, big)
    fine = gx.gen_grid((8, 8), seed=4, shift=1, bound=3)
    with pytest.raises(AssertionError, match="finer"):
        gx.assert_exact_bound(a, b, fine)


def test_fp32_accumulation_exact_in_any_k_order_k65536():
    K = 65536
    a = gx.gen_bf16((24, K), seed=5, shift=2, zero_share=0.0)
    b = gx.gen_bf16((K, 16), seed=6, shift=1, zero_share=0.0)
    worst = gx.assert_exact_bound(a, b)
    assert 500_000 < worst < gx.EXACT
    want = (a.i @ b.i).double() * 2.0 ** -3                              # int64 product
    got = a.t.float() @ b.t.float()                                      # fp32 accumulation
    assert torch.equal(got.double(), want)
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(7))
    got_p = a.t.float()[:, perm] @ b.t.float()[perm]
    assert torch.equal(got_p, got)
    assert torch.equal(gx.product(a, b), want)
    assert torch.equal(gx.to_f32(want), got)


def test_views_are_aligned_and_poisoned():
    t = gx.gen_bf16((5, 24), seed=8).t
    v = gx.place_operand(t, "cpu")
    assert torch.equal(v, t) and v.stride(0) > 24 and v.stride(0) % 8 == 0
    assert v.data_ptr() % 16 == 0 and v.storage_offset() > 0
    q = gx.place_operand(gx.gen_e4m3((5, 32), seed=9).t, "cpu")
    assert q.stride(0) % 16 == 0 and q.data_ptr() % 16 == 0
    base = q._base.view(torch.uint8)
    assert int((base == gx.E4M3_NAN).sum()) == base.numel() - 5 * 32 + int((q.view(torch.uint8) == gx.E4M3_NAN).sum())
    buf, o = gx.place_output((5, 24), torch.float32, "cpu")
    assert torch.isnan(o).all() and o.stride(0) % 4 == 0 and o.data_ptr() % 16 == 0
    gx.assert_canary(buf, o)
    buf, o = gx.place_output((5, 24), torch.float32, "cpu", init=torch.ones(5, 24))
    assert (o == 1).all()
    vb, vv = gx.place_vector(40, torch.float32, "cpu")
    assert torch.isnan(vv).all() and vv.data_ptr() % 16 == 0
    gx.assert_canary(vb, vv)


# ----------------------------------------------------------------------------- sensitivity
M, N, K = 300, 800, 416


@pytest.fixture(scope="module")
def case():
    """x [M, K], W [N, K], a bf16 bias spanning a large range: y = bf16(x W^T + b)."""
    x = gx.gen_bf16((M, K), seed=11, shift=1)
    wt = gx.Exact(gx.gen_bf16((N, K), seed=12, shift=2).i.t().contiguous(), 2, torch.bfloat16)
    # bf16 holds 8 significant bits: |integer| <= 255, times 2^10 on the product grid 2^-3
    bi = gx._ints((N,), 255, seed=13) * 1024
    b = gx.Exact(bi, 3, torch.bfloat16)
    gx.assert_exact_bound(x, wt, b)
    ref64 = gx.product(x, wt) + b.d
    return x, wt, b, ref64


def _gpu_suite_check():
    from test_gemm_gpu import _check

    return _check


def test_assert_exact_accepts_the_reference(case):
    *_, ref64 = case
    gx.assert_exact(gx.to_bf16(ref64), gx.to_bf16(ref64.clone()))
    gx.assert_exact(gx.to_f32(ref64), gx.to_f32(ref64.clone()))


def test_rejects_one_bf16_ulp_that_the_max_normalised_check_accepts(case):
    *_, ref64 = case
    ref = gx.to_bf16(ref64)
    out = ref.clone()
    i, j = 299, 797                                   # an edge row, the last 16-column group
    out.view(torch.int16)[i, j] += 1
    assert out[i, j] != ref[i, j]
    with pytest.raises(AssertionError, match=r"1 of 240000 .*\n.*\(299, 797\).*tile256 \(1, 3\) "
                                             r"tile128 \(2, 6\) colgroup16 49"):
        gx.assert_exact(out, ref, "ulp")
    _gpu_suite_check()(out, ref.float(), 1e-2)        # the gap: passes the existing bound


def test_rejects_a_missing_k_step_that_the_max_normalised_check_accepts(case):
    x, wt, b, ref64 = case
    ref = gx.to_bf16(ref64)
    r0, c0, k0 = 288, 784, 384                        # edge fragment, the 32-deep K tail
    out64 = ref64.clone()
    out64[r0:r0 + 16, c0:c0 + 16] -= x.d[r0:r0 + 16, k0:k0 + 32] @ wt.d[k0:k0 + 32, c0:c0 + 16]
    out = gx.to_bf16(out64)
    nbad = int((out.view(torch.int16) != ref.view(torch.int16)).sum())
    assert nbad >= 64                                 # most of the 12 x 16 fragment is wrong
    with pytest.raises(AssertionError, match="tile256 \\(1, 3\\)"):
        gx.assert_exact(out, ref, "kstep")
    _gpu_suite_check()(out, ref.float(), 1e-2)        # the gap: passes the existing bound


def test_rejects_nan_left_in_the_output(case):
    *_, ref64 = case
    ref = gx.to_f32(ref64)
    out = ref.clone()
    out[128, 256] = float("nan")
    with pytest.raises(AssertionError, match="1 NaN"):
        gx.assert_exact(out, ref)


def test_rejects_swapped_rows(case):
    *_, ref64 = case
    ref = gx.to_bf16(ref64)
    out = ref.clone()
    out[[16, 17]] = ref[[17, 16]]
    with pytest.raises(AssertionError, match="differ bitwise"):
        gx.assert_exact(out, ref)


def test_rejects_a_tie_rounded_away_from_even():
    ref64 = torch.full((4, 16), 3.0, dtype=torch.float64)
    ref64[2, 5] = 257.0                               # tie between 256 and 258
    ref = gx.to_bf16(ref64)
    assert ref[2, 5].item() == 256.0
    out = ref.clone()
    out[2, 5] = 258.0                                 # round-half-away
    with pytest.raises(AssertionError, match=r"\(2, 5\): got 258.0 .* want 256.0"):
        gx.assert_exact(out, ref)


def test_rejects_a_flipped_canary_byte():
    for dtype in (torch.bfloat16, torch.float32, torch.uint8, torch.float8_e4m3fn):
        buf, view = gx.place_output((9, 40), dtype, "cpu")
        gx.assert_canary(buf, view)
        raw = buf.view(torch.uint8)
        es = buf.element_size()
        raw[2, (view.storage_offset() % buf.stride(0) + 40) * es] ^= 1   # first byte right of row 0
        with pytest.raises(AssertionError, match="outside the output view"):
            gx.assert_canary(buf, view)
    vb, vv = gx.place_vector(24, torch.float32, "cpu")
    vb.view(torch.uint8)[-1] ^= 0x80
    with pytest.raises(AssertionError, match="outside the output view"):
        gx.assert_canary(vb, vv)


def test_rejects_a_flipped_bitmask_bit(case):
    *_, ref64 = case
    y = gx.to_bf16(ref64.clamp_min(0))
    bits = gx.pack_bits(y > 0)
    assert 0.2 < (y > 0).double().mean() < 0.8
    for j in range(N // 8):                           # bit e of byte j <-> column 8 j + e
        for e in range(8):
            assert bool((bits[7, j] >> e) & 1) == bool(y[7, 8 * j + e] > 0)
    out = bits.clone()
    out[299, 99] ^= 0x10
    with pytest.raises(AssertionError, match=r"\(299, 99\)"):
        gx.assert_exact(out, bits)
