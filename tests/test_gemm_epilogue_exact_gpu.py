"""The straight-line epilogues of the lane-private ReLU-mask products (csrc/include/gemm_tile.h,
epi_tile_lanes), pinned bitwise on the helpers of gemm_exact: exact operands, expected bytes
from the fp64 product, canaries around every output, each case run twice into fresh outputs.

Shapes are the smallest that reach every path of the new code: 256 x 256 is one tile;
1024 x 768 is 12 tiles, and with the grid held to 8 blocks the fixed lists have 2 and 1 tiles
(tile-boundary burst, second-tile epilogue); K = 128 is two K-tiles, the shortest the persistent
kernel accepts, K = 160 ends in a 32-deep tail. The claimed-tile mode gets the 12-tile shape once.

The mask's encoding is private to the kernels, so it is read back the way
test_relu_mask_lanes_gpu.py does: through the input gradient with dy = 1 and W = I.

The fused coupling epilogues (gemm_nt_cpl / gemm_nn_cpl), which only changed in how they pack
bf16 pairs, are covered at Dh = 136, K = 128 and M = 520 (two full row tiles and an 8-row edge)
by test_gemm_exact_gpu.py::test_coupling_forward_epilogue / test_coupling_backward_epilogue.
"""
import functools

import pytest
import torch

import gemm_exact as gx

pytestmark = pytest.mark.gpu

BF, U8 = torch.bfloat16, torch.uint8
SWITCHES = ("gemm_set_mode", "gemm_persist", "gemm_grid_reserve")
GUARD = 64   # canary bytes in front of and behind the flat lane-layout mask

# (persist mode, hold the grid to 8 blocks, M, N, K)
CASES = [(1, False, 256, 256, 128), (1, False, 256, 256, 160),
         (1, True, 1024, 768, 128), (1, True, 1024, 768, 160),
         (2, True, 1024, 768, 128)]
IDS = [f"persist{p}-{'grid8-' if g else ''}{M}x{N}x{K}" for p, g, M, N, K in CASES]


@pytest.fixture
def ops(gpu):
    """torch.ops.vinf with the process-global GEMM switches used here saved and restored."""
    o = torch.ops.vinf
    saved = [(n, getattr(o, n)(-1)) for n in SWITCHES]
    try:
        yield o
    finally:
        for n, v in saved:
            getattr(o, n)(v)


def _state(o, persist, grid8):
    o.gemm_set_mode(2)
    o.gemm_persist(persist)
    o.gemm_grid_reserve(torch.cuda.get_device_properties(0).multi_processor_count if grid8 else 0)


def _lane_mask(dev, M, N, fill):
    """A flat, 16-B aligned M*N/8-byte mask between two canary guards. Returns (buffer, view)."""
    buf = torch.full((M * N // 8 + 2 * GUARD,), gx.CANARY, dtype=U8, device=dev)
    view = buf[GUARD:GUARD + M * N // 8]
    view.fill_(fill)
    return buf, view.view(M, N // 8)


def _mask_as_matrix(o, dev, mask, M, N, wt):
    """The 0 / 1 matrix a lane-layout mask stands for: 1 * I * mask."""
    ones = torch.ones(M, N, dtype=BF, device=dev)
    eye = torch.eye(N, dtype=BF, device=dev)
    out = torch.full((M, N), float("nan"), dtype=BF, device=dev)
    assert o.gemm_nn(ones, eye, None, out, False, mask, eye if wt else None, True) == 0
    return out


# ------------------------------------------------------------------------------ forward
@functools.lru_cache(maxsize=None)
def fwd_data(M, N, K):
    x = gx.gen_bf16((M, K), seed=8100 + M + 3 * K, shift=1)
    w = gx.gen_bf16((N, K), seed=8200 + N + 5 * K, shift=2)
    b = gx.gen_grid((N,), seed=8300 + N, shift=1, bound=255, dtype=BF)
    # rows whose product is exactly zero under +0 and under non-zero biases
    x.i[5::64] = 0
    x = gx.Exact(x.i, x.shift, BF)
    w_t = gx.Exact(w.i.t().contiguous(), w.shift, BF)
    gx.assert_exact_bound(x, w_t, b)
    pre = gx.product(x, w_t) + b.d
    assert (pre > 0).any() and (pre < 0).any() and (pre == 0).any()
    return x, w, b, pre


@pytest.mark.parametrize("persist,grid8,M,N,K", CASES, ids=IDS)
def test_lane_mask_forward(ops, gpu, persist, grid8, M, N, K):
    """gemm_nt(..., mask, mask_lanes=True): y = bf16(relu(x W^T + b)) and the mask, exact."""
    x, w, b, pre = fwd_data(M, N, K)
    ref = gx.to_bf16(pre.clamp_min(0))
    xv, wv, bd = gx.place_operand(x.t, gpu), gx.place_operand(w.t, gpu), b.to(gpu)
    _state(ops, persist, grid8)
    masks = []
    for rep in range(2):
        what = f"lane-mask forward M{M} N{N} K{K} persist{persist} rep{rep}"
        yb, y = gx.place_output((M, N), BF, gpu)
        mb, m = _lane_mask(gpu, M, N, 0x00 if rep else 0xFF)
        assert ops.gemm_nt(xv, wv, bd, y, 1, m, True) == 0, "lane mode refused"
        gx.assert_exact(y, ref, what + " y")
        gx.assert_canary(yb, y, what + " y")
        assert (mb[:GUARD] == gx.CANARY).all() and (mb[-GUARD:] == gx.CANARY).all(), what
        for wt in (False, True):
            got = _mask_as_matrix(ops, gpu, m, M, N, wt)
            gx.assert_exact(got, (ref > 0).to(BF), f"{what} mask read back, Wt {wt}")
        masks.append(m.clone())
    # every mask byte is written: the same bytes over a 0xFF and over a 0x00 prefill
    gx.assert_exact(masks[0], masks[1], "lane mask bytes, rep 0 vs rep 1")


# ----------------------------------------------------------------------- input gradient
@functools.lru_cache(maxsize=None)
def dgrad_data(M, N, K):
    dy = gx.gen_bf16((M, K), seed=8400 + M + 3 * K, shift=2)
    w = gx.gen_bf16((K, N), seed=8500 + N + 5 * K, shift=1)
    h = gx.gen_bf16((M, N), seed=8600 + M + N, shift=0, zero_share=0.3)
    gx.assert_exact_bound(dy, w)
    return dy, w, h, gx.product(dy, w)


def _lanes_of(o, dev, h):
    """The lane-layout mask of 1(h > 0), written by the forward product h I^T (no bias)."""
    M, N = h.shape
    eye = torch.eye(N, dtype=BF, device=dev)
    y = torch.empty(M, N, dtype=BF, device=dev)
    _, m = _lane_mask(dev, M, N, 0xFF)
    assert o.gemm_nt(h.to(dev), eye, None, y, 1, m, True) == 0, "lane mode refused"
    return m


@pytest.mark.parametrize("persist,grid8,M,N,K", CASES, ids=IDS)
def test_lane_mask_input_gradient(ops, gpu, persist, grid8, M, N, K):
    """gemm_nn(..., hbits, Wt, hbits_lanes=True), with and without Wt: dx = bf16(dy W) where the
    bit is set and +0 elsewhere, exact."""
    dy, w, h, p = dgrad_data(M, N, K)
    keep = h.d > 0
    ref = gx.to_bf16(torch.where(keep, p, torch.zeros((), dtype=torch.float64)))
    dyv, wv = gx.place_operand(dy.t, gpu), gx.place_operand(w.t, gpu)
    wtv = gx.place_operand(w.t.t().contiguous(), gpu)
    _state(ops, persist, grid8)
    bits = _lanes_of(ops, gpu, h.t)
    before = bits.clone()
    for rep in range(2):
        for wt in (None, wtv):
            what = (f"lane-mask input gradient M{M} N{N} K{K} persist{persist} "
                    f"{'Wt' if wt is not None else 'W'} rep{rep}")
            ob, out = gx.place_output((M, N), BF, gpu)
            assert ops.gemm_nn(dyv, wv, None, out, False, bits, wt, True) == 0, "lane mode refused"
            gx.assert_exact(out, ref, what)
            gx.assert_canary(ob, out, what)
    gx.assert_exact(bits, before, "the mask is only read")
