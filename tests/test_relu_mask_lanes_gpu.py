"""Lane-private ReLU mask of the 256x256 GEMM (csrc/include/gemm_tile.h, "Lane-private ReLU
mask"): the forward product writes each lane's 128 mask bits as that lane's own 16 bytes and the
input gradient reads them back the same way. The encoding is private to the kernel, so nothing
here decodes it: the mask is read THROUGH the input gradient (dy = 1, W = I turns it into the
0 / 1 matrix it stands for), and everything else is compared bitwise with the row-major mode on
the same inputs. No tolerance anywhere: results must not depend on the mask's layout."""
import functools

import pytest
import torch

import gemm_exact as gx

pytestmark = pytest.mark.gpu

BF, U8 = torch.bfloat16, torch.uint8
SWITCHES = ("gemm_set_mode", "gemm_persist", "gemm_grid_reserve")


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


def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def _state(o, persist, grid8=False):
    """The 256x256 kernel, launch form `persist` (0 one block per tile, 1 fixed tile lists,
    2 claimed tiles); grid8: every CU but 8 reserved, so 8 blocks walk several tiles each."""
    o.gemm_set_mode(2)
    o.gemm_persist(persist)
    o.gemm_grid_reserve(_cus() if grid8 else 0)


# ------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def edge_inputs(M, N, K):
    """x [M, K], W [N, K], b [N] (CPU bf16, small integers as in gemm_exact: every fp32 sum is
    exact) whose pre-activations x W^T + b also hold, in every 256x256 tile, wave row, wave
    column and 64-row pass:
      - rows that are all positive / all negative, columns that are all positive / all negative;
      - on special rows (only x[:, 0] = 2^-70 non-zero): 2^-133 (the smallest positive bf16
        subnormal), +2^-140 and -2^-140 (fp32 values that round to +0 / -0 in bf16), and +0 /
        -0 biases under an all-zero product.
    The mask bit is defined on the STORED bf16, so the tests take it from the kernel's own
    output; these inputs only make sure the hard values occur."""
    x = gx.gen_bf16((M, K), seed=11 + M + 3 * K).t.clone()
    w = gx.gen_bf16((N, K), seed=23 + N + 5 * K).t.clone()
    b = gx.gen_grid((N,), seed=31 + N, shift=0, bound=7, dtype=BF).t.clone()
    n = torch.arange(N)
    m = torch.arange(M)
    x[:, 0] = 0
    # column 2 of K carries the row sign: +-16 beats |b| <= 7
    w[:, 2] = 1
    for r, v in ((9, 16.0), (201, 16.0), (77, -16.0), (150, -16.0)):
        rows = m[m % 256 == r]
        x[rows] = 0
        x[rows, 2] = v
    tiny = m[(m % 256 == 5) | (m % 256 == 70) | (m % 256 == 133) | (m % 256 == 200)]
    x[tiny] = 0
    x[tiny, 0] = 2.0 ** -70
    w[:, 0] = 0
    w[n % 37 == 0, 0] = 2.0 ** -63      # product 2^-133
    w[n % 37 == 1, 0] = -(2.0 ** -70)   # product -2^-140
    w[n % 37 == 2, 0] = 2.0 ** -70      # product +2^-140
    b[n % 37 <= 3] = 0.0
    b[n % 37 == 4] = -0.0
    for c, v in ((11, 1.0), (190, -1.0)):   # whole columns of one sign
        cols = n[n % 256 == c]
        w[cols] = 0
        b[cols] = v
    return x, w, b


@functools.lru_cache(maxsize=None)
def plain_inputs(M, N, K):
    x = gx.gen_bf16((M, K), seed=101 + M + 3 * K).t
    w = gx.gen_bf16((N, K), seed=202 + N + 5 * K).t
    b = gx.gen_grid((N,), seed=303 + N, shift=0, bound=7, dtype=BF).t
    return x, w, b


@functools.lru_cache(maxsize=None)
def dgrad_inputs(M, N, K):
    dy = gx.gen_bf16((M, K), seed=404 + M + K).t
    w = gx.gen_bf16((K, N), seed=505 + N + K).t
    return dy, w, w.t().contiguous()


def _fwd(dev, x, w, b, lanes, guard=64):
    """(y, mask, guard bytes behind the mask) of linear_fwd with bias + ReLU."""
    from vi_normflows_amd.ops import gemm

    M, N = x.shape[0], w.shape[0]
    y = torch.full((M, N), float("nan"), dtype=BF, device=dev)
    raw = torch.full((M * N // 8 + guard,), gx.CANARY, dtype=U8, device=dev)
    mask = raw[:M * N // 8].view(M, N // 8)
    gemm.linear_fwd(x.to(dev), w.to(dev), b.to(dev), y, relu=True, mask_out=mask,
                    mask_lanes=lanes)
    return y, mask, raw[M * N // 8:]


def _mask_as_matrix(dev, mask, M, N, lanes, wt):
    """The 0 / 1 matrix a mask stands for, read through the input gradient: 1 * I * mask."""
    from vi_normflows_amd.ops import gemm

    Kp = (N + 31) // 32 * 32   # the products need K % 32 == 0: zero rows below the identity
    ones = torch.ones(M, Kp, dtype=BF, device=dev)
    eye = torch.zeros(Kp, N, dtype=BF, device=dev)
    eye[:N] = torch.eye(N, dtype=BF, device=dev)
    out = torch.full((M, N), float("nan"), dtype=BF, device=dev)
    gemm.linear_dgrad(ones, eye, out, relu_bits=mask, Wt=eye.t().contiguous() if wt else None,
                      bits_lanes=lanes)
    return out


# ------------------------------------------------------------------------------ 1. the mask
@pytest.mark.parametrize("K", [32, 96, 416, 1024])
@pytest.mark.parametrize("M,N", [(256, 256), (512, 512), (768, 1024)])
def test_mask_is_right(ops, gpu, M, N, K):
    """Forward in lane mode, then the input gradient in lane mode with dy = 1 and W = I: the
    output is exactly 1(act > 0). K = 32 runs the one-tile-per-block kernel (persistent launches
    need K > 64), the others the persistent one; 768 x 1024 on 8 blocks also walks the tile
    boundary (mask load ahead of the next tile's operand burst)."""
    x, w, b = edge_inputs(M, N, K)
    _state(ops, 1, grid8=(M, N) == (768, 1024))
    y, mask, _ = _fwd(gpu, x, w, b, lanes=True)
    got = _mask_as_matrix(gpu, mask, M, N, lanes=True, wt=True)
    gx.assert_exact(got, (y > 0).to(BF), f"lane mask M{M} N{N} K{K}")
    # the hard values did occur, and the forward output is the row-major mode's
    y_rm, mask_rm, _ = _fwd(gpu, x, w, b, lanes=False)
    gx.assert_exact(y, y_rm, f"forward output M{M} N{N} K{K}")
    assert torch.equal(mask_rm, gx.pack_bits(y > 0))
    pos, n = (y > 0), torch.arange(N, device=gpu)
    assert pos[9, n % 256 != 190].all() and not pos[77, n % 256 != 11].any()
    assert pos[:, 11].all() and not pos[:, 190].any()
    # -2^-140, +2^-140 (stored as 0) and an all-zero product: none of them is > 0 as stored
    assert not pos[5, 1:4].any() and not pos[200, 38:41].any()


@pytest.mark.parametrize("persist", [0, 1, 2])
def test_mask_is_right_nn_form(ops, gpu, persist):
    """The input gradient without W^T (the NN instantiation) reads the same bytes."""
    M, N, K = 512, 512, 96
    x, w, b = edge_inputs(M, N, K)
    _state(ops, persist)
    y, mask, _ = _fwd(gpu, x, w, b, lanes=True)
    got = _mask_as_matrix(gpu, mask, M, N, lanes=True, wt=False)
    gx.assert_exact(got, (y > 0).to(BF), f"lane mask, NN input gradient, persist {persist}")


# ------------------------------------------------------------------------ 2. equivalence
def _equivalence(ops, gpu, M, N, K, persist, grid8):
    from vi_normflows_amd.ops import gemm

    x, w, b = plain_inputs(M, N, K)
    dy, wd, wdt = dgrad_inputs(M, N, K)
    _state(ops, persist, grid8)
    y_l, mask_l, _ = _fwd(gpu, x, w, b, lanes=True)
    y_r, mask_r, _ = _fwd(gpu, x, w, b, lanes=False)
    gx.assert_exact(y_l, y_r, "forward output, lane vs row-major")
    outs = []
    for kw in (dict(relu_bits=mask_l, bits_lanes=True), dict(relu_bits=mask_r),
               dict(relu_of=y_r)):
        o = torch.full((M, N), float("nan"), dtype=BF, device=gpu)
        gemm.linear_dgrad(dy.to(gpu), wd.to(gpu), o, Wt=wdt.to(gpu), **kw)
        outs.append(o)
    gx.assert_exact(outs[0], outs[1], "input gradient, lane bits vs row-major bits")
    gx.assert_exact(outs[0], outs[2], "input gradient, lane bits vs relu_of")
    return y_l, outs[0]


@pytest.mark.parametrize("persist", [0, 1, 2])
@pytest.mark.parametrize("K", [800, 1024])
def test_equals_row_major(ops, gpu, K, persist):
    _equivalence(ops, gpu, 512, 1024, K, persist, grid8=False)


@pytest.mark.parametrize("persist", [1, 2])
def test_equals_row_major_many_tiles_per_block(ops, gpu, persist):
    """16 tiles on 8 blocks: every block crosses a tile boundary (fixed lists and claims)."""
    _equivalence(ops, gpu, 1024, 1024, 800, persist, grid8=True)


# ---------------------------------------------------------------------- 3. repeatability
def test_repeatable(ops, gpu):
    """Twenty runs, identical bytes: the race screen of the 256x256 kernel."""
    first = None
    for _ in range(20):
        y, dx = _equivalence(ops, gpu, 1024, 1024, 800, 2, grid8=True)
        cur = (y.clone(), dx.clone())
        if first is None:
            first = cur
        assert torch.equal(first[0].view(torch.int16), cur[0].view(torch.int16))
        assert torch.equal(first[1].view(torch.int16), cur[1].view(torch.int16))


# ------------------------------------------------------------------------- 4. guard bytes
@pytest.mark.parametrize("persist", [0, 1, 2])
def test_guard_bytes(ops, gpu, persist):
    x, w, b = plain_inputs(512, 512, 416)
    _state(ops, persist)
    _, mask, guard = _fwd(gpu, x, w, b, lanes=True)
    assert (guard == gx.CANARY).all(), "bytes behind the lane-private mask were written"
    assert not (mask == gx.CANARY).all()


@pytest.mark.parametrize("M,N", [(300, 256), (256, 264)])
def test_ineligible_shape_falls_back(ops, gpu, M, N):
    """M or N off the 256 grid: the launcher refuses lane mode, both wrappers use the row-major
    mask, and the results are the row-major ones."""
    from vi_normflows_amd.ops import gemm

    K = 96
    x, w, b = plain_inputs(M, N, K)
    _state(ops, 1)
    y = torch.empty(M, N, dtype=BF, device=gpu)
    mk = torch.zeros(M, N // 8, dtype=U8, device=gpu)
    assert ops.gemm_nt(x.to(gpu), w.to(gpu), b.to(gpu), y, 1, mk, True) == gemm.LANES_SHAPE
    assert (mk == 0).all(), "a refused launch must not run"
    assert not gemm.mask_lanes_route(M, N, K, N, True)
    y_l, mask_l, guard = _fwd(gpu, x, w, b, lanes=True)
    y_r, mask_r, _ = _fwd(gpu, x, w, b, lanes=False)
    gx.assert_exact(y_l, y_r, "fallback forward")
    assert torch.equal(mask_l, mask_r) and torch.equal(mask_l, gx.pack_bits(y_l > 0))
    assert (guard == gx.CANARY).all()
    got = _mask_as_matrix(gpu, mask_l, M, N, lanes=True, wt=True)
    gx.assert_exact(got, (y_l > 0).to(BF), "fallback input gradient")


def test_small_kernel_route_is_an_error(ops, gpu):
    """A shape on the grid whose product runs the 128x128 kernel: never a silent row-major
    mask under a lane-mode request (the reading side could not tell)."""
    from vi_normflows_amd.ops import gemm

    x, w, b = plain_inputs(256, 256, 96)
    ops.gemm_set_mode(1)
    assert not gemm.mask_lanes_route(256, 256, 96, 256, False)
    with pytest.raises(RuntimeError, match="128x128"):
        _fwd(gpu, x, w, b, lanes=True)


# ------------------------------------------------------------------------------ 5. engine
def _engine_run(gpu, hidden, lanes):
    from vi_normflows_amd.models.realnvp import RealNVPConfig, RealNVPVI
    from vi_normflows_amd.utils.config import KernelPaths

    paths = KernelPaths()
    paths.relu_mask_lanes = lanes
    cfg = RealNVPConfig(dim=16, n_layers=2, hidden=hidden, anneal="none", paths=paths)
    eng = RealNVPVI(cfg, batch=512, device=gpu, lr=1e-3, seed=3)
    g = torch.Generator().manual_seed(7)
    eng.eps_override = torch.randn(512, 16, generator=g).to(gpu)
    eng.train_step()
    eng.train_step()
    torch.cuda.synchronize()
    P = eng.params
    return eng.loss.clone(), P.grad.clone(), P.master.clone(), list(eng.mk_lanes)


@pytest.mark.parametrize("hidden,eligible", [(256, True), (264, False), (288, False)])
def test_engine_bitwise(ops, gpu, hidden, eligible):
    """Two training steps with the KernelPaths switch on and off: loss, gradients and master
    weights bitwise equal. The 256x256 kernel is forced so that hidden = 256 really keeps its
    masks lane-private at this small batch; hidden = 264 and 288 are off the 256 grid and must
    fall back. (hidden = 264 is not a multiple of the MFMA K step either: the bf16 GPU engine
    stores it as 288 with 24 inert zero units per hidden layer, see test_padded_hidden_is_inert.)"""
    ops.gemm_set_mode(2)
    on = _engine_run(gpu, hidden, True)
    off = _engine_run(gpu, hidden, False)
    assert on[3] == [eligible] * len(on[3]) and not any(off[3])
    for a, b_, what in zip(on[:3], off[:3], ("loss", "grad", "master")):
        assert torch.equal(a.view(torch.int32), b_.view(torch.int32)), what


def test_engine_auto_kernel_choice(gpu):
    """Under the automatic kernel choice a batch this small runs the 128x128 kernel, and the
    engine keeps the row-major masks without being told."""
    on = _engine_run(gpu, 256, True)
    off = _engine_run(gpu, 256, False)
    assert not any(on[3])
    for a, b_ in zip(on[:3], off[:3]):
        assert torch.equal(a.view(torch.int32), b_.view(torch.int32))


def test_padded_hidden_is_inert(gpu):
    """hidden = 264 on the bf16 GPU engine is stored 288 wide. The 24 extra units of each hidden
    layer have zero weights and biases, and two training steps leave every one of those entries,
    and its gradient, exactly zero: the model trained is the 264-wide one. Its initial weights
    are the ones the unpadded (CPU) engine draws from the same seed."""
    from vi_normflows_amd.models.realnvp import RealNVPConfig, RealNVPVI

    cfg = RealNVPConfig(dim=16, n_layers=2, hidden=264, anneal="none")
    eng = RealNVPVI(cfg, batch=512, device=gpu, lr=1e-3, seed=3)
    ref = RealNVPVI(cfg, batch=512, device="cpu", lr=1e-3, seed=3)
    assert eng.Hp == 288 and ref.Hp == 264
    P, R = eng.params, ref.params
    for l in range(2):
        for i in range(3):
            W, Wr = P.p(f"l{l}.W{i}").cpu(), R.p(f"l{l}.W{i}")
            assert torch.equal(W[:Wr.shape[0], :Wr.shape[1]], Wr)
    eng.eps_override = torch.randn(512, 16, generator=torch.Generator().manual_seed(7)).to(gpu)
    eng.train_step()
    eng.train_step()
    torch.cuda.synchronize()
    assert torch.isfinite(eng.loss).item()
    for l in range(2):
        for get in (P.p, P.g):
            for i in (0, 1):   # rows of the padded units (weights into them, their biases)
                assert (get(f"l{l}.W{i}")[264:] == 0).all() and (get(f"l{l}.b{i}")[264:] == 0).all()
            for i in (1, 2):   # columns reading the padded units
                assert (get(f"l{l}.W{i}")[:, 264:] == 0).all()
        assert (P.p(f"l{l}.W1")[:264, :264] != 0).any()

