"""The fused LU / triangular solve (csrc/kernels/lu_solve.hip) on the MI355X: accuracy against the
fp64 composite, bitwise row independence, strides, gradients and the modules' dispatch.

Bound form (that of tests/test_made_sweep_gpu.py): ``|kernel - ref64| <= K max(err32, 8 eps32
max|ref64|)`` with ``err32`` the error of the fp32 CPU composite against the fp64 one on the same
(fp32-rounded) inputs. K is twice the worst ratio measured on the MI355X over the cases below,
rounded up to a power of two; a kernel that needs more than 16 is wrong.

Measured worst ratios (docs/PERF_NOTES.md, "LU solve"): solves 1.149 (D = 257, B = 1, lu, perm +
bias; 1.138 at D = 1024, 1.05 at D = 64, below 0.8 elsewhere) -> K = 4; gradients 0.851 (dA at
D = 200, lu; below 0.43 elsewhere) -> K = 2.
"""
import functools
import math

import pytest
import torch

from vi_normflows_amd.ops import linear_flow as lf

pytestmark = pytest.mark.gpu

WORST_SOLVE = 1.149  # measured worst |kernel - ref64| / max(err32, 8 eps32 max|ref64|), solves
WORST_GRAD = 0.851   # the same for the gradients of y, A and bias
K_SOLVE = 4
K_GRAD = 2
EPS32 = torch.finfo(torch.float32).eps


def test_k_rule():
    for worst, K in ((WORST_SOLVE, K_SOLVE), (WORST_GRAD, K_GRAD)):
        assert K == 2 ** math.ceil(math.log2(2 * worst)) and K <= 16


@functools.lru_cache(maxsize=None)
def recipe(D, B=37):
    g = torch.Generator().manual_seed(D)
    G = torch.randn(D, D, generator=g, dtype=torch.float64) / math.sqrt(D)
    L = torch.eye(D, dtype=torch.float64) + torch.tril(G, -1)
    U = torch.triu(G, 1) + torch.diag(0.5 + 1.5 * torch.rand(D, generator=g, dtype=torch.float64))
    g = torch.Generator().manual_seed(1000 + D)
    perm = torch.randperm(D, generator=g)
    b = torch.randn(D, generator=g, dtype=torch.float64)
    x = torch.randn(B, D, generator=g, dtype=torch.float64)
    return L, U, perm, b, x


@functools.lru_cache(maxsize=None)
def case(D, mode, transpose, with_perm):
    """fp32 inputs (CPU) with the fp64 and fp32 CPU composites on exactly those inputs."""
    L, U, perm, b, x = recipe(D)
    A = torch.tril(L, -1) + (U if mode == "lu" else torch.diag(torch.diagonal(U)))
    M = L @ U if mode == "lu" else A
    perm = perm if with_perm else None
    b = b if with_perm and not transpose else None
    if transpose:
        y = x
    else:
        y = x @ (M if perm is None else M[perm]).T + (0 if b is None else b)
    y32, A32 = y.float(), A.float()
    b32 = None if b is None else b.float()
    ref64 = lf.lu_solve_reference(y32.double(), A32.double(), perm,
                                  None if b32 is None else b32.double(), mode=mode,
                                  transpose=transpose)
    c32 = lf.lu_solve_reference(y32, A32, perm, b32, mode=mode, transpose=transpose)
    return y32, A32, perm, b32, ref64, (c32.double() - ref64).abs()


def on(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


def ratio(got, ref64, err32):
    bound = max(err32.max().item(), 8 * EPS32 * ref64.abs().max().item())
    return (got.double().cpu() - ref64).abs().max().item() / bound


@pytest.mark.parametrize("with_perm", [True, False])
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("mode", ["lu", "lower"])
@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("D", [1, 2, 5, 33, 64, 65, 200, 257, 1024])
def test_accuracy(gpu, D, B, mode, transpose, with_perm):
    y, A, perm, b, ref64, err32 = case(D, mode, transpose, with_perm)
    yd, Ad, pd, bd = on(gpu, y[:B], A, perm, b)
    n0 = lf.solve_launches()
    got = lf.lu_solve(yd, Ad, pd, bd, mode=mode, transpose=transpose)
    assert lf.solve_launches() == n0 + 1
    r = ratio(got, ref64[:B], err32[:B])
    print(f"lu_solve ratio D={D} B={B} {mode} T={int(transpose)} perm={int(with_perm)}: {r:.3f}")
    assert r <= K_SOLVE


@pytest.mark.parametrize("mode,D", [("lu", 65), ("lower", 200), ("lu", 1024)])
@pytest.mark.parametrize("transpose", [False, True])
def test_row_is_bitwise_independent_of_the_batch(gpu, mode, D, transpose):
    y, A, perm, b, _, _ = case(D, mode, transpose, True)
    yd, Ad, pd, bd = on(gpu, y, A, perm, b)
    full = lf.lu_solve(yd, Ad, pd, bd, mode=mode, transpose=transpose)
    one = lf.lu_solve(yd[:1], Ad, pd, bd, mode=mode, transpose=transpose)
    assert torch.equal(one[0], full[0])
    last = lf.lu_solve(yd[36:], Ad, pd, bd, mode=mode, transpose=transpose)
    assert torch.equal(last[0], full[36])           # another place in the tile
    assert torch.equal(lf.lu_solve(yd, Ad, pd, bd, mode=mode, transpose=transpose), full)


@pytest.mark.parametrize("transpose", [False, True])
def test_lower_mode_ignores_the_upper_triangle(gpu, transpose):
    y, A, perm, b, _, _ = case(65, "lower", transpose, True)
    yd, Ad, pd, bd = on(gpu, y, A, perm, b)
    An = Ad + torch.triu(torch.full_like(Ad, float("nan")), 1)
    assert torch.equal(lf.lu_solve(yd, An, pd, bd, mode="lower", transpose=transpose),
                       lf.lu_solve(yd, Ad, pd, bd, mode="lower", transpose=transpose))


@pytest.mark.parametrize("transpose", [False, True])
def test_row_strides(gpu, transpose):
    D = 65
    y, A, perm, b, _, _ = case(D, "lu", transpose, True)
    yd, Ad, pd, bd = on(gpu, y, A, perm, b)
    want = lf.lu_solve(yd, Ad, pd, bd, transpose=transpose)
    wide = torch.full((37, D + 9), float("nan"), device=gpu)
    wide[:, 3:3 + D] = yd
    assert torch.equal(lf.lu_solve(wide[:, 3:3 + D], Ad, pd, bd, transpose=transpose), want)
    out = torch.full((37, D + 7), -7.0, device=gpu)
    lf.lu_solve_kernel(wide[:, 3:3 + D], Ad, pd, bd, transpose=transpose, out=out[:, 5:5 + D])
    assert torch.equal(out[:, 5:5 + D], want)
    assert (out[:, :5] == -7).all() and (out[:, 5 + D:] == -7).all()   # nothing else written


def grads(fn, y, A, perm, b, mode, w):
    y, A, b = [t.clone().requires_grad_() for t in (y, A, b)]
    (fn(y, A, perm, b, mode=mode) * w).sum().backward()
    return y.grad, A.grad, b.grad


@pytest.mark.parametrize("mode", ["lu", "lower"])
@pytest.mark.parametrize("D", [5, 65, 200])
def test_gradients(gpu, D, mode):
    y, A, perm, b, _, _ = case(D, mode, False, True)
    w = torch.randn(37, D, generator=torch.Generator().manual_seed(D + 7), dtype=torch.float64)
    ref64 = grads(lf.lu_solve_reference, y.double(), A.double(), perm, b.double(), mode, w)
    c32 = grads(lf.lu_solve_reference, y, A, perm, b, mode, w.float())
    yd, Ad, pd, bd, wd = on(gpu, y, A, perm, b, w.float())
    n0 = lf.solve_launches()
    got = grads(lf.lu_solve, yd, Ad, pd, bd, mode, wd)
    assert lf.solve_launches() == n0 + 2          # the solve and its transpose
    for name, g, r64, r32 in zip(("y", "A", "bias"), got, ref64, c32):
        r = ratio(g, r64, (r32.double() - r64).abs())
        print(f"lu_solve grad ratio D={D} {mode} d{name}: {r:.3f}")
        assert r <= K_GRAD
    if mode == "lower":
        assert got[1].triu(1).abs().max() == 0


def test_modules_launch_the_kernel_once(gpu):
    from vi_normflows_amd.distributions.base import FullRankNormal
    from vi_normflows_amd.flows import LULinear

    torch.manual_seed(0)
    f = LULinear(64, seed=2).to(gpu)
    q = FullRankNormal(16).to(gpu)
    with torch.no_grad():
        for p in (*f.parameters(), *q.parameters()):
            p.add_(0.2 * torch.randn_like(p))
    z = torch.randn(37, 64, device=gpu)
    y, ldj = f(z)
    n0 = lf.solve_launches()
    x, ldj_inv = f.inverse(y.detach())
    assert lf.solve_launches() == n0 + 1
    assert (x - z).abs().max() < 1e-4 and torch.allclose(ldj_inv, -ldj)
    x.sum().backward()
    assert lf.solve_launches() == n0 + 2          # the backward: one more launch
    assert f.lower.grad is not None and f.lower.grad.triu().abs().max() == 0
    s = torch.randn(37, 16, device=gpu)
    n0 = lf.solve_launches()
    lp = q.log_prob(s)
    assert lf.solve_launches() == n0 + 1
    ref = torch.distributions.MultivariateNormal(
        q.mean.detach().double().cpu(), scale_tril=q.scale_tril.detach().double().cpu())
    assert (lp.detach().double().cpu() - ref.log_prob(s.double().cpu())).abs().max() < 1e-3
    lp.sum().backward()
    assert lf.solve_launches() == n0 + 2


def test_composite_outside_the_kernel(gpu):
    # fp64 tensors
    y, A, perm, b, ref64, _ = case(65, "lu", False, True)
    yd, Ad, pd, bd = on(gpu, y.double(), A.double(), perm, b.double())
    n0 = lf.solve_launches()
    got = lf.lu_solve(yd, Ad, pd, bd)
    assert got.dtype == torch.float64 and (got.cpu() - ref64).abs().max() < 1e-11
    # D above the kernel's limit
    D = 2049
    assert lf.kernel_supported(2048) and not lf.kernel_supported(D) and lf.kernel_rows(D) == 0
    y, A, perm, b, ref64, err32 = case(D, "lower", False, True)
    got = lf.lu_solve(*on(gpu, y[:3], A, perm, b), mode="lower")
    assert lf.solve_launches() == n0
    assert ratio(got, ref64[:3], err32[:3]) <= 16
    with pytest.raises(RuntimeError):
        lf.lu_solve(*on(gpu, y[:3], A, perm, b), mode="lower", impl="kernel")


def test_binding_checks(gpu):
    from vi_normflows_amd.ops._ext import native

    ops = native()
    y, A, perm, b, _, _ = case(5, "lu", False, True)
    yd, Ad, pd, bd = on(gpu, y, A, perm.int(), b)
    At = Ad.t().contiguous()
    x = torch.empty_like(yd)
    ops.lu_solve(yd, None, At, pd, bd, 0, False, True, x)
    assert torch.equal(x, lf.lu_solve(yd, Ad, pd, bd))
    assert lf.kernel_rows(5) >= 1 and lf.kernel_rows(1024) >= 1 and lf.kernel_rows(0) == 0
    bad = pd.clone()
    bad[2] = 5
    for args in ((yd, None, At, pd.long(), bd, 0, False, True, x),      # perm dtype
                 (yd, None, At, bad, bd, 0, False, True, x),            # perm range
                 (yd, Ad, None, pd, bd, 0, False, True, x),             # the orientation it reads
                 (yd, Ad, None, pd, bd, 0, True, True, x),              # a bias with transpose
                 (yd.double(), None, At, pd, bd, 0, False, True, x),    # dtype
                 (yd, None, At[:, :4], pd, bd, 0, False, True, x),      # shape
                 (yd, None, At, pd, bd, 2, False, True, x),             # mode
                 (yd, None, At, pd, bd, 0, False, True, x.t()),         # inner stride of x
                 (yd, None, At, pd, bd.cpu(), 0, False, True, x)):      # device
        with pytest.raises(RuntimeError):
            ops.lu_solve(*args)
    n0 = lf.solve_launches()
    empty = lf.lu_solve(yd[:0], Ad, pd, bd)
    assert empty.shape == (0, 5) and lf.solve_launches() == n0
