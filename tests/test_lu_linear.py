"""LU-linear flows and the full-rank Gaussian on the CPU: the composite solve against a dense
solve, the custom backward against finite differences, the modules' conventions, and full-rank
black-box VI on a correlated Gaussian target."""
import math

import pytest
import torch

from vi_normflows_amd.distributions.base import FullRankNormal
from vi_normflows_amd.flows import LULinear, NeuralSplineFlow, TriangularAffine
from vi_normflows_amd.inference import black_box_vi_full_rank
from vi_normflows_amd.inference.flow_vi import build_flow
from vi_normflows_amd.ops.linear_flow import lu_solve, lu_solve_reference, solve_launches


def recipe(D, B=37):
    """The matrix recipe of the LU-solve tests, in fp64: well-conditioned L, U, a permutation, a
    bias and the true x."""
    g = torch.Generator().manual_seed(D)
    G = torch.randn(D, D, generator=g, dtype=torch.float64) / math.sqrt(D)
    L = torch.eye(D, dtype=torch.float64) + torch.tril(G, -1)
    U = torch.triu(G, 1) + torch.diag(0.5 + 1.5 * torch.rand(D, generator=g, dtype=torch.float64))
    g = torch.Generator().manual_seed(1000 + D)
    perm = torch.randperm(D, generator=g)
    b = torch.randn(D, generator=g, dtype=torch.float64)
    x = torch.randn(B, D, generator=g, dtype=torch.float64)
    return L, U, perm, b, x


def packed(L, U, mode):
    if mode == "lu":
        return torch.tril(L, -1) + U
    return torch.tril(L, -1) + torch.diag(torch.diagonal(U))


def dense(L, U, perm, mode):
    M = L @ U if mode == "lu" else torch.tril(L, -1) + torch.diag(torch.diagonal(U))
    return M if perm is None else M[perm]


@pytest.mark.parametrize("D", [1, 5, 65])
@pytest.mark.parametrize("mode", ["lu", "lower"])
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("with_perm", [False, True])
def test_composite_matches_dense_solve(D, mode, transpose, with_perm):
    L, U, perm, b, x = recipe(D)
    perm = perm if with_perm else None
    b = b if with_perm and not transpose else None
    A, W = packed(L, U, mode), dense(L, U, perm, mode)
    y = x @ W.T + (0 if b is None else b)
    if not transpose:       # W x = y - b
        want = torch.linalg.solve(W, (y - (0 if b is None else b)).T).T
        got = lu_solve_reference(y, A, perm, b, mode=mode)
        assert (got - x).abs().max() < 1e-11
    else:                   # W^T g = y
        want = torch.linalg.solve(W.T, y.T).T
        got = lu_solve_reference(y, A, perm, None, mode=mode, transpose=True)
    assert (got - want).abs().max() <= 1e-11 * max(1.0, want.abs().max().item())
    assert torch.equal(lu_solve(y, A, perm, b, mode=mode, transpose=transpose), got)


def test_lower_mode_never_reads_the_upper_triangle():
    L, U, perm, b, x = recipe(5)
    A = packed(L, U, "lower")
    An = A + torch.triu(torch.full((5, 5), float("nan"), dtype=torch.float64), 1)
    for tr in (False, True):
        assert torch.equal(lu_solve_reference(x, An, perm, None, mode="lower", transpose=tr),
                           lu_solve_reference(x, A, perm, None, mode="lower", transpose=tr))


@pytest.mark.parametrize("mode", ["lu", "lower"])
@pytest.mark.parametrize("transpose", [False, True])
def test_custom_backward_gradcheck(mode, transpose):
    L, U, perm, b, _ = recipe(5, B=3)
    A = packed(L, U, mode).requires_grad_()
    y = torch.randn(3, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    y.requires_grad_()
    n0 = solve_launches()
    if transpose:
        f = lambda y, A: lu_solve(y, A, perm, None, mode=mode, transpose=True)
        assert torch.autograd.gradcheck(f, (y, A))
    else:
        b = b.clone().requires_grad_()
        f = lambda y, A, b: lu_solve(y, A, perm, b, mode=mode)
        assert torch.autograd.gradcheck(f, (y, A, b))
    out = f(*((y, A) if transpose else (y, A, b)))
    assert type(out.grad_fn).__name__.startswith("_LuSolveFn")   # the custom Function ran
    assert solve_launches() == n0                                # and never the kernel


def test_custom_backward_matches_autograd_of_composite():
    L, U, perm, b, x = recipe(33, B=7)
    for mode in ("lu", "lower"):
        leaves = [t.clone().requires_grad_() for t in (x, packed(L, U, mode), b)]
        ref = [t.clone().requires_grad_() for t in (x, packed(L, U, mode), b)]
        w = torch.randn(7, 33, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
        (lu_solve(leaves[0], leaves[1], perm, leaves[2], mode=mode) * w).sum().backward()
        (lu_solve_reference(ref[0], ref[1], perm, ref[2], mode=mode) * w).sum().backward()
        for a, r in zip(leaves, ref):
            assert (a.grad - r.grad).abs().max() <= 1e-11 * max(1.0, r.grad.abs().max().item())


def test_double_backward_raises():
    L, U, perm, b, x = recipe(5, B=3)
    y, A = x.clone().requires_grad_(), packed(L, U, "lu").requires_grad_()
    (gy,) = torch.autograd.grad(lu_solve(y, A, perm).sum(), y, create_graph=True)
    with pytest.raises(RuntimeError):
        gy.sum().backward()


def test_lu_linear_fresh_layer_is_its_permutation():
    f = LULinear(7, seed=3)
    z = torch.randn(11, 7, generator=torch.Generator().manual_seed(0))
    y, ldj = f(z)
    assert torch.equal(y, z[:, f.perm]) or torch.allclose(y, z[:, f.perm], atol=1e-6)
    assert ldj.shape == (11,) and ldj.dtype == torch.float32 and ldj.abs().max() < 1e-6
    assert torch.equal(LULinear(7, permute=False).perm, torch.arange(7))
    x, ldj_inv = f.inverse(y)
    assert torch.allclose(x, z, atol=1e-6) and ldj_inv.abs().max() < 1e-6


def _randomise(f, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in f.parameters():
            p.add_(0.3 * torch.randn(p.shape, generator=g))


def test_lu_linear_round_trip_logdet_and_state_dict():
    f = LULinear(9, seed=1).double()
    _randomise(f)
    z = torch.randn(13, 9, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    y, ldj = f(z)
    x, ldj_inv = f.inverse(y)
    assert (x - z).abs().max() < 1e-10
    W = f.weight()
    assert (y - (z @ W.T + f.bias)).abs().max() < 1e-12
    sign, logabs = torch.linalg.slogdet(W)
    assert ldj.dtype == torch.float32 and ldj.shape == (13,)
    assert abs(ldj[0].item() - logabs.item()) < 1e-5
    assert torch.allclose(ldj_inv, -ldj)
    g = LULinear(9, seed=5).double()
    assert set(f.state_dict()) == {"lower", "upper", "raw_diag", "bias", "perm"}
    g.load_state_dict(f.state_dict())
    y2, _ = g(z)
    assert torch.equal(y2, y) and torch.equal(g.inverse(y)[0], x)
    # the unused triangles get no gradient
    f.zero_grad()
    (f.inverse(y)[0].sum() + f(z)[0].sum()).backward()
    assert f.lower.grad.triu().abs().max() == 0 and f.upper.grad.tril().abs().max() == 0
    assert f.raw_diag.grad.abs().min() > 0


def test_triangular_affine():
    f = TriangularAffine(6).double()
    z = torch.randn(8, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    y0, l0 = f(z)
    assert (y0 - z).abs().max() < 1e-6 and l0.abs().max() < 1e-6   # raw_diag is stored in fp32
    _randomise(f)
    y, ldj = f(z)
    Lm = f.scale_tril()
    assert (y - (f.mu + z @ Lm.T)).abs().max() < 1e-12
    assert abs(ldj[0].item() - torch.linalg.slogdet(Lm)[1].item()) < 1e-5
    x, ldj_inv = f.inverse(y)
    assert (x - z).abs().max() < 1e-10 and torch.allclose(ldj_inv, -ldj)
    assert isinstance(build_flow("affine-full", 6, 1), TriangularAffine)


def test_neural_spline_flow_default_is_unchanged():
    torch.manual_seed(0)
    f = NeuralSplineFlow(6, n_layers=2)
    torch.manual_seed(0)
    g = NeuralSplineFlow(6, n_layers=2, linear=None)
    keys = list(f.state_dict())
    assert keys == list(g.state_dict()) and not any("linear" in k for k in keys)
    assert len(list(f.children())) == 1 and f.linears is None     # the couplings alone
    # recorded before the linear= option existed
    assert keys == [f"layers.{i}.net.{j}.{w}" for i in range(2) for j in (0, 2, 4)
                    for w in ("weight", "bias")]
    # the same parameters in the same order as a stack of the couplings built by hand, and the
    # same outputs
    from vi_normflows_amd.flows.spline import RQSCoupling

    torch.manual_seed(0)
    hand = [RQSCoupling(6, 8, 3.0, 256, 2, parity=i % 2, context_dim=0) for i in range(2)]
    x = torch.linspace(-2, 2, 12).view(2, 6)
    y, ldj = f(x)
    assert (y - x).abs().max() < 1e-6 and ldj.abs().max() < 1e-5   # as recorded: the identity
    yh, lh = x, torch.zeros(2)
    for c in hand:
        yh, l = c(yh, None)
        lh = lh + l
    assert torch.equal(y, yh) and torch.equal(ldj, lh)
    for (k, v), c in zip(f.state_dict().items(),
                         [t for h in hand for t in h.state_dict().values()]):
        assert torch.equal(v, c), k


def test_neural_spline_flow_with_lu_layers():
    torch.manual_seed(0)
    f = NeuralSplineFlow(6, n_layers=2, hidden=32, linear="lu")
    assert len(f.linears) == 2 and all(isinstance(l, LULinear) for l in f.linears)
    assert any(k.startswith("linears.0.") for k in f.state_dict())
    _randomise(f.linears[0]), _randomise(f.linears[1], 1)
    x = torch.randn(16, 6, generator=torch.Generator().manual_seed(1))
    y, ldj = f(x)
    xr, ldj_inv = f.inverse(y)
    assert (xr - x).abs().max() < 1e-4 and (ldj + ldj_inv).abs().max() < 1e-4
    assert build_flow("nsf", 6, 2, hidden=32, linear="lu").linears is not None
    assert build_flow("nsf", 6, 2, hidden=32).linears is None
    with pytest.raises(ValueError):
        NeuralSplineFlow(6, n_layers=2, linear="qr")


def test_full_rank_normal_matches_torch():
    q = FullRankNormal(5).double()
    z = torch.randn(9, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    std = torch.distributions.MultivariateNormal(torch.zeros(5, dtype=torch.float64),
                                                 scale_tril=torch.eye(5, dtype=torch.float64))
    assert (q.log_prob(z) - std.log_prob(z)).abs().max() < 1e-6     # starts at N(0, I)
    _randomise(q)
    ref = torch.distributions.MultivariateNormal(q.mean, scale_tril=q.scale_tril)
    assert (q.log_prob(z) - ref.log_prob(z)).abs().max() < 1e-10
    assert abs(q.entropy().item() - ref.entropy().item()) < 1e-10
    assert (q.covariance - ref.covariance_matrix).abs().max() < 1e-12
    s, lp = q.rsample_with_log_prob(7, torch.Generator().manual_seed(1))
    assert s.shape == (7, 5) and (lp - q.log_prob(s)).abs().max() < 1e-10
    (q.log_prob(s.detach()).sum() + s.sum()).backward()
    assert all(p.grad is not None for p in q.parameters())


def test_full_rank_bbvi_recovers_a_correlated_gaussian():
    g = torch.Generator().manual_seed(7)
    Am = torch.randn(4, 4, generator=g, dtype=torch.float64)
    cov = Am @ Am.T + 0.1 * torch.eye(4, dtype=torch.float64)
    mean = torch.tensor([1.0, -2.0, 0.5, 3.0], dtype=torch.float64)
    target = torch.distributions.MultivariateNormal(mean, covariance_matrix=cov)
    res = black_box_vi_full_rank(target.log_prob, 4, num_samples=500, iters=3000, lr=0.05, seed=0)
    cov_err = ((res.cov - cov).abs().max() / cov.abs().max()).item()
    mean_err = (res.mean - mean).abs().max().item()
    print(f"full-rank BBVI: cov_err {cov_err:.4f} mean_err {mean_err:.4f}")
    assert cov_err <= 0.2 and mean_err <= 0.1
    assert torch.equal(res.scale_tril, torch.tril(res.scale_tril)) and res.trace[-1][0] == 2999
    # what the full-rank family buys: the optimal mean-field sds are far too narrow here
    ratio = (1 / torch.sqrt(torch.diag(torch.linalg.inv(cov)))) / torch.sqrt(torch.diag(cov))
    print("mean-field / true marginal sd:", [round(r, 3) for r in ratio.tolist()])
    assert (ratio < 0.75).all()
