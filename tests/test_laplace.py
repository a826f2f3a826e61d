"""Laplace approximations on the CPU: the Hessian composite against autograd, Newton's method on
the three GLM families in fp64, the closed form of the Gaussian family and the wiring
(inference/laplace.py, ops/reference.py glm_hessian_reference)."""
import math

import pytest
import torch

from vi_normflows_amd.distributions.energies import Target, get_target
from vi_normflows_amd.distributions.posteriors import bayes_glm, make_glm_data
from vi_normflows_amd.flows.linear import DIAG_FLOOR
from vi_normflows_amd.inference.bbvi import black_box_vi_full_rank, linreg_posterior
from vi_normflows_amd.inference.laplace import (LaplaceResult, fit_laplace, laplace, newton_map,
                                                newton_stats)
from vi_normflows_amd.ops import glm
from vi_normflows_amd.ops.reference import (glm_hessian_reference, glm_logp_grad_reference,
                                            glm_prior_prec, glm_terms_reference)

FAMILIES = ("bernoulli", "poisson", "gaussian")


def _prior(kind, D):
    if kind == "vector":   # one flat coordinate
        p = 0.5 + 1.5 * torch.rand(D, generator=torch.Generator().manual_seed(D),
                                   dtype=torch.float64)
        p[D // 2] = 0.0
        return p
    return 0.8 if kind == "scalar" else None


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("prior", ("scalar", "vector", None))
def test_reference_against_autograd(family, prior):
    B, N, D = 3, 50, 4
    g = torch.Generator().manual_seed(7)
    theta = 0.5 * torch.randn(B, D, generator=g, dtype=torch.float64)
    X = torch.randn(N, D, generator=g, dtype=torch.float64)
    y = torch.randint(0, 2 if family == "bernoulli" else 5, (N,), generator=g).double()
    p, nv, scale = _prior(prior, D), 0.7, 3.5
    lp, gr, H, A, G, W = glm_hessian_reference(theta, X, y, family, p, nv, scale, return_abs=True)
    lp0, gr0, A0, G0 = glm_logp_grad_reference(theta, X, y, family, p, nv, scale, return_abs=True)
    assert ((lp - lp0).abs() <= 1e-12 * A0).all() and ((gr - gr0).abs() <= 1e-12 * G0).all()
    assert torch.equal(A, A0) and torch.equal(G, G0)
    prec = glm_prior_prec(p, theta)

    def score(t):   # the reference's score of one row, on the graph (the reference detaches)
        r = glm_terms_reference(y, X @ t, family, nv)[1]
        return scale * (r @ X) - (prec * t if prec is not None else 0.0)
    for b in range(B):
        assert (score(theta[b]) - gr[b]).abs().max() <= 1e-12 * G[b].max()
        J = torch.autograd.functional.jacobian(score, theta[b])
        err = (H[b] + J).abs()
        print(f"{family} {prior} row {b}: max |H + d score| / W = {(err / W[b]).max():.2e}")
        assert (err <= 1e-10 * W[b]).all()
    plain = glm_hessian_reference(theta, X, y, family, p, nv, scale, chunk=2)
    assert len(plain) == 3 and torch.allclose(plain[2], H, rtol=1e-13, atol=0)
    assert H.dtype == torch.float64
    assert glm_hessian_reference(theta.float(), X, y, family, p, nv, scale)[2].dtype == torch.float32


def test_linreg_closed_form():
    tgt = get_target("linreg", dim=8, n=500)
    d = tgt.meta["glm"]
    X, y = d.X.double(), d.y.double()
    mu, cov = linreg_posterior(X, y, torch.eye(8, dtype=torch.float64), d.noise_var)
    S = d.noise_var * torch.eye(500, dtype=torch.float64) + X @ X.T
    log_marginal = float(torch.distributions.MultivariateNormal(
        torch.zeros(500, dtype=torch.float64), S).log_prob(y))
    g = torch.Generator().manual_seed(1)
    for theta0 in (torch.zeros(1, 8, dtype=torch.float64),
                   5.0 * torch.randn(4, 8, generator=g, dtype=torch.float64)):
        res = laplace(tgt, theta0)
        assert res.converged.all() and (res.n_iter <= 3).all()
        assert (res.mode - mu).abs().max() <= 1e-9 * mu.abs().max()
        assert (res.covariance - cov).abs().max() <= 1e-9 * cov.abs().max()
        assert abs(res.log_evidence - log_marginal) <= 1e-9 * abs(log_marginal)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n,d", [(200, 3), (500, 8), (1000, 40), (300, 64)])
def test_newton_convergence_fp64(family, n, d):
    X, y, _ = make_glm_data(family, n, d, seed=11)
    tgt = bayes_glm(X.double(), y.double(), family, 1.0, 0.7)
    g = torch.Generator().manual_seed(0)
    theta0 = torch.cat([torch.zeros(1, d), 2 * torch.randn(7, d, generator=g) / d ** 0.5]).double()
    seen = []
    res = newton_map(tgt, theta0, max_iter=25,
                     callback=lambda it, th, lp, act: seen.append((th.clone(), act.clone())))
    spread = (res.theta - res.theta[0]).abs().max().item()
    print(f"{family} n={n} d={d}: iterations {res.n_iter.tolist()}, max |grad| "
          f"{res.grad.abs().max():.2e}, spread {spread:.2e}, {res.n_backtracks} backtracks")
    assert res.converged.all() and (res.n_iter <= 25).all()
    assert res.grad.abs().max() <= 1e-6 and spread <= 1e-7
    assert res.n_evals == 1 + len(seen) + res.n_backtracks
    # the statistics that come back are those of the point that comes back
    lp, gr, H = tgt.hessian(res.theta)
    assert torch.equal(lp, res.logp) and torch.equal(gr, res.grad) and torch.equal(H, res.H)
    # a row that has stopped does not move afterwards
    for (th_a, act_a), (th_b, _) in zip(seen[:-1], seen[1:]):
        assert torch.equal(th_a[~act_a], th_b[~act_a])
    assert len(set(res.n_iter.tolist())) > 1 or family == "gaussian"
    for b in range(8):
        assert torch.equal(seen[int(res.n_iter[b]) - 1][0][b], res.theta[b])


def test_distribution_and_minv():
    res = fit_laplace("logreg", dim=8, n=500, seed=11, dtype=torch.float64)
    assert isinstance(res, LaplaceResult) and res.converged.all()
    assert res.mode.shape == (8,) and res.precision.shape == (8, 8)
    assert torch.allclose(res.covariance @ res.precision, torch.eye(8, dtype=torch.float64),
                          atol=1e-10)
    D = 8
    expect = res.logp + 0.5 * D * math.log(2 * math.pi) - 0.5 * float(torch.logdet(res.precision))
    assert abs(res.log_evidence - expect) <= 1e-10 * abs(expect)
    q = res.distribution()
    L = q.scale_tril.detach().double()
    eps32 = torch.finfo(torch.float32).eps
    # L is the fp64 factor rounded to fp32 (the diagonal through softplus and back): each entry
    # of L L^T carries a few roundings of its D terms
    bound = 8 * eps32 * (L.abs() @ L.abs().T)
    assert ((L @ L.T - res.covariance).abs() <= bound).all()
    assert torch.equal(q.mean.detach(), res.mode.float())
    lp_mode = float(q.log_prob(res.mode.float()[None]).detach())
    want = -0.5 * float(torch.logdet(2 * math.pi * res.covariance))
    terms = 0.5 * D * math.log(2 * math.pi) + float(torch.log(torch.diagonal(L)).abs().sum())
    assert abs(lp_mode - want) <= 64 * eps32 * terms   # fp32 log and sum of 2 D terms
    assert torch.equal(res.minv(), torch.diagonal(res.covariance)) and (res.minv() > 0).all()
    tiny = LaplaceResult(res.mode, res.precision * 1e8, res.covariance * 1e-8,
                         res.scale_tril * 1e-4, 0.0, 0.0, res.n_iter, res.converged)
    assert torch.diagonal(tiny.scale_tril).min() <= DIAG_FLOOR
    with pytest.raises(ValueError, match="diagonal entry"):
        tiny.distribution()


def test_full_rank_vi_starts_from_the_laplace_fit():
    res = fit_laplace("logreg", dim=3, n=200, seed=11, dtype=torch.float64)
    tgt = res.target
    seen = []
    black_box_vi_full_rank(tgt.log_prob, 3, num_samples=8, iters=1, lr=1e-3, init=res,
                           callback=lambda t, lb, m, L: seen.append((m.clone(), L.clone())))
    m, L = seen[0]
    assert torch.allclose(m, res.mode, atol=2e-3) and torch.allclose(L, res.scale_tril, atol=2e-3)
    for init in (res, res.distribution()):
        fit = black_box_vi_full_rank(tgt.log_prob, 3, num_samples=8, iters=0, init=init)
        assert torch.allclose(fit.mean, res.mode, atol=1e-6)
        assert torch.allclose(fit.scale_tril, res.scale_tril, atol=1e-6)
    with pytest.raises(ValueError, match="not both"):
        black_box_vi_full_rank(tgt.log_prob, 3, iters=0, init=res, init_mean=torch.zeros(3))
    with pytest.raises(ValueError, match=r"init must have mean \[4\]"):
        black_box_vi_full_rank(tgt.log_prob, 4, iters=0, init=res)


def test_multi_start_picks_the_best_mode():
    # two Gaussian bumps of different height: the starts find both, laplace returns the higher
    def fn(z):
        a = -0.5 * ((z - 2.0) ** 2).sum(1) / 0.25
        b = -0.5 * ((z + 2.0) ** 2).sum(1) / 0.25 - 1.0
        return torch.logaddexp(a, b)
    tgt = Target("bumps", 2, fn)
    theta0 = torch.tensor([[-1.5, -1.5], [1.5, 1.5]], dtype=torch.float64)
    res = laplace(tgt, theta0)
    assert res.converged.all()
    assert torch.allclose(res.newton.theta, torch.tensor([[-2.0, -2.0], [2.0, 2.0]],
                                                         dtype=torch.float64), atol=1e-6)
    assert torch.allclose(res.mode, torch.full((2,), 2.0, dtype=torch.float64), atol=1e-6)
    assert torch.allclose(res.covariance, 0.25 * torch.eye(2, dtype=torch.float64), atol=1e-6)


def test_fallback_through_autograd():
    tgt = get_target("U1")
    assert tgt.hessian is None and tgt.dim == 2
    z = torch.tensor([[1.9, 0.1], [-2.1, 0.3]], dtype=torch.float64)
    lp, g, H = newton_stats(tgt)(z)
    assert torch.allclose(lp, tgt.fn(z))
    for b in range(2):
        Hb = torch.autograd.functional.hessian(lambda t: tgt.fn(t[None])[0], z[b])
        assert torch.allclose(H[b], -Hb, rtol=1e-12, atol=1e-12)
    # a 2-D Gaussian through the same fallback: the Laplace approximation is exact
    P = torch.tensor([[2.0, 0.6], [0.6, 1.0]], dtype=torch.float64)
    m = torch.tensor([0.5, -1.0], dtype=torch.float64)
    gauss = Target("gauss2", 2, lambda t: -0.5 * (((t - m) @ P) * (t - m)).sum(1))
    res = laplace(gauss, z)
    assert res.converged.all() and (res.n_iter <= 3).all()
    assert torch.allclose(res.mode, m, atol=1e-12) and torch.allclose(res.precision, P, atol=1e-12)
    want = math.log(2 * math.pi) - 0.5 * float(torch.logdet(P))   # log of the integral
    assert abs(res.log_evidence - want) <= 1e-12


def test_errors():
    tgt = get_target("logreg", dim=3, n=50)
    with pytest.raises(ValueError, match="neither a hessian nor an fn"):
        laplace(Target("empty", 2, None), torch.zeros(1, 2))
    with pytest.raises(ValueError, match=r"theta0 must be \[B, 3\]"):
        laplace(tgt, torch.zeros(2, 4))
    with pytest.raises(ValueError, match="the target has dim 3"):
        newton_map(tgt, torch.zeros(2, 4))
    with pytest.raises(ValueError, match="n_starts"):
        laplace(tgt, n_starts=0)
    d = tgt.meta["glm"]
    with pytest.raises(RuntimeError, match="impl='kernel' needs fp32 GPU"):
        glm.glm_logp_grad_hess(torch.zeros(2, 3), d.X, d.y, impl="kernel")
    with pytest.raises(ValueError, match="impl must be"):
        glm.glm_logp_grad_hess(torch.zeros(2, 3), d.X, d.y, impl="fast")
    with pytest.raises(ValueError, match="theta must be"):
        glm.glm_logp_grad_hess(torch.zeros(2, 4), d.X, d.y)
    n0 = glm.glm_launches()
    lp, g, H = glm.glm_logp_grad_hess(torch.zeros(2, 3), d.X, d.y, const=1.5)
    ref = glm_hessian_reference(torch.zeros(2, 3), d.X, d.y)
    assert torch.equal(lp, ref[0] + 1.5) and torch.equal(g, ref[1]) and torch.equal(H, ref[2])
    assert glm.glm_launches() == n0
