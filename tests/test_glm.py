"""GLM posteriors on the CPU: the composite of ops/reference.py behind ops/glm.py, the targets of
distributions/posteriors.py and their hooks in get_target and score_fn."""
import math

import pytest
import torch

from vi_normflows_amd.distributions.energies import TARGETS, Target, get_target
from vi_normflows_amd.distributions.posteriors import (bayes_glm, make_glm_data,
                                                       minibatch_log_prob)
from vi_normflows_amd.inference.bbvi import linreg_log_joint, linreg_posterior
from vi_normflows_amd.inference.svgd import score_fn
from vi_normflows_amd.ops import glm
from vi_normflows_amd.ops.reference import glm_logp_grad_reference

FAMILIES = ("bernoulli", "poisson", "gaussian")


def _data(family, B, N, D, seed=0, dtype=torch.float64):
    X, y, _ = make_glm_data(family, N, D, seed)
    g = torch.Generator().manual_seed(seed + 1)
    theta = 0.5 * torch.randn(B, D, generator=g, dtype=torch.float64) / math.sqrt(D)
    return theta.to(dtype), X.to(dtype), y.to(dtype)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("prior", [2.0, "vector", None])
def test_gradcheck(family, prior):
    theta, X, y = _data(family, 3, 7, 4)
    if prior == "vector":
        prior = torch.tensor([0.5, 1.0, 0.0, 3.0], dtype=torch.float64)
    theta.requires_grad_(True)
    assert torch.autograd.gradcheck(
        lambda t: glm.glm_log_prob(t, X, y, family, prior, 0.7, 1.5, const=0.25), (theta,))


def test_log_prob_is_once_differentiable_in_theta_only():
    theta, X, y = _data("bernoulli", 3, 7, 4)
    theta.requires_grad_(True)
    lp = glm.glm_log_prob(theta, X, y)
    (g,) = torch.autograd.grad(lp.sum(), theta, create_graph=True)
    assert torch.equal(g, glm.glm_logp_grad(theta, X, y)[1])
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g.sum(), theta)
    for bad in ({"X": X.clone().requires_grad_(True)}, {"y": y.clone().requires_grad_(True)},
                {"prior_prec": torch.ones(4, dtype=torch.float64, requires_grad=True)}):
        kw = {"X": X, "y": y, **bad}
        with pytest.raises(RuntimeError, match=next(iter(bad))):
            glm.glm_log_prob(theta, **kw)


@pytest.mark.parametrize("prior_var,noise_var", [(1.0, 1.0), (4.0, 0.5)])
def test_gaussian_family_is_the_linear_regression_closed_form(prior_var, noise_var):
    N, D = 50, 3
    X, y, _ = make_glm_data("gaussian", N, D, 3, noise_var=noise_var)
    X, y = X.double(), y.double()
    tgt = bayes_glm(X, y, "gaussian", prior_var, noise_var)
    assert tgt.dim == D and tgt.logZ is None
    g = torch.Generator().manual_seed(4)
    W = torch.randn(11, D, generator=g, dtype=torch.float64)
    want = linreg_log_joint(X, y, prior_var * torch.eye(D, dtype=torch.float64), noise_var)(W)
    got = tgt.log_prob(W)
    assert got.dtype == torch.float64
    assert ((got - want).abs() <= 1e-12 * want.abs()).all()
    mu, _ = linreg_posterior(X, y, prior_var * torch.eye(D, dtype=torch.float64), noise_var)
    s = tgt.score(mu[None])
    assert s.abs().max() <= 1e-9 * (X.T @ y).abs().max() / noise_var


def test_bernoulli_is_finite_at_huge_eta():
    X = torch.tensor([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [1.0, 1.0]], dtype=torch.float32)
    y = torch.tensor([1.0, 1.0, 0.0, 0.0])
    theta = torch.tensor([[1e4, -1e4], [-1e4, 1e4], [1e4, 1e4]])
    logp, grad = glm.glm_logp_grad(theta, X, y, "bernoulli", 1e-8)
    ref_lp, ref_g = glm_logp_grad_reference(theta.double(), X.double(), y.double(), "bernoulli",
                                            1e-8)
    assert torch.isfinite(logp).all() and torch.isfinite(grad).all()
    assert torch.allclose(logp.double(), ref_lp, rtol=1e-6, atol=0)
    assert torch.allclose(grad.double(), ref_g, rtol=1e-6, atol=1e-6)
    # eta = (1e4, -1e4, -1e4, 0) for the first row: rows 2 and 4 cost 1e4 and log 2, row 3 nothing
    assert abs(ref_lp[0].item() - (-1e4 - math.log(2) - 0.5 * 1e-8 * 2e8
                                   + math.log(1e-8) - math.log(2 * math.pi))) < 1e-6


@pytest.mark.parametrize("family", FAMILIES)
def test_minibatches_average_to_the_full_density(family):
    N, D, parts = 60, 3, 4
    X, y, _ = make_glm_data(family, N, D, 5)
    tgt = bayes_glm(X.double(), y.double(), family, 2.0, 0.8)
    W = 0.3 * torch.randn(5, D, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    full = tgt.log_prob(W)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(7))
    for split in ([slice(k * N // parts, (k + 1) * N // parts) for k in range(parts)],
                  list(perm.reshape(parts, -1))):
        mean = sum(minibatch_log_prob(tgt, idx)(W) for idx in split) / parts
        assert ((mean - full).abs() <= 1e-12 * full.abs()).all()
    with pytest.raises(ValueError, match="not a GLM target"):
        minibatch_log_prob(get_target("U1"), slice(0, 3))


def test_score_fn_prefers_the_targets_own_score():
    tgt = get_target("logreg", dim=3, n=200, seed=1)
    assert tgt.dim == 3 and tgt.meta["theta_true"].shape == (3,) and tgt.score is not None
    assert score_fn(tgt) == tgt.score
    z = 0.3 * torch.randn(9, 3, generator=torch.Generator().manual_seed(2))
    s = score_fn(tgt)(z)
    zz = z.clone().requires_grad_(True)
    (want,) = torch.autograd.grad(tgt.log_prob(zz).sum(), zz)
    assert not s.requires_grad and torch.equal(s, want)
    # a target without a score takes the autograd branch, as before
    u1 = get_target("U1")
    assert u1.score is None and Target("t", 2, u1.fn).score is None
    z2 = torch.randn(9, 2, generator=torch.Generator().manual_seed(3))
    zz = z2.clone().requires_grad_(True)
    (want,) = torch.autograd.grad(u1.fn(zz).sum(), zz)
    assert score_fn(u1) is not u1.score and torch.equal(score_fn(u1)(z2), want)


def test_get_target_builds_seeded_glm_targets_outside_the_target_list():
    for name, family in (("logreg", "bernoulli"), ("poisreg", "poisson"), ("linreg", "gaussian")):
        assert name not in TARGETS
        a, b = get_target(name, dim=4, n=50, seed=3), get_target(name, dim=4, n=50, seed=3)
        data = a.meta["glm"]
        assert a.name == name and a.dim == 4 and data.family == family and data.n == 50
        assert torch.equal(data.X, b.meta["glm"].X) and torch.equal(data.y, b.meta["glm"].y)
        assert not torch.equal(data.y, get_target(name, dim=4, n=50, seed=4).meta["glm"].y)
        assert (data.X[:, 0] == 1).all()
        z = torch.zeros(2, 4)
        assert torch.isfinite(a.log_prob(z)).all() and a.log_prob(z).shape == (2,)


def test_constants_and_flat_coordinates():
    theta, X, y = _data("poisson", 4, 9, 3)
    base, _ = glm.glm_logp_grad(theta, X, y, "poisson", None)
    want = (torch.distributions.Poisson(torch.exp(theta @ X.T)).log_prob(y[None])).sum(1)
    got = base + glm.likelihood_const(y, "poisson")
    assert torch.allclose(got, want, rtol=1e-12, atol=0)
    # a coordinate with precision 0 is flat: no quadratic term and no normaliser for it
    prec = torch.tensor([2.0, 0.0, 0.5], dtype=torch.float64)
    lp, g = glm.glm_logp_grad(theta, X, y, "poisson", prec)
    on = torch.tensor([0, 2])
    prior = torch.distributions.Normal(0.0, prec[on] ** -0.5).log_prob(theta[:, on]).sum(1)
    assert torch.allclose(lp, base + prior, rtol=1e-12, atol=0)
    assert torch.equal(g[:, 1], glm.glm_logp_grad(theta, X, y, "poisson", None)[1][:, 1])


def test_argument_errors():
    theta, X, y = _data("bernoulli", 3, 7, 4)
    with pytest.raises(ValueError, match="family"):
        glm.glm_logp_grad(theta, X, y, "probit")
    with pytest.raises(ValueError, match="y must have"):
        glm.glm_logp_grad(theta, X, y[:-1])
    with pytest.raises(ValueError, match="scale"):
        glm.glm_logp_grad(theta, X, y, scale=0.0)
    with pytest.raises(ValueError, match="noise_var"):
        glm.glm_logp_grad(theta, X, y, "gaussian", noise_var=-1.0)
    with pytest.raises(ValueError, match="prior_prec"):
        glm.glm_logp_grad(theta, X, y, prior_prec=-1.0)
    with pytest.raises(RuntimeError, match="impl='kernel'"):
        glm.glm_logp_grad(theta, X, y, impl="kernel")
    assert glm.TILE_B >= 1 and glm.TILE_N >= 1 and not glm.kernel_supported(theta, X, y)
