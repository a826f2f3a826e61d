"""Bayesian generalised-linear-model posteriors as :class:`Target` objects.

``bayes_glm(X, y, family)`` is the posterior of the weights ``theta`` of

    y_n ~ Bernoulli(sigmoid(theta . x_n)) | Poisson(exp(theta . x_n)) | N(theta . x_n, noise_var)

under the prior ``theta ~ N(0, prior_var I)`` (or a per-coordinate ``prior_var`` [D]),
unnormalised in ``theta`` (``logZ = None``: the evidence) but with every likelihood constant in
place, so the Gaussian family is :func:`inference.bbvi.linreg_log_joint` by definition. The
density and its score come from ``ops/glm.py``: one fused HIP pass over the data for fp32 GPU
samples, the torch composite elsewhere (CPU, fp64, D > 64). ``Target.score`` is set, so SVGD and
KSD take the score from the same pass without building a graph.

Data are held as given and moved to (and cached on) the device and dtype of the samples.
"""
from __future__ import annotations

import torch

from ..ops import glm
from .energies import Target

FAMILY_NAMES = {"logreg": "bernoulli", "poisreg": "poisson", "linreg": "gaussian"}


class GLMData:
    """The data, prior and constants of one GLM posterior, with per-(device, dtype) copies."""

    def __init__(self, X, y, family: str, prior_var=1.0, noise_var: float = 1.0,
                 impl: str = "auto"):
        X, y = torch.as_tensor(X).detach(), torch.as_tensor(y).detach().reshape(-1)
        if X.dim() != 2 or y.shape[0] != X.shape[0]:
            raise ValueError(f"bayes_glm: X must be [N, D] and y [N], got {tuple(X.shape)} and "
                             f"{tuple(y.shape)}")
        if family not in glm.GLM_FAMILIES:
            raise ValueError(f"bayes_glm: family must be one of {sorted(glm.GLM_FAMILIES)}, got "
                             f"{family!r}")
        if not X.is_floating_point():
            X = X.to(torch.get_default_dtype())
        self.X, self.y = X, y.to(X.dtype)
        self.family, self.noise_var, self.impl = family, float(noise_var), impl
        if isinstance(prior_var, torch.Tensor):
            pv = prior_var.detach().double().reshape(-1)
            if pv.numel() not in (1, X.shape[1]) or not bool((pv > 0).all()):
                raise ValueError("bayes_glm: prior_var must be positive, a float or one per column")
            self.prec = float(1.0 / pv) if pv.numel() == 1 else 1.0 / pv
        else:
            if not float(prior_var) > 0:
                raise ValueError(f"bayes_glm: prior_var must be positive, got {prior_var}")
            self.prec = 1.0 / float(prior_var)
        self.const = glm.likelihood_const(self.y, family, self.noise_var)
        self._cache = {}

    @property
    def n(self) -> int:
        return self.X.shape[0]

    def on(self, z):
        """``(X, y, prec)`` on the device and in the dtype of ``z``."""
        key = (z.device, z.dtype)
        if key not in self._cache:
            prec = self.prec.to(device=z.device, dtype=z.dtype) \
                if isinstance(self.prec, torch.Tensor) else self.prec
            self._cache[key] = (self.X.to(device=z.device, dtype=z.dtype),
                                self.y.to(device=z.device, dtype=z.dtype), prec)
        return self._cache[key]

    def log_prob(self, z, rows=None):
        """The posterior density at ``z`` [B, D], differentiable in ``z``; on ``rows`` (a slice
        or an index tensor) the minibatch estimate: those rows' likelihood times ``N / len(rows)``
        and the prior once."""
        X, y, prec = self.on(z)
        scale, const = 1.0, self.const
        if rows is not None:
            if isinstance(rows, torch.Tensor):
                rows = rows.to(X.device)
            X, y = X[rows], y[rows]
            scale = self.n / X.shape[0]
            const = scale * glm.likelihood_const(y, self.family, self.noise_var)
        return glm.glm_log_prob(z, X, y, self.family, prec, self.noise_var, scale, self.impl,
                                const=const)

    def score(self, z):
        """``grad log p(z)`` [B, D], detached and without a graph."""
        X, y, prec = self.on(z)
        return glm.glm_logp_grad(z.detach(), X, y, self.family, prec, self.noise_var,
                                 impl=self.impl)[1]

    def hessian(self, z):
        """The Newton statistics ``(logp [B], grad [B, D], H [B, D, D])`` at ``z`` from one pass
        over the data, detached: ``logp`` with the likelihood constants, ``H`` the negative
        Hessian of ``logp`` (``ops/glm.py`` ``glm_logp_grad_hess``)."""
        X, y, prec = self.on(z)
        return glm.glm_logp_grad_hess(z.detach(), X, y, self.family, prec, self.noise_var,
                                      impl=self.impl, const=self.const)


def bayes_glm(X, y, family: str = "bernoulli", prior_var=1.0, noise_var: float = 1.0,
              name: str | None = None, impl: str = "auto") -> Target:
    """The posterior of GLM weights on data ``X`` [N, D], ``y`` [N] as a :class:`Target` with
    ``dim = D``. ``prior_var`` is a float or a ``[D]`` tensor; ``noise_var`` is used by the
    Gaussian family only; ``impl`` goes to ``ops/glm.py`` (``target.meta["glm"].impl`` changes
    it later)."""
    data = GLMData(X, y, family, prior_var, noise_var, impl)
    return Target(name or f"glm_{family}", data.X.shape[1], data.log_prob, logZ=None,
                  meta={"glm": data}, score=data.score, hessian=data.hessian)


def minibatch_log_prob(target: Target, idx):
    """``z -> log p`` of a GLM target estimated from the data rows ``idx`` (a slice or an index
    tensor): their likelihood terms times ``N / len(idx)`` plus the prior, counted once. Its
    expectation over uniformly drawn ``idx`` is ``target.log_prob``. A slice reaches the kernel
    as a row-offset view, without a copy."""
    data = target.meta.get("glm")
    if data is None:
        raise ValueError(f"minibatch_log_prob: {target.name} is not a GLM target")
    return lambda z: data.log_prob(z, idx)


def make_glm_data(family: str, n: int, d: int, seed: int = 0, intercept: bool = True,
                  noise_var: float = 1.0):
    """A seeded synthetic dataset ``(X [n, d], y [n], theta_true [d])`` in fp32: ``X ~ N(0, 1)``
    with a first column of ones if ``intercept``, ``theta_true ~ N(0, 1) / sqrt(d)`` (so the
    linear predictor is O(1)), and ``y`` drawn from the family at ``theta_true``."""
    if family not in glm.GLM_FAMILIES:
        raise ValueError(f"make_glm_data: family must be one of {sorted(glm.GLM_FAMILIES)}, got "
                         f"{family!r}")
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, d, generator=g)
    if intercept:
        X[:, 0] = 1.0
    theta = torch.randn(d, generator=g) / d ** 0.5
    eta = X @ theta
    if family == "bernoulli":
        y = torch.bernoulli(torch.sigmoid(eta), generator=g)
    elif family == "poisson":
        y = torch.poisson(torch.exp(eta), generator=g)
    else:
        y = eta + noise_var ** 0.5 * torch.randn(n, generator=g)
    return X, y, theta


def glm_target(name: str, dim: int | None = None, n: int = 1000, seed: int = 0,
               intercept: bool = True, prior_var=1.0, noise_var: float = 1.0) -> Target:
    """``get_target("logreg" | "poisreg" | "linreg", dim=d, n=..., seed=...)``: the posterior on
    a :func:`make_glm_data` dataset; ``meta["theta_true"]`` holds the generating weights."""
    family = FAMILY_NAMES[name]
    X, y, theta = make_glm_data(family, n, dim or 8, seed, intercept, noise_var)
    tgt = bayes_glm(X, y, family, prior_var, noise_var, name=name)
    tgt.meta["theta_true"] = theta
    return tgt
