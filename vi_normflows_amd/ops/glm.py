"""Log-density and score of generalised-linear-model posteriors over a batch of parameters.

For ``B`` parameter rows ``theta_i`` and ``N`` data rows ``(x_n, y_n)``, with ``eta_in = theta_i .
x_n``

    logp_i = scale sum_n ll(y_n, eta_in) + log prior(theta_i) + const
    grad_i = scale sum_n r(y_n, eta_in) x_n - prec theta_i

for ``family="bernoulli"`` (logit link: ``ll = y eta - softplus(eta)``, ``r = y - sigmoid(eta)``),
``"poisson"`` (log link: ``y eta - exp(eta)``, ``y - exp(eta)``) or ``"gaussian"`` (identity:
``-(y - eta)^2 / (2 noise_var)``, ``(y - eta) / noise_var``) and the prior ``N(0, diag(1 /
prior_prec))`` (a float, a ``[D]`` tensor, or ``None`` for a flat prior); definitions:
``ops/reference.py`` ``glm_logp_grad_reference``. ``const`` is whatever the caller wants added
once (the likelihood's theta-free terms, :func:`likelihood_const`); it never enters the sum.

fp32 GPU tensors with D <= 64 run the fused HIP pass of ``csrc/kernels/glm.hip``: the ``[B, N]``
matrix of ``eta`` is never stored, ``theta`` and ``X`` may be row-strided views (column slices,
row-offset minibatches), and the partial sums of ``n_splits`` ranges of data rows are added in
fixed order, so a result is bitwise repeatable for a given ``(B, N, D, n_splits)``;
``n_splits=None`` lets the launcher choose from ``(B, N, D)`` alone.

:func:`glm_logp_grad_hess` adds the curvature in the same pass: ``H_i = scale sum_n w(eta_in) x_n
x_n^T + diag(prec)``, the negative Hessian of ``logp_i`` (``csrc/kernels/glm_hess.hip``), what
Newton's method and the Laplace approximation of ``inference/laplace.py`` need.

:func:`glm_logp_grad` runs without grad. :func:`glm_log_prob` is differentiable in ``theta`` (once):
its backward is ``g[:, None] * grad`` from the same launch.
"""
from __future__ import annotations

import re
from pathlib import Path

import torch

from . import reference
from ._ext import native
from .reference import GLM_FAMILIES
from .reference import glm_likelihood_const as likelihood_const  # noqa: F401  (public here)

MAX_DIM = 64


def _tiles():
    """The kernel's tile sizes, read from the header the kernel is compiled with."""
    hdr = Path(__file__).resolve().parents[2] / "csrc" / "include" / "glm_tiles.h"
    vals = dict(re.findall(r"#define\s+NF_GLM_(TILE_[BN])\s+(\d+)", hdr.read_text()))
    return int(vals["TILE_B"]), int(vals["TILE_N"])


TILE_B, TILE_N = _tiles()

_glm_launches = 0


def glm_launches(reset: bool = False) -> int:
    """Number of GLM kernel launches so far (evidence that the HIP path ran)."""
    global _glm_launches
    n = _glm_launches
    if reset:
        _glm_launches = 0
    return n


def kernel_supported(theta, X, y) -> bool:
    """fp32 GPU tensors inside the kernel's limits."""
    return (theta.is_cuda and X.is_cuda and y.is_cuda
            and theta.dtype == X.dtype == y.dtype == torch.float32
            and theta.dim() == 2 and X.dim() == 2 and theta.shape[0] >= 1 and X.shape[0] >= 1
            and 1 <= theta.shape[1] <= MAX_DIM)


def _check(theta, X, y, family, prior_prec, noise_var, scale, impl):
    if family not in GLM_FAMILIES:
        raise ValueError(f"glm: family must be one of {sorted(GLM_FAMILIES)}, got {family!r}")
    if impl not in ("auto", "kernel", "composite"):
        raise ValueError(f"glm: impl must be auto, kernel or composite, got {impl!r}")
    if theta.dim() != 2 or X.dim() != 2 or X.shape[1] != theta.shape[1]:
        raise ValueError(f"glm: theta must be [B, D] and X [N, D], got {tuple(theta.shape)} and "
                         f"{tuple(X.shape)}")
    if y.dim() != 1 or y.shape[0] != X.shape[0]:
        raise ValueError(f"glm: y must have one entry per row of X ([{X.shape[0]}]), got "
                         f"{tuple(y.shape)}")
    if not float(scale) > 0:
        raise ValueError(f"glm: scale must be positive, got {scale}")
    if not float(noise_var) > 0:
        raise ValueError(f"glm: noise_var must be positive, got {noise_var}")
    if prior_prec is not None and not isinstance(prior_prec, torch.Tensor) \
            and not float(prior_prec) >= 0:
        raise ValueError(f"glm: prior_prec must be >= 0, got {prior_prec}")
    if impl == "kernel" and not kernel_supported(theta, X, y):
        raise RuntimeError(f"glm: impl='kernel' needs fp32 GPU theta, X and y with 1 <= D <= "
                           f"{MAX_DIM}; got theta {theta.dtype} on {theta.device}, X {X.dtype} "
                           f"on {X.device}, y {y.dtype} on {y.device} with D = {theta.shape[1]}")
    # auto: the kernel wherever it is supported. From (256, 512, 2) to (65536, 8192, 64) it
    # measured 3.7x - 8.8x faster than the composite on one MI355X (bench/glm_bench.py,
    # docs/PERF_NOTES.md "GLM likelihood"), so there is no crossover rule on (B, N, D), and none
    # could send a shape whose [B, N] logits pass 1 GiB back to the composite.
    return impl == "kernel" or (impl == "auto" and kernel_supported(theta, X, y))


def _rows(t):
    """Unit inner stride and a non-negative row stride, without a copy where the view has them."""
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < 0):
        return t.contiguous()
    return t


@torch.no_grad()
def glm_logp_grad(theta, X, y, family: str = "bernoulli", prior_prec=1.0, noise_var: float = 1.0,
                  scale: float = 1.0, impl: str = "auto", n_splits=None, const: float = 0.0):
    """``(logp [B], grad [B, D])`` of the parameter rows ``theta`` [B, D] on data ``X`` [N, D],
    ``y`` [N]; no-grad. ``impl="auto"`` takes the HIP kernel for fp32 GPU tensors with D <= 64
    and the torch composite otherwise; ``"kernel"`` raises outside those limits; ``"composite"``
    is the composite on any device and dtype. ``const`` is added to every ``logp``."""
    global _glm_launches
    if not _check(theta, X, y, family, prior_prec, noise_var, scale, impl):
        logp, grad = reference.glm_logp_grad_reference(theta, X, y, family, prior_prec, noise_var,
                                                       float(scale))
        return (logp + const if const else logp), grad
    theta, X, y = _rows(theta.detach()), _rows(X.detach()), y.detach().contiguous()
    B, D = theta.shape
    N = X.shape[0]
    prec_dev, prec_host = None, 0.0
    if isinstance(prior_prec, torch.Tensor):
        prec_dev = reference.glm_prior_prec(prior_prec, theta).contiguous()
    elif prior_prec is not None:
        prec_host = float(prior_prec)
    ops, ns = native(), int(n_splits or 0)
    logp = torch.empty(B, device=theta.device, dtype=torch.float32)
    grad = torch.empty(B, D, device=theta.device, dtype=torch.float32)
    work = torch.empty(ops.glm_workspace(B, N, D, ns), device=theta.device, dtype=torch.float32)
    ops.glm_logp_grad(theta, X, y, prec_dev, prec_host, prior_prec is not None,
                      GLM_FAMILIES[family], 1.0 / float(noise_var), float(scale), ns, logp, grad,
                      work)
    _glm_launches += 1
    if const:
        logp += const
    return logp, grad


class _GlmLogProb(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, X, y, family, prior_prec, noise_var, scale, impl, n_splits, const):
        logp, grad = glm_logp_grad(theta, X, y, family, prior_prec, noise_var, scale, impl,
                                   n_splits, const)
        ctx.save_for_backward(grad)
        return logp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (g[:, None] * grad,) + (None,) * 9


def glm_log_prob(theta, X, y, family: str = "bernoulli", prior_prec=1.0, noise_var: float = 1.0,
                 scale: float = 1.0, impl: str = "auto", n_splits=None, const: float = 0.0):
    """``logp`` [B] of :func:`glm_logp_grad`, differentiable in ``theta`` only and only once: the
    score of the same launch is kept for the backward. Raises if the data or the prior require
    grad."""
    for name, t in (("X", X), ("y", y), ("prior_prec", prior_prec)):
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise RuntimeError(f"glm_log_prob is differentiable in theta only: {name} requires "
                               "grad (detach it)")
    return _GlmLogProb.apply(theta, X, y, family, prior_prec, noise_var, scale, impl, n_splits,
                             const)


@torch.no_grad()
def glm_logp_grad_hess(theta, X, y, family: str = "bernoulli", prior_prec=1.0,
                       noise_var: float = 1.0, scale: float = 1.0, impl: str = "auto",
                       n_splits=None, const: float = 0.0):
    """The Newton statistics ``(logp [B], grad [B, D], H [B, D, D])`` of the parameter rows
    ``theta`` on data ``X`` [N, D], ``y`` [N] from one pass over the data; no-grad. ``H_b = scale
    sum_n w(theta_b . x_n) x_n x_n^T + diag(prior_prec)`` is the negative Hessian of ``logp_b``
    (``w``: ``ops/reference.py`` ``glm_weights_reference``). fp32 GPU tensors with D <= 64 run
    ``csrc/kernels/glm_hess.hip`` (``H`` exactly symmetric, bitwise repeatable for a given ``(B,
    N, D, n_splits)``, strided views as for :func:`glm_logp_grad`); ``impl`` and ``const`` as
    there. A kernel launch counts in :func:`glm_launches`."""
    global _glm_launches
    # auto: the kernel wherever it is supported; bench/glm_hess_bench.py against the composite is
    # in docs/PERF_NOTES.md "GLM Hessian"
    if not _check(theta, X, y, family, prior_prec, noise_var, scale, impl):
        logp, grad, H = reference.glm_hessian_reference(theta, X, y, family, prior_prec,
                                                        noise_var, float(scale))
        return (logp + const if const else logp), grad, H
    theta, X, y = _rows(theta.detach()), _rows(X.detach()), y.detach().contiguous()
    B, D = theta.shape
    N = X.shape[0]
    prec_dev, prec_host = None, 0.0
    if isinstance(prior_prec, torch.Tensor):
        prec_dev = reference.glm_prior_prec(prior_prec, theta).contiguous()
    elif prior_prec is not None:
        prec_host = float(prior_prec)
    ops, ns = native(), int(n_splits or 0)
    logp = torch.empty(B, device=theta.device, dtype=torch.float32)
    grad = torch.empty(B, D, device=theta.device, dtype=torch.float32)
    H = torch.empty(B, D, D, device=theta.device, dtype=torch.float32)
    work = torch.empty(ops.glm_hess_workspace(B, N, D, ns), device=theta.device,
                       dtype=torch.float32)
    ops.glm_logp_grad_hess(theta, X, y, prec_dev, prec_host, prior_prec is not None,
                           GLM_FAMILIES[family], 1.0 / float(noise_var), float(scale), ns, logp,
                           grad, H, work)
    _glm_launches += 1
    if const:
        logp += const
    return logp, grad, H
