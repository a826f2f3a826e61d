"""Leapfrog trajectories and the Metropolis accept step of Hamiltonian Monte Carlo.

One leapfrog step of size ``eps`` under the diagonal inverse mass ``minv`` is, with ``h = eps / 2``,

    p     = p + h g                 half kick
    theta = theta + eps minv p      drift
    (lp, g) = log p, score at theta
    p     = p + h g                 half kick

and the two half kicks of consecutive steps are deliberately not merged, so a trajectory of L steps
is the same arithmetic as L trajectories of one step. After L steps

    kin(p) = 0.5 sum_c minv_c p_c^2
    dH     = (kin(p_L) - kin(p_0)) + (logp_0 - lp_L)
    accept = isfinite(dH) and log_u < -dH

:func:`leapfrog_reference` is the torch composite for any ``logp_grad`` callable, on any device and
in any dtype. :func:`glm_hmc_step` is one HMC iteration on a GLM posterior (``ops/glm.py``): fp32
GPU chains with D <= 64 can run the whole trajectory and the accept step in one launch of
``csrc/kernels/glm_hmc.hip`` (``impl="kernel"``, opt-in); ``impl="stepwise"`` is the composite over
:func:`glm.glm_logp_grad`, one likelihood launch per leapfrog step, and what ``impl="auto"`` takes:
below 65536 chains: it measured faster at every sampler shape (docs/PERF_NOTES.md, "HMC
trajectory"). A chain's result from the
kernel is bitwise repeatable and does not depend on the other chains, on its place among them or
on the row tile.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import glm, reference
from ._ext import native
from .reference import GLM_FAMILIES

MAX_DIM = glm.MAX_DIM
MAX_LEAPFROG = 1024
ROW_TILES = (32, 64, 128)   # chains per workgroup the kernel is built for

HMCStep = namedtuple("HMCStep", "theta logp grad accept dH theta_prop p_prop")

_hmc_launches = 0


def hmc_launches(reset: bool = False) -> int:
    """Number of trajectory-kernel launches so far (evidence that the HIP path ran)."""
    global _hmc_launches
    n = _hmc_launches
    if reset:
        _hmc_launches = 0
    return n


def _eps_col(eps, theta):
    """``eps`` (a float or a [B] tensor) as something that multiplies [B, D] row-wise."""
    if isinstance(eps, torch.Tensor):
        eps = eps.to(device=theta.device, dtype=theta.dtype)
        if eps.dim() == 1:
            if eps.shape[0] != theta.shape[0]:
                raise ValueError(f"hmc: eps has {eps.shape[0]} entries, there are "
                                 f"{theta.shape[0]} chains")
            return eps[:, None]
        if eps.dim() != 0:
            raise ValueError(f"hmc: eps must be a float or a [B] tensor, got {tuple(eps.shape)}")
    return eps


def _minv_row(minv, theta):
    if minv is None:
        return None
    minv = torch.as_tensor(minv).to(device=theta.device, dtype=theta.dtype)
    if minv.shape != (theta.shape[1],):
        raise ValueError(f"hmc: minv must be [{theta.shape[1]}], got {tuple(minv.shape)}")
    return minv


def _check_L(L):
    if int(L) != L or L < 1:
        raise ValueError(f"hmc: the number of leapfrog steps must be an integer >= 1, got {L}")
    return int(L)


@torch.no_grad()
def leapfrog_reference(theta, p, logp_grad, eps, L: int, minv=None, grad=None):
    """``L`` leapfrog steps from ``(theta, p)`` [B, D]: returns ``(theta_L, p_L, logp_L,
    grad_L)``. ``logp_grad(theta) -> (logp [B], grad [B, D])``; ``eps`` is a float or a ``[B]``
    tensor of per-chain step sizes; ``minv`` a ``[D]`` inverse diagonal mass or ``None`` for the
    identity; ``grad`` the score at ``theta`` if the caller has it (else one more call)."""
    L = _check_L(L)
    if theta.dim() != 2 or p.shape != theta.shape:
        raise ValueError(f"hmc: theta and p must both be [B, D], got {tuple(theta.shape)} and "
                         f"{tuple(p.shape)}")
    e, mi = _eps_col(eps, theta), _minv_row(minv, theta)
    h = 0.5 * e
    drift = e if mi is None else e * mi
    lp = None
    g = logp_grad(theta)[1] if grad is None else grad
    for _ in range(L):
        p = p + h * g
        theta = theta + drift * p
        lp, g = logp_grad(theta)
        p = p + h * g
    return theta, p, lp, g


def kinetic(p, minv=None):
    """``0.5 sum_c minv_c p_c^2`` per chain."""
    return 0.5 * ((p * p).sum(1) if minv is None else (minv * p * p).sum(1))


def accept_rule(logp0, logp1, p0, p1, log_u, minv=None):
    """``(accept [B] bool, dH [B])`` of the Metropolis step: ``dH = (kin_1 - kin_0) + (logp_0 -
    logp_1)``, accepted where ``dH`` is finite and ``log_u < -dH``."""
    dH = (kinetic(p1, minv) - kinetic(p0, minv)) + (logp0 - logp1)
    return torch.isfinite(dH) & (log_u < -dH), dH


def metropolis(theta, logp, grad, p, log_u, theta1, p1, logp1, grad1, minv=None) -> HMCStep:
    """The accept step in torch: the proposal where accepted, the inputs (unchanged) elsewhere."""
    acc, dH = accept_rule(logp, logp1, p, p1, log_u, minv)
    a = acc[:, None]
    return HMCStep(torch.where(a, theta1, theta), torch.where(acc, logp1, logp),
                   torch.where(a, grad1, grad), acc.to(theta.dtype), dH, theta1, p1)


def kernel_supported(theta, X, y) -> bool:
    """fp32 GPU tensors inside the trajectory kernel's limits (those of the GLM kernel)."""
    return glm.kernel_supported(theta, X, y)


def _use_kernel(theta, X, y, L, impl):
    if impl not in ("auto", "kernel", "stepwise"):
        raise ValueError(f"hmc: impl must be auto, kernel or stepwise, got {impl!r}")
    ok = kernel_supported(theta, X, y) and L <= MAX_LEAPFROG
    if impl == "kernel" and not ok:
        raise RuntimeError(f"hmc: impl='kernel' needs fp32 GPU theta, X and y with 1 <= D <= "
                           f"{MAX_DIM} and L <= {MAX_LEAPFROG}; got theta {theta.dtype} on "
                           f"{theta.device}, X {X.dtype} on {X.device}, y {y.dtype} on "
                           f"{y.device} with D = {theta.shape[1]}, L = {L}")
    return impl == "kernel" or (impl == "auto" and ok and auto_takes_kernel(
        theta.shape[0], X.shape[0], theta.shape[1], L))


def auto_takes_kernel(B: int, N: int, D: int, L: int) -> bool:
    """Where ``impl="auto"`` takes the fused trajectory kernel: where it measured faster than the
    stepwise path on one MI355X (bench/hmc_bench.py; the table is in docs/PERF_NOTES.md under
    "HMC trajectory"). Over the whole sampler grid, (256 .. 16384 chains) x (1024, 16384 data
    rows) x (D = 8, 16, 64) x (L = 4, 16, 64), stepwise was 1.2x - 40x faster: without a split
    over N the fused grid is B / rows workgroups of one sequential row loop each, too few waves to
    hide that loop's latency, while the stepwise path splits N across the card. The fused kernel
    was ahead (1.10x) only once the chains alone fill the card: B = 262144 at D = 8 and 16, B =
    65536 at D = 64. That is the rule; everywhere else the kernel is opt-in
    (``impl="kernel"``)."""
    return B >= 262144 or (D > 32 and B >= 65536)


@torch.no_grad()
def glm_hmc_step(theta, logp, grad, p, log_u, eps, L: int, X, y, family: str = "bernoulli",
                 prior_prec=1.0, noise_var: float = 1.0, scale: float = 1.0, minv=None,
                 impl: str = "auto", rows=None) -> HMCStep:
    """One HMC iteration of the chains ``theta`` [B, D] on the GLM posterior of ``ops/glm.py``:
    ``L`` leapfrog steps from ``(theta, p)`` and the accept step against ``log_u`` [B].

    ``logp`` [B] and ``grad`` [B, D] are the (const-free) log-density and score at ``theta``,
    ``eps`` a float or ``[B]`` step sizes, ``minv`` a ``[D]`` inverse mass or ``None``. Returns
    :class:`HMCStep` ``(theta, logp, grad, accept, dH, theta_prop, p_prop)``: the state after the
    accept step (bitwise the inputs where rejected), ``accept`` as 0 / 1 in the dtype of
    ``theta``, and the end of the trajectory. ``impl="kernel"`` raises outside the kernel's
    limits; ``"stepwise"`` runs anywhere; ``rows`` overrides the kernel's chains per workgroup
    (one of :data:`ROW_TILES`; the result does not depend on it)."""
    global _hmc_launches
    L = _check_L(L)
    if family not in GLM_FAMILIES:
        raise ValueError(f"hmc: family must be one of {sorted(GLM_FAMILIES)}, got {family!r}")
    if theta.dim() != 2 or X.dim() != 2 or X.shape[1] != theta.shape[1]:
        raise ValueError(f"hmc: theta must be [B, D] and X [N, D], got {tuple(theta.shape)} and "
                         f"{tuple(X.shape)}")
    B, D = theta.shape
    if y.dim() != 1 or y.shape[0] != X.shape[0]:
        raise ValueError(f"hmc: y must have one entry per row of X ([{X.shape[0]}]), got "
                         f"{tuple(y.shape)}")
    if p.shape != (B, D) or grad.shape != (B, D):
        raise ValueError(f"hmc: p and grad must be [{B}, {D}] like theta, got {tuple(p.shape)} "
                         f"and {tuple(grad.shape)}")
    if logp.shape != (B,) or log_u.shape != (B,):
        raise ValueError(f"hmc: logp and log_u must be [{B}], got {tuple(logp.shape)} and "
                         f"{tuple(log_u.shape)}")
    if not float(scale) > 0 or not float(noise_var) > 0:
        raise ValueError(f"hmc: scale and noise_var must be positive, got {scale} and "
                         f"{noise_var}")
    if rows not in (None, 0) and rows not in ROW_TILES:
        raise ValueError(f"hmc: rows must be None or one of {ROW_TILES}, got {rows}")
    mi = _minv_row(minv, theta)
    e = _eps_col(eps, theta)   # validates the shape
    if not _use_kernel(theta, X, y, L, impl):
        def logp_grad(t):
            return glm.glm_logp_grad(t, X, y, family, prior_prec, noise_var, scale)
        th1, p1, lp1, g1 = leapfrog_reference(theta, p, logp_grad, eps, L, mi, grad=grad)
        return metropolis(theta, logp, grad, p, log_u, th1, p1, lp1, g1, mi)

    theta, X, y = glm._rows(theta.detach()), glm._rows(X.detach()), y.detach().contiguous()
    dev = theta.device
    if isinstance(e, torch.Tensor) and e.dim() == 2:
        eps_dev = e[:, 0].contiguous()
    else:
        eps_dev = torch.full((B,), float(e), device=dev, dtype=torch.float32)
    prec_dev, prec_host = None, 0.0
    if isinstance(prior_prec, torch.Tensor):
        prec_dev = reference.glm_prior_prec(prior_prec, theta).contiguous()
    elif prior_prec is not None:
        if not float(prior_prec) >= 0:
            raise ValueError(f"hmc: prior_prec must be >= 0, got {prior_prec}")
        prec_host = float(prior_prec)

    def new(*shape):
        return torch.empty(*shape, device=dev, dtype=torch.float32)
    out = [new(B, D), new(B, D), new(B, D), new(B), new(B, D), new(B), new(B)]
    native().glm_hmc_trajectory(
        theta, p.contiguous(), logp.contiguous(), grad.contiguous(), eps_dev,
        None if mi is None else mi.contiguous(), log_u.contiguous(), L, X, y, prec_dev, prec_host,
        prior_prec is not None, GLM_FAMILIES[family], 1.0 / float(noise_var), float(scale),
        int(rows or 0), *out)
    _hmc_launches += 1
    theta_prop, p_prop, theta_out, logp_out, grad_out, accept, dH = out
    return HMCStep(theta_out, logp_out, grad_out, accept, dH, theta_prop, p_prop)


def kernel_rows(B: int, D: int, rows: int = 0) -> int:
    """Chains per workgroup the launcher takes for ``(B, D)`` (``rows=0``) or the validated
    override."""
    return native().glm_hmc_rows(B, D, rows)
