"""Laplace approximations: the MAP by a damped Newton iteration and the Gaussian around it.

For a posterior ``p`` with mode ``theta*`` and ``H = -d^2 log p / d theta^2`` there,

    p ~ N(theta*, H^-1),    log Z ~ log p(theta*) + D/2 log 2 pi - 1/2 log det H

is the classic baseline the variational fits and HMC are read against: exact for the Gaussian
family (``linreg``), an approximation for the other links. :func:`newton_map` runs ``B`` Newton
iterations side by side (multi-start); every iteration takes the Newton statistics ``(log p, grad,
H)`` of all rows from one call. A GLM target (``distributions/posteriors.py``) answers that call
with one launch of ``csrc/kernels/glm_hess.hip`` for fp32 GPU rows with D <= 64 and with the torch
composite elsewhere; any other :class:`Target` goes through ``torch.func.hessian`` of its ``fn``.
The ``B`` solves of size ``D x D`` are not the hot path: they run in fp64 on the host.

A :class:`LaplaceResult` turns into a ``FullRankNormal`` (:meth:`LaplaceResult.distribution`, to
sample from or to start ``black_box_vi_full_rank(init=...)``) and into the diagonal inverse mass of
``HMC(minv=...)`` (:meth:`LaplaceResult.minv`).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from ..distributions.energies import Target, get_target

LOG2PI = math.log(2 * math.pi)


def newton_stats(target: Target):
    """``theta [B, D] -> (logp [B], grad [B, D], H [B, D, D])`` of a target, ``H`` the negative
    Hessian of ``logp``: ``target.hessian`` where it is set (the fused pass of a GLM target), else
    autograd through ``target.fn``."""
    if target.hessian is not None:
        return target.hessian
    if target.fn is None:
        raise ValueError(f"laplace: target {target.name!r} has neither a hessian nor an fn to "
                         "differentiate")
    fn = target.fn

    def one(t):
        return fn(t[None])[0]

    def stats(theta):
        theta = theta.detach()
        with torch.enable_grad():
            t = theta.clone().requires_grad_(True)
            lp = fn(t)
            (g,) = torch.autograd.grad(lp.sum(), t)
        H = torch.func.vmap(torch.func.hessian(one))(theta)
        return lp.detach(), g.detach(), -H.detach()
    return stats


def _solve(H, g):
    """``(H^-1 g, g . H^-1 g)`` per row in fp64 on the host; a row whose ``H`` is not positive
    definite (a flat prior on separable data, a non-concave target) gets the smallest ridge
    ``10^k tr(H) / D`` that makes it so."""
    H64, g64 = H.detach().double().cpu(), g.detach().double().cpu()
    D = H64.shape[-1]
    L, info = torch.linalg.cholesky_ex(H64)
    bad = (info > 0) | ~torch.isfinite(H64).all(-1).all(-1)
    if bool(bad.any()):
        Hb = torch.nan_to_num(H64[bad], nan=0.0, posinf=0.0, neginf=0.0)
        Hb = 0.5 * (Hb + Hb.mT)
        ridge = Hb.diagonal(dim1=-2, dim2=-1).abs().mean(-1).clamp_min(1.0) * 1e-8
        eye = torch.eye(D, dtype=torch.float64)
        for _ in range(40):
            Lb, ib = torch.linalg.cholesky_ex(Hb + ridge[:, None, None] * eye)
            if not bool((ib > 0).any()):
                break
            ridge = torch.where(ib > 0, 10.0 * ridge, ridge)
        else:
            raise RuntimeError("newton_map: no ridge makes the negative Hessian positive definite")
        L[bad] = Lb
    delta = torch.cholesky_solve(g64[:, :, None], L)[:, :, 0]
    return delta, (g64 * delta).sum(1)


@dataclass
class NewtonResult:
    theta: torch.Tensor       # [B, D], on the device and in the dtype of theta0
    logp: torch.Tensor        # [B]
    grad: torch.Tensor        # [B, D]
    H: torch.Tensor           # [B, D, D], the negative Hessian of logp at theta
    n_iter: torch.Tensor      # [B] int64 (host): Newton steps taken
    converged: torch.Tensor   # [B] bool (host)
    n_evals: int = 0          # calls of the Newton statistics: 1 + iterations + backtracks
    n_backtracks: int = 0     # of which line-search retries


@torch.no_grad()
def newton_map(target, theta0, max_iter: int = 50, xtol: float | None = None,
               ftol: float | None = None, armijo: float = 1e-4, max_backtracks: int = 30,
               callback=None) -> NewtonResult:
    """Maximise ``log p`` from the ``B`` starts ``theta0`` [B, D] by Newton's method with
    backtracking. ``target`` is a :class:`Target` or a callable ``theta -> (logp, grad, H)``.

    One iteration solves ``H delta = grad`` per row and tries ``theta + t delta`` with ``t = 1,
    1/2, ...`` until ``logp`` rises by ``armijo t grad . delta`` (undamped Newton diverges for the
    Poisson link from poor starts); every trial is one call of the statistics for all rows, and the
    accepted trial's statistics are the next iteration's, so an iteration without backtracking
    costs exactly one call. A row is converged once its step is small, ``|delta_c| <= xtol (1 +
    |theta_c|)`` for every c, or its Newton decrement ``grad . delta / 2``, the rise of ``logp``
    the quadratic model still promises, is at most ``ftol (1 + |logp|)``: below that Armijo would
    be judged on the rounding noise of ``logp`` and a step-only rule would never stop. Such a row
    takes that last full step unchecked and is frozen: later iterations do not move it. Defaults:
    ``xtol = sqrt(eps)`` and ``ftol = 4 eps`` of the dtype of ``theta0``. A row whose line search
    fails stops where it is with ``converged = False``.

    ``callback(it, theta, logp, active)`` is called after every iteration."""
    stats = newton_stats(target) if isinstance(target, Target) else target
    if theta0.dim() != 2:
        raise ValueError(f"newton_map: theta0 must be [B, D], got {tuple(theta0.shape)}")
    if isinstance(target, Target) and target.dim != theta0.shape[1]:
        raise ValueError(f"newton_map: the target has dim {target.dim}, theta0 has D = "
                         f"{theta0.shape[1]}")
    if max_iter < 1 or max_backtracks < 0:
        raise ValueError("newton_map: need max_iter >= 1 and max_backtracks >= 0")
    eps = torch.finfo(theta0.dtype).eps
    xtol = math.sqrt(eps) if xtol is None else float(xtol)
    ftol = 4.0 * eps if ftol is None else float(ftol)
    theta = theta0.detach().clone()
    B = theta.shape[0]
    dev, dt = theta.device, theta.dtype

    def to_dev(t):
        return t.to(device=dev, dtype=dt)

    lp, g, H = stats(theta)
    n_evals, n_back = 1, 0
    active = torch.ones(B, dtype=torch.bool)
    converged = torch.zeros(B, dtype=torch.bool)
    n_iter = torch.zeros(B, dtype=torch.int64)
    for it in range(max_iter):
        delta, dec = _solve(H, g)
        lp64, th64 = lp.double().cpu(), theta.double().cpu()
        small = ((delta.abs() <= xtol * (1 + th64.abs())).all(1)
                 | (0.5 * dec <= ftol * (1 + lp64.abs())))
        last = active & small               # the last, unchecked step of these rows
        pending = active & ~small           # rows whose step goes through the line search
        t = torch.where(active, 1.0, 0.0).double()
        delta = torch.where(active[:, None], delta, torch.zeros_like(delta))
        for bt in range(max_backtracks + 1):
            trial = theta + to_dev(t[:, None] * delta)
            lp_t, g_t, H_t = stats(trial)
            n_evals += 1
            ok = lp_t.double().cpu() >= lp64 + armijo * t * dec   # False for nan
            ok &= torch.isfinite(g_t).all(1).cpu() & torch.isfinite(H_t).all(-1).all(-1).cpu()
            pending &= ~ok
            if bt == max_backtracks or not bool(pending.any()):
                break
            n_back += 1
            t = torch.where(pending, 0.5 * t, t)   # accepted rows keep their trial point
        failed = pending                           # the search is over: these stay where they are
        moved = active & ~failed
        sel = to_dev(moved.double()).bool()
        theta = torch.where(sel[:, None], trial, theta)
        lp = torch.where(sel, lp_t, lp)
        g = torch.where(sel[:, None], g_t, g)
        H = torch.where(sel[:, None, None], H_t, H)
        n_iter += moved.long()
        converged |= last
        active = active & ~last & ~failed
        if callback:
            callback(it, theta, lp, active)
        if not bool(active.any()):
            break
    return NewtonResult(theta, lp, g, H, n_iter, converged, n_evals, n_back)


@dataclass
class LaplaceResult:
    """N(mode, precision^-1) around the best of the starts; everything fp64 on the host."""
    mode: torch.Tensor          # [D]
    precision: torch.Tensor     # [D, D], the negative Hessian of log p at the mode
    covariance: torch.Tensor    # [D, D]
    scale_tril: torch.Tensor    # [D, D], the Cholesky factor of the covariance
    logp: float                 # log p(mode), with the target's likelihood constants
    log_evidence: float         # logp + D/2 log 2 pi - 1/2 log det precision
    n_iter: torch.Tensor        # [n_starts]
    converged: torch.Tensor     # [n_starts]
    newton: NewtonResult | None = None
    target: Target | None = None

    @property
    def mean(self):
        return self.mode

    def distribution(self):
        """The approximation as a ``FullRankNormal`` (fp32 parameters on the host): ``mean``,
        ``lower`` and ``raw_diag`` reproduce N(mode, covariance), ``raw_diag`` through the inverse
        of ``positive_diag``. Raises if a diagonal entry of the factor is at or below
        ``DIAG_FLOOR``, which that parametrisation cannot reach."""
        from ..distributions.base import FullRankNormal
        from ..flows.linear import DIAG_FLOOR

        d = torch.diagonal(self.scale_tril)
        if not bool((d > DIAG_FLOOR).all()):
            raise ValueError(f"LaplaceResult.distribution: the scale factor has a diagonal entry "
                             f"of {float(d.min()):.3g}, FullRankNormal needs more than "
                             f"{DIAG_FLOOR}")
        raw = torch.log(torch.expm1(d - DIAG_FLOOR))
        return FullRankNormal(self.mode.numel(), mean=self.mode,
                              lower=torch.tril(self.scale_tril, -1), raw_diag=raw)

    def minv(self):
        """The diagonal of the covariance [D]: the inverse diagonal mass for ``HMC(minv=...)``."""
        return torch.diagonal(self.covariance).clone()


def laplace(target: Target, theta0=None, n_starts: int = 1, init_std: float = 0.1, seed: int = 0,
            device="cpu", dtype=torch.float32, **newton_kw) -> LaplaceResult:
    """The Laplace approximation of ``target``: :func:`newton_map` from ``theta0`` [B, D] (or
    from ``n_starts`` starts: zero, then ``init_std N(0, I)`` draws of ``seed``, on ``device`` in
    ``dtype``), then the Gaussian around the start with the highest ``log p`` among the converged
    ones (among all, if none converged)."""
    if theta0 is None:
        if n_starts < 1:
            raise ValueError(f"laplace: n_starts must be >= 1, got {n_starts}")
        g = torch.Generator().manual_seed(seed)
        theta0 = init_std * torch.randn(n_starts, target.dim, generator=g, dtype=torch.float64)
        theta0[0] = 0.0
        theta0 = theta0.to(device=device, dtype=dtype)
    else:
        theta0 = torch.as_tensor(theta0)
        if theta0.dim() == 1:
            theta0 = theta0[None]
    if theta0.dim() != 2 or theta0.shape[1] != target.dim:
        raise ValueError(f"laplace: theta0 must be [B, {target.dim}] for target {target.name!r}, "
                         f"got {tuple(theta0.shape)}")
    res = newton_map(target, theta0, **newton_kw)
    lp = res.logp.double().cpu()
    lp = torch.where(torch.isfinite(lp), lp, torch.full_like(lp, -math.inf))
    pick = lp if not bool(res.converged.any()) else \
        torch.where(res.converged, lp, torch.full_like(lp, -math.inf))
    b = int(pick.argmax())
    mode = res.theta[b].double().cpu()
    prec = res.H[b].double().cpu()
    prec = 0.5 * (prec + prec.T)
    Lp = torch.linalg.cholesky(prec)
    cov = torch.cholesky_inverse(Lp)
    cov = 0.5 * (cov + cov.T)
    D = mode.numel()
    logdet = 2.0 * torch.log(torch.diagonal(Lp)).sum()
    log_ev = float(lp[b]) + 0.5 * D * LOG2PI - 0.5 * float(logdet)
    return LaplaceResult(mode, prec, cov, torch.linalg.cholesky(cov), float(lp[b]), log_ev,
                         res.n_iter, res.converged, res, target)


def fit_laplace(target="logreg", n_starts: int = 1, device="cpu", seed: int = 0,
                dtype=torch.float32, init=None, init_std: float = 0.1, **kw) -> LaplaceResult:
    """:func:`laplace` of ``target`` (a :class:`Target` or a name :func:`get_target` knows, with
    its keywords such as ``dim``, ``n``, ``seed`` of the data in ``kw``; the keywords of
    :func:`newton_map` go there). Starts at ``init`` [B, D] or at ``n_starts`` seeded starts."""
    newton_names = ("max_iter", "xtol", "ftol", "armijo", "max_backtracks", "callback")
    newton_kw = {k: kw.pop(k) for k in newton_names if k in kw}
    if isinstance(target, str):
        kw.setdefault("seed", seed)
        tgt = get_target(target, **kw)
    else:
        tgt = target
    theta0 = None if init is None else torch.as_tensor(init).to(device=device, dtype=dtype)
    return laplace(tgt, theta0, n_starts, init_std, seed, device, dtype, **newton_kw)
