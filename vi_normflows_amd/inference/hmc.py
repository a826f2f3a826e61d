"""Hamiltonian Monte Carlo: the reference sampler the variational fits are judged against.

Many chains run side by side (``[C, D]``); one iteration draws momenta ``p ~ N(0, M)`` with the
diagonal mass ``M = 1 / minv``, runs ``n_leapfrog`` leapfrog steps of a (jittered) per-chain step
size and accepts or rejects the end point (``ops/hmc.py`` has the arithmetic). ``(theta, logp,
grad)`` of the current state are kept, so an iteration costs ``n_leapfrog`` score evaluations.

A GLM posterior (``distributions/posteriors.py``) with fp32 GPU chains and D <= 64 runs the whole
iteration in one launch of ``csrc/kernels/glm_hmc.hip``; every other target goes through its
``log_prob`` and score with the torch composite.

Warm-up adapts the step size by dual averaging (Hoffman & Gelman 2014) on the mean over chains of
``min(1, exp(-dH))`` and can set the diagonal mass from the cross-chain variance; both are frozen
afterwards. :func:`split_rhat` and :func:`ess` are the usual convergence diagnostics, and
:func:`moment_gap` is what one reads to judge a variational posterior against the HMC one.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from ..distributions.energies import Target, get_target
from ..ops import glm
from ..ops import hmc as hmc_ops
from .svgd import score_fn


class HMC:
    """HMC on the chains ``theta0`` [C, D] (``self.theta`` after each :meth:`step`).

    ``target_or_fns`` is a :class:`Target`, a callable ``theta -> (logp [C], grad [C, D])`` or a
    pair ``(log_prob, score)`` of callables. ``minv`` is the ``[D]`` inverse diagonal mass (``None``:
    identity), ``jitter`` in [0, 1) spreads the per-chain step size uniformly over ``step_size (1
    +- jitter)``, ``generator`` (on the device of the chains) makes the run repeatable. ``impl``
    and ``rows`` go to :func:`ops.hmc.glm_hmc_step` for GLM targets."""

    def __init__(self, target_or_fns, theta0, step_size: float, n_leapfrog: int, minv=None,
                 jitter: float = 0.0, generator=None, impl: str = "auto", rows=None):
        if theta0.dim() != 2:
            raise ValueError(f"HMC: theta0 must be [C, D], got {tuple(theta0.shape)}")
        if not float(step_size) > 0:
            raise ValueError(f"HMC: step_size must be positive, got {step_size}")
        if int(n_leapfrog) != n_leapfrog or n_leapfrog < 1:
            raise ValueError(f"HMC: n_leapfrog must be an integer >= 1, got {n_leapfrog}")
        if not 0.0 <= float(jitter) < 1.0:
            raise ValueError(f"HMC: jitter must be in [0, 1), got {jitter}")
        if impl not in ("auto", "kernel", "stepwise"):
            raise ValueError(f"HMC: impl must be auto, kernel or stepwise, got {impl!r}")
        self.theta = theta0.detach().clone()
        self.step_size, self.n_leapfrog, self.jitter = float(step_size), int(n_leapfrog), float(jitter)
        self.generator, self.impl, self.rows = generator, impl, rows
        self.minv = None
        self.target = target_or_fns if isinstance(target_or_fns, Target) else None
        self._glm = self.target.meta.get("glm") if self.target is not None else None
        if self.target is not None and self.target.dim != theta0.shape[1]:
            raise ValueError(f"HMC: the target has dim {self.target.dim}, theta0 has D = "
                             f"{theta0.shape[1]}")
        if self._glm is not None:
            d = self._glm
            X, y, prec = d.on(self.theta)
            self._glm_args = dict(X=X, y=y, family=d.family, prior_prec=prec,
                                  noise_var=d.noise_var)
            self.const = d.const
            self._logp_grad = lambda t: glm.glm_logp_grad(t, X, y, d.family, prec, d.noise_var)
        else:
            self.const = 0.0
            if self.target is not None:
                lp_fn, sc_fn = self.target.log_prob, score_fn(self.target)
            elif callable(target_or_fns):
                lp_fn = sc_fn = None
                self._logp_grad = target_or_fns
            else:
                try:
                    lp_fn, sc_fn = target_or_fns
                except (TypeError, ValueError):
                    raise ValueError("HMC: target_or_fns must be a Target, a callable theta -> "
                                     "(logp, grad) or a pair (log_prob, score)") from None
            if lp_fn is not None:
                def logp_grad(t):
                    with torch.no_grad():
                        return lp_fn(t).detach(), sc_fn(t)
                self._logp_grad = logp_grad
        self.set_minv(minv)
        with torch.no_grad():
            self._logp, self.grad = self._logp_grad(self.theta)
        self.steps, self.last = 0, None

    @property
    def logp(self):
        """The log-density of the current states (with the target's constant)."""
        return self._logp + self.const if self.const else self._logp

    def set_minv(self, minv):
        if minv is None:
            self.minv = None
            return
        minv = torch.as_tensor(minv).detach().to(device=self.theta.device, dtype=self.theta.dtype)
        if minv.shape != (self.theta.shape[1],) or not bool((minv > 0).all()):
            raise ValueError(f"HMC: minv must be a positive [{self.theta.shape[1]}] tensor")
        self.minv = minv.contiguous()

    def _rand(self, *shape, normal=False):
        f = torch.randn if normal else torch.rand
        return f(*shape, generator=self.generator, device=self.theta.device,
                 dtype=self.theta.dtype)

    @torch.no_grad()
    def step(self):
        """One iteration; returns the :class:`ops.hmc.HMCStep` (also kept as ``self.last``)."""
        C, D = self.theta.shape
        p = self._rand(C, D, normal=True)
        if self.minv is not None:
            p = p / self.minv.sqrt()
        log_u = torch.log(self._rand(C))
        eps = torch.full((C,), self.step_size, device=self.theta.device, dtype=self.theta.dtype)
        if self.jitter:
            eps = eps * (1.0 + self.jitter * (2.0 * self._rand(C) - 1.0))
        if self._glm is not None:
            r = hmc_ops.glm_hmc_step(self.theta, self._logp, self.grad, p, log_u, eps,
                                     self.n_leapfrog, minv=self.minv, impl=self.impl,
                                     rows=self.rows, **self._glm_args)
        else:
            th1, p1, lp1, g1 = hmc_ops.leapfrog_reference(self.theta, p, self._logp_grad, eps,
                                                          self.n_leapfrog, self.minv,
                                                          grad=self.grad)
            r = hmc_ops.metropolis(self.theta, self._logp, self.grad, p, log_u, th1, p1, lp1, g1,
                                   self.minv)
        self.theta, self._logp, self.grad, self.last = r.theta, r.logp, r.grad, r
        self.steps += 1
        return r

    def accept_stat(self) -> float:
        """Mean over chains of ``min(1, exp(-dH))`` of the last iteration (0 where dH is not
        finite)."""
        dH = self.last.dH.double()
        a = torch.where(torch.isfinite(dH), torch.exp(-dH.clamp_min(0.0)), torch.zeros_like(dH))
        return float(a.mean())

    def warmup(self, n: int, target_accept: float = 0.8, adapt_mass: bool = False,
               gamma: float = 0.05, t0: float = 10.0, kappa: float = 0.75):
        """``n`` iterations of dual-averaging step-size adaptation towards the mean acceptance
        ``target_accept``; the averaged step size is kept and frozen at the end. With
        ``adapt_mass`` the first half ends by setting ``minv`` to the cross-chain variance of the
        states, and the step size is adapted afresh in the second half."""
        if not 0.0 < target_accept < 1.0:
            raise ValueError(f"HMC: target_accept must be in (0, 1), got {target_accept}")
        if adapt_mass and self.theta.shape[0] < 2:
            raise ValueError("HMC: adapt_mass needs at least two chains")
        windows = [n // 2, n - n // 2] if adapt_mass else [n]
        for w, m_win in enumerate(windows):
            mu, hbar, log_bar = math.log(10.0 * self.step_size), 0.0, 0.0
            for m in range(1, m_win + 1):
                self.step()
                hbar = (1.0 - 1.0 / (m + t0)) * hbar + (target_accept - self.accept_stat()) / (m + t0)
                log_eps = mu - math.sqrt(m) / gamma * hbar
                eta = m ** -kappa
                log_bar = eta * log_eps + (1.0 - eta) * log_bar
                self.step_size = math.exp(log_eps)
            if m_win:
                self.step_size = math.exp(log_bar)
            if adapt_mass and w == 0 and m_win:
                self.set_minv(self.theta.double().var(0).clamp_min(1e-12).to(self.theta.dtype))
        return self.step_size


def _chains(samples, who):
    s = torch.as_tensor(samples).detach().double().cpu()
    if s.dim() == 2:
        s = s[:, :, None]
    if s.dim() != 3:
        raise ValueError(f"{who}: samples must be [S, C, D], got {tuple(s.shape)}")
    if s.shape[0] < 4:
        raise ValueError(f"{who}: needs at least 4 draws per chain, got S = {s.shape[0]}")
    return s


def split_rhat(samples):
    """Split-R-hat per coordinate of ``samples`` [S, C, D] (fp64): every chain is cut into its
    first and last ``S // 2`` draws, and ``sqrt(((n - 1) / n W + B / n) / W)`` compares the
    variance between the 2C half-chains with the variance within them. Raises if a half-chain is
    constant."""
    s = _chains(samples, "split_rhat")
    S = s.shape[0]
    n = S // 2
    halves = torch.cat([s[:n], s[S - n:]], dim=1)            # [n, 2C, D]
    W = halves.var(0, unbiased=True).mean(0)
    if bool((W <= 0).any()):
        raise ValueError("split_rhat: constant chains (zero within-chain variance)")
    Bn = halves.mean(0).var(0, unbiased=True)                # B / n
    return torch.sqrt(((n - 1) / n * W + Bn) / W)


def ess(samples):
    """Effective sample size per coordinate of ``samples`` [S, C, D] (fp64): ``C S / tau`` with
    ``tau = -1 + 2 sum_k P_k``, ``P_k = rho(2k) + rho(2k + 1)`` summed over Geyer's initial
    positive sequence, and the multi-chain autocorrelation ``rho(t) = 1 - (W - mean_c acov_c(t))
    / var+`` from FFT autocovariances. Raises on constant chains."""
    s = _chains(samples, "ess")
    S, C, D = s.shape
    x = s - s.mean(0, keepdim=True)
    f = torch.fft.rfft(x, n=2 * S, dim=0)
    acov = torch.fft.irfft(f * f.conj(), n=2 * S, dim=0)[:S] / S        # [S, C, D], biased
    W = (acov[0] * S / (S - 1)).mean(0)
    if bool((W <= 0).any()):
        raise ValueError("ess: constant chains (zero within-chain variance)")
    var_plus = W * (S - 1) / S
    if C > 1:
        var_plus = var_plus + s.mean(0).var(0, unbiased=True)
    rho = 1.0 - (W - acov.mean(1)) / var_plus                           # [S, D]
    K = S // 2
    P = rho[0:2 * K:2] + rho[1:2 * K:2]                                 # [K, D]
    keep = torch.cumprod((P > 0).to(torch.float64), dim=0)
    tau = -1.0 + 2.0 * (P * keep).sum(0)
    return C * S / tau


def moment_gap(samples_a, samples_b):
    """``(|mean_a - mean_b| / std_b, std_a / std_b)`` per coordinate of two sample sets
    ``[..., D]`` (fp64): how far set ``a`` (say a flow's samples) is from set ``b`` (the HMC
    draws) in units of the reference's posterior standard deviation."""
    a = torch.as_tensor(samples_a).detach().double().cpu()
    b = torch.as_tensor(samples_b).detach().double().cpu()
    if a.dim() < 2 or b.dim() < 2 or a.shape[-1] != b.shape[-1]:
        raise ValueError(f"moment_gap: need two sample sets [..., D] of one D, got "
                         f"{tuple(a.shape)} and {tuple(b.shape)}")
    a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    if a.shape[0] < 2 or b.shape[0] < 2:
        raise ValueError("moment_gap: each set needs at least two samples")
    sb = b.std(0)
    return (a.mean(0) - b.mean(0)).abs() / sb, a.std(0) / sb


@dataclass
class HMCResult:
    samples: torch.Tensor      # [S, C, D]
    accept_rate: float
    step_size: float
    minv: torch.Tensor | None
    rhat: torch.Tensor         # [D]
    ess: torch.Tensor          # [D]
    target: Target | None = None


def fit_hmc(target="logreg", n_chains: int = 256, n_samples: int = 500, warmup: int = 500,
            n_leapfrog: int = 16, device="cpu", seed: int = 0, init=None, step_size: float = 0.1,
            target_accept: float = 0.8, adapt_mass: bool = False, jitter: float = 0.1,
            init_std: float = 0.1, dtype=torch.float32, impl: str = "auto",
            **target_kw) -> HMCResult:
    """Sample ``target`` (a :class:`Target` or a name :func:`get_target` knows, with
    ``target_kw``) with ``n_chains`` chains: ``warmup`` adapting iterations, then ``n_samples``
    kept ones. Chains start at ``init`` [n_chains, D] or at ``init_std N(0, I)``."""
    tgt = get_target(target, **target_kw) if isinstance(target, str) else target
    if n_samples < 4:
        raise ValueError(f"fit_hmc: n_samples must be >= 4 (for the diagnostics), got {n_samples}")
    g = torch.Generator(device=device).manual_seed(seed)
    if init is None:
        theta0 = init_std * torch.randn(n_chains, tgt.dim, generator=g, device=device, dtype=dtype)
    else:
        theta0 = torch.as_tensor(init).to(device=device, dtype=dtype)
        if theta0.shape != (n_chains, tgt.dim):
            raise ValueError(f"fit_hmc: init must be [{n_chains}, {tgt.dim}], got "
                             f"{tuple(theta0.shape)}")
    sampler = HMC(tgt, theta0, step_size, n_leapfrog, jitter=jitter, generator=g, impl=impl)
    sampler.warmup(warmup, target_accept, adapt_mass)
    samples = torch.empty(n_samples, n_chains, tgt.dim, device=device, dtype=dtype)
    acc = torch.zeros((), device=device, dtype=torch.float64)
    for t in range(n_samples):
        r = sampler.step()
        samples[t] = r.theta
        acc += r.accept.double().mean()
    return HMCResult(samples, float(acc) / n_samples, sampler.step_size, sampler.minv,
                     split_rhat(samples), ess(samples), tgt)
