"""Stein variational gradient descent (Liu & Wang 2016) and KSD diagnostics.

Particle-based, non-parametric VI next to the parametric flows: N particles move along

    phi(x_i) = (1/N) sum_j [ k(x_j, x_i) grad log p(x_j) + grad_{x_j} k(x_j, x_i) ],

the steepest-descent direction of KL(q || p) in the kernel's RKHS. The all-pairs pass runs in one
HIP kernel on the GPU (``ops/stein.py``), and for the 2-D reference targets the scores come from
the fused target kernel (``csrc/kernels/energy2d.hip``), so a step is three launches plus the
optimizer. The kernel Stein discrepancy (:func:`flow_ksd`, :meth:`SVGD.ksd`) measures how far a
set of samples is from an unnormalised target, which the free energy cannot say.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from ..distributions.energies import Target, get_target
from ..ops import stein
from .optimizers import make_optimizer


def score_fn(target: Target):
    """``z -> grad log p(z)`` [N, D] of a target, detached. fp32 GPU samples of a 2-D target with
    a ``kernel_kind`` take the fused target kernel; everything else autograd on ``target.fn``.
    A target that brings its own ``score`` (the GLM posteriors) is asked first."""
    if target.score is not None:
        return target.score

    def score(z):
        z = z.detach()
        if (target.fused and target.kernel_kind is not None and z.is_cuda
                and z.dtype == torch.float32 and z.dim() == 2 and z.shape[1] == 2):
            from ..ops import fused

            zc = z.contiguous()
            g = torch.empty_like(zc)
            fused.energy2d(target.kernel_kind, zc, grad=g)
            return g
        with torch.enable_grad():
            zz = z.clone().requires_grad_(True)
            (g,) = torch.autograd.grad(target.fn(zz).sum(), zz)
        return g
    return score


class SVGD:
    """SVGD on a set of particles [N, D] (updated in place; ``self.particles``).

    ``target_or_score`` is a :class:`Target` or a callable ``z -> grad log p(z)``; ``bandwidth``
    is ``"median"`` (the median heuristic, recomputed every step on the device) or a float;
    ``optimizer`` and ``opt_kw`` go to :func:`make_optimizer`."""

    def __init__(self, target_or_score, particles, lr: float, optimizer: str = "adam",
                 kernel: str = "rbf", bandwidth="median", **opt_kw):
        if isinstance(target_or_score, Target):
            self.target = target_or_score
            self.score = score_fn(target_or_score)
        else:
            self.target = None
            self.score = target_or_score
        if bandwidth != "median" and not float(bandwidth) > 0:
            raise ValueError(f"SVGD: bandwidth must be 'median' or a positive float, got "
                             f"{bandwidth!r}")
        self.particles = particles.detach()
        self.kernel = kernel
        self.bandwidth = bandwidth
        self.opt = make_optimizer(optimizer, [self.particles], lr, **opt_kw)
        self.steps = 0

    def _h(self, x):
        return stein.median_bandwidth(x) if self.bandwidth == "median" else float(self.bandwidth)

    @torch.no_grad()
    def direction(self):
        x = self.particles
        return stein.svgd_direction(x, self.score(x), self._h(x), kernel=self.kernel)

    @torch.no_grad()
    def step(self):
        """One update: ``particles.grad = -phi``, then the optimizer's step."""
        self.particles.grad = self.direction().neg_()
        self.opt.step()
        self.steps += 1

    @torch.no_grad()
    def ksd(self, kernel: str = "imq", h=1.0, stat: str = "u"):
        x = self.particles
        return stein.ksd(x, self.score(x), h, kernel, stat)


@dataclass
class SVGDResult:
    particles: torch.Tensor
    target: Target
    history: list


def fit_svgd(target="U1", n_particles: int = 1000, iters: int = 500, lr: float = 0.05,
             device="cpu", seed: int = 0, init_std: float = 1.0, log_every: int = 100,
             optimizer: str = "adam", kernel: str = "rbf", bandwidth="median",
             dtype=torch.float32, callback=None) -> SVGDResult:
    """SVGD from ``init_std * N(0, I)`` particles. ``history`` has a row ``{"step", "mean_logp",
    "ksd"}`` (IMQ, h = 1, U-statistic) at step 0, every ``log_every`` steps and at the end;
    ``callback(row)`` sees each one."""
    tgt = get_target(target) if isinstance(target, str) else target
    g = torch.Generator(device=device).manual_seed(seed)
    x = init_std * torch.randn(n_particles, tgt.dim, generator=g, device=device, dtype=dtype)
    sv = SVGD(tgt, x, lr, optimizer=optimizer, kernel=kernel, bandwidth=bandwidth)
    history = []

    def log(t):
        with torch.no_grad():
            row = {"step": t, "mean_logp": float(tgt.log_prob(sv.particles).mean()),
                   "ksd": float(sv.ksd())}
        history.append(row)
        if callback is not None:
            callback(row)

    log(0)
    for t in range(1, iters + 1):
        sv.step()
        if (log_every and t % log_every == 0) or t == iters:
            log(t)
    return SVGDResult(sv.particles, tgt, history)


@torch.no_grad()
def flow_ksd(model, n_samples: int = 1000, generator=None, kernel: str = "imq", h=1.0,
             stat: str = "u"):
    """Squared KSD of ``n_samples`` samples of a :class:`FlowVI` model against its target."""
    z = model.sample(n_samples, generator)
    return stein.ksd(z, score_fn(model.target)(z), h, kernel, stat)
