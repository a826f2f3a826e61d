"""Bayesian logistic regression: the Laplace approximation, and what it is good for.

    python examples/glm_laplace.py [--dim 4] [--n 200] [--chains 64] [--samples 200]

Fits the ``logreg`` posterior (``get_target("logreg")``) three ways:

- ``fit_laplace``: the MAP by Newton's method and the Gaussian N(mode, H^-1) around it, with its
  evidence estimate ``log Z ~ log p(mode) + D/2 log 2 pi - 1/2 log det H``;
- full-rank Gaussian VI (``black_box_vi_full_rank``) started from that Gaussian instead of N(0, I);
- HMC whose diagonal mass is the Laplace covariance's diagonal (``HMC(minv=...)``), the reference.

``moment_gap`` reports how far the Laplace and the VI Gaussians are from the HMC draws, and how
far VI moved from its Laplace start. The free energy F of a variational fit is an upper bound of
``-log Z``, so ``F + log_evidence`` says how the Laplace estimate sits against the bound: it may
fall on either side of it, because the Laplace evidence is an approximation for the logit link.
The defaults run in a few seconds on the CPU.
"""
from _common import outdir, parser, report

import torch

from vi_normflows_amd.distributions.energies import get_target
from vi_normflows_amd.inference import HMC, black_box_vi_full_rank, fit_laplace, moment_gap


def main(argv=None):
    ap = parser(__doc__, iters=300, out="glm_laplace")
    ap.add_argument("--dim", type=int, default=4)
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--leapfrog", type=int, default=8)
    a = ap.parse_args(argv)
    out = outdir(a.out)
    tgt = get_target("logreg", dim=a.dim, n=a.n, seed=a.seed)
    lap = fit_laplace(tgt, device=a.device, seed=a.seed)
    g = torch.Generator().manual_seed(a.seed + 1)
    draws = 4000
    z_lap = lap.mode + torch.randn(draws, a.dim, generator=g, dtype=torch.float64) @ lap.scale_tril.T

    vi = black_box_vi_full_rank(tgt.log_prob, a.dim, num_samples=256, iters=a.iters, lr=5e-3,
                                seed=a.seed, init=lap, log_every=a.iters)
    z_vi = vi.mean + torch.randn(draws, a.dim, generator=g, dtype=torch.float64) @ vi.scale_tril.T
    free_energy = -vi.trace[-1][1]

    gd = torch.Generator(device=a.device).manual_seed(a.seed)
    theta0 = (lap.mode + 0.1 * torch.randn(a.chains, a.dim, dtype=torch.float64)).to(
        device=a.device, dtype=torch.float32)
    hmc = HMC(tgt, theta0, 0.5, a.leapfrog, minv=lap.minv(), jitter=0.1, generator=gd)
    hmc.warmup(a.warmup)
    samples = torch.stack([hmc.step().theta for _ in range(a.samples)])

    gap_lap, ratio_lap = moment_gap(z_lap, samples)
    gap_vi, ratio_vi = moment_gap(z_vi, samples)
    gap_move, ratio_move = moment_gap(z_vi, z_lap)
    return report(out, {
        "dim": a.dim, "n": a.n, "newton_iterations": lap.n_iter.tolist(),
        "converged": bool(lap.converged.all()), "mode": lap.mode.tolist(),
        "log_evidence_laplace": lap.log_evidence, "free_energy_vi": free_energy,
        "free_energy_plus_log_evidence": free_energy + lap.log_evidence,
        "hmc_step_size": hmc.step_size,
        "laplace_vs_hmc": {"mean_gap_in_std": gap_lap.tolist(), "std_ratio": ratio_lap.tolist()},
        "vi_vs_hmc": {"mean_gap_in_std": gap_vi.tolist(), "std_ratio": ratio_vi.tolist()},
        "vi_vs_laplace": {"mean_gap_in_std": gap_move.tolist(), "std_ratio": ratio_move.tolist()}})


if __name__ == "__main__":
    main()
