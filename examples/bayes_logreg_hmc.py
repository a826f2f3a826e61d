"""Bayesian logistic regression: a planar-flow posterior judged against HMC.

    python examples/bayes_logreg_hmc.py [--dim 4] [--n 200] [--chains 64] [--samples 200]

Fits the ``logreg`` posterior (``get_target("logreg")``) twice: with ``fit_hmc`` (many chains,
dual-averaging warm-up; R-hat and ESS say whether to believe it) and with a planar ``FlowVI``.
``moment_gap`` then reports, per coordinate, how far the flow's mean is from the HMC mean in
posterior standard deviations, and the ratio of the two standard deviations: the numbers the free
energy cannot give. The defaults run in a few seconds on the CPU.
"""
from _common import outdir, parser, report

import torch

from vi_normflows_amd.distributions.energies import get_target
from vi_normflows_amd.inference import fit_flow_vi, fit_hmc, moment_gap


def main(argv=None):
    ap = parser(__doc__, iters=600, out="bayes_logreg_hmc")
    ap.add_argument("--dim", type=int, default=4)
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=150)
    ap.add_argument("--leapfrog", type=int, default=8)
    ap.add_argument("--K", type=int, default=4)
    a = ap.parse_args(argv)
    out = outdir(a.out)
    tgt = get_target("logreg", dim=a.dim, n=a.n, seed=a.seed)
    h = fit_hmc(tgt, n_chains=a.chains, n_samples=a.samples, warmup=a.warmup,
                n_leapfrog=a.leapfrog, device=a.device, seed=a.seed)
    r = fit_flow_vi(tgt, flow="planar", K=a.K, iters=a.iters, lr=1e-2, n_samples=128,
                    device=a.device, seed=a.seed, log_every=a.iters)
    with torch.no_grad():
        z0 = r.base.sample(4000, torch.Generator(device=a.device).manual_seed(a.seed + 1))
        z = r.flow(z0)[0]
    gap, ratio = moment_gap(z, h.samples)
    return report(out, {
        "dim": a.dim, "n": a.n, "hmc_accept_rate": h.accept_rate, "hmc_step_size": h.step_size,
        "rhat_max": float(h.rhat.max()), "ess_min": float(h.ess.min()),
        "hmc_mean": h.samples.double().mean((0, 1)).tolist(),
        "flow_free_energy": r.final["free_energy"],
        "mean_gap_in_std": gap.tolist(), "std_ratio": ratio.tolist()})


if __name__ == "__main__":
    main()
