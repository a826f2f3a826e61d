"""Bayesian logistic regression three ways: planar-flow VI, full-rank Gaussian BBVI and SVGD.

One seeded synthetic dataset (``make_glm_data``: N rows, D columns with an intercept, labels
drawn at ``theta_true``), prior ``theta ~ N(0, prior_var I)``. The posterior is the GLM target of
``distributions/posteriors.py``; on ``--device cuda`` its density and score are one fused HIP pass
over the data per evaluation, on the CPU the torch composite. Each method's posterior mean is
printed next to ``theta_true`` together with the kernel Stein discrepancy (IMQ, U-statistic, the
median bandwidth of the SVGD particles for all three) of a sample set of its own, all against the
same score. The U-statistic is unbiased, so a good fit scatters around zero with either sign; the
Stein kernel's own scale here is D / sd^2, a few hundred.

    python examples/bayes_logreg.py [--device cuda] [--n 500] [--dim 4]
    python examples/bayes_logreg.py --reduced        # seconds, the test mode
"""
from _common import outdir, parser, report

import math

import torch

from vi_normflows_amd.distributions.energies import get_target
from vi_normflows_amd.inference.bbvi import black_box_vi_full_rank
from vi_normflows_amd.inference.flow_vi import FlowVI, fit_flow_vi
from vi_normflows_amd.inference.svgd import fit_svgd, score_fn
from vi_normflows_amd.ops import stein


def main(argv=None):
    ap = parser(__doc__, 1500, "bayes_logreg")
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--dim", type=int, default=4)
    ap.add_argument("--prior-var", type=float, default=4.0)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--bbvi-iters", type=int, default=400)
    ap.add_argument("--svgd-iters", type=int, default=300)
    ap.add_argument("--particles", type=int, default=300)
    ap.add_argument("--reduced", action="store_true", help="tiny settings (the test mode)")
    a = ap.parse_args(argv)
    if a.reduced:
        a.n, a.iters, a.bbvi_iters, a.svgd_iters, a.particles = 200, 150, 60, 40, 100
    out = outdir(a.out)
    tgt = get_target("logreg", dim=a.dim, n=a.n, seed=a.seed, prior_var=a.prior_var)
    score = score_fn(tgt)
    truth = tgt.meta["theta_true"]


    # planar flow on a learned diagonal Gaussian base (the posterior is far from N(0, I))
    r = fit_flow_vi(tgt, "planar", a.K, a.iters, a.lr, a.samples, "adam", device=a.device,
                    seed=a.seed, log_every=max(a.iters, 1), learn_base=True, init="random")
    model = FlowVI(tgt, r.flow, learn_base=True).to(a.device)
    model.base = r.base
    z_flow = model.sample(a.particles, torch.Generator(device=a.device).manual_seed(a.seed + 1))

    # full-rank Gaussian, fp64 on the CPU (the composite path of the same target)
    fr = black_box_vi_full_rank(tgt.log_prob, a.dim, num_samples=a.samples, iters=a.bbvi_iters,
                                lr=0.05, seed=a.seed, init_log_std=[-1.0] * a.dim)
    eps = torch.randn(a.particles, a.dim, dtype=torch.float64,
                      generator=torch.Generator().manual_seed(a.seed + 2))
    z_full = fr.mean + eps @ fr.scale_tril.T

    sv = fit_svgd(tgt, a.particles, a.svgd_iters, 0.05, device=a.device, seed=a.seed,
                  init_std=0.5, log_every=0)
    z_svgd = sv.particles

    # one bandwidth for all three sample sets, on the scale of the posterior
    h = float(stein.median_bandwidth(z_svgd)) * math.log(a.particles + 1.0)   # median r2

    def ksd(z):
        return float(stein.ksd(z, score(z), h, "imq", "u"))

    rows = {"planar_vi": z_flow, "full_rank_bbvi": z_full, "svgd": z_svgd}
    summary = {"n": a.n, "dim": a.dim, "device": a.device, "theta_true": truth.tolist(),
               "free_energy_planar": r.final["free_energy"], "elbo_full_rank": fr.trace[-1][1],
               "methods": {k: {"mean": z.double().mean(0).tolist(), "sd": z.double().std(0).tolist(),
                               "ksd": ksd(z)} for k, z in rows.items()}}
    fmt = lambda v: " ".join(f"{x:7.3f}" for x in v)
    print(f"{'theta_true':16s} {fmt(truth.tolist())}")
    for k, v in summary["methods"].items():
        print(f"{k:16s} {fmt(v['mean'])}   KSD {v['ksd']:.5f}")
    return report(out, summary)


if __name__ == "__main__":
    main()
