"""Mean-field black-box VI on Bayesian linear regression vs the closed-form posterior
(reference ``"Final (master).ipynb"`` cells 5-8, data ``data/HW0_data.csv``).

Prints the VI mean / sd next to the exact posterior mean / sd: the means agree
(mu_post ~ [8.820, 5.216], Experimentation.ipynb:183) and the mean-field sds are the optimal
1 / sqrt(diag(precision)) - smaller than the true marginal sds. ``--family full`` fits the
full-rank Gaussian instead (``black_box_vi_full_rank``): its sds and its correlation match the
exact posterior's.

    python examples/bbvi_linreg.py [--data /path/to/HW0_data.csv] [--family mean-field|full]
"""
from _common import ROOT, outdir, parser, report

import torch

from vi_normflows_amd.inference.bbvi import black_box_vi, black_box_vi_full_rank, design, linreg_log_joint, linreg_posterior, load_hw0


def main(argv=None):
    ap = parser(__doc__, 4000, "bbvi")
    ap.add_argument("--data", default=None)
    ap.add_argument("--noise-var", type=float, default=0.5)
    ap.add_argument("--family", choices=("mean-field", "full"), default="mean-field")
    a = ap.parse_args(argv)
    out = outdir(a.out)
    path = a.data
    if path is None:
        for cand in (ROOT / "data" / "HW0_data.csv", ROOT.parent / "reference" / "data" / "HW0_data.csv"):
            if cand.exists():
                path = cand
                break
    if path is None:
        g = torch.Generator().manual_seed(a.seed)   # synthetic stand-in with the same shape
        x = torch.rand(100, generator=g, dtype=torch.float64) * 10
        y = 8.8 + 5.2 * x + torch.randn(100, generator=g, dtype=torch.float64) * 0.7
    else:
        x, y = load_hw0(path)
    X = design(x)
    prior = [[1.0, 0.0], [0.0, 0.5]]
    fit = black_box_vi_full_rank if a.family == "full" else black_box_vi
    res = fit(linreg_log_joint(X, y, prior, a.noise_var), 2, num_samples=500, iters=a.iters,
              lr=0.05, seed=a.seed)
    mu, cov = linreg_posterior(X, y, prior, a.noise_var)
    sd_vi = torch.sqrt(torch.diag(res.cov))
    corr = lambda c: (c[0, 1] / torch.sqrt(c[0, 0] * c[1, 1])).item()
    return report(out, {"data": str(path) if path else "synthetic", "family": a.family,
                        "mu_vi": res.mean.tolist(), "sd_vi": sd_vi.tolist(),
                        "corr_vi": corr(res.cov), "corr_post": corr(cov), "mu_post": mu.tolist(),
                        "sd_post": torch.sqrt(torch.diag(cov)).tolist(),
                        "sd_meanfield_optimum": (1 / torch.sqrt(torch.diag(torch.linalg.inv(cov)))).tolist()})


if __name__ == "__main__":
    main()
