"""Timing of the fused HMC trajectory kernel (csrc/kernels/glm_hmc.hip) against the stepwise path
on the same device and inputs.

    python -m vi_normflows_amd.bench.hmc_bench [--shapes 1024,16384,16,16 ...]
        [--families bernoulli] [--reps 20] [--out profiles/hmc_bench.jsonl]

For every (C, N, D, L) and family, after a warm-up, the median of ``--reps`` (>= 20) HIP-event
timings of one HMC iteration (``ops.hmc.glm_hmc_step``: L leapfrog steps and the accept step) as

* ``rows32`` / ``rows64`` / ``rows128``: ``impl="kernel"`` with that many chains per workgroup,
  one launch each;
* ``stepwise``: ``impl="stepwise"``, L launches of the GLM likelihood kernel with the launcher's
  own n-split plus the element-wise torch updates between them and the accept step in torch:
  only kernels the project had before the fused one.

The callables take turns rep by rep. One JSON line per (family, C, N, D, L), printed and appended
to ``--out``; ``auto`` in ``ops/hmc.py`` and the launcher's row-tile rule are decided from these
numbers (docs/PERF_NOTES.md, "HMC trajectory"). Needs a GPU and the native library: there is no
fallback.
"""
from __future__ import annotations

import argparse
import itertools
import json
import math
from pathlib import Path

import torch

from .timing import alternate

SHAPES = [f"{c},{n},{d},{l}" for c, n, d, l in itertools.product(
    (256, 1024, 4096, 16384), (1024, 16384), (8, 16, 64), (4, 16, 64))]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=SHAPES, help="C,N,D,L quadruples")
    ap.add_argument("--families", nargs="+", default=["bernoulli"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("hmc_bench: needs a GPU (no CPU fallback)")
    if a.reps < 20:
        raise SystemExit("hmc_bench: --reps must be >= 20")
    from ..distributions.posteriors import make_glm_data
    from ..ops import glm, hmc

    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    for shape in a.shapes:
        C, N, D, L = (int(v) for v in shape.split(","))
        for family in a.families:
            X, y, theta_true = (t.to(dev) for t in make_glm_data(family, N, D, seed=0))
            theta = theta_true + 0.1 * torch.randn(C, D, device=dev, generator=g)
            p = torch.randn(C, D, device=dev, generator=g)
            log_u = torch.log(torch.rand(C, device=dev, generator=g))
            eps = (0.5 / math.sqrt(N)) * (0.9 + 0.2 * torch.rand(C, device=dev, generator=g))
            lp0, g0 = glm.glm_logp_grad(theta, X, y, family, 1.0, impl="kernel")

            def run(impl, rows=None):
                return hmc.glm_hmc_step(theta, lp0, g0, p, log_u, eps, L, X, y, family, 1.0,
                                        impl=impl, rows=rows)
            fns = {f"rows{r}": (lambda r=r: run("kernel", r)) for r in hmc.ROW_TILES}
            fns["stepwise"] = lambda: run("stepwise")
            us = alternate(fns, a.reps)
            k, s = run("kernel"), run("stepwise")
            best = min(hmc.ROW_TILES, key=lambda r: us[f"rows{r}"])
            line = json.dumps({
                "bench": "hmc", "family": family, "C": C, "N": N, "D": D, "L": L,
                "reps": a.reps, "device": torch.cuda.get_device_name(0),
                "us": {n: round(v, 1) for n, v in us.items()},
                "launcher_rows": hmc.kernel_rows(C, D), "best_rows": best,
                "speedup_vs_stepwise": {n: round(us["stepwise"] / v, 2) for n, v in us.items()
                                        if n != "stepwise"},
                "us_per_leapfrog_best": round(us[f"rows{best}"] / L, 2),
                "accept_rate": {"kernel": k.accept.mean().item(), "stepwise": s.accept.mean().item()},
                "max_abs_diff_over_max_abs": {
                    "theta_prop": (k.theta_prop - s.theta_prop).abs().max().item()
                    / s.theta_prop.abs().max().item(),
                    "dH": (k.dH - s.dH).abs().max().item() / max(s.dH.abs().max().item(), 1e-30)},
            })
            print(line, flush=True)
            if a.out:
                Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            del X, y, theta, p


if __name__ == "__main__":
    main()
