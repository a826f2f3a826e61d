"""Reference CLI equivalent: ``python -m vi_normflows_amd.get_data K num_iter lr [target]``.

Non-amortized planar VI on U1 (``p1``) with 100 samples, W = U = b = 0.1 init and RMSProp,
printing the Energy / Joint / Entropy lines every 100 iterations (``get_data.py:144-148``),
with the corrected estimator (the final free energy respects F >= -log Z).

Extensions (not in the reference): ``--device cuda`` runs the step on the MI355X - the K-layer
planar stack in one HIP kernel (csrc/kernels/planar.hip) and the target log-density with its
gradient in another (csrc/kernels/energy2d.hip) - and ``--samples N`` sets the Monte-Carlo
batch (the reference's 100 by default; millions fit easily on the GPU). ``--method svgd`` moves
``--particles`` particles by Stein variational gradient descent instead (``K`` is ignored,
``num_iter`` and ``lr`` keep their meaning) and reports the kernel Stein discrepancy.
"""
from __future__ import annotations

import argparse
import sys
import time

from .inference.flow_vi import optimise


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    ap = argparse.ArgumentParser(prog="get_data", description=__doc__.splitlines()[0])
    ap.add_argument("K", type=int)
    ap.add_argument("num_iter", type=int)
    ap.add_argument("lr", type=float)
    ap.add_argument("target", nargs="?", default="p1")
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--composite-target", action="store_true",
                    help="evaluate the target with the torch composite instead of the HIP kernel")
    ap.add_argument("--method", choices=("planar", "svgd"), default="planar")
    ap.add_argument("--particles", type=int, default=1000, help="SVGD particles (--method svgd)")
    def _usage_error(message):   # reference-style usage text, then argparse's own message
        print(__doc__)
        ap.exit(2, f"{ap.prog}: error: {message}\n")

    ap.error = _usage_error
    a = ap.parse_args(argv)
    from .distributions.energies import get_target
    from .ops import fused

    tgt = get_target(a.target)
    tgt.fused = not a.composite_target
    fused.energy2d_launches(reset=True)
    if a.method == "svgd":
        return _svgd(a, tgt)
    t0 = time.perf_counter()
    res = optimise(tgt, a.samples, a.num_iter, a.lr, a.K, verbose=not a.quiet,
                   device=a.device, seed=a.seed)
    dt = time.perf_counter() - t0
    if a.device != "cpu":
        print(f"[get_data] device {a.device}: {a.num_iter} iterations x {a.samples} samples in "
              f"{dt:.2f} s ({a.num_iter * a.samples / dt:.3e} samples/s); fused target kernel "
              f"launches: {fused.energy2d_launches()}; final F {res.final['free_energy']:.4f}")
    return res


def _svgd(a, tgt):
    from .inference.svgd import fit_svgd
    from .ops import fused, stein

    def cb(row):
        if not a.quiet:
            print(f"Iteration {row['step']}; Mean log p: {row['mean_logp']}; KSD: {row['ksd']}")

    stein.stein_launches(reset=True)
    t0 = time.perf_counter()
    res = fit_svgd(tgt, a.particles, a.num_iter, a.lr, device=a.device, seed=a.seed, callback=cb)
    dt = time.perf_counter() - t0
    if not a.quiet:
        print("\nFINAL METRICS\n")
        print("Mean log p: ", res.history[-1]["mean_logp"])
        print("KSD (IMQ, U-statistic): ", res.history[-1]["ksd"])
    if a.device != "cpu":
        print(f"[get_data] device {a.device}: {a.num_iter} SVGD iterations x {a.particles} "
              f"particles in {dt:.2f} s; Stein kernel launches: {stein.stein_launches()}; fused "
              f"target kernel launches: {fused.energy2d_launches()}")
    return res


if __name__ == "__main__":
    main()
