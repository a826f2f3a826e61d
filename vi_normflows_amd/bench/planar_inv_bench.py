"""Timing of the fused planar-stack inverse kernels (csrc/kernels/planar.hip) against the
existing forward kernel and the torch composite inverse on the same device.

    python -m vi_normflows_amd.bench.planar_inv_bench [--batch 16384] [--d 2] [--layers 16]
        [--reps 20] [--per-sample]

After a warm-up, the median of ``--reps`` (>= 20) HIP-event timings each of: the inverse kernel
alone, the inverse followed by its backward (through ``planar_stack_inverse`` under autograd,
``get_uhat`` and the row sums for shared parameters included), the forward kernel alone, the
forward + backward step, and the composite inverse (no autograd), all taking turns rep by rep
within one run. One JSON line. Needs a GPU and the native library: there is no fallback.
"""
from __future__ import annotations

import argparse
import json

import torch

from .timing import alternate

KERNEL_BISECTIONS, KERNEL_NEWTON = 30, 2   # kInvBisect / kInvNewton of csrc/kernels/planar.hip


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--d", type=int, default=2)
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--per-sample", action="store_true")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("planar_inv_bench: needs a GPU (no CPU fallback)")
    if a.reps < 20:
        raise SystemExit("planar_inv_bench: --reps must be >= 20")
    from ..flows import planar as pl
    from ..ops._ext import native

    ops = native()
    dev = torch.device("cuda")
    N, D, K = a.batch, a.d, a.layers
    g = torch.Generator(device=dev).manual_seed(0)
    shp = (K, N, D) if a.per_sample else (K, D)
    W = torch.randn(*shp, device=dev, generator=g) / D ** 0.5
    U = torch.randn(*shp, device=dev, generator=g) / D ** 0.5
    B = torch.randn(*shp[:-1], device=dev, generator=g)
    z = torch.randn(N, D, device=dev, generator=g)
    gx = torch.randn(N, D, device=dev, generator=g)
    gl = torch.randn(N, device=dev, generator=g)
    Uh = pl.get_uhat(U, W)
    y = pl.planar_stack(z, W, U, B)[0]      # a valid input for the inverse
    out, ldj = torch.empty_like(z), torch.empty(N, device=dev)
    saved = torch.empty(K, N, D, device=dev)

    def step(fn, v):
        def run():
            Wg, Ug, Bg = (t.detach().requires_grad_(True) for t in (W, U, B))
            vg = v.detach().requires_grad_(True)
            o, l = fn(vg, Wg, Ug, Bg)
            ((o * gx).sum() + (l * gl).sum()).backward()
        return run

    def no_grad(f):
        def run():
            with torch.no_grad():
                f()
        return run

    us = alternate({
        "inv": lambda: ops.planar_stack_inv(y, W, Uh, B, a.per_sample, False, out, ldj, saved),
        "inv_step": step(pl.planar_stack_inverse, y),
        "fwd": lambda: ops.planar_stack_fwd(z, W, Uh, B, a.per_sample, False, out, ldj, saved),
        "fwd_step": step(pl.planar_stack, z),
        "inv_composite": no_grad(lambda: pl.planar_stack_inverse_reference(y, W, U, B)),
    }, a.reps)
    x = pl.planar_stack_inverse(y, W, U, B)[0]
    print(json.dumps({
        "bench": "planar_inv", "N": N, "D": D, "K": K, "per_sample": bool(a.per_sample),
        "reps": a.reps, "bisections": KERNEL_BISECTIONS, "newton": KERNEL_NEWTON,
        "composite_bisections": pl.INV_BISECTIONS, "composite_newton": pl.INV_NEWTON,
        "device": torch.cuda.get_device_name(0),
        "us": {k: round(v, 1) for k, v in us.items()},
        "inv_over_fwd": round(us["inv"] / us["fwd"], 2),
        "speedup_vs_composite": round(us["inv_composite"] / us["inv"], 1),
        "roundtrip_max_abs_err": float((x - z).abs().max()),
    }), flush=True)


if __name__ == "__main__":
    main()
