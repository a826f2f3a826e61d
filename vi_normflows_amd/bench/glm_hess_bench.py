"""Timing of the GLM Newton-statistics kernel (csrc/kernels/glm_hess.hip) against the fp32 torch
composite on the same device.

    python -m vi_normflows_amd.bench.glm_hess_bench [--shapes 1,8192,8 64,262144,64 ...]
        [--families bernoulli] [--reps 20] [--limit 120] [--out profiles/glm_hess_bench.jsonl]

Every (B, N, D) runs in a child process of its own under ``--limit`` seconds; the parent never
opens the GPU and stops at the first child that fails or runs out of time. A child takes, after a
warm-up, the median of ``--reps`` (>= 20) HIP-event timings of the kernel (``impl="kernel"``, the
launcher's own n-split) and of the composite (``ops/reference.py`` ``glm_hessian_reference``,
which streams X for eta, builds ``[chunk, N, D]`` of weighted rows and multiplies per parameter
row), the two taking turns rep by rep. Both compute log p, the score and the negative Hessian
under a scalar prior.

Bytes: the kernel reads X and y once per parameter row, ``4 B N (D + 1)``, and writes ``4 S B
(D^2 + D + 1)`` of partials that the finalize kernel reads back; ``kernel_GBps`` is the first
over the kernel time. X of one shape is at most 64 MiB and stays in the 256 MiB Infinity Cache
between the B rows and between repetitions, so the rate is a cache rate unless B = 1 and the
shape is the first touch; it is set against the HBM copy rate only as a yardstick. Flops: the
upper triangle's ``D (D + 1)`` per pair plus ``4 D`` for eta and the score plus ``D`` for w x.
One JSON line per shape, printed and appended to ``--out`` (docs/PERF_NOTES.md, "GLM Hessian").
Needs a GPU and the native library: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
from pathlib import Path

SHAPES = [f"{B},{N},{D}" for N in (8192, 262144) for D in (8, 32, 64) for B in (1, 8, 64)]


def _child(a):
    import torch

    from ..distributions.posteriors import make_glm_data
    from ..ops import glm, reference
    from ..ops._ext import native
    from .timing import alternate

    if not torch.cuda.is_available():
        raise SystemExit("glm_hess_bench: needs a GPU (no CPU fallback)")
    ops = native()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    (shape,) = a.shapes
    B, N, D = (int(v) for v in shape.split(","))
    for family in a.families:
        X, y, theta_true = (t.to(dev) for t in make_glm_data(family, N, D, seed=0))
        theta = theta_true + 0.1 * torch.randn(B, D, device=dev, generator=g)

        def kern():
            return glm.glm_logp_grad_hess(theta, X, y, family, 1.0, impl="kernel")

        def comp():
            return reference.glm_hessian_reference(theta, X, y, family, 1.0)
        us = alternate({"kernel": kern, "composite": comp}, a.reps)
        got, ref = kern(), comp()
        E = D * D + D + 1
        S = ops.glm_hess_workspace(B, N, D, 0) // (B * E)
        flop = B * N * (D * (D + 1) + 5 * D + 8)
        line = json.dumps({
            "bench": "glm_hess", "family": family, "B": B, "N": N, "D": D, "n_splits": S,
            "reps": a.reps, "device": torch.cuda.get_device_name(0),
            "us": {k: round(v, 1) for k, v in us.items()},
            "speedup_vs_composite": round(us["composite"] / us["kernel"], 2),
            "kernel_GBps": round(4 * B * N * (D + 1) / us["kernel"] / 1e3, 1),
            "kernel_partials_MB": round(4 * S * B * E / 1e6, 2),
            "kernel_TFLOPs": round(flop / us["kernel"] / 1e6, 3),
            "max_abs_diff_over_max_abs": {
                k: (u - v).abs().max().item() / v.abs().max().item()
                for k, u, v in zip(("logp", "grad", "hess"), got, ref)},
        })
        print(line, flush=True)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=SHAPES, help="B,N,D triples")
    ap.add_argument("--families", nargs="+", default=["bernoulli"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds per shape")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.reps < 20:
        raise SystemExit("glm_hess_bench: --reps must be >= 20")
    if a.child:
        return _child(a)
    for shape in a.shapes:
        cmd = [sys.executable, "-m", "vi_normflows_amd.bench.glm_hess_bench", "--child",
               "--shapes", shape, "--families", *a.families, "--reps", str(a.reps)]
        if a.out:
            cmd += ["--out", a.out]
        try:
            r = subprocess.run(cmd, timeout=a.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"glm_hess_bench: {shape} ran past {a.limit} s; stopping") from None
        if r.returncode != 0:
            raise SystemExit(f"glm_hess_bench: {shape} exited with {r.returncode}; stopping")


if __name__ == "__main__":
    main()
