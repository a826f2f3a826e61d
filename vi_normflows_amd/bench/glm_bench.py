"""Timing of the GLM likelihood kernel (csrc/kernels/glm.hip) against the fp32 torch composite on
the same device.

    python -m vi_normflows_amd.bench.glm_bench [--shapes 1024,1024,8 4096,8192,16 ...]
        [--families bernoulli poisson gaussian] [--reps 20] [--out profiles/glm_bench.jsonl]

For every (B, N, D) and family, after a warm-up, the median of ``--reps`` (>= 20) HIP-event
timings of the kernel (``impl="kernel"``, the launcher's own n-split) and of the composite
(``ops/reference.py``, rows of theta chunked so that one [chunk, N] block of logits stays within
``--chunk-bytes``), the two taking turns rep by rep. Both compute log p and the score under a
scalar prior. The arithmetic rate counts the operations the definition needs per (i, n) pair:
4 D for the two products plus 8 for the link (the exponential, logarithm and reciprocal as one
each). One JSON line per (family, B, N, D), printed and appended to ``--out``; ``auto`` in
``ops/glm.py`` is decided from these numbers (docs/PERF_NOTES.md, "GLM likelihood"). Needs a GPU
and the native library: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path

import torch

from .timing import alternate

SHAPES = ["256,512,2", "1024,1024,8", "4096,8192,16", "1024,65536,32", "4096,65536,54",
          "65536,8192,64"]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=SHAPES, help="B,N,D triples")
    ap.add_argument("--families", nargs="+", default=["bernoulli"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunk-bytes", type=int, default=256 << 20)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("glm_bench: needs a GPU (no CPU fallback)")
    if a.reps < 20:
        raise SystemExit("glm_bench: --reps must be >= 20")
    from ..distributions.posteriors import make_glm_data
    from ..ops import glm, reference
    from ..ops._ext import native

    ops = native()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    for shape in a.shapes:
        B, N, D = (int(v) for v in shape.split(","))
        for family in a.families:
            X, y, theta_true = (t.to(dev) for t in make_glm_data(family, N, D, seed=0))
            theta = theta_true + 0.1 * torch.randn(B, D, device=dev, generator=g)
            chunk = max(1, min(B, a.chunk_bytes // (4 * N)))

            def kern():
                return glm.glm_logp_grad(theta, X, y, family, 1.0, impl="kernel")

            def comp():
                return reference.glm_logp_grad_reference(theta, X, y, family, 1.0, chunk=chunk)
            us = alternate({"kernel": kern, "composite": comp}, a.reps)
            (lp, gr), (lp_c, gr_c) = kern(), comp()
            line = json.dumps({
                "bench": "glm", "family": family, "B": B, "N": N, "D": D,
                "n_splits": ops.glm_workspace(B, N, D, 0) // (B * (D + 1)),
                "composite_chunk_rows": chunk, "composite_logits_MiB": round(4 * B * N / 2 ** 20, 1),
                "reps": a.reps, "device": torch.cuda.get_device_name(0),
                "us": {k: round(v, 1) for k, v in us.items()},
                "speedup_vs_composite": round(us["composite"] / us["kernel"], 2),
                "kernel_Gpairs_per_s": round(B * N / us["kernel"] / 1e3, 2),
                "kernel_TFLOPs": round(B * N * (4 * D + 8) / us["kernel"] / 1e6, 3),
                "max_abs_diff_over_max_abs": {
                    "logp": (lp - lp_c).abs().max().item() / lp_c.abs().max().item(),
                    "grad": (gr - gr_c).abs().max().item() / gr_c.abs().max().item()},
            })
            print(line, flush=True)
            if a.out:
                Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            del X, y, theta


if __name__ == "__main__":
    main()
