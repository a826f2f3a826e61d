"""Timing of the all-pairs Stein kernels (csrc/kernels/stein.hip) against the row-chunked fp32
torch composite on the same device.

    python -m vi_normflows_amd.bench.stein_bench [--n 1024 4096 16384 65536] [--dims 2 40]
        [--reps 20] [--out profiles/r11/stein_bench.jsonl]

For every (N, D) and both ops (``svgd``: the SVGD direction, RBF; ``ksd``: the Stein-kernel row
sums, IMQ), after a warm-up, the median of ``--reps`` (>= 20) HIP-event timings of the kernel
(``impl="kernel"``, the launcher's own j-split) and of the composite (``ops/reference.py``, rows
chunked so that one [chunk, N, D] temporary stays within ``--chunk-bytes``), the two taking
turns rep by rep. The bandwidth is the median heuristic as a device tensor. The arithmetic rate
counts the operations the definition needs per pair (svgd 7 D + 4, ksd 8 D + 12: differences,
r2, the dot products and the accumulation; the exponential or rsqrt as one). One JSON line per
(op, N, D), printed and appended to ``--out``. Needs a GPU and the native library: there is no
fallback.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path

import torch

from .timing import alternate


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="+", default=[1024, 4096, 16384, 65536])
    ap.add_argument("--dims", type=int, nargs="+", default=[2, 40])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunk-bytes", type=int, default=256 << 20)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("stein_bench: needs a GPU (no CPU fallback)")
    if a.reps < 20:
        raise SystemExit("stein_bench: --reps must be >= 20")
    from ..ops import reference, stein
    from ..ops._ext import native

    ops = native()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    for D in a.dims:
        for N in a.n:
            x = 1.5 * torch.randn(N, D, device=dev, generator=g)
            s = -x + 0.3 * torch.randn(N, D, device=dev, generator=g)
            h = stein.median_bandwidth(x)
            chunk = max(1, min(N, a.chunk_bytes // (4 * N * D)))
            runs = {
                "svgd": (lambda: stein.svgd_direction(x, s, h, "rbf", impl="kernel"),
                         lambda: reference.svgd_direction_reference(x, s, h, "rbf", chunk=chunk),
                         7 * D + 4),
                "ksd": (lambda: stein.ksd_rows(x, s, h, "imq", impl="kernel"),
                        lambda: reference.ksd_rows_reference(x, s, h, "imq", chunk=chunk),
                        8 * D + 12),
            }
            for op, (kern, comp, flops_per_pair) in runs.items():
                us = alternate({"kernel": kern, "composite": comp}, a.reps)
                got, want = kern(), comp()
                got, want = (got, want) if op == "svgd" else (got[0], want[0])
                scale = want.abs().max().item()
                line = json.dumps({
                    "bench": "stein", "op": op, "kernel_fn": "rbf" if op == "svgd" else "imq",
                    "N": N, "D": D, "j_splits": ops.stein_workspace(N, D, 0, 1) // N,
                    "composite_chunk_rows": chunk, "reps": a.reps,
                    "device": torch.cuda.get_device_name(0),
                    "us": {k: round(v, 1) for k, v in us.items()},
                    "speedup_vs_composite": round(us["composite"] / us["kernel"], 1),
                    "kernel_Gpairs_per_s": round(N * N / us["kernel"] / 1e3, 2),
                    "kernel_TFLOPs": round(N * N * flops_per_pair / us["kernel"] / 1e6, 3),
                    "max_abs_diff_over_max_abs": (got - want).abs().max().item() / scale,
                })
                print(line, flush=True)
                if a.out:
                    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
            del x, s


if __name__ == "__main__":
    main()
