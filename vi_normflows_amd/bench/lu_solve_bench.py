"""Timing of the fused LU solve (csrc/kernels/lu_solve.hip) against the composite of two
``torch.linalg.solve_triangular`` calls (plus the gather through ``perm`` and the bias) on the
same tensors, on the same device in the same process, the two taking turns rep by rep.

    python -m vi_normflows_amd.bench.lu_solve_bench [--reps 10] [--mode lu|lower]
        [--shapes 65536x784,32768x1024,8192x256,4096x64] [--out DIR]

Per (B, D) and per ``transpose`` off / on one JSON line: the median HIP-event time of one call of
either path (the kernel's includes the D^2 transpose it makes for ``transpose=False``; the range
check of ``perm`` is off, as in the modules after their first call), the ratio, the rows per
block and the largest difference between the two results. The lines are printed and written to
``lu_solve_bench.jsonl`` in ``--out`` (default: the next unused ``profiles/rNN/``). Needs a GPU and
the native library: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import math
import re
from pathlib import Path

import torch

from .timing import alternate

SHAPES = "65536x784,32768x1024,8192x256,4096x64"


def next_profile_dir(root: Path) -> Path:
    used = [int(m.group(1)) for p in root.glob("r*") if p.is_dir()
            and (m := re.fullmatch(r"r(\d+)", p.name))]
    return root / f"r{max(used, default=0) + 1}"


def factors(D, device, mode):
    """The well-conditioned packed factor of the tests' recipe, a permutation and a bias."""
    g = torch.Generator().manual_seed(D)
    G = torch.randn(D, D, generator=g, dtype=torch.float64) / math.sqrt(D)
    A = torch.tril(G, -1) + torch.diag(0.5 + 1.5 * torch.rand(D, generator=g, dtype=torch.float64))
    if mode == "lu":
        A = A + torch.triu(G, 1)
    perm = torch.randperm(D, generator=g)
    b = torch.randn(D, generator=g)
    return A.float().to(device), perm.to(device), b.to(device)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--mode", choices=("lu", "lower"), default="lu")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("lu_solve_bench: needs a GPU (no CPU fallback)")
    from ..ops import linear_flow as lf
    from ..ops._ext import native

    native()
    dev = torch.device("cuda")
    out = Path(a.out) if a.out else next_profile_dir(
        Path(__file__).resolve().parents[2] / "profiles")
    out.mkdir(parents=True, exist_ok=True)
    lines = []
    for shape in a.shapes.split(","):
        B, D = (int(v) for v in shape.split("x"))
        A, perm, b = factors(D, dev, a.mode)
        p32 = perm.int()
        y = torch.randn(B, D, device=dev, generator=torch.Generator(device=dev).manual_seed(B))
        for transpose in (False, True):
            bias = None if transpose else b
            n0 = lf.solve_launches()
            fns = {
                "kernel": lambda: lf.lu_solve_kernel(y, A, p32, bias, mode=a.mode,
                                                     transpose=transpose, check_perm=False),
                "composite": lambda: lf.lu_solve_reference(y, A, perm, bias, mode=a.mode,
                                                           transpose=transpose)}
            with torch.no_grad():
                us = alternate(fns, a.reps)
                diff = float((fns["kernel"]() - fns["composite"]()).abs().max())
            assert lf.solve_launches() > n0, "the kernel did not run"
            rec = {"bench": "lu_solve", "mode": a.mode, "B": B, "D": D, "transpose": transpose,
                   "reps": a.reps, "rows_per_block": lf.kernel_rows(D),
                   "us": {k: round(v, 1) for k, v in us.items()},
                   "kernel_over_composite": round(us["kernel"] / us["composite"], 3),
                   "max_abs_diff": diff, "device": torch.cuda.get_device_name(0)}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        del y
    (out / "lu_solve_bench.jsonl").write_text("\n".join(lines) + "\n")
    print(f"wrote {out / 'lu_solve_bench.jsonl'}", flush=True)


if __name__ == "__main__":
    main()
