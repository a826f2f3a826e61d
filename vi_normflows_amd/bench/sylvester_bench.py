"""Timing of the fused Sylvester stack kernels (csrc/kernels/sylvester.hip) against the torch
composite on the same device, with per-sample parameters at the latent width of the VAE.

    python -m vi_normflows_amd.bench.sylvester_bench [--rows 1024 16384] [--dim 40]
        [--layers 4] [--householders 8] [--reps 20] [--out profiles/r8/sylvester_bench.jsonl]

For every row count, after a warm-up, the median of ``--reps`` (>= 20) HIP-event timings each
of: the forward (``fwd``: the raw op, layer inputs saved as in training; ``fwd_composite``) and
forward + backward through the public ``sylvester_stack`` (``fwdbwd``: impl="kernel",
``fwdbwd_composite``: impl="composite", the autograd graph built inside the timed region in
both), plus the raw backward op (``bwd``); kernel and composite alternate within one run. The
effective bytes/s come from the compulsory bytes of the shapes (forward: parameters, z, z_K,
ldj and the saved layer inputs once; backward: parameters, saved inputs, both cotangents, dz
and the per-row parameter gradients once) and are set against the device-to-device copy rate
measured in the same run. One JSON line per row count, printed and appended to ``--out``.
Needs a GPU and the native library: there is no fallback.
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
    ap.add_argument("--rows", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--dim", type=int, default=40)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--householders", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("sylvester_bench: needs a GPU (no CPU fallback)")
    if a.reps < 20:
        raise SystemExit("sylvester_bench: --reps must be >= 20")
    from ..ops import sylvester as syl
    from ..ops._ext import native

    native()
    dev = torch.device("cuda")
    D, K, H = a.dim, a.layers, a.householders
    P = D * (D - 1) // 2
    width = K * (2 * P + 3 * D + H * D)           # parameter floats of a row
    g = torch.Generator(device=dev).manual_seed(0)
    # device-to-device copy rate (read + write) on a buffer of the largest parameter block
    src = torch.empty(max(a.rows) * width, device=dev, dtype=torch.float32).normal_(generator=g)
    dst = torch.empty_like(src)
    copy_us = alternate({"copy": lambda: dst.copy_(src)}, a.reps)["copy"]
    copy_bps = 2 * src.numel() * 4 / (copy_us * 1e-6)
    del src, dst
    flips = [k % 2 for k in range(K)]
    for N in a.rows:
        def rn(*shape, scale=1.0):
            return torch.randn(*shape, device=dev, generator=g) * scale

        z, gz, gl = rn(N, D), rn(N, D), rn(N)
        R1, R2 = rn(N, K, P, scale=1.5 / D ** 0.5), rn(N, K, P, scale=1.5 / D ** 0.5)
        d1, d2 = torch.tanh(rn(N, K, D, scale=0.8)), torch.tanh(rn(N, K, D, scale=0.8))
        params = [R1, R2, d1, d2, rn(N, K, D), rn(N, K, H, D)]
        saved = syl.sylvester_fwd(z, *params, flips)[2]
        bytes_fwd = 4 * N * (width + 2 * D + 1 + K * D)
        bytes_bwd = 4 * N * (2 * width + K * D + 2 * D + 1 + D)

        def fwdbwd(impl):
            def run():
                leaves = [t.detach().requires_grad_(True) for t in (z, *params)]
                zK, ldj = syl.sylvester_stack(*leaves, flips, impl=impl)
                torch.autograd.grad((zK * gz).sum() + (ldj * gl).sum(), leaves)
            return run

        def no_grad(f):
            def run():
                with torch.no_grad():
                    return f()
            return run

        us = alternate({
            "fwd": no_grad(lambda: syl.sylvester_fwd(z, *params, flips)),
            "fwd_composite": no_grad(
                lambda: syl.sylvester_stack(z, *params, flips, impl="composite")),
            "bwd": no_grad(lambda: syl.sylvester_bwd(saved, *params, flips, gz, gl)),
            "fwdbwd": fwdbwd("kernel"),
            "fwdbwd_composite": fwdbwd("composite"),
        }, a.reps)
        bts = {"fwd": bytes_fwd, "bwd": bytes_bwd, "fwdbwd": bytes_fwd + bytes_bwd}
        gbps = {k: b / (us[k] * 1e-6) / 1e9 for k, b in bts.items()}
        line = json.dumps({
            "bench": "sylvester", "params": "per_sample", "N": N, "D": D, "K": K, "H": H,
            "reps": a.reps, "device": torch.cuda.get_device_name(0),
            "us": {k: round(v, 1) for k, v in us.items()},
            "compulsory_bytes": bts,
            "eff_GBps": {k: round(v, 1) for k, v in gbps.items()},
            "copy_GBps": round(copy_bps / 1e9, 1),
            "share_of_copy": {k: round(v * 1e9 / copy_bps, 3) for k, v in gbps.items()},
            "speedup_vs_composite": {k: round(us[k + "_composite"] / us[k], 1)
                                     for k in ("fwd", "fwdbwd")},
        })
        print(line, flush=True)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del params, saved, R1, R2, d1, d2


if __name__ == "__main__":
    main()
