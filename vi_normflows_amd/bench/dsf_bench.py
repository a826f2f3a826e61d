"""Timing of the fused deep sigmoidal flow kernels (csrc/kernels/dsf.hip) against the torch
composite on the same device.

    python -m vi_normflows_amd.bench.dsf_bench [--batch 16384] [--d 40] [--units 8] [--reps 20]

For fp32 and bf16 params: after a warm-up, the median of ``--reps`` (>= 20) HIP-event timings
each of a training step of the transform (forward + backward through ``dsf_transform``, kernel
path and composite under torch autograd), of the three kernels alone (forward, inverse,
backward) and of the composite's forward and inverse, all taking turns rep by rep within one
run; the effective bytes/s of each kernel from the compulsory bytes of the shapes (params, x
and y once for the forward and inverse; params, x, g_out, dparams and gx once for the
backward); and their share of the device-to-device copy rate measured in the same run. One JSON
line per params dtype. Needs a GPU and the native library: there is no fallback.
"""
from __future__ import annotations

import argparse
import json

import torch

from .spline_bench import _alternate


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--d", type=int, default=40)
    ap.add_argument("--units", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("dsf_bench: needs a GPU (no CPU fallback)")
    if a.reps < 20:
        raise SystemExit("dsf_bench: --reps must be >= 20")
    from ..ops import dsf as ds
    from ..ops import reference
    from ..ops._ext import native

    native()
    dev = torch.device("cuda")
    B, D, H = a.batch, a.d, a.units
    P = 3 * H * D
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, D, device=dev, generator=g) * 1.5
    g_out = torch.randn(B, D, device=dev, generator=g)
    g_ldj = torch.randn(B, device=dev, generator=g)
    # device-to-device copy rate (read + write) on a buffer of the params' size
    src = torch.empty(B * P, device=dev, dtype=torch.float32).normal_(generator=g)
    dst = torch.empty_like(src)
    copy_us = _alternate({"copy": lambda: dst.copy_(src)}, a.reps)["copy"]
    copy_bps = 2 * src.numel() * 4 / (copy_us * 1e-6)
    del dst
    for dtype, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        params = (src.view(B, P) * 0.5).to(dtype)
        es = params.element_size()
        y = ds.dsf_fwd(params, x, H)[0]    # a valid input for the inverse
        bytes_fwd = B * (P * es + 8 * D + 4)
        bytes_bwd = B * (2 * P * es + 12 * D + 4)

        def step(transform):
            def run():
                p = params.detach().requires_grad_(True)
                v = x.detach().requires_grad_(True)
                out, ldj = transform(p, v, H)
                ((out * g_out).sum() + (ldj * g_ldj).sum()).backward()
            return run

        def no_grad(f):
            def run():
                with torch.no_grad():
                    f()
            return run

        us = _alternate({
            "step": step(ds.dsf_transform),
            "step_composite": step(reference.dsf_transform),
            "fwd": no_grad(lambda: ds.dsf_fwd(params, x, H, False)),
            "fwd_composite": no_grad(lambda: reference.dsf_transform(params, x, H, False)),
            "inv": no_grad(lambda: ds.dsf_fwd(params, y, H, True)),
            "inv_composite": no_grad(lambda: reference.dsf_transform(params, y, H, True)),
            "bwd": no_grad(lambda: ds.dsf_bwd(params, x, g_out, g_ldj, H, False)),
            "bwd_inv": no_grad(lambda: ds.dsf_bwd(params, x, g_out, g_ldj, H, True)),   # x-side
        }, a.reps)
        kernels = ("fwd", "inv", "bwd", "bwd_inv")
        gbps = {k: (bytes_bwd if k.startswith("bwd") else bytes_fwd) / (us[k] * 1e-6) / 1e9
                for k in kernels}
        print(json.dumps({
            "bench": "dsf", "params": name, "B": B, "D": D, "H": H, "reps": a.reps,
            "inverse_bisections": 40, "device": torch.cuda.get_device_name(0),
            "us": {k: round(v, 1) for k, v in us.items()},
            "compulsory_bytes": {"fwd": bytes_fwd, "bwd": bytes_bwd},
            "eff_GBps": {k: round(v, 1) for k, v in gbps.items()},
            "copy_GBps": round(copy_bps / 1e9, 1),
            "share_of_copy": {k: round(v * 1e9 / copy_bps, 3) for k, v in gbps.items()},
            "speedup_vs_composite": {k: round(us[k + "_composite"] / us[k], 1)
                                     for k in ("step", "fwd", "inv")},
        }), flush=True)
        del params, y


if __name__ == "__main__":
    main()
