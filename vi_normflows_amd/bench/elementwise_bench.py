"""Shared body of the element-wise transform benchmarks (``spline_bench``, ``dsf_bench``).

For fp32 and bf16 params: after a warm-up, the median of ``--reps`` (>= 20) HIP-event timings of
every case of the transform, all taking turns rep by rep within one run; the effective bytes/s
of the four kernels from the compulsory bytes of the shapes (params, x and y once for the forward
and inverse; params, x, g_out, dparams and gx once for the backward); and their share of the
device-to-device copy rate measured in the same run. One JSON line per params dtype.
"""
from __future__ import annotations

import argparse
import json
from typing import Callable, NamedTuple

import torch

from .timing import alternate

KERNELS = ("fwd", "inv", "bwd", "bwd_inv")


class Transform(NamedTuple):
    D: int              # elements per row
    planes: int         # params planes per element
    x_scale: float      # std of the input
    shape: dict         # JSON entries after "B"
    extra: dict         # JSON entries after "reps"
    forward: Callable   # (params, x) -> y, a valid input for the inverse
    cases: Callable     # (params, x, y, g_out, g_ldj) -> {name: callable}, run under no_grad;
    #                     holds the KERNELS and "<k>_composite" for every k of speedup
    speedup: tuple


def run(name: str, doc: str, argv, batch: int, options, transform) -> None:
    """``options``: (flag, type, default) of the transform's own arguments, after ``--batch``;
    ``transform(args)`` gives the Transform."""
    ap = argparse.ArgumentParser(description=doc,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=batch)
    for flag, typ, default in options:
        ap.add_argument(flag, type=typ, default=default)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit(f"{name}_bench: needs a GPU (no CPU fallback)")
    if a.reps < 20:
        raise SystemExit(f"{name}_bench: --reps must be >= 20")
    from ..ops._ext import native

    native()
    t = transform(a)
    dev = torch.device("cuda")
    B, D, P = a.batch, t.D, t.planes * t.D
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, D, device=dev, generator=g) * t.x_scale
    g_out = torch.randn(B, D, device=dev, generator=g)
    g_ldj = torch.randn(B, device=dev, generator=g)
    # device-to-device copy rate (read + write) on a buffer of the params' size
    src = torch.empty(B * P, device=dev, dtype=torch.float32).normal_(generator=g)
    dst = torch.empty_like(src)
    copy_us = alternate({"copy": lambda: dst.copy_(src)}, a.reps)["copy"]
    copy_bps = 2 * src.numel() * 4 / (copy_us * 1e-6)
    del dst
    for dtype, pname in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        params = (src.view(B, P) * 0.5).to(dtype)
        es = params.element_size()
        y = t.forward(params, x)
        bytes_fwd = B * (P * es + 8 * D + 4)
        bytes_bwd = B * (2 * P * es + 12 * D + 4)
        with torch.no_grad():
            us = alternate(t.cases(params, x, y, g_out, g_ldj), a.reps)
        gbps = {k: (bytes_bwd if k.startswith("bwd") else bytes_fwd) / (us[k] * 1e-6) / 1e9
                for k in KERNELS}
        print(json.dumps({
            "bench": name, "params": pname, "B": B, **t.shape, "reps": a.reps, **t.extra,
            "device": torch.cuda.get_device_name(0),
            "us": {k: round(v, 1) for k, v in us.items()},
            "compulsory_bytes": {"fwd": bytes_fwd, "bwd": bytes_bwd},
            "eff_GBps": {k: round(v, 1) for k, v in gbps.items()},
            "copy_GBps": round(copy_bps / 1e9, 1),
            "share_of_copy": {k: round(v * 1e9 / copy_bps, 3) for k, v in gbps.items()},
            "speedup_vs_composite": {k: round(us[k + "_composite"] / us[k], 1)
                                     for k in t.speedup},
        }), flush=True)
        del params, y
