"""Timing of the fused rational-quadratic spline kernels (csrc/kernels/spline.hip) against the
torch composite on the same device, at the shape of the headline model's coupling half.

    python -m vi_normflows_amd.bench.spline_bench [--batch 65536] [--dh 392] [--bins 8] [--reps 20]

For fp32 and bf16 params: after a warm-up, the median of ``--reps`` (>= 20) HIP-event timings
each of forward, inverse and backward, kernel and composite alternating within one run; the
effective bytes/s from the compulsory bytes of the shapes (params, x and y once for the forward
and inverse; params, x, g_out, dparams and gx once for the backward); and their share of the
device-to-device copy rate measured in the same run. One JSON line per params dtype. Needs a GPU
and the native library: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import statistics

import torch


def _event_us(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1000.0


def _alternate(fns: dict, reps: int, warmup: int = 3) -> dict:
    """Median us of each callable, the callables taking turns rep by rep. A callable marked
    ``self_timed`` returns its own event time (it has untimed set-up of its own)."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            t[k].append(f() if getattr(f, "self_timed", False) else _event_us(f))
    return {k: statistics.median(v) for k, v in t.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--dh", type=int, default=392)
    ap.add_argument("--bins", type=int, default=8)
    ap.add_argument("--bound", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("spline_bench: needs a GPU (no CPU fallback)")
    if a.reps < 20:
        raise SystemExit("spline_bench: --reps must be >= 20")
    from ..ops import reference
    from ..ops import spline as sp
    from ..ops._ext import native

    native()
    dev = torch.device("cuda")
    B, Dh, K, bound = a.batch, a.dh, a.bins, a.bound
    P = (3 * K - 1) * Dh
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, Dh, device=dev, generator=g) * (1.6 * bound / 3)
    g_out = torch.randn(B, Dh, device=dev, generator=g)
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
        y = sp.rqs_fwd(params, x, K, bound)[0]    # a valid input for the inverse
        bytes_fwd = B * (P * es + 8 * Dh + 4)
        bytes_bwd = B * (2 * P * es + 12 * Dh + 4)

        def comp_bwd(inverse):
            # the graph is built outside the timed region: the events bracket the backward only
            def run():
                with torch.enable_grad():
                    p = params.detach().requires_grad_(True)
                    v = (y if inverse else x).detach().requires_grad_(True)
                    out, ldj = reference.rqs_transform(p, v, K, bound, inverse)
                    loss = (out * g_out).sum() + (ldj * g_ldj).sum()
                    return _event_us(lambda: torch.autograd.grad(loss, (p, v)))
            run.self_timed = True
            return run

        with torch.no_grad():
            us = _alternate({
                "fwd": lambda: sp.rqs_fwd(params, x, K, bound, False),
                "fwd_composite": lambda: reference.rqs_transform(params, x, K, bound, False),
                "inv": lambda: sp.rqs_fwd(params, y, K, bound, True),
                "inv_composite": lambda: reference.rqs_transform(params, y, K, bound, True),
                "bwd": lambda: sp.rqs_bwd(params, x, g_out, g_ldj, K, bound, False),
                "bwd_composite": comp_bwd(False),
                "bwd_inv": lambda: sp.rqs_bwd(params, y, g_out, g_ldj, K, bound, True),
                "bwd_inv_composite": comp_bwd(True),
            }, a.reps)
        gbps = {k: (bytes_bwd if k.startswith("bwd") else bytes_fwd) / (us[k] * 1e-6) / 1e9
                for k in ("fwd", "inv", "bwd", "bwd_inv")}
        print(json.dumps({
            "bench": "spline", "params": name, "B": B, "Dh": Dh, "K": K, "bound": bound,
            "reps": a.reps, "device": torch.cuda.get_device_name(0),
            "us": {k: round(v, 1) for k, v in us.items()},
            "compulsory_bytes": {"fwd": bytes_fwd, "bwd": bytes_bwd},
            "eff_GBps": {k: round(v, 1) for k, v in gbps.items()},
            "copy_GBps": round(copy_bps / 1e9, 1),
            "share_of_copy": {k: round(v * 1e9 / copy_bps, 3) for k, v in gbps.items()},
            "speedup_vs_composite": {k: round(us[k + "_composite"] / us[k], 1)
                                     for k in ("fwd", "inv", "bwd", "bwd_inv")},
        }), flush=True)
        del params, y


if __name__ == "__main__":
    main()
