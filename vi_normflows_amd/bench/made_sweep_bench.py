"""Timing of one MAF layer's sampling direction (u -> x): the degree-sweep HIP kernel
(csrc/kernels/made_sweep.hip) and, with ``--baseline``, the sequential loop of D MADE passes it
replaces, on the same device in the same process. ``--flow dsf --units U`` times the inverse of
one ``DSFAutoregressive`` layer instead (csrc/kernels/dsf_sweep.hip against the loop of D MADE
passes and root solves that ``DSFAutoregressive.inverse`` runs when the sweep does not apply);
``--flow rqs --bins K`` the sequential direction of one ``RQSAutoregressive`` layer
(csrc/kernels/rqs_sweep.hip against the loop of D MADE passes and spline inverses).

    python -m vi_normflows_amd.bench.made_sweep_bench [--flow maf|dsf|rqs] [--units 8] [--bins 8]
        [--batch 4096] [--d 256] [--hidden 512] [--layers 1] [--reps 20] [--baseline]
        [--baseline-reps 3] [--density N]

After a warm-up, the median of ``--reps`` HIP-event timings of the sweep; with ``--baseline`` the
loop takes turns with it for ``--baseline-reps`` reps (it is D MADE passes: keep that small).
``--density N`` adds the end-to-end time of ``MAFDensity(MAFConfig()).sample(N)`` (config 5's
64-layer model, sweep path only). One JSON line. Needs a GPU and the native library: there is no
fallback.
"""
from __future__ import annotations

import argparse
import json
import statistics

import torch

from .timing import alternate, event_us


def sequential_sample(flow, u):
    """The D-pass loop of ``MAF.forward`` (what runs when the sweep does not apply)."""
    x = torch.zeros_like(u)
    for i in torch.argsort(flow.made.order).tolist():
        mu, alpha = flow._mu_alpha(x, None)
        x = x.clone()
        x[:, i] = u[:, i] * torch.exp(alpha[:, i]) + mu[:, i]
    _, ldj_inv = flow.inverse(x, None)
    return x, -ldj_inv


def sequential_dsf_inverse(flow, y):
    """The D-pass loop of ``DSFAutoregressive.inverse`` (what runs when the sweep does not
    apply)."""
    from ..ops.dsf import dsf_transform

    z = torch.zeros_like(y)
    for i in torch.argsort(flow.made.order).tolist():
        p_i = flow.made(z, None)[:, :, i].contiguous()
        z[:, i] = dsf_transform(p_i, y[:, i:i + 1].contiguous(), flow.units,
                                inverse=True)[0][:, 0].to(y.dtype)
    _, ldj = flow.forward(z, None)
    return z, -ldj


def sequential_rqs_inverse(flow, y):
    """The D-pass loop of ``RQSAutoregressive``'s sequential direction (what runs when the sweep
    does not apply)."""
    from ..ops.spline import rqs_transform

    z = torch.zeros_like(y)
    for i in torch.argsort(flow.made.order).tolist():
        p_i = flow.made(z, None)[:, :, i].contiguous()
        z[:, i] = rqs_transform(p_i, y[:, i:i + 1].contiguous(), flow.bins, flow.bound,
                                inverse=True)[0][:, 0].to(y.dtype)
    _, ldj = flow.forward(z, None)
    return z, -ldj


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--flow", choices=("maf", "dsf", "rqs"), default="maf")
    ap.add_argument("--units", type=int, default=8, help="sigmoid units per coordinate (dsf)")
    ap.add_argument("--bins", type=int, default=8, help="spline bins per coordinate (rqs)")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--layers", type=int, default=1, help="hidden layers of the MADE")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--baseline-reps", type=int, default=3)
    ap.add_argument("--density", type=int, default=0)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("made_sweep_bench: needs a GPU (no CPU fallback)")
    from ..flows.made import MAF
    from ..flows.naf import DSFAutoregressive
    from ..flows.spline import RQSAutoregressive
    from ..ops import autoregressive as ar
    from ..ops._ext import native

    native()
    dev = torch.device("cuda")
    B, D, H, L = a.batch, a.d, a.hidden, a.layers
    torch.manual_seed(0)
    dsf, rqs = a.flow == "dsf", a.flow == "rqs"
    if rqs:
        flow = RQSAutoregressive(D, a.bins, hidden=H, n_hidden=L).to(dev)
    else:
        flow = (DSFAutoregressive(D, a.units, H, L) if dsf else MAF(D, H, L)).to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():   # well-conditioned, not near-identity: N(0, 1) * 0.7 / sqrt(fan_in)
        for layer in flow.made.layers:
            layer.weight.copy_(torch.randn(layer.weight.shape, device=dev, generator=g)
                               * 0.7 / layer.weight.shape[1] ** 0.5)
            layer.bias.copy_(torch.randn(layer.bias.shape, device=dev, generator=g) * 0.3)
    u = torch.randn(B, D, device=dev, generator=g)
    rec = {"bench": "rqs_sweep" if rqs else "dsf_sweep" if dsf else "made_sweep", "B": B, "D": D,
           "H": H, "L": L, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "rows_per_block": (ar.rqs_kernel_rows(D, H, L, a.bins) if rqs
                              else ar.dsf_kernel_rows(D, H, L, a.units) if dsf
                              else ar.kernel_rows(D, H, L))}
    if dsf:
        rec["units"] = a.units
    if rqs:
        rec["bins"] = a.bins
    run = flow.inverse if dsf or rqs else flow
    sequential = (sequential_rqs_inverse if rqs else sequential_dsf_inverse if dsf
                  else sequential_sample)
    with torch.no_grad():
        assert ar.dispatch(flow, u, None), "shape outside the sweep kernel's limits"
        fns = {"sweep": lambda: run(u)}
        if a.baseline:
            for _ in range(3):
                run(u)
            us = alternate({**fns, "sequential": lambda: sequential(flow, u)},
                           a.baseline_reps, warmup=1)
            rec["us_ab"] = {k: round(v, 1) for k, v in us.items()}
            rec["baseline_reps"] = a.baseline_reps
            rec["speedup_vs_sequential"] = round(us["sequential"] / us["sweep"], 1)
            # the loop runs the MADE products in bf16: how far its sample is from the sweep's
            rec["max_abs_diff_vs_sequential"] = float(
                (run(u)[0] - sequential(flow, u)[0]).abs().max())
        rec["us"] = round(alternate(fns, a.reps)["sweep"], 1)
        rec["rows_per_s"] = round(B / rec["us"] * 1e6)
        if a.density:
            from ..models.maf_density import MAFConfig, MAFDensity

            model = MAFDensity(MAFConfig()).to(dev)
            model.sample(a.density, generator=g)
            t = [event_us(lambda: model.sample(a.density, generator=g)) for _ in range(5)]
            rec["density_sample"] = {"n": a.density, "layers": model.cfg.n_layers,
                                     "dim": model.cfg.dim,
                                     "ms": round(statistics.median(t) / 1e3, 2)}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
