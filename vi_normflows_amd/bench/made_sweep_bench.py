"""Timing of one MAF layer's sampling direction (u -> x): the degree-sweep HIP kernel
(csrc/kernels/made_sweep.hip) and, with ``--baseline``, the sequential loop of D MADE passes it
replaces, on the same device in the same process. ``--flow dsf --units U`` times the inverse of
one ``DSFAutoregressive`` layer instead (csrc/kernels/dsf_sweep.hip against the loop of D MADE
passes and root solves that ``DSFAutoregressive.inverse`` runs when the sweep does not apply);
``--flow rqs --bins K`` the sequential direction of one ``RQSAutoregressive`` layer
(csrc/kernels/rqs_sweep.hip against the loop of D MADE passes and spline inverses).

    python -m vi_normflows_amd.bench.made_sweep_bench [--flow maf|dsf|rqs] [--units 8] [--bins 8]
        [--batch 4096] [--d 256] [--hidden 512] [--layers 1] [--reps 20] [--baseline]
        [--baseline-reps 3] [--density N] [--backward]

After a warm-up, the median of ``--reps`` HIP-event timings of the sweep; with ``--baseline`` the
loop takes turns with it for ``--baseline-reps`` reps (it is D MADE passes: keep that small).
``--density N`` adds the end-to-end time of ``MAFDensity(MAFConfig()).sample(N)`` (config 5's
64-layer model, sweep path only). ``--backward`` times the implicit gradient instead
(csrc/kernels/sweep_adjoint.hip): the adjoint sweep alone next to the forward sweep, the fp32
pieces of the backward (masked pass, element derivatives, weight-gradient products) and the whole
forward + backward of the layer with ``implicit_grad=True``; with ``--baseline`` (maf only) the
differentiable D-pass loop under autograd takes turns with it. One JSON line. Needs a GPU and the
native library: there is no fallback.
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


def backward_record(flow, u, spec, run, reps, baseline_reps):
    """Timings of the implicit gradient of one layer (see the module docstring)."""
    from ..ops import autoregressive as ar

    made = flow.made
    W = [l.weight.detach() for l in made.layers]
    b = [l.bias.detach() for l in made.layers]
    plan = ar._plan_of(made)
    P = ar._spec_planes(spec)
    masks = plan.masks(P, u.device, u.dtype)
    lbar = torch.ones(u.shape[0], device=u.device)
    with torch.no_grad():
        x, _ = run(u)
        p, hidden = ar._masked_pass(x, W, b, masks, None)
        le, d, q, c = ar._element_derivatives(spec, x, p, lbar)
        gx = torch.ones_like(x) - le
        w, pbar, a = ar.sweep_adjoint(gx, d, q, c, hidden, W, made.order, plan=plan)
        pbar_pm = pbar.transpose(1, 2).reshape(u.shape[0], -1)

        def wgrads():
            for l in range(len(W)):
                ar._wgrad(a[l] if l < len(W) - 1 else pbar_pm, x if l == 0 else hidden[l - 1],
                          masks[l])

        us = alternate({
            "forward_sweep": lambda: run(u),
            "adjoint_sweep": lambda: ar.sweep_adjoint(gx, d, q, c, hidden, W, made.order,
                                                      plan=plan),
            "masked_pass_fp32": lambda: ar._masked_pass(x, W, b, masks, None),
            "element_derivatives": lambda: ar._element_derivatives(spec, x, p, lbar),
            "weight_gradients_fp32": wgrads}, reps)
    rec = {"us": {k: round(v, 1) for k, v in us.items()},
           "adjoint_over_forward": round(us["adjoint_sweep"] / us["forward_sweep"], 2),
           "adjoint_rows_per_block": ar.adjoint_kernel_rows(
               made.dim, W[0].shape[0], len(W) - 1, P)}
    ug = u.clone().requires_grad_()

    def step(flag):
        def f():
            flow.implicit_grad = flag
            flow.zero_grad(set_to_none=True)
            ug.grad = None
            x, l = run(ug)
            (x.sum() + l.sum()).backward()
        return f

    n0 = ar.sweep_adjoint_launches()
    rec["us"]["forward_backward_implicit"] = round(alternate({"i": step(True)}, reps)["i"], 1)
    assert ar.sweep_adjoint_launches() > n0, "the implicit path did not run"
    if baseline_reps:
        ab = alternate({"implicit": step(True), "loop_autograd": step(False)}, baseline_reps,
                       warmup=1)
        rec["us_ab"] = {k: round(v, 1) for k, v in ab.items()}
        rec["baseline_reps"] = baseline_reps
        rec["speedup_vs_loop_autograd"] = round(ab["loop_autograd"] / ab["implicit"], 2)
    flow.implicit_grad = False
    return rec


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
    ap.add_argument("--backward", action="store_true",
                    help="time the implicit gradient (sweep_adjoint.hip) instead")
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
    if a.backward:
        if a.baseline and (dsf or rqs):
            raise SystemExit("made_sweep_bench: --backward --baseline needs --flow maf (the other "
                             "layers have no differentiable loop)")
        spec = (("rqs", a.bins, float(flow.bound)) if rqs else ("dsf", a.units) if dsf
                else ("made", "maf_sample", float(flow.bound), 1.0, 1.0))
        rec["bench"] = "sweep_adjoint"
        rec["flow"] = a.flow
        rec.update(backward_record(flow, u, spec, run, a.reps,
                                   a.baseline_reps if a.baseline else 0))
        print(json.dumps(rec), flush=True)
        return
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
