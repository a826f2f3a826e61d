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

import torch

from . import elementwise_bench as eb
from .timing import event_us


def _transform(a):
    from ..ops import reference
    from ..ops import spline as sp

    K, bound = a.bins, a.bound

    def cases(params, x, y, g_out, g_ldj):
        def comp_bwd(inverse):
            # the graph is built outside the timed region: the events bracket the backward only
            def run():
                with torch.enable_grad():
                    p = params.detach().requires_grad_(True)
                    v = (y if inverse else x).detach().requires_grad_(True)
                    out, ldj = reference.rqs_transform(p, v, K, bound, inverse)
                    loss = (out * g_out).sum() + (ldj * g_ldj).sum()
                    return event_us(lambda: torch.autograd.grad(loss, (p, v)))
            run.self_timed = True
            return run

        return {
            "fwd": lambda: sp.rqs_fwd(params, x, K, bound, False),
            "fwd_composite": lambda: reference.rqs_transform(params, x, K, bound, False),
            "inv": lambda: sp.rqs_fwd(params, y, K, bound, True),
            "inv_composite": lambda: reference.rqs_transform(params, y, K, bound, True),
            "bwd": lambda: sp.rqs_bwd(params, x, g_out, g_ldj, K, bound, False),
            "bwd_composite": comp_bwd(False),
            "bwd_inv": lambda: sp.rqs_bwd(params, y, g_out, g_ldj, K, bound, True),
            "bwd_inv_composite": comp_bwd(True),
        }

    return eb.Transform(
        D=a.dh, planes=3 * K - 1, x_scale=1.6 * bound / 3,
        shape={"Dh": a.dh, "K": K, "bound": bound}, extra={},
        forward=lambda params, x: sp.rqs_fwd(params, x, K, bound)[0], cases=cases,
        speedup=eb.KERNELS)


def main(argv=None):
    eb.run("spline", __doc__, argv, 65536,
           (("--dh", int, 392), ("--bins", int, 8), ("--bound", float, 3.0)), _transform)


if __name__ == "__main__":
    main()
