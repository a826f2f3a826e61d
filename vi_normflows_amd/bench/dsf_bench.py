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

import torch

from . import elementwise_bench as eb


def _transform(a):
    from ..ops import dsf as ds
    from ..ops import reference

    H = a.units

    def cases(params, x, y, g_out, g_ldj):
        def step(transform):
            def run():
                with torch.enable_grad():
                    p = params.detach().requires_grad_(True)
                    v = x.detach().requires_grad_(True)
                    out, ldj = transform(p, v, H)
                    ((out * g_out).sum() + (ldj * g_ldj).sum()).backward()
            return run

        return {
            "step": step(ds.dsf_transform),
            "step_composite": step(reference.dsf_transform),
            "fwd": lambda: ds.dsf_fwd(params, x, H, False),
            "fwd_composite": lambda: reference.dsf_transform(params, x, H, False),
            "inv": lambda: ds.dsf_fwd(params, y, H, True),
            "inv_composite": lambda: reference.dsf_transform(params, y, H, True),
            "bwd": lambda: ds.dsf_bwd(params, x, g_out, g_ldj, H, False),
            "bwd_inv": lambda: ds.dsf_bwd(params, x, g_out, g_ldj, H, True),   # x-side
        }

    return eb.Transform(
        D=a.d, planes=3 * H, x_scale=1.5, shape={"D": a.d, "H": H},
        extra={"inverse_bisections": 40},
        forward=lambda params, x: ds.dsf_fwd(params, x, H)[0], cases=cases,
        speedup=("step", "fwd", "inv"))


def main(argv=None):
    eb.run("dsf", __doc__, argv, 16384, (("--d", int, 40), ("--units", int, 8)), _transform)


if __name__ == "__main__":
    main()
