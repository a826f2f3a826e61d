"""Shared GPU path of the element-wise flow transforms (``ops/spline.py``, ``ops/dsf.py``).

Each is a monotone map over ``x`` [B, D] with plane-major ``params`` [B, planes D] (fp32 or
bf16), run by a pair of fused HIP kernels on the frame of ``csrc/include/elementwise_flow.h``:
``<name>_fwd(params, x, *scalars, inverse, ldj_init, y, ldj)`` and ``<name>_bwd(params, x,
g_out, g_ldj, *scalars, inverse, dparams, gx)``. A ``Spec`` names one transform; ``fwd`` / ``bwd``
are the raw pair and ``ElementwiseFn`` the one ``autograd.Function`` over them. Its backward
saves nothing but ``params`` and one [B, D] tensor; there is no fallback when the native library
is missing.
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import torch

from ._ext import native


class Spec(NamedTuple):
    name: str                      # public prefix, for messages
    fwd: str                       # native op names
    bwd: str
    planes: Callable[[int], int]   # planes per element from the count (bins, units)
    x_side: bool                   # the backward is fed the x-side value (the inverse's output)
    #                                instead of the input of the direction taken


def fwd(spec: Spec, params, x, scalars: tuple, inverse: bool, ldj=None):
    y = torch.empty_like(x)
    init = ldj is None
    if init:
        ldj = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
    getattr(native(), spec.fwd)(params, x, *scalars, bool(inverse), init, y, ldj)
    return y, ldj


def bwd(spec: Spec, params, x, g_out, g_ldj, scalars: tuple, inverse: bool):
    dparams = torch.empty_like(params)
    gx = torch.empty_like(x)
    getattr(native(), spec.bwd)(params, x, g_out, g_ldj, *scalars, bool(inverse), dparams, gx)
    return dparams, gx


class ElementwiseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, x, spec: Spec, scalars: tuple, inverse: bool):
        if params.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"{spec.name}_transform: GPU params must be fp32 or bf16, "
                            f"got {params.dtype}")
        pc = params.contiguous()
        xc = x.to(torch.float32).contiguous()
        y, ldj = fwd(spec, pc, xc, scalars, inverse)
        ctx.save_for_backward(pc, y if spec.x_side and inverse else xc)
        ctx.spec, ctx.scalars, ctx.inverse, ctx.x_dtype = spec, scalars, inverse, x.dtype
        return y, ldj

    @staticmethod
    def backward(ctx, gy, gldj):
        # gradients are materialised (the default): an unused output arrives as zeros
        pc, xs = ctx.saved_tensors
        dparams, gx = bwd(ctx.spec, pc, xs, gy.to(torch.float32).contiguous(),
                          gldj.to(torch.float32).contiguous(), ctx.scalars, ctx.inverse)
        return dparams, gx.to(ctx.x_dtype), None, None, None
