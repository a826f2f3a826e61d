"""Rational-quadratic spline coupling transform (Durkan et al. 2019), public wrapper.

``rqs_transform(params, x, K, bound, inverse=False) -> (y, ldj)`` transforms every element of
``x`` [B, Dh] by its own monotone K-bin spline on (-bound, bound) with linear tails outside;
``params`` [B, (3K-1) Dh] is the plane-major conditioner output (widths, heights, interior
derivatives; see ``ops/reference.py`` ``rqs_knots``). GPU tensors run the fused HIP kernels of
``csrc/kernels/spline.hip`` through an ``autograd.Function`` whose backward recomputes the
spline from ``params`` and the input (nothing else is saved); there is no fallback when the
native library is missing. CPU tensors run the torch composite under torch autograd.
"""
from __future__ import annotations

import torch

from . import reference
from ._ext import native, use_native


def rqs_fwd(params, x, K: int, bound: float, inverse: bool = False, ldj=None):
    """Raw fused forward on GPU tensors: returns ``(y, ldj)``; a given ``ldj`` [B] is
    accumulated into instead of initialised."""
    y = torch.empty_like(x)
    init = ldj is None
    if init:
        ldj = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
    native().rqs_fwd(params, x, int(K), float(bound), bool(inverse), init, y, ldj)
    return y, ldj


def rqs_bwd(params, x, g_out, g_ldj, K: int, bound: float, inverse: bool = False):
    """Raw fused backward on GPU tensors: returns ``(dparams, gx)``; ``x`` is the input of the
    direction taken."""
    dparams = torch.empty_like(params)
    gx = torch.empty_like(x)
    native().rqs_bwd(params, x, g_out, g_ldj, int(K), float(bound), bool(inverse), dparams, gx)
    return dparams, gx


class _RqsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, x, K: int, bound: float, inverse: bool):
        if params.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"rqs_transform: GPU params must be fp32 or bf16, got {params.dtype}")
        pc = params.contiguous()
        xc = x.to(torch.float32).contiguous()
        y, ldj = rqs_fwd(pc, xc, K, bound, inverse)
        ctx.save_for_backward(pc, xc)
        ctx.K, ctx.bound, ctx.inverse, ctx.x_dtype = K, bound, inverse, x.dtype
        return y, ldj

    @staticmethod
    def backward(ctx, gy, gldj):
        pc, xc = ctx.saved_tensors
        gy = (gy if gy is not None else torch.zeros_like(xc)).to(torch.float32).contiguous()
        gl = (gldj if gldj is not None else torch.zeros(xc.shape[0], device=xc.device))
        gl = gl.to(torch.float32).contiguous()
        dparams, gx = rqs_bwd(pc, xc, gy, gl, ctx.K, ctx.bound, ctx.inverse)
        return dparams, gx.to(ctx.x_dtype), None, None, None


def rqs_transform(params, x, K: int, bound: float, inverse: bool = False):
    """Element-wise RQ-spline transform, differentiable w.r.t. ``params`` and ``x``.

    Returns ``(y, ldj)``: ``y`` [B, Dh] and the per-row log|det| [B] of the direction taken
    (fp32 on the GPU, the dtype of ``x`` on the CPU)."""
    if x.dim() != 2 or params.dim() != 2 or params.shape[0] != x.shape[0] \
            or params.shape[1] != (3 * K - 1) * x.shape[1]:
        raise ValueError(f"rqs_transform: params {tuple(params.shape)} does not match x "
                         f"{tuple(x.shape)} with K={K} (need [B, (3K-1) Dh])")
    if use_native(params, x):
        return _RqsFn.apply(params, x, int(K), float(bound), bool(inverse))
    return reference.rqs_transform(params, x, int(K), float(bound), bool(inverse))
