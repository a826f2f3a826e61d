"""Deep sigmoidal flow transformer (Huang et al. 2018, "Neural Autoregressive Flows"), public
wrapper.

``dsf_transform(params, x, H, inverse=False) -> (y, ldj)`` transforms every element of ``x``
[B, D] by its own monotone map y = logit(sum_h w_h sigmoid(a_h x + b_h)) with H sigmoid units;
``params`` [B, 3H D] is the plane-major conditioner output (raw slopes, shifts, mixture logits;
see ``ops/reference.py`` ``dsf_units``). GPU tensors run the fused HIP kernels of
``csrc/kernels/dsf.hip`` through an ``autograd.Function`` whose backward recomputes the units
from ``params`` and the x-side value (nothing else is saved); there is no fallback when the
native library is missing. CPU tensors run the torch composite under torch autograd.
"""
from __future__ import annotations

import torch

from . import reference
from ._ext import native, use_native


def dsf_fwd(params, x, H: int, inverse: bool = False, ldj=None):
    """Raw fused forward on GPU tensors: returns ``(y, ldj)``; a given ``ldj`` [B] is
    accumulated into instead of initialised. With ``inverse`` ``x`` holds y and the recovered
    x is returned."""
    y = torch.empty_like(x)
    init = ldj is None
    if init:
        ldj = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
    native().dsf_fwd(params, x, int(H), bool(inverse), init, y, ldj)
    return y, ldj


def dsf_bwd(params, x, g_out, g_ldj, H: int, inverse: bool = False):
    """Raw fused backward on GPU tensors: returns ``(dparams, gx)``; ``x`` is the x-side value
    in both directions (the inverse's output), ``gx`` the gradient of the direction's input."""
    dparams = torch.empty_like(params)
    gx = torch.empty_like(x)
    native().dsf_bwd(params, x, g_out, g_ldj, int(H), bool(inverse), dparams, gx)
    return dparams, gx


class _DsfFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, x, H: int, inverse: bool):
        if params.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"dsf_transform: GPU params must be fp32 or bf16, got {params.dtype}")
        pc = params.contiguous()
        xc = x.to(torch.float32).contiguous()
        y, ldj = dsf_fwd(pc, xc, H, inverse)
        ctx.save_for_backward(pc, y if inverse else xc)   # the x-side value
        ctx.H, ctx.inverse, ctx.x_dtype = H, inverse, x.dtype
        return y, ldj

    @staticmethod
    def backward(ctx, gy, gldj):
        pc, xs = ctx.saved_tensors
        gy = (gy if gy is not None else torch.zeros_like(xs)).to(torch.float32).contiguous()
        gl = (gldj if gldj is not None else torch.zeros(xs.shape[0], device=xs.device))
        gl = gl.to(torch.float32).contiguous()
        dparams, gx = dsf_bwd(pc, xs, gy, gl, ctx.H, ctx.inverse)
        return dparams, gx.to(ctx.x_dtype), None, None


def dsf_transform(params, x, H: int, inverse: bool = False):
    """Element-wise deep-sigmoidal-flow transform, differentiable w.r.t. ``params`` and ``x``.

    Returns ``(y, ldj)``: ``y`` [B, D] and the per-row log|det| [B] of the direction taken
    (fp32 on the GPU, the dtype of ``x`` on the CPU)."""
    if x.dim() != 2 or params.dim() != 2 or params.shape[0] != x.shape[0] \
            or not 1 <= H <= 32 or params.shape[1] != 3 * H * x.shape[1]:
        raise ValueError(f"dsf_transform: params {tuple(params.shape)} does not match x "
                         f"{tuple(x.shape)} with H={H} (need [B, 3H D], 1 <= H <= 32)")
    if use_native(params, x):
        return _DsfFn.apply(params, x, int(H), bool(inverse))
    return reference.dsf_transform(params, x, int(H), bool(inverse))
