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

from . import _elementwise as ew
from . import reference
from ._ext import use_native

DSF = ew.Spec("dsf", "dsf_fwd", "dsf_bwd", planes=lambda H: 3 * H, x_side=True)


def dsf_fwd(params, x, H: int, inverse: bool = False, ldj=None):
    """Raw fused forward on GPU tensors: returns ``(y, ldj)``; a given ``ldj`` [B] is
    accumulated into instead of initialised. With ``inverse`` ``x`` holds y and the recovered
    x is returned."""
    return ew.fwd(DSF, params, x, (int(H),), inverse, ldj)


def dsf_bwd(params, x, g_out, g_ldj, H: int, inverse: bool = False):
    """Raw fused backward on GPU tensors: returns ``(dparams, gx)``; ``x`` is the x-side value
    in both directions (the inverse's output), ``gx`` the gradient of the direction's input."""
    return ew.bwd(DSF, params, x, g_out, g_ldj, (int(H),), inverse)


def dsf_transform(params, x, H: int, inverse: bool = False):
    """Element-wise deep-sigmoidal-flow transform, differentiable w.r.t. ``params`` and ``x``.

    Returns ``(y, ldj)``: ``y`` [B, D] and the per-row log|det| [B] of the direction taken
    (fp32 on the GPU, the dtype of ``x`` on the CPU)."""
    if x.dim() != 2 or params.dim() != 2 or params.shape[0] != x.shape[0] \
            or not 1 <= H <= 32 or params.shape[1] != DSF.planes(H) * x.shape[1]:
        raise ValueError(f"dsf_transform: params {tuple(params.shape)} does not match x "
                         f"{tuple(x.shape)} with H={H} (need [B, 3H D], 1 <= H <= 32)")
    if use_native(params, x):
        return ew.ElementwiseFn.apply(params, x, DSF, (int(H),), bool(inverse))
    return reference.dsf_transform(params, x, int(H), bool(inverse))
