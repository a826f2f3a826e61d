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

from . import _elementwise as ew
from . import reference
from ._ext import use_native

RQS = ew.Spec("rqs", "rqs_fwd", "rqs_bwd", planes=lambda K: 3 * K - 1, x_side=False)


def rqs_fwd(params, x, K: int, bound: float, inverse: bool = False, ldj=None):
    """Raw fused forward on GPU tensors: returns ``(y, ldj)``; a given ``ldj`` [B] is
    accumulated into instead of initialised."""
    return ew.fwd(RQS, params, x, (int(K), float(bound)), inverse, ldj)


def rqs_bwd(params, x, g_out, g_ldj, K: int, bound: float, inverse: bool = False):
    """Raw fused backward on GPU tensors: returns ``(dparams, gx)``; ``x`` is the input of the
    direction taken."""
    return ew.bwd(RQS, params, x, g_out, g_ldj, (int(K), float(bound)), inverse)


def rqs_transform(params, x, K: int, bound: float, inverse: bool = False):
    """Element-wise RQ-spline transform, differentiable w.r.t. ``params`` and ``x``.

    Returns ``(y, ldj)``: ``y`` [B, Dh] and the per-row log|det| [B] of the direction taken
    (fp32 on the GPU, the dtype of ``x`` on the CPU)."""
    if x.dim() != 2 or params.dim() != 2 or params.shape[0] != x.shape[0] \
            or params.shape[1] != RQS.planes(K) * x.shape[1]:
        raise ValueError(f"rqs_transform: params {tuple(params.shape)} does not match x "
                         f"{tuple(x.shape)} with K={K} (need [B, (3K-1) Dh])")
    if use_native(params, x):
        return ew.ElementwiseFn.apply(params, x, RQS, (int(K), float(bound)), bool(inverse))
    return reference.rqs_transform(params, x, int(K), float(bound), bool(inverse))
