"""Sylvester normalizing-flow stack (van den Berg et al. 2018), public wrapper.

``sylvester_stack(z, R1, R2, d1, d2, b, V, flips, impl="auto") -> (z_K, ldj)`` runs K layers

    t = Q^T z,  h = tanh(d2 * t + R2 t + b),  z' = z + Q (d1 * h + R1 h),
    ldj += sum_i log(|1 + (1 - h_i^2) d1_i d2_i| + 1e-7),   Q = P^flip H_1 ... H_H

(definition: ``ops/reference.py`` ``sylvester_stack_reference``). ``R1`` / ``R2`` are strictly
upper triangular and packed by column, entry (i, j), i < j, at index ``j (j - 1) / 2 + i``
(:func:`tri_pack` / :func:`tri_unpack`); ``d1`` / ``d2`` are the squashed diagonals. Parameters
are shared ``[K, ...]`` or per-sample ``[N, K, ...]`` (sample-major, the row layout of an
encoder output), ``V`` is ``[.., K, H, D]``.

fp32 GPU tensors with 1 <= D <= 64 and 0 <= H <= 16 run the fused HIP kernels of
``csrc/kernels/sylvester.hip`` through an ``autograd.Function``. The ops take a row stride per
parameter tensor, so per-sample views with a dense ``[K, ...]`` block per row (column slices of
an encoder output reshaped to ``[N, K, ...]``) reach the kernel without a copy, and a shared
parameter is row stride 0. For shared parameters the backward kernel's per-row gradients are
produced and summed in row chunks of at most ``SHARED_GRAD_BUDGET_BYTES``: always in blocks of
``SHARED_GRAD_BLOCK_ROWS`` rows, each block summed on its own and the block sums summed once at
the end, so the result does not depend on the chunking and is bitwise repeatable.
"""
from __future__ import annotations

import torch

from . import reference
from ._ext import native
from .reference import tri_index, tri_pack, tri_unpack  # noqa: F401  (public here)

MAX_DIM = 64
MAX_HOUSEHOLDERS = 16
# per-row gradient buffer of the shared-parameter backward: at most this many bytes at a time
# (never less than one block of rows)
SHARED_GRAD_BUDGET_BYTES = 64 << 20
SHARED_GRAD_BLOCK_ROWS = 256

_PARAMS = ("R1", "R2", "d1", "d2", "b", "V")


def _widths(D: int, H: int):
    P = D * (D - 1) // 2
    return (P, P, D, D, D, H * D)


def _per_row(t, name):
    return t.dim() == (4 if name == "V" else 3)


def _row_dense(t, per_row: bool):
    """True when the [K, ...] block of a row is dense (what the ops require)."""
    inner = t[0] if per_row else t
    return inner.numel() == 0 or inner.is_contiguous()


def kernel_supported(z, R1, R2, d1, d2, b, V) -> bool:
    """fp32 GPU tensors inside the kernel's limits."""
    ts = (z, R1, R2, d1, d2, b, V)
    return (all(t.is_cuda and t.dtype == torch.float32 for t in ts) and z.dim() == 2
            and 1 <= z.shape[1] <= MAX_DIM and V.shape[-2] <= MAX_HOUSEHOLDERS
            and d1.shape[-2] >= 1)


def sylvester_fwd(z, R1, R2, d1, d2, b, V, flips, save: bool = True):
    """Raw fused forward on GPU tensors: ``(z_K, ldj, saved)`` with ``saved`` [N, K, D] the
    input of every layer (empty with ``save=False``)."""
    N, D = z.shape
    K = d1.shape[-2]
    zK = torch.empty_like(z)
    ldj = torch.empty(N, device=z.device, dtype=torch.float32)
    saved = torch.empty((N, K, D) if save else (0,), device=z.device, dtype=torch.float32)
    native().sylvester_fwd(z, R1, R2, d1, d2, b, V, [int(bool(f)) for f in flips], zK, ldj, saved)
    return zK, ldj, saved


def sylvester_bwd(saved, R1, R2, d1, d2, b, V, flips, gz, gl, grads=None, dz=None):
    """Raw fused backward on GPU tensors: ``(dz, (dR1, dR2, dd1, dd2, db, dV))`` with per-row
    gradients ``[N, K, ...]``; ``grads`` may supply the six output tensors (row-strided views
    with dense inner dimensions are allowed) and ``dz`` the dense [N, D] one."""
    N, K, D = saved.shape
    H = V.shape[-2]
    if grads is None:
        grads = tuple(torch.empty((N, K, H, D) if n == "V" else (N, K, w), device=saved.device,
                                  dtype=torch.float32)
                      for n, w in zip(_PARAMS, _widths(D, H)))
    if dz is None:
        dz = torch.empty(N, D, device=saved.device, dtype=torch.float32)
    native().sylvester_bwd(saved, R1, R2, d1, d2, b, V, [int(bool(f)) for f in flips], gz, gl, dz,
                           *grads)
    return dz, grads


def _shared_grads(saved, params, flips, gz, gl, shared):
    """Backward with some parameters shared: per-row gradients of all six parameters go to one
    [rows, W] buffer per chunk; shared ones are summed block by block (fixed blocks of
    SHARED_GRAD_BLOCK_ROWS rows, whatever the chunk size), per-sample ones copied out."""
    N, K, D = saved.shape
    H = params[5].shape[-2]
    widths = [K * w for w in _widths(D, H)]
    W = -(-sum(widths) // 4) * 4   # rows stay 16-byte aligned: every block sum runs alike
    blk = SHARED_GRAD_BLOCK_ROWS
    rows = max(blk, SHARED_GRAD_BUDGET_BYTES // max(4 * W, 1) // blk * blk)
    rows = min(rows, -(-N // blk) * blk)
    dev = saved.device
    buf = torch.empty(min(rows, N), W, device=dev, dtype=torch.float32)
    nblk = -(-N // blk)
    part = torch.empty(nblk, W, device=dev, dtype=torch.float32)
    dz = torch.empty(N, D, device=dev, dtype=torch.float32)
    dense = [None if s else torch.empty((N, K, H, D) if n == "V" else (N, K, w // K), device=dev,
                                        dtype=torch.float32)
             for n, w, s in zip(_PARAMS, widths, shared)]
    offs = [sum(widths[:i]) for i in range(6)]
    for r0 in range(0, N, rows):
        r1 = min(r0 + rows, N)
        n = r1 - r0
        views = []
        for name, w, o in zip(_PARAMS, widths, offs):
            v = buf[:n, o:o + w]
            views.append(v.view(n, K, H, D) if name == "V" else v.view(n, K, w // K))
        ps = [p if s else p[r0:r1] for p, s in zip(params, shared)]
        sylvester_bwd(saved[r0:r1], *ps, flips, gz[r0:r1], gl[r0:r1], grads=views, dz=dz[r0:r1])
        for c0 in range(0, n, blk):
            torch.sum(buf[c0:min(c0 + blk, n)], 0, out=part[(r0 + c0) // blk])
        for d, v in zip(dense, views):
            if d is not None:
                d[r0:r1] = v
    total = part.sum(0)
    out = []
    for name, w, o, s, d in zip(_PARAMS, widths, offs, shared, dense):
        if s:
            t = total[o:o + w]
            out.append(t.view(K, H, D) if name == "V" else t.view(K, w // K))
        else:
            out.append(d)
    return dz, tuple(out)


class _SylvesterFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, R1, R2, d1, d2, b, V, flips):
        params = []
        for name, t in zip(_PARAMS, (R1, R2, d1, d2, b, V)):
            # strided per-sample views go through untouched; anything else is made dense
            params.append(t if _row_dense(t, _per_row(t, name)) else t.contiguous())
        zc = z.contiguous()
        zK, ldj, saved = sylvester_fwd(zc, *params, flips)
        ctx.save_for_backward(saved, *params)
        ctx.flips = tuple(flips)
        return zK, ldj

    @staticmethod
    def backward(ctx, gz, gldj):
        saved, *params = ctx.saved_tensors
        N, K, D = saved.shape
        gz = (gz if gz is not None else torch.zeros(N, D, device=saved.device)).contiguous()
        gl = (gldj if gldj is not None else torch.zeros(N, device=saved.device)).contiguous()
        shared = [not _per_row(t, n) for n, t in zip(_PARAMS, params)]
        if any(shared):
            dz, grads = _shared_grads(saved, params, ctx.flips, gz, gl, shared)
        else:
            dz, grads = sylvester_bwd(saved, *params, ctx.flips, gz, gl)
        return (dz, *grads, None)


def sylvester_stack(z, R1, R2, d1, d2, b, V, flips, impl: str = "auto"):
    """K Sylvester layers, differentiable in every tensor argument; returns ``(z_K, ldj[N])``.

    ``impl="auto"`` takes the fused kernel for fp32 GPU tensors inside its limits and the torch
    composite otherwise; ``"kernel"`` insists on the kernel (the op raises outside its limits,
    and there is no fallback when the native library is missing); ``"composite"`` is the torch
    composite on any device and dtype."""
    if impl not in ("auto", "kernel", "composite"):
        raise ValueError(f"sylvester_stack: impl must be auto, kernel or composite, got {impl!r}")
    flips = [bool(f) for f in flips]
    if impl == "kernel" or (impl == "auto" and kernel_supported(z, R1, R2, d1, d2, b, V)):
        return _SylvesterFn.apply(z, R1, R2, d1, d2, b, V, flips)
    return reference.sylvester_stack_reference(z, R1, R2, d1, d2, b, V, flips)
