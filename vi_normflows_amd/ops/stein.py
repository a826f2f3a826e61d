"""Stein operators over N particles: the SVGD direction and the kernel Stein discrepancy.

With ``f`` a function of ``r2 = |x_i - x_j|^2`` and ``s_j = grad log p(x_j)``

    phi_i = (1/N) sum_j [ f_ij s_j - 2 f'_ij (x_i - x_j) ]                       (SVGD, Liu & Wang 2016)
    u_ij  = f s_i.s_j + 2 f' (s_j - s_i).(x_i - x_j) - 2 D f' - 4 f'' r2         (Stein kernel)

for ``kernel="rbf"`` (f = exp(-r2 / h)) or ``"imq"`` (f = (h + r2)^(-1/2)); definitions:
``ops/reference.py`` ``svgd_direction_reference`` / ``ksd_rows_reference``. KSD only needs samples
and scores, so it measures the fit to an unnormalised target.

fp32 GPU tensors with D <= 64 run the all-pairs HIP kernels of ``csrc/kernels/stein.hip``:
neither N x N matrix is stored, ``x`` and ``score`` may be row-strided views, and ``h`` may be a
1-element device tensor (the median bandwidth changes every step without a host sync). The
partial sums of ``j_splits`` column ranges are added in fixed order, so a result is bitwise
repeatable for a given ``(N, D, j_splits)``; ``j_splits=None`` lets the launcher choose from
``(N, D)`` alone.

Neither op is differentiable: phi is applied as ``particles.grad = -phi`` and KSD is a
diagnostic. Both raise when an input requires grad while grad mode is on.
"""
from __future__ import annotations

import math
import re
from pathlib import Path

import torch

from . import reference
from ._ext import native
from .reference import STEIN_KINDS

MAX_DIM = 64


def _tiles():
    """The kernel's tile sizes, read from the header the kernel is compiled with."""
    hdr = Path(__file__).resolve().parents[2] / "csrc" / "include" / "stein_tiles.h"
    vals = dict(re.findall(r"#define\s+NF_STEIN_(TILE_[IJ])\s+(\d+)", hdr.read_text()))
    return int(vals["TILE_I"]), int(vals["TILE_J"])


TILE_I, TILE_J = _tiles()

_stein_launches = 0


def stein_launches(reset: bool = False) -> int:
    """Number of Stein kernel launches so far (evidence that the HIP path ran)."""
    global _stein_launches
    n = _stein_launches
    if reset:
        _stein_launches = 0
    return n


def kernel_supported(x, score) -> bool:
    """fp32 GPU tensors inside the kernel's limits."""
    return (x.is_cuda and score.is_cuda and x.dtype == torch.float32
            and score.dtype == torch.float32 and x.dim() == 2 and x.shape[0] >= 1
            and 1 <= x.shape[1] <= MAX_DIM)


def _check(name, x, score, h, kernel, impl):
    if kernel not in STEIN_KINDS:
        raise ValueError(f"{name}: kernel must be rbf or imq, got {kernel!r}")
    if impl not in ("auto", "kernel", "composite"):
        raise ValueError(f"{name}: impl must be auto, kernel or composite, got {impl!r}")
    if x.dim() != 2 or score.shape != x.shape:
        raise ValueError(f"{name}: x and score must both be [N, D], got {tuple(x.shape)} and "
                         f"{tuple(score.shape)}")
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                       for t in (x, score, h)):
        raise RuntimeError(f"{name} is not differentiable: detach the inputs or call it under "
                           "torch.no_grad()")
    if impl == "kernel" and not kernel_supported(x, score):
        raise RuntimeError(f"{name}: impl='kernel' needs fp32 GPU tensors with 1 <= D <= "
                           f"{MAX_DIM}; got {x.dtype} on {x.device} with D = {x.shape[1]}")
    return impl == "kernel" or (impl == "auto" and kernel_supported(x, score))


def _kernel_inputs(x, score, h):
    """Unit inner stride for the rows, and ``h`` as (device tensor or None, host float)."""
    x, score = x.detach(), score.detach()
    if x.shape[1] > 1 and x.stride(1) != 1:
        x = x.contiguous()
    if score.shape[1] > 1 and score.stride(1) != 1:
        score = score.contiguous()
    if isinstance(h, torch.Tensor):
        if h.numel() != 1:
            raise ValueError(f"stein: h must have one element, got {tuple(h.shape)}")
        if h.is_cuda:
            return x, score, h.detach().to(device=x.device, dtype=torch.float32).reshape(1), 1.0
        h = float(h)
    return x, score, None, float(h)


def svgd_direction(x, score, h, kernel: str = "rbf", impl: str = "auto", j_splits=None):
    """SVGD direction ``phi`` [N, D] of particles ``x`` with scores ``score``; no-grad.

    ``h`` is a float or a 1-element tensor. ``impl="auto"`` takes the HIP kernel for fp32 GPU
    tensors with D <= 64 and the torch composite otherwise; ``"kernel"`` raises outside those
    limits; ``"composite"`` is the composite on any device and dtype."""
    global _stein_launches
    if not _check("svgd_direction", x, score, h, kernel, impl):
        return reference.svgd_direction_reference(x, score, h, kernel)
    x, score, h_dev, h_host = _kernel_inputs(x, score, h)
    N, D = x.shape
    ops, js = native(), int(j_splits or 0)
    phi = torch.empty(N, D, device=x.device, dtype=torch.float32)
    work = torch.empty(ops.stein_workspace(N, D, js, 0), device=x.device, dtype=torch.float32)
    ops.stein_svgd(x, score, h_dev, h_host, STEIN_KINDS[kernel], js, phi, work)
    _stein_launches += 1
    return phi


def ksd_rows(x, score, h, kernel: str = "imq", impl: str = "auto", j_splits=None):
    """``(rows, diag)`` of the Stein kernel matrix: ``rows[i] = sum_j u_ij``, ``diag[i] = u_ii``;
    no-grad. Arguments as :func:`svgd_direction`."""
    global _stein_launches
    if not _check("ksd_rows", x, score, h, kernel, impl):
        return reference.ksd_rows_reference(x, score, h, kernel)
    x, score, h_dev, h_host = _kernel_inputs(x, score, h)
    N, D = x.shape
    ops, js = native(), int(j_splits or 0)
    rows = torch.empty(N, device=x.device, dtype=torch.float32)
    diag = torch.empty_like(rows)
    work = torch.empty(ops.stein_workspace(N, D, js, 1), device=x.device, dtype=torch.float32)
    ops.stein_ksd_rows(x, score, h_dev, h_host, STEIN_KINDS[kernel], js, rows, diag, work)
    _stein_launches += 1
    return rows, diag


def ksd_from_rows(rows, diag, stat: str = "u"):
    """Squared KSD from the row sums, reduced in fp64: the V-statistic ``sum rows / N^2`` or the
    U-statistic ``(sum rows - sum diag) / (N (N - 1))`` (unbiased; may be slightly negative)."""
    N = rows.shape[0]
    if stat == "v":
        return rows.double().sum() / (N * N)
    if stat == "u":
        if N < 2:
            raise ValueError("ksd: the U-statistic needs at least 2 samples")
        return (rows.double().sum() - diag.double().sum()) / (N * (N - 1))
    raise ValueError(f"ksd: stat must be u or v, got {stat!r}")


def ksd(x, score, h=1.0, kernel: str = "imq", stat: str = "u", impl: str = "auto"):
    """Squared kernel Stein discrepancy of samples ``x`` against the density whose score at the
    samples is ``score``, as a 0-dim fp64 tensor; no-grad."""
    if stat == "u" and x.shape[0] < 2:
        raise ValueError("ksd: the U-statistic needs at least 2 samples")
    rows, diag = ksd_rows(x, score, h, kernel, impl)
    return ksd_from_rows(rows, diag, stat)


@torch.no_grad()
def median_bandwidth(x, max_points: int = 1024):
    """Median-heuristic bandwidth ``median(r2) / log(N + 1)`` as a 1-element tensor on the device
    of ``x`` (no host sync). The median runs over the full square matrix of a subsample of at
    most ``max_points`` rows taken at a fixed stride; 1.0 when that median is 0."""
    N = x.shape[0]
    xs = x.detach()[::max(1, -(-N // max_points))]
    r2 = torch.zeros(xs.shape[0], xs.shape[0], device=x.device, dtype=x.dtype)
    for c in range(0, xs.shape[1], 8):   # 8 coordinates at a time: the temporary stays small
        d = xs[:, None, c:c + 8] - xs[None, :, c:c + 8]
        r2 += (d * d).sum(-1)
    med = r2.reshape(-1).median()
    h = med / math.log(N + 1.0)
    return torch.where(med > 0, h, torch.ones_like(h)).reshape(1)
