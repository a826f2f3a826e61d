"""Learned dense linear flows: the LU-parameterised invertible layer and the triangular affine.

``LULinear`` is the mixing layer of Glow-style and neural-spline stacks (Kingma & Dhariwal 2018;
Durkan et al. 2019): ``y = z W^T + b`` with ``W = (L U)[perm, :]``, ``L`` unit lower triangular,
``U`` upper triangular with a positive diagonal and ``perm`` a fixed permutation, so the
log-determinant is ``sum(log diag U)`` and the inverse is two triangular solves.
``TriangularAffine`` is ``z -> mu + L z`` with one lower-triangular factor: the full-rank
counterpart of ``DiagAffine``.

The forward direction composes the weight and runs ``ops.linear.linear``; the inverse is
``ops.linear_flow.lu_solve`` (``csrc/kernels/lu_solve.hip`` for fp32 GPU tensors at the shapes
where it measured at least as fast as the composite, docs/PERF_NOTES.md "LU solve").
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import nn

from ..ops.linear import linear
from ..ops.linear_flow import lu_solve
from .base import Flow

DIAG_FLOOR = 1e-3
RAW_DIAG_ONE = math.log(math.expm1(1.0 - DIAG_FLOOR))   # softplus^-1(1 - floor): diagonal 1


def positive_diag(raw: torch.Tensor) -> torch.Tensor:
    """``1e-3 + softplus(raw)``: the diagonal of ``U`` / of a scale factor."""
    return DIAG_FLOOR + F.softplus(raw)


def _expand(v: torch.Tensor, n: int) -> torch.Tensor:
    return v.float().expand(n)


class LULinear(Flow):
    """``y = (z (L U)^T)[:, perm] + bias``. ``lower`` holds ``L`` in its strict lower triangle,
    ``upper`` holds ``U`` in its strict upper triangle and ``diag(U) = 1e-3 + softplus(raw_diag)``;
    the other entries of the two matrices are not used and get no gradient. A fresh layer is
    exactly its permutation with ``ldj = 0`` (the splines' identity-at-initialisation
    convention). ``permute=False`` keeps the identity permutation."""

    invertible = True

    def __init__(self, dim: int, permute: bool = True, seed: int = 0, bias: bool = True):
        super().__init__()
        self.dim = int(dim)
        self.lower = nn.Parameter(torch.zeros(dim, dim))
        self.upper = nn.Parameter(torch.zeros(dim, dim))
        self.raw_diag = nn.Parameter(torch.full((dim,), RAW_DIAG_ONE))
        if bias:
            self.bias = nn.Parameter(torch.zeros(dim))
        else:
            self.register_parameter("bias", None)
        if permute:
            p = torch.randperm(dim, generator=torch.Generator().manual_seed(seed))
        else:
            p = torch.arange(dim)
        self.register_buffer("perm", p)
        self._perm_checked = False

    def _load_from_state_dict(self, *args, **kw):
        self._perm_checked = False
        return super()._load_from_state_dict(*args, **kw)

    def diag(self) -> torch.Tensor:
        return positive_diag(self.raw_diag)

    def packed(self) -> torch.Tensor:
        """``A``: strict lower triangle ``L``, upper triangle with the diagonal ``U``."""
        return torch.tril(self.lower, -1) + torch.triu(self.upper, 1) + torch.diag(self.diag())

    def weight(self) -> torch.Tensor:
        """The dense ``W = (L U)[perm, :]``."""
        d = self.diag()
        L = torch.tril(self.lower, -1) + torch.eye(self.dim, dtype=d.dtype, device=d.device)
        Ut = (torch.triu(self.upper, 1) + torch.diag(d)).T.contiguous()
        return linear(L, Ut)[self.perm]     # L U

    def forward(self, z, context=None):
        y = linear(z, self.weight(), self.bias)
        return y, _expand(torch.log(self.diag()).sum(), z.shape[0])

    def inverse(self, y, context=None):
        check, self._perm_checked = not self._perm_checked, True
        x = lu_solve(y, self.packed(), self.perm, self.bias, mode="lu", impl="auto",
                     check_perm=check)
        return x, _expand(-torch.log(self.diag()).sum(), y.shape[0])


class TriangularAffine(Flow):
    """``z -> mu + L z`` with ``L`` lower triangular: ``lower`` holds its strict lower triangle
    and ``diag(L) = 1e-3 + softplus(raw_diag)``. Starts at the identity. The full-rank
    counterpart of ``DiagAffine``: it turns N(0, I) into N(mu, L L^T)."""

    invertible = True

    def __init__(self, dim: int):
        super().__init__()
        self.dim = int(dim)
        self.mu = nn.Parameter(torch.zeros(dim))
        self.lower = nn.Parameter(torch.zeros(dim, dim))
        self.raw_diag = nn.Parameter(torch.full((dim,), RAW_DIAG_ONE))

    def diag(self) -> torch.Tensor:
        return positive_diag(self.raw_diag)

    def scale_tril(self) -> torch.Tensor:
        return torch.tril(self.lower, -1) + torch.diag(self.diag())

    def forward(self, z, context=None):
        y = linear(z, self.scale_tril(), self.mu)
        return y, _expand(torch.log(self.diag()).sum(), z.shape[0])

    def inverse(self, y, context=None):
        x = lu_solve(y, self.scale_tril(), None, self.mu, mode="lower", impl="auto")
        return x, _expand(-torch.log(self.diag()).sum(), y.shape[0])
