"""Sylvester normalizing flows (van den Berg, Hasenclever, Tomczak, Welling, UAI 2018).

The rank-D generalisation of the planar layer, with M = D:

    z' = z + Q (d1 * h + R1 h),   h = tanh(d2 * Q^T z + R2 Q^T z + b),
    log|det J| = sum_i log|1 + (1 - h_i^2) d1_i d2_i|

R1, R2 strictly upper triangular, d1 = tanh(raw), d2 = tanh(raw) so that |d1 d2| < 1 and the
layer is invertible, Q orthogonal:

* ``basis="householder"`` (H-SNF): Q = H_1 ... H_H, a product of ``householders`` reflections
  H_h = I - 2 v_h v_h^T / v_h.v_h;
* ``basis="triangular"`` (T-SNF): no reflections, Q alternates between the identity and the
  coordinate reversal from layer to layer.

The squashing of the raw diagonals is plain torch (differentiated by autograd, like ``get_uhat``
for planar); everything else of the K-layer stack is one fused HIP kernel on the GPU
(``csrc/kernels/sylvester.hip`` through ``ops/sylvester.py``), the torch composite on the CPU.
Not in the reference.
"""
from __future__ import annotations

import torch
from torch import nn

from ..ops.sylvester import sylvester_stack
from .base import Flow

BASES = ("householder", "triangular")


def _basis(K: int, householders: int, basis: str):
    """(H, flips) of a K-layer stack."""
    if basis not in BASES:
        raise ValueError(f"sylvester: basis must be one of {BASES}, got {basis!r}")
    if basis == "triangular":
        return 0, [k % 2 for k in range(K)]
    if not 1 <= householders <= 16:
        raise ValueError(f"sylvester: need 1 <= householders <= 16, got {householders}")
    return int(householders), [0] * K


class SylvesterStack(Flow):
    """K Sylvester layers with shared (non-amortized) parameters."""

    def __init__(self, dim: int, K: int, householders: int = 1, basis: str = "householder",
                 impl: str = "auto", generator=None):
        super().__init__()
        self.dim, self.K, self.basis, self.impl = dim, K, basis, impl
        self.householders, self.flips = _basis(K, householders, basis)
        P, H = dim * (dim - 1) // 2, self.householders

        def small(*shape):
            return nn.Parameter(torch.randn(*shape, generator=generator) * 0.01)

        self.R1, self.R2 = small(K, P), small(K, P)
        self.d1_raw, self.d2_raw, self.b = small(K, dim), small(K, dim), small(K, dim)
        self.V = nn.Parameter(torch.randn(K, H, dim, generator=generator))

    def forward(self, z, context=None):
        return sylvester_stack(z, self.R1, self.R2, torch.tanh(self.d1_raw),
                               torch.tanh(self.d2_raw), self.b, self.V, self.flips, self.impl)


class AmortizedSylvester(Flow):
    """Sylvester stack whose parameters come from an inference network, one set per sample.

    ``forward(z, params)`` with ``params = split(phi_block)``: the ``param_width()`` flow
    columns of an encoder output [N, ...], laid out per row as
    ``[R1 (K P) | R2 (K P) | d1_raw (K D) | d2_raw (K D) | b (K D) | V (K H D)]`` with
    P = D (D - 1) / 2. ``split`` returns views ``[N, K, ...]`` of the block (no copy); the
    kernel reads them in place through their row stride.
    """

    uses_context = True

    def __init__(self, dim: int, K: int, householders: int = 1, basis: str = "householder",
                 impl: str = "auto"):
        super().__init__()
        self.dim, self.K, self.basis, self.impl = dim, K, basis, impl
        self.householders, self.flips = _basis(K, householders, basis)

    def _widths(self):
        D, K, H = self.dim, self.K, self.householders
        P = D * (D - 1) // 2
        return [K * P, K * P, K * D, K * D, K * D, K * H * D]

    def param_width(self) -> int:
        return sum(self._widths())

    def split(self, phi_block):
        N = phi_block.shape[0]
        if phi_block.shape[1] != self.param_width():
            raise ValueError(f"AmortizedSylvester: block has {phi_block.shape[1]} columns, "
                             f"expected {self.param_width()}")
        out, o = [], 0
        for i, w in enumerate(self._widths()):
            blk = phi_block[:, o:o + w]
            out.append(blk.unflatten(1, (self.K, self.householders, self.dim) if i == 5
                                     else (self.K, w // self.K)))
            o += w
        return tuple(out)

    def forward(self, z, context=None):
        R1, R2, d1_raw, d2_raw, b, V = context
        return sylvester_stack(z, R1, R2, torch.tanh(d1_raw), torch.tanh(d2_raw), b, V,
                               self.flips, self.impl)


__all__ = ["SylvesterStack", "AmortizedSylvester", "BASES"]
