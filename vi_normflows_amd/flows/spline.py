"""Rational-quadratic spline coupling layers (Durkan et al. 2019, "Neural Spline Flows").

y_a = x_a, y_b = RQS(x_b; NN(x_a)): every coordinate of the transformed half goes through its
own monotone K-bin rational-quadratic spline on (-bound, bound), the identity outside, whose
3K-1 parameters per coordinate (bin widths, bin heights, interior knot derivatives) are the
conditioner's output, plane-major [B, (3K-1) d_b]. The transform and its inverse are closed
form, so the same layer serves VI (forward) and density estimation (``log_prob`` through
``inverse``). The conditioner's last layer starts at zero, which makes every spline the
identity with ldj 0 at initialisation.

Not in the reference. The element-wise part runs in the fused HIP kernels of
``csrc/kernels/spline.hip`` on the GPU (``ops/spline.py``); conditioners are the same
``MfmaLinear`` MLPs as the affine couplings'.
"""
from __future__ import annotations

import torch
from torch import nn

from ..ops.spline import rqs_transform
from .base import Flow
from .coupling import mlp


class RQSCoupling(Flow):
    """Half-split spline coupling; ``parity`` 0 conditions on the first half, 1 on the second."""

    invertible = True

    def __init__(self, dim: int, bins: int = 8, bound: float = 3.0, hidden: int = 256,
                 n_hidden: int = 2, parity: int = 0, context_dim: int = 0):
        super().__init__()
        if not 2 <= bins <= 32:
            raise ValueError(f"RQSCoupling: need 2 <= bins <= 32, got {bins}")
        if not bound > 0:
            raise ValueError(f"RQSCoupling: need bound > 0, got {bound}")
        self.dim, self.parity, self.bins, self.bound = dim, parity, int(bins), float(bound)
        self.d_a = dim // 2 if parity == 0 else dim - dim // 2
        self.d_b = dim - self.d_a
        self.uses_context = context_dim > 0
        self.net = mlp(self.d_a + context_dim, hidden, n_hidden, (3 * self.bins - 1) * self.d_b,
                       zero_last=True)

    def _split(self, x):
        if self.parity == 0:
            return x[:, :self.d_a], x[:, self.d_a:]
        return x[:, self.d_b:], x[:, :self.d_b]

    def _join(self, a, b):
        return torch.cat([a, b], 1) if self.parity == 0 else torch.cat([b, a], 1)

    def _params(self, xa, context):
        inp = xa if context is None else torch.cat([xa, context], 1)
        return self.net(inp)

    def forward(self, x, context=None):
        xa, xb = self._split(x)
        yb, ldj = rqs_transform(self._params(xa, context), xb, self.bins, self.bound)
        return self._join(xa, yb.to(x.dtype)), ldj

    def inverse(self, y, context=None):
        ya, yb = self._split(y)
        xb, ldj = rqs_transform(self._params(ya, context), yb, self.bins, self.bound,
                                inverse=True)
        return self._join(ya, xb.to(y.dtype)), ldj


class NeuralSplineFlow(Flow):
    """Stack of alternating-parity spline couplings."""

    invertible = True

    def __init__(self, dim: int, n_layers: int = 4, bins: int = 8, bound: float = 3.0,
                 hidden: int = 256, n_hidden: int = 2, context_dim: int = 0):
        super().__init__()
        self.layers = nn.ModuleList(
            RQSCoupling(dim, bins, bound, hidden, n_hidden, parity=i % 2, context_dim=context_dim)
            for i in range(n_layers))
        self.uses_context = context_dim > 0

    def forward(self, x, context=None):
        ldj = torch.zeros(x.shape[0], device=x.device)
        for f in self.layers:
            x, l = f(x, context)
            ldj = ldj + l
        return x, ldj

    def inverse(self, y, context=None):
        ldj = torch.zeros(y.shape[0], device=y.device)
        for f in reversed(self.layers):
            y, l = f.inverse(y, context)
            ldj = ldj + l
        return y, ldj
