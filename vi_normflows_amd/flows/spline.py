"""Rational-quadratic spline layers (Durkan et al. 2019, "Neural Spline Flows"): couplings and
MADE-conditioned autoregressive layers.

y_a = x_a, y_b = RQS(x_b; NN(x_a)): every coordinate of the transformed half goes through its
own monotone K-bin rational-quadratic spline on (-bound, bound), the identity outside, whose
3K-1 parameters per coordinate (bin widths, bin heights, interior knot derivatives) are the
conditioner's output, plane-major [B, (3K-1) d_b]. The transform and its inverse are closed
form, so the same layer serves VI (forward) and density estimation (``log_prob`` through
``inverse``). The conditioner's last layer starts at zero, which makes every spline the
identity with ldj 0 at initialisation.

``RQSAutoregressive`` / ``MaskedSplineFlow`` are RQ-NSF (AR) of the same paper: the spline's
parameters come from a MADE, so one direction is one pass and the other solves coordinate by
coordinate in degree order - on the GPU one degree sweep (``csrc/kernels/rqs_sweep.hip``,
``ops/autoregressive.py``) instead of D MADE passes.

Not in the reference. The element-wise part runs in the fused HIP kernels of
``csrc/kernels/spline.hip`` on the GPU (``ops/spline.py``); the couplings' conditioners are the
same ``MfmaLinear`` MLPs as the affine couplings'.
"""
from __future__ import annotations

import torch
from torch import nn

from ..ops.spline import rqs_transform
from .base import Flow, Reverse
from .coupling import mlp
from .made import MADE


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
    """Stack of alternating-parity spline couplings. ``linear="lu"`` puts an ``LULinear``
    (seeded by its position) before every coupling, as in neural spline flows; the default
    ``None`` has the couplings alone."""

    invertible = True

    def __init__(self, dim: int, n_layers: int = 4, bins: int = 8, bound: float = 3.0,
                 hidden: int = 256, n_hidden: int = 2, context_dim: int = 0, linear=None):
        super().__init__()
        if linear not in (None, "lu"):
            raise ValueError(f"NeuralSplineFlow: linear must be None or 'lu', got {linear!r}")
        self.layers = nn.ModuleList(
            RQSCoupling(dim, bins, bound, hidden, n_hidden, parity=i % 2, context_dim=context_dim)
            for i in range(n_layers))
        if linear == "lu":
            from .linear import LULinear

            self.linears = nn.ModuleList(LULinear(dim, seed=i) for i in range(n_layers))
        else:
            self.linears = None
        self.uses_context = context_dim > 0

    def forward(self, x, context=None):
        ldj = torch.zeros(x.shape[0], device=x.device)
        for i, f in enumerate(self.layers):
            if self.linears is not None:
                x, l = self.linears[i](x)
                ldj = ldj + l
            x, l = f(x, context)
            ldj = ldj + l
        return x, ldj

    def inverse(self, y, context=None):
        ldj = torch.zeros(y.shape[0], device=y.device)
        for i in reversed(range(len(self.layers))):
            y, l = self.layers[i].inverse(y, context)
            ldj = ldj + l
            if self.linears is not None:
                y, l = self.linears[i].inverse(y)
                ldj = ldj + l
        return y, ldj


class RQSAutoregressive(Flow):
    """MADE-conditioned spline layer: MAF / IAF with the affine transformer replaced by the
    rational-quadratic spline. ``T(x) = RQS(x; MADE(x))`` is one differentiable pass; the other
    direction solves ``T(z) = y`` coordinate by coordinate in degree order, without a graph.

    ``density=False`` (VI, like ``IAF`` / ``DSFAutoregressive``): ``forward`` is the one-pass
    ``T`` and ``inverse`` the sequential solve. ``density=True`` (like ``MAF``): ``inverse`` is the
    one-pass ``T``, so ``FlowDistribution.log_prob`` trains by maximum likelihood in one pass, and
    ``forward`` is the sequential solve used for sampling. Either method returns the log|det| of
    the map it applies: ``ldj_T(x)`` with ``T(x)``, ``-ldj_T(z)`` with the solve. The MADE's last
    layer starts small (1e-2 of its default), so the layer starts near the identity."""

    invertible = True

    def __init__(self, dim: int, bins: int = 8, bound: float = 3.0, hidden: int = 64,
                 n_hidden: int = 1, context_dim: int = 0, reverse: bool = False,
                 density: bool = False, implicit_grad: bool = False):
        super().__init__()
        self.implicit_grad = bool(implicit_grad)
        if not 2 <= bins <= 32:
            raise ValueError(f"RQSAutoregressive: need 2 <= bins <= 32, got {bins}")
        if not bound > 0:
            raise ValueError(f"RQSAutoregressive: need bound > 0, got {bound}")
        self.dim, self.bins, self.bound = dim, int(bins), float(bound)
        self.density = bool(density)
        order = torch.arange(dim, 0, -1) if reverse else None
        self.made = MADE(dim, hidden, n_hidden, 3 * self.bins - 1, context_dim, order)
        self.uses_context = context_dim > 0

    def _params(self, x, context):
        return self.made(x, context).reshape(x.shape[0], (3 * self.bins - 1) * self.dim)

    def _one_pass(self, x, context=None):
        """``(T(x), ldj_T(x))``, differentiable."""
        from ..ops import made_fused

        if made_fused.supported(self.made, x, context):   # GPU: the kernels read the bf16 output
            return made_fused.rqs_autoregressive(self, x, context)
        y, ldj = rqs_transform(self._params(x, context), x, self.bins, self.bound)
        return y.to(x.dtype), ldj

    def _sequential(self, y, context=None):
        """``(z, -ldj_T(z))`` with ``T(z) = y``. By default it runs without a graph and is not
        differentiated; with ``implicit_grad=True`` a call that needs a graph takes the degree
        sweep (on the CPU its torch composite, in any dtype) with the implicit gradient of
        ``ops.autoregressive``, and raises where the sweep is not supported: the layer has no
        other differentiable solve."""
        from ..ops import autoregressive as ar

        if self.implicit_grad and ar.needs_graph(self, y, context):
            if not ar.grad_supported(self.made, y, context, 3 * self.bins - 1):
                raise RuntimeError(
                    "RQSAutoregressive: implicit_grad needs a ReLU MADE with 1 .. 4 hidden layers "
                    "and, on the GPU, fp32 tensors and a shape inside the sweep kernels' LDS "
                    f"budget; got {tuple(y.shape)} {y.dtype} with hidden "
                    f"{self.made.layers[0].weight.shape[0]} x {len(self.made.layers) - 1}")
            return ar.rqs_sweep_flow_grad(self, y, context)
        return self._sequential_no_grad(y, context)

    @torch.no_grad()
    def _sequential_no_grad(self, y, context=None):
        """``(z, -ldj_T(z))`` with ``T(z) = y`` without a graph, for sampling and checks. fp32
        GPU tensors with a supported MADE (ReLU, 1 .. 4 hidden layers, a bias on every layer, a shape inside the kernel's LDS budget) take the degree
        sweep of ``ops.autoregressive``: one masked pass with the closed-form spline inverse as
        the per-coordinate transform, ldj from the same kernel. Every other call (CPU, fp64,
        other shapes) runs the sequential loop: D MADE passes, each followed by the spline
        inverse of one coordinate, and ldj from one one-pass evaluation at z."""
        from ..ops import autoregressive as ar

        if y.is_cuda and ar.supported(self.made, y, context, 3 * self.bins - 1):
            return ar.rqs_sweep_flow(self, y, context)
        z = torch.zeros_like(y)
        for i in torch.argsort(self.made.order).tolist():
            p_i = self.made(z, context)[:, :, i].contiguous()          # [N, 3 bins - 1]
            z[:, i] = rqs_transform(p_i, y[:, i:i + 1].contiguous(), self.bins, self.bound,
                                    inverse=True)[0][:, 0].to(y.dtype)
        _, ldj = self._one_pass(z, context)
        return z, -ldj

    def forward(self, x, context=None):
        if self.density:
            return self._sequential(x, context)
        return self._one_pass(x, context)

    def inverse(self, y, context=None):
        if self.density:
            return self._one_pass(y, context)
        return self._sequential(y, context)


class MaskedSplineFlow(Flow):
    """Stack of ``RQSAutoregressive`` layers with the coordinate order reversed between them
    (RQ-NSF (AR)); ``density`` as in the layer."""

    invertible = True

    def __init__(self, dim: int, n_layers: int = 4, bins: int = 8, bound: float = 3.0,
                 hidden: int = 64, n_hidden: int = 1, context_dim: int = 0,
                 density: bool = False, implicit_grad: bool = False):
        super().__init__()
        layers = []
        for i in range(n_layers):
            layers.append(RQSAutoregressive(dim, bins, bound, hidden, n_hidden, context_dim,
                                            density=density, implicit_grad=implicit_grad))
            if i < n_layers - 1:
                layers.append(Reverse())
        self.density = bool(density)
        self.layers = nn.ModuleList(layers)
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
