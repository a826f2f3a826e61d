"""Neural autoregressive flows (Huang et al. 2018): deep sigmoidal flow (DSF) layers.

Every transformed coordinate goes through its own monotone map
y = logit(sum_h w_h sigmoid(a_h x + b_h)) with ``units`` sigmoid units, whose 3 * units
parameters per coordinate (raw slopes, shifts, mixture logits) are the conditioner's output,
plane-major [B, 3 units d]. Unlike the spline it is smooth and acts on the whole real line, so
the scale of the posterior need not be known in advance. The conditioner is either a MADE
(``DSFAutoregressive``: the drop-in upgrade of IAF, one pass in the VI direction) or a
half-split coupling MLP (``DSFCoupling``: one pass in both directions, the inverse being a root
solve per element). Zero raw parameters give the identity with ldj 0.

Not in the reference. The element-wise part runs in the fused HIP kernels of
``csrc/kernels/dsf.hip`` on the GPU (``ops/dsf.py``); the dense DDSF variant is not built.
"""
from __future__ import annotations

import torch
from torch import nn

from ..ops.dsf import dsf_transform
from .base import Flow, Reverse
from .coupling import mlp
from .made import MADE


def _check_units(name: str, units: int) -> int:
    if not 1 <= units <= 32:
        raise ValueError(f"{name}: need 1 <= units <= 32, got {units}")
    return int(units)


class DSFCoupling(Flow):
    """Half-split DSF coupling; ``parity`` 0 conditions on the first half, 1 on the second.
    The conditioner's last layer starts at zero: the layer is the identity at initialisation."""

    invertible = True

    def __init__(self, dim: int, units: int = 8, hidden: int = 256, n_hidden: int = 2,
                 parity: int = 0, context_dim: int = 0):
        super().__init__()
        self.dim, self.parity, self.units = dim, parity, _check_units("DSFCoupling", units)
        self.d_a = dim // 2 if parity == 0 else dim - dim // 2
        self.d_b = dim - self.d_a
        self.uses_context = context_dim > 0
        self.net = mlp(self.d_a + context_dim, hidden, n_hidden, 3 * self.units * self.d_b,
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
        yb, ldj = dsf_transform(self._params(xa, context), xb, self.units)
        return self._join(xa, yb.to(x.dtype)), ldj

    def inverse(self, y, context=None):
        ya, yb = self._split(y)
        xb, ldj = dsf_transform(self._params(ya, context), yb, self.units, inverse=True)
        return self._join(ya, xb.to(y.dtype)), ldj


class DSFAutoregressive(Flow):
    """MADE-conditioned DSF layer: IAF with the affine transformer replaced by the DSF.
    ``forward`` is one pass (the VI direction). The MADE's last layer starts small (1e-2 of
    its default), so the layer starts near the identity."""

    invertible = True

    def __init__(self, dim: int, units: int = 8, hidden: int = 64, n_hidden: int = 1,
                 context_dim: int = 0, reverse: bool = False, implicit_grad: bool = False):
        super().__init__()
        self.implicit_grad = bool(implicit_grad)
        self.dim, self.units = dim, _check_units("DSFAutoregressive", units)
        order = torch.arange(dim, 0, -1) if reverse else None
        self.made = MADE(dim, hidden, n_hidden, 3 * self.units, context_dim, order)
        self.uses_context = context_dim > 0

    def _params(self, z, context):
        return self.made(z, context).reshape(z.shape[0], 3 * self.units * self.dim)

    def forward(self, z, context=None):
        from ..ops import made_fused

        if made_fused.supported(self.made, z, context):   # GPU: the kernels read the bf16 output
            return made_fused.dsf_autoregressive(self, z, context)
        y, ldj = dsf_transform(self._params(z, context), z, self.units)
        return y.to(z.dtype), ldj

    def inverse(self, y, context=None):
        """Inverse ``(z, -ldj)``. By default it runs without a graph and is not differentiated;
        with ``implicit_grad=True`` a call that needs a graph takes the degree sweep (on the CPU
        its torch composite, in any dtype) with the implicit gradient of ``ops.autoregressive``,
        and raises where the sweep is not supported: the layer has no other differentiable
        inverse."""
        from ..ops import autoregressive as ar

        if self.implicit_grad and ar.needs_graph(self, y, context):
            if not ar.grad_supported(self.made, y, context, 3 * self.units):
                raise RuntimeError(
                    "DSFAutoregressive.inverse: implicit_grad needs a ReLU MADE with 1 .. 4 hidden "
                    "layers and, on the GPU, fp32 tensors and a shape inside the sweep kernels' "
                    f"LDS budget; got {tuple(y.shape)} {y.dtype} with hidden "
                    f"{self.made.layers[0].weight.shape[0]} x {len(self.made.layers) - 1}")
            return ar.dsf_sweep_flow_grad(self, y, context)
        return self._inverse_no_grad(y, context)

    @torch.no_grad()
    def _inverse_no_grad(self, y, context=None):
        """``(z, -ldj)`` without a graph, for sampling and checks. fp32 GPU tensors with a
        supported MADE (ReLU, 1 .. 4 hidden layers, a bias on every layer, a shape inside the kernel's LDS budget) take the degree sweep of
        ``ops.autoregressive``: one masked pass with the root solve as the per-coordinate
        transform, ldj from the same kernel. Every other call (CPU, fp64, other shapes) runs
        the sequential loop: D MADE passes, each followed by the root solve of one coordinate,
        and ldj from one forward pass at z."""
        from ..ops import autoregressive as ar

        if y.is_cuda and ar.supported(self.made, y, context, 3 * self.units):
            return ar.dsf_sweep_flow(self, y, context)
        z = torch.zeros_like(y)
        for i in torch.argsort(self.made.order).tolist():
            p_i = self.made(z, context)[:, :, i].contiguous()          # [N, 3 units]
            z[:, i] = dsf_transform(p_i, y[:, i:i + 1].contiguous(), self.units,
                                    inverse=True)[0][:, 0].to(y.dtype)
        _, ldj = self.forward(z, context)
        return z, -ldj


class NeuralAutoregressiveFlow(Flow):
    """Stack of DSF layers. ``conditioner="made"``: autoregressive layers with the coordinate
    order reversed between them; ``"coupling"``: couplings of alternating parity."""

    invertible = True

    def __init__(self, dim: int, n_layers: int = 4, units: int = 8, hidden: int = 64,
                 n_hidden: int = 1, conditioner: str = "made", context_dim: int = 0,
                 implicit_grad: bool = False):
        super().__init__()
        if implicit_grad and conditioner != "made":
            raise ValueError("NeuralAutoregressiveFlow: implicit_grad needs conditioner='made'")
        layers = []
        if conditioner == "made":
            for i in range(n_layers):
                layers.append(DSFAutoregressive(dim, units, hidden, n_hidden, context_dim,
                                                implicit_grad=implicit_grad))
                if i < n_layers - 1:
                    layers.append(Reverse())
        elif conditioner == "coupling":
            layers = [DSFCoupling(dim, units, hidden, n_hidden, parity=i % 2,
                                  context_dim=context_dim) for i in range(n_layers)]
        else:
            raise ValueError(f"NeuralAutoregressiveFlow: conditioner must be 'made' or "
                             f"'coupling', got {conditioner!r}")
        self.conditioner = conditioner
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
