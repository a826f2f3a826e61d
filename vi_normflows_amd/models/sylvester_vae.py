"""Amortized Sylvester-flow VAE: the planar VAE of ``models/vae.py`` with its rank-1 planar
layers replaced by Sylvester layers (``flows/sylvester.py``).

Same encoder / decoder MLPs, sampling, likelihood and free energy as :class:`PlanarVAE`; the
encoder emits ``2 dz + AmortizedSylvester.param_width()`` columns per image, and the flow reads
its per-sample parameters as strided views of that output. Trains on the module path (torch
autograd around the fused flow kernels); ``PlanarVAEEngine`` does not take it.
"""
from __future__ import annotations

from torch import nn

from ..flows.sylvester import AmortizedSylvester
from .mlp import FlatMLP
from .vae import PlanarVAE, VAEConfig


class SylvesterVAE(PlanarVAE):
    def __init__(self, cfg: VAEConfig, householders: int = 1, basis: str = "householder",
                 impl: str = "auto"):
        nn.Module.__init__(self)   # PlanarVAE's constructor sizes the encoder for planar layers
        if cfg.K < 1:
            raise ValueError("SylvesterVAE: need K >= 1 (K = 0 is PlanarVAE without a flow)")
        self.cfg = cfg
        dz = cfg.dim_z
        self.flow = AmortizedSylvester(dz, cfg.K, householders, basis, impl)
        self.encoder = FlatMLP(cfg.dim_x, cfg.width, cfg.hidden_layers,
                               2 * dz + self.flow.param_width())
        self.decoder = FlatMLP(dz, cfg.width, cfg.hidden_layers, cfg.dim_x)

    def split(self, phi):
        """Encoder output (N, Dout) -> mu0, logvar0, flow parameter views."""
        dz = self.cfg.dim_z
        return phi[:, :dz], phi[:, dz:2 * dz], self.flow.split(phi[:, 2 * dz:])
