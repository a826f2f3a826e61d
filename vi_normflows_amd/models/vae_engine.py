"""Explicit-step engine for the reference's main workload: the amortized planar-flow VAE.

Reference: ``src/learning_mnist.py:89-99`` (encoder 784 -> 64 x3 -> 2dz + 2dz K + K, K
per-sample planar flows, Bernoulli decoder dz -> 64 x3 -> 784, Adam lr 1e-3, batch 128) and
the annealed objective ``normflows/normflows/optimization.py:66-92`` with the estimator fixes
of :mod:`..inference.elbo` (exact log-det of the applied transform with the reference's
log(|psi| + 1e-7) guard, base entropy kept, Bernoulli from logits, per-sample terms averaged).

The model is tiny (145k parameters) and the reference batch is 128, so the autograd module
path (:class:`..models.vae.PlanarVAE`) is bound by ~60 kernel launches per step even inside a
hipGraph. This engine runs a training step as:

* ``vinf::vae_step`` (``csrc/kernels/vae.hip``): phase 1 - one block per 8 rows does the whole
  forward (in-kernel Philox noise) and the input-gradient chain with every activation in LDS;
  phase 2 - every weight / bias gradient as a batch-reduction tile kernel (plain stores, no
  atomics) plus the loss;
* the fused non-finite guard and the flat Adam kernel over ONE fp32 parameter buffer;
* device-side step / noise-offset / beta updates, so the whole step captures into a hipGraph.

Parameters live in a flat fp32 buffer whose per-layer views have the FlatMLP shapes, so the
engine imports / exports :class:`PlanarVAE` modules (and through them the reference's
``models/*/weights_*.npy`` checkpoints). On CPU the same step runs through the autograd module
(the numerics reference the GPU tests compare against).
"""
from __future__ import annotations

import math

import torch

from ..utils.flat import FlatLayout, FlatParams
from .engine_core import FlatEngine, anneal_beta
from .vae import PlanarVAE, VAEConfig

_H = 64


def _mlp_names(prefix: str, L: int):
    return ([f"{prefix}.W{l}" for l in range(L)] + [f"{prefix}.b{l}" for l in range(L)]
            + [f"{prefix}.Wo", f"{prefix}.bo"])


class PlanarVAEEngine(FlatEngine):
    """Flat-buffer planar-flow VAE trainer (GPU: two-launch HIP step + fused Adam)."""

    def __init__(self, cfg: VAEConfig | None = None, batch: int = 128, device="cuda",
                 seed: int = 0, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 anneal: str = "none", anneal_iters: int = 10000, init_scale: float = 0.05,
                 optimizer="adam"):
        cfg = cfg or VAEConfig()
        if cfg.flow_variant != "paper" or cfg.encode_layout != "paper":
            raise ValueError("the engine implements the paper planar update / encoder layout")
        if cfg.width != _H:
            raise ValueError("the engine's kernels assume width 64 (one wave)")
        self.cfg = cfg
        self.B = int(batch)
        self.device = torch.device(device)
        self.seed = int(seed)
        self._init_core(optimizer, betas, eps, lr)
        self.anneal, self.anneal_iters = anneal, anneal_iters
        dz, K, L, Din = cfg.dim_z, cfg.K, cfg.hidden_layers, cfg.dim_x
        self.De = 2 * dz + 2 * dz * K + K
        layout = FlatLayout()
        dims_e = [Din] + [_H] * L
        dims_d = [dz] + [_H] * L
        for prefix, dims, dout in (("dec", dims_d, Din), ("enc", dims_e, self.De)):
            ts = [(f"{prefix}.W{l}", (_H, dims[l])) for l in range(L)]
            ts += [(f"{prefix}.b{l}", (_H,)) for l in range(L)]
            ts += [(f"{prefix}.Wo", (dout, _H)), (f"{prefix}.bo", (dout,))]
            layout.add_unit(ts)
        self.layout = layout
        self.params = FlatParams(layout, self.device, torch.float32)
        self._alloc_state()
        self.params.reset_optimizer_state()
        self.offs = [layout.slots[n].offset for n in _mlp_names("enc", L) + _mlp_names("dec", L)]
        dev = self.device
        self.x = torch.zeros(self.B, Din, device=dev)
        self.beta = torch.ones((), device=dev)
        self.frow = torch.zeros(self.B, device=dev)
        ldg = (self.De + 3) // 4 * 4   # gphi rows padded to 16 B (vae.hip wgrad float4 loads)
        self.ws = torch.zeros(4 * L * self.B * _H + self.B * (ldg + dz + Din), device=dev)
        self.eps_override = None
        self.zk_out = self.ldj_out = None
        g = torch.Generator().manual_seed(int(seed))
        with torch.no_grad():
            for n in layout.order:       # get_init_params: every weight ~ N(0, 1) * 0.05
                self.params.p(n).copy_(torch.randn(self.params.p(n).shape, generator=g) * init_scale)

    # ------------------------------------------------------------------ module interop
    def _module_pairs(self, model: PlanarVAE):
        L = self.cfg.hidden_layers
        pairs = []
        for prefix, mlp in (("enc", model.encoder), ("dec", model.decoder)):
            for l in range(L):
                pairs += [(f"{prefix}.W{l}", mlp.linears[l].weight), (f"{prefix}.b{l}", mlp.linears[l].bias)]
            pairs += [(f"{prefix}.Wo", mlp.linears[L].weight), (f"{prefix}.bo", mlp.linears[L].bias)]
        return pairs

    @torch.no_grad()
    def load_module(self, model: PlanarVAE) -> "PlanarVAEEngine":
        for n, t in self._module_pairs(model):
            self.params.p(n).copy_(t.detach().to(self.params.p(n)))
        return self

    @torch.no_grad()
    def to_module(self, model: PlanarVAE | None = None) -> PlanarVAE:
        model = model or PlanarVAE(self.cfg)
        for n, t in self._module_pairs(model):
            t.copy_(self.params.p(n).to(t))
        return model

    def set_batch(self, x: torch.Tensor) -> None:
        self.x.copy_(x)

    # ------------------------------------------------------------------ checkpoint
    # The state dict (FlatEngine) holds parameters + optimizer moments, step and the RNG counter;
    # beta is a function of the step. The batch is the caller's (set_batch), so a resumed run
    # replays the same batches by iterating its data from the restored step.
    def _cfg_state(self) -> dict:
        return {k: v for k, v in self.cfg.__dict__.items()
                if isinstance(v, (int, float, str, bool))}

    def _set_beta(self) -> None:
        if self.anneal == "reference":
            anneal_beta("reference", self.step_t, self.anneal_iters, self.beta)

    _post_load = _set_beta

    # ------------------------------------------------------------------ step
    def _update_schedule(self):
        self._advance()
        self._set_beta()

    def forward_backward(self):
        """Loss into ``self.loss`` and every parameter gradient into the flat grad buffer."""
        cfg = self.cfg
        if self.device.type == "cuda":
            from ..ops._ext import native

            native().vae_step(self.params.master, self.params.grad, self.offs, self.x,
                              self.eps_override, self.seed, self.rng_offset, self.beta, self.B,
                              cfg.dim_x, cfg.dim_z, cfg.K, cfg.hidden_layers, self.ws, self.frow,
                              self.loss, self.zk_out, self.ldj_out)
            return
        self._reference_forward_backward()

    def _reference_forward_backward(self):
        """Autograd through the PlanarVAE composite on views of the flat buffer (CPU path and
        the GPU tests' fp32 reference: its dense layers run the explicit fp32 torch oracle,
        ``ops.gemm.oracle()``, not the bf16 MFMA module path)."""
        from ..ops import gemm

        with gemm.oracle():
            self._reference_fb()

    def _reference_fb(self):
        model = self.to_module(PlanarVAE(self.cfg).to(self.device))
        eps = self.eps_override
        if eps is None:
            gen = torch.Generator(device=self.device).manual_seed(self.seed + int(self.step_t.item()))
            eps = torch.randn(self.B, self.cfg.dim_z, generator=gen, device=self.device)
        mu, lv, fp = model.encode(self.x)
        z0 = mu + torch.exp(0.5 * lv) * eps
        dz = self.cfg.dim_z
        lq0 = -0.5 * dz * math.log(2 * math.pi) - 0.5 * lv.sum(1) - 0.5 * (eps * eps).sum(1)
        zK, ldj = model.flow(z0, fp)
        # pure torch composite (the module path's log_joint uses the fused elbo.hip kernel)
        from ..distributions.functional import log_bern_logits, log_std_norm

        lp = log_bern_logits(self.x, model.decode_logits(zK)) + log_std_norm(zK)
        frow = lq0 - ldj - self.beta * lp
        F = frow.mean()
        model.zero_grad(set_to_none=True)
        F.backward()
        with torch.no_grad():
            self.loss.copy_(F.detach())
            self.frow.copy_(frow.detach())
            if self.zk_out is not None:
                self.zk_out.copy_(zK.detach())
            if self.ldj_out is not None:
                self.ldj_out.copy_(ldj.detach())
            self.params.grad.zero_()
            for n, t in self._module_pairs(model):
                self.params.g(n).copy_(t.grad)

    @staticmethod
    def supported(cfg: VAEConfig) -> bool:
        """Whether the HIP step takes this configuration (the same limits ``vinf::vae_step``
        checks): width 64, 1-4 hidden layers, dz <= 64 (multiple of 4), K <= 8, Din <= 1024
        (multiple of 4), paper flow / encoder layout, and the rows kernel's LDS image within
        160 KiB (vinf::vae_rows_lds_bytes)."""
        if cfg.flow_variant != "paper" or cfg.encode_layout != "paper" or cfg.width != _H:
            return False
        dz, K, L, Din = cfg.dim_z, cfg.K, cfg.hidden_layers, cfg.dim_x
        if not (1 <= L <= 4 and 1 <= dz <= 64 and dz % 4 == 0 and 0 <= K <= 8
                and Din % 4 == 0 and 4 <= Din <= 1024):
            return False
        # the native library's own LDS budget: a missing / broken library raises here (a GPU job
        # never drops to the module path because the engine could not load)
        from ..ops._ext import native

        return int(native().vae_rows_lds_bytes(Din, dz, K)) <= 163840

    # FlatEngine.train_step: the step's gradients are final after the one vae_step launch pair,
    # so the "backward" only hands every unit to the bucketed all-reduce, last to first
    def forward(self):
        self.forward_backward()

    def backward(self):
        for u in range(len(self.layout.unit_ranges) - 1, -1, -1):
            self._mark_ready(u)

    def capture(self, warmup: int = 2):
        """Capture one train_step into a hipGraph (static x buffer: refill it with set_batch)."""
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self.train_step()
        torch.cuda.current_stream(self.device).wait_stream(s)
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.train_step()
        self._graph = g
        return g

    def n_params(self) -> int:
        return self.layout.n_params()
