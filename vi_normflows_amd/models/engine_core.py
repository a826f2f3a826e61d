"""The training core the explicit-backward engines share (``RealNVPVI``, ``MAFEngine``,
``IAFEngine``, ``PlanarVAEEngine``): device-side step state, the fused guard + flat optimizer,
the step / annealing schedule, ``train_step`` and the checkpoint format.
"""
from __future__ import annotations

import contextlib
import math

import torch

from ..ops import fused
from ..utils.profiling import trace_range


def anneal_beta(kind: str, step_t: torch.Tensor, anneal_iters, out: torch.Tensor) -> None:
    """beta_t of the 1-based device step ``step_t`` into the device scalar ``out``:

    ``"reference"``: min(1, 0.001 + t / min(max_iter / 4, 1e4)), t = step - 1
    (normflows/optimization.py:71-72); ``"theano"``: min(1, 0.01 + t / 1e4)
    (theano_implement.py:169-175)."""
    if kind == "reference":
        cool, start = min(anneal_iters / 4.0, 1e4), 0.001
    elif kind == "theano":
        cool, start = 1e4, 0.01
    else:
        raise ValueError(f"no annealing schedule {kind!r}")
    torch.clamp((step_t - 1.0) * (1.0 / cool) + start, max=1.0, out=out)


class FlatEngine:
    """One training step over flat parameter buffers, with the backward written out.

    A subclass supplies ``layout`` (``FlatLayout``) and ``params`` (``FlatParams``),
    ``forward()`` (loss into ``self.loss``), ``backward()`` (every gradient into
    ``params.grad``) and, in ``_update_schedule``, whatever schedule state is its own. It calls
    ``_init_core`` first and ``_alloc_state`` once ``layout`` and ``params`` exist.

    The data-parallel contract (``parallel.runner.DataParallelRunner``):

    * the engine offers ``params``, ``layout.unit_ranges``, ``grad_scale_host`` (the 1/world
      average, folded into the optimizer's gradient multiplier), ``unit_ready_hook`` and
      ``train_step(reduce_fn)``;
    * during a step every unit index of ``layout.unit_ranges`` is passed to
      ``unit_ready_hook`` exactly once, after that unit's gradient slice is final and before
      ``reduce_fn`` runs (the bucketed all-reduce counts units down per bucket: a unit marked
      twice or never corrupts or hangs the step); the order is the engine's;
    * ``reduce_fn`` runs once, and the optimizer only after it.

    ``supports_forward_persist``: the forward is GEMMs on the persistent-grid kernels with no
    collective in flight, so the runner may ask for the full persistent grid there
    (``persist_forward_only``) while the backward runs the runner's grid policy.
    """

    supports_forward_persist = False
    trace_forward = trace_backward = None   # trace_range names of the two phases

    # ------------------------------------------------------------------ setup
    def _init_core(self, optimizer, betas, eps, lr, weight_decay: float = 0.0,
                   max_grad_norm: float = 0.0, lr_warmup: float = 0.0) -> None:
        # update rule: adam | rmsprop | sgd | rmsprop_momentum (or an OPT_* kind), fused flat kernel
        self.opt = fused.resolve_optimizer(optimizer, betas, eps)
        self.lr, self.wd = lr, weight_decay
        self.opt_kind, self.betas, self.eps = self.opt.kind, (self.opt.b1, self.opt.b2), self.opt.eps
        self.max_grad_norm = float(max_grad_norm)
        self.lr_warmup = float(lr_warmup)   # linear lr ramp over the first steps (device step)
        self.grad_scale_host = 1.0
        self.unit_ready_hook = None   # callable(unit_idx) after a unit's grads are final
        # DP runner: persistent GEMM grid in the forward only (parallel/runner.py)
        self.persist_forward_only = False

    def _alloc_state(self) -> None:
        dev, f32 = self.device, torch.float32
        self.params.v_init = self.opt.v_init
        self.step_t = torch.zeros((), dtype=f32, device=dev)   # 1-based once a step has run
        self.rng_offset = torch.zeros((), dtype=torch.int64, device=dev)
        self.loss = torch.zeros((), dtype=f32, device=dev)
        self.gnorm2 = torch.zeros((), dtype=f32, device=dev)
        self.skip = torch.zeros((), dtype=f32, device=dev)
        self.gscale = torch.ones((), dtype=f32, device=dev)
        self.n_skipped = torch.zeros((), dtype=f32, device=dev)
        self._partials = torch.zeros(512, dtype=f32, device=dev)

    # ------------------------------------------------------------------ step
    def _advance(self) -> None:
        self.step_t.add_(1.0)      # the optimizer's bias correction reads the 1-based step
        self.rng_offset.add_(1)

    def _update_schedule(self) -> None:
        """Device-side step / schedule update (captured into the step graph)."""
        self._advance()

    def _mark_ready(self, unit: int) -> None:
        if self.unit_ready_hook is not None:
            self.unit_ready_hook(unit)

    def optimizer_step(self) -> None:
        P = self.params
        # non-finite guard (+ optional clipping); folds 1/world averaging into gscale
        fused.sumsq_guard(P.grad, self._partials, out_sumsq=self.gnorm2, skip=self.skip,
                          scale=self.gscale, max_norm=self.max_grad_norm,
                          base_scale=self.grad_scale_host)
        b1, b2 = self.betas
        fused.flat_optimizer(self.opt_kind, P.master, P.grad, P.m, P.v,
                             pbf=None if P.compute is P.master else P.compute, lr=self.lr,
                             b1=b1, b2=b2, eps=self.eps, wd=self.wd, step=self.step_t,
                             gscale=self.gscale, skip=self.skip, warmup=self.lr_warmup)
        self.n_skipped.add_(self.skip)

    def train_step(self, reduce_fn=None) -> None:
        """One full step: schedule, forward, backward, [grad all-reduce], optimizer."""
        self._update_schedule()
        fwd_persist = self.persist_forward_only and self.device.type == "cuda"
        if fwd_persist:
            # DP: no collective is in flight during the forward (the optimizer waited for every
            # bucket), so the full one-block-per-CU persistent grid is safe there; the backward,
            # where RCCL all-reduces hold CUs beside the GEMMs, runs the runner's policy (one
            # block per tile, or a persistent grid with CUs reserved)
            from ..ops._ext import native

            prev = native().gemm_persist(1)
            prev_r = native().gemm_grid_reserve(0)
        with _range(self.trace_forward):
            self.forward()
        if fwd_persist:
            native().gemm_persist(prev)
            native().gemm_grid_reserve(prev_r)
        with _range(self.trace_backward):
            self.backward()
        if reduce_fn is not None:
            with trace_range("grad_allreduce_wait"):
                reduce_fn()
        with trace_range("optimizer"):
            self.optimizer_step()

    def reset_after_warmup(self) -> None:
        """Undo what a capture warm-up's steps did to the optimizer and the schedule (the
        caller restores the parameters); the RNG counter keeps running."""
        self.params.reset_optimizer_state()
        self.step_t.zero_()
        self.n_skipped.zero_()

    def log_record(self) -> dict:
        """The step's gradient norm and the skipped-step count (host sync: for logging)."""
        return {"grad_norm": math.sqrt(max(float(self.gnorm2.item()), 0.0)),
                "skipped": float(self.n_skipped.item())}

    # ------------------------------------------------------------------ checkpoint
    def _cfg_state(self) -> dict:
        return self.cfg.__dict__

    def state_dict(self) -> dict:
        return {"params": self.params.state_dict(), "step": self.step_t.detach().cpu(),
                "rng_offset": self.rng_offset.detach().cpu(), "cfg": self._cfg_state()}

    def load_state_dict(self, sd: dict) -> None:
        self.params.load_state_dict(sd["params"])
        self.step_t.copy_(sd["step"])
        self.rng_offset.copy_(sd["rng_offset"])
        self._post_load()

    def _post_load(self) -> None:
        """State that is a function of what ``load_state_dict`` restored."""

    def rank_state_dict(self) -> dict:
        """State that differs between data-parallel ranks and is not in :meth:`state_dict`
        (saved per rank by ``utils.checkpoint.save_engine``)."""
        return {}

    def load_rank_state_dict(self, sd: dict) -> None:
        return None


def _range(name):
    return trace_range(name) if name else contextlib.nullcontext()
