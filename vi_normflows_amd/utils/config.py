"""Typed run configuration: dataclasses, YAML/JSON files, ``key=value`` CLI overrides, presets.

Replaces the reference's scattered module constants / arch dicts / sys.argv parsing
(SURVEY §5.6). One seed per run, derived per rank. The five north-star configurations
of BASELINE.json are shipped as presets:

    config1_two_moons_cpu   2-D two-moons (U1) planar-flow VI on CPU (plumbing)
    config2_realnvp8        8-layer RealNVP on 784-d synthetic, bf16, 1 GPU
    config3_realnvp32_dp8   32-layer RealNVP on 784-d synthetic, data-parallel (the headline)
    config4_iaf10_vae       IAF-10 amortized VI (VAE encoder) on 3x32x32 synthetic, DP
    config5_maf64           MAF-64 density estimation on 1024-d synthetic, DP
plus ``mnist_planar_vae`` (the reference's main workload, src/learning_mnist.py).

Divergence from the reference schedule (recorded, not hidden): ``config2_realnvp8`` and
``config3_realnvp32_dp8`` train with beta = 1 and Adam lr 1e-3 after a 100-step warm-up - the
model ``bench.py`` times - NOT the reference's annealed objective (``normflows/optimization.py:
71-72``, lr 1e-4). ``config3_realnvp32_annealed`` is the reference-faithful variant (annealed
beta_t, lr 1e-4; the warm-up is the one addition, without it the first Adam step diverged).
"""
from __future__ import annotations

import copy
import json
from dataclasses import asdict, dataclass, field, fields, is_dataclass
from pathlib import Path


@dataclass
class RunConfig:
    name: str = "custom"
    task: str = "flow_vi"          # flow_vi | realnvp_vi | planar_vae | iaf_vae | maf_density | bbvi
    device: str = "auto"           # auto | cpu | cuda
    seed: int = 0
    iters: int = 1000
    lr: float = 1e-3
    optimizer: str = "adam"
    schedule: str = "none"         # reference | theano | linear | none
    batch: int = 256               # per-rank batch / MC samples per step
    log_every: int = 100
    ckpt_every: int = 0
    out_dir: str = "runs"
    # flow / model
    target: str = "U1"
    flow: str = "planar"
    K: int = 8
    dim: int = 2
    hidden: int = 64
    n_hidden: int = 2
    dim_z: int = 40
    # optimizer / estimator knobs of the explicit-backward engines (realnvp_vi): linear lr ramp
    # over the first steps, global-norm clip (0 = off), twisted-Gaussian target pairing
    lr_warmup: float = 0.0
    max_grad_norm: float = 0.0
    pairing: str = "split"         # split: (z_i, z_{D/2+i}) | interleaved: (z_2i, z_2i+1)
    extra: dict = field(default_factory=dict)

    def override(self, items: list[str]) -> "RunConfig":
        """Apply ``key=value`` overrides (values parsed as JSON when possible)."""
        c = copy.deepcopy(self)
        names = {f.name: f for f in fields(c)}
        for it in items:
            if "=" not in it:
                raise ValueError(f"override must be key=value: {it}")
            k, v = it.split("=", 1)
            try:
                val = json.loads(v)
            except json.JSONDecodeError:
                val = v
            if k.startswith("extra."):
                c.extra[k[6:]] = val
            elif k in names:
                setattr(c, k, type(getattr(c, k))(val) if getattr(c, k) is not None and
                        not isinstance(getattr(c, k), dict) else val)
            else:
                raise KeyError(f"unknown config key {k}")
        return c

    def validate(self) -> "RunConfig":
        """Reject values no task understands (a typo must not silently select a default)."""
        from ..inference.annealing import SCHEDULES

        if self.schedule not in SCHEDULES:
            raise ValueError(f"unknown schedule {self.schedule!r}; expected one of {sorted(SCHEDULES)}")
        if self.pairing not in ("split", "interleaved"):
            raise ValueError(f"unknown pairing {self.pairing!r}; expected 'split' or 'interleaved'")
        if self.lr_warmup < 0 or self.max_grad_norm < 0:
            raise ValueError("lr_warmup and max_grad_norm must be >= 0")
        return self

    def to_dict(self) -> dict:
        return asdict(self)

    def save(self, path) -> None:
        Path(path).parent.mkdir(parents=True, exist_ok=True)
        Path(path).write_text(json.dumps(self.to_dict(), indent=2))


PRESETS: dict[str, RunConfig] = {
    "config1_two_moons_cpu": RunConfig(name="config1_two_moons_cpu", task="flow_vi", device="cpu",
                                       target="U1", flow="planar", K=16, dim=2, iters=10000,
                                       lr=1e-2, batch=256, optimizer="adam"),
    # the RealNVP presets train exactly the model bench.py times: Adam lr 1e-3 with a 100-step
    # linear warm-up (the first bias-corrected Adam step is a sign step on every parameter),
    # beta = 1, target pairs straddling the coupling split. The reference annealing schedule
    # with lr 1e-4 and no ramp diverged at step 1 on this model.
    "config2_realnvp8": RunConfig(name="config2_realnvp8", task="realnvp_vi", device="cuda",
                                  K=8, dim=784, hidden=1024, batch=65536, iters=200, lr=1e-3,
                                  lr_warmup=100.0, schedule="none", pairing="split"),
    "config3_realnvp32_dp8": RunConfig(name="config3_realnvp32_dp8", task="realnvp_vi",
                                       device="cuda", K=32, dim=784, hidden=1024, batch=65536,
                                       iters=200, lr=1e-3, lr_warmup=100.0, schedule="none",
                                       pairing="split"),
    # the reference's annealed objective on the headline model: beta_t = min(1, 0.001 +
    # t / min(iters / 4, 1e4)) (normflows/optimization.py:71-72) with the reference's Adam lr
    # 1e-4 - plus the 100-step warm-up this 72 M-parameter flow needs (without it the first
    # sign step diverged); the non-annealed presets above are what bench.py times
    "config3_realnvp32_annealed": RunConfig(name="config3_realnvp32_annealed", task="realnvp_vi",
                                            device="cuda", K=32, dim=784, hidden=1024,
                                            batch=65536, iters=2000, lr=1e-4, lr_warmup=100.0,
                                            schedule="reference", pairing="split"),
    "config4_iaf10_vae": RunConfig(name="config4_iaf10_vae", task="iaf_vae", device="cuda", K=10,
                                   dim=3072, hidden=1024, dim_z=256, batch=1024, iters=200,
                                   lr=3e-4),
    "config5_maf64": RunConfig(name="config5_maf64", task="maf_density", device="cuda", K=64,
                               dim=1024, hidden=1024, n_hidden=1, batch=8192, iters=200, lr=1e-4,
                               extra={"precision": "fp8", "impl": "engine"}),
    "mnist_planar_vae": RunConfig(name="mnist_planar_vae", task="planar_vae", device="auto", K=4,
                                  dim=784, hidden=64, n_hidden=3, dim_z=40, batch=128,
                                  iters=10000, lr=1e-3, schedule="reference"),
}


def load(spec: str | None, overrides: list[str] | None = None) -> RunConfig:
    """``spec``: preset name, path to .json/.yaml, or None (defaults)."""
    if spec is None:
        cfg = RunConfig()
    elif spec in PRESETS:
        cfg = copy.deepcopy(PRESETS[spec])
    else:
        p = Path(spec)
        text = p.read_text()
        if p.suffix in (".yaml", ".yml"):
            import yaml

            data = yaml.safe_load(text)
        else:
            data = json.loads(text)
        base = copy.deepcopy(PRESETS.get(data.get("preset", ""), RunConfig()))
        data.pop("preset", None)
        cfg = base.override([f"{k}={json.dumps(v)}" for k, v in data.items()
                             if k != "extra"])
        cfg.extra.update(data.get("extra", {}))
    return cfg.override(overrides or []).validate()


def rank_seed(seed: int, rank: int) -> int:
    """Per-rank seed derivation (one seed per run)."""
    return (int(seed) * 1_000_003 + 7919 * int(rank)) % (2 ** 31 - 1)


def is_config(obj) -> bool:
    return is_dataclass(obj)


@dataclass
class KernelPaths:
    """Which fused / deferred kernel paths the explicit-backward engines take.

    Every field defaults to the measured-fastest path (docs/PERF_NOTES.md); switching one off
    runs the unfused composition of the same math, which is what the equivalence tests compare
    the fused kernels against. ``VINF_KERNEL_PATHS="wgrad_defer=0,wgrad_stream=1"`` overrides
    the defaults for a whole process (subprocess tests, A/B scripts) - the one environment knob
    of the engines (docs/ARCHITECTURE.md, "Runtime switches")."""
    wgrad_defer: bool = True     # weight gradients of many layers as one multi-layer launch
    dgrad_nt: bool = True        # input gradients as NT products against a per-step W^T copy
    cpl_fuse: bool = True        # coupling backward fused into the conditioner's input gradient
    cpl_fwd_fuse: bool = True    # coupling forward fused into the conditioner's last product
    cpl_xbf16: bool = True       # fused coupling backward reads x as its bf16 operand copy
    relu_mask_lanes: bool = True  # conditioner ReLU bitmasks in the 256x256 kernel's lane order
    wgrad_stream: bool = False   # per-layer weight gradients on a side stream (DP tests)
    maf_fuse: bool = True        # MAF transform fused into the MADE GEMM epilogues
    fp8_dgrad: bool = True       # MAF fp8: e4m3 input gradients
    fp8_wgrad: bool = True       # MAF fp8: e4m3 weight gradients
    maf_bf16_state: bool = False  # MAF fused engine: u_1 .. u_{L-1} kept in bf16 only (opt-in)
    made_fused: bool = True      # module path: fused MADE autograd function (ops.made_fused)

    @classmethod
    def from_env(cls) -> "KernelPaths":
        import os

        p = cls()
        spec = os.environ.get("VINF_KERNEL_PATHS", "").strip()
        if not spec:
            return p
        names = {f.name for f in fields(cls)}
        for item in spec.split(","):
            k, _, v = item.strip().partition("=")
            if k not in names:
                raise ValueError(f"VINF_KERNEL_PATHS: unknown path {k!r} (known: {sorted(names)})")
            setattr(p, k, v.strip().lower() not in ("0", "false", "off", "no"))
        return p
