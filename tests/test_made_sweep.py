"""The degree sweep (ops/autoregressive.py) on the CPU: the torch composite against the sequential
D-pass code of ``MAF.forward`` / ``IAF.inverse``, ``MAFEngine.sample`` and ``train.py``'s
``extra.sample_n``.

Weight recipe shared by every case: every weight entry, masked ones included, is
N(0, 1) * 0.7 / sqrt(fan_in), biases N(0, 0.3), v = randn, fixed seed. Noise in the masked entries
shows that the sweep ignores them, as the module does (it multiplies by the mask).
"""
import numpy as np
import pytest
import torch

from vi_normflows_amd.flows.made import IAF, MAF
from vi_normflows_amd.ops.autoregressive import made_sweep, made_sweep_flow

EPS32 = float(torch.finfo(torch.float32).eps)
KINDS = ("maf_sample", "iaf_gated", "iaf_affine")
# (D, H, n_hidden, reverse, context_dim); (12, 5, 1) has degrees with no hidden unit
SHAPES = [(1, 4, 1, False, 0), (2, 3, 1, True, 0), (5, 7, 2, False, 0), (12, 5, 1, True, 0),
          (12, 5, 3, False, 3), (33, 70, 2, True, 4)]


def make_flow(kind, D, H, n_hidden, reverse, C, seed=0, order=None, batch=6):
    """An fp64 flow with the shared weight recipe, plus (v, context) of ``batch`` rows."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * D + H)
    if kind == "maf_sample":
        flow = MAF(D, H, n_hidden, context_dim=C, reverse=reverse)
    else:
        flow = IAF(D, H, n_hidden, context_dim=C, reverse=reverse,
                   mode="gated" if kind == "iaf_gated" else "affine")
    flow = flow.double()
    made = flow.made
    if order is not None:   # any permutation: rebuild the masks the way MADE.__init__ does
        from vi_normflows_amd.flows.made import made_degrees, made_masks

        d_in, hs = made_degrees(D, H, n_hidden, order)
        made.order.copy_(d_in)
        for layer, m in zip(made.layers, made_masks(d_in, hs, 2)):
            layer.mask.copy_(m)
    with torch.no_grad():
        for layer in [*made.layers] + ([made.ctx] if made.ctx is not None else []):
            fan_in = layer.weight.shape[1]
            layer.weight.copy_(torch.randn(layer.weight.shape, generator=g, dtype=torch.float64)
                               * 0.7 / fan_in ** 0.5)
            layer.bias.copy_(torch.randn(layer.bias.shape, generator=g, dtype=torch.float64) * 0.3)
    v = torch.randn(batch, D, generator=g, dtype=torch.float64)
    ctx = torch.randn(batch, C, generator=g, dtype=torch.float64) if C else None
    return flow, v, ctx


def sequential(flow, v, ctx):
    """The existing D-pass code (CPU tensors never dispatch to the sweep)."""
    with torch.no_grad():
        return flow(v, ctx) if isinstance(flow, MAF) else flow.inverse(v, ctx)


def err(a, ref):
    return float((a.double() - ref).abs().max())


def bound32(flow, v, ctx, x64, l64, mult):
    """mult * max(err32, 8 eps32 max|ref|) for x and ldj: err32 is the error of the existing
    fp32 sequential path against the fp64 result."""
    f32 = flow.float()
    x32, l32 = sequential(f32, v.float(), None if ctx is None else ctx.float())
    flow.double()
    return (mult * max(err(x32, x64), 8 * EPS32 * float(x64.abs().max())),
            mult * max(err(l32, l64), 8 * EPS32 * float(l64.abs().max())))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(str(int(v)) for v in s))
def test_composite_matches_sequential_fp64(kind, shape):
    flow, v, ctx = make_flow(kind, *shape)
    x_ref, l_ref = sequential(flow, v, ctx)
    x, l = made_sweep_flow(flow, v, ctx)
    assert x.dtype == torch.float64
    assert err(x, x_ref) <= 1e-12 * max(1.0, float(x_ref.abs().max()))
    assert err(l, l_ref) <= 1e-12 * max(1.0, float(l_ref.abs().max()))


@pytest.mark.parametrize("kind", KINDS)
def test_composite_random_order_fp64(kind):
    D = 9
    order = torch.randperm(D, generator=torch.Generator().manual_seed(3)) + 1
    flow, v, ctx = make_flow(kind, D, 14, 2, False, 2, order=order)
    assert not torch.equal(flow.made.order, torch.arange(1, D + 1))
    x_ref, l_ref = sequential(flow, v, ctx)
    x, l = made_sweep_flow(flow, v, ctx)
    assert err(x, x_ref) <= 1e-12 * max(1.0, float(x_ref.abs().max()))
    assert err(l, l_ref) <= 1e-12 * max(1.0, float(l_ref.abs().max()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(str(int(v)) for v in s))
def test_composite_fp32_against_fp64(kind, shape):
    flow, v, ctx = make_flow(kind, *shape)
    x64, l64 = sequential(flow, v, ctx)
    bx, bl = bound32(flow, v, ctx, x64, l64, 4.0)
    made = flow.made
    kw = ({"bound": flow.bound} if kind == "maf_sample"
          else {"gate_bias": flow.gate_bias, "scale": flow.scale})
    with torch.no_grad():
        ctx_bias = None if ctx is None else made.ctx(ctx).float()
        x, l = made_sweep(v.float(), [p.weight.float() for p in made.layers],
                          [p.bias.float() for p in made.layers], made.order, kind,
                          ctx_bias=ctx_bias, **kw)
    assert x.dtype == torch.float32 and l.dtype == torch.float32
    print(f"{kind} {shape}: x err {err(x, x64):.3e} (bound {bx:.3e}), "
          f"ldj err {err(l, l64):.3e} (bound {bl:.3e})")
    assert err(x, x64) <= bx and err(l, l64) <= bl


def test_sweep_is_not_differentiable():
    flow, v, _ = make_flow("maf_sample", 5, 7, 1, False, 0)
    made = flow.made
    with pytest.raises(RuntimeError, match="not differentiable"):
        made_sweep(v, [p.weight for p in made.layers], [p.bias for p in made.layers],
                   made.order, "maf_sample")
    with pytest.raises(ValueError):
        made_sweep(v, [p.weight.detach() for p in made.layers],
                   [p.bias.detach() for p in made.layers], made.order, "maf")


def test_cpu_flows_keep_the_sequential_path():
    """No CPU call dispatches to the sweep: the MADE runs D (+1) times, also under no_grad."""
    flow, v, _ = make_flow("maf_sample", 5, 7, 1, False, 0)
    calls = []
    flow.made.register_forward_hook(lambda *a: calls.append(1))
    with torch.no_grad():
        flow(v)
    assert len(calls) > 1


def test_engine_sample_inverts_forward():
    from vi_normflows_amd.models.maf_engine import MAFEngine, MAFEngineConfig

    cfg = MAFEngineConfig(dim=8, hidden=12, n_layers=3)
    eng = MAFEngine(cfg, batch=5, device="cpu", seed=1)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():   # the shared recipe instead of the near-identity initialisation
        for l in range(cfg.n_layers):
            for name, fan_in in (("W1", 8), ("W2", 12)):
                p = eng.params.p(f"l{l}.{name}")
                p.copy_(torch.randn(p.shape, generator=g) * 0.7 / fan_in ** 0.5
                        * eng._mask(l)["M1" if name == "W1" else "M2"])
            for name in ("b1", "b2"):
                p = eng.params.p(f"l{l}.{name}")
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
    eng.params.sync_compute()
    P = eng.params
    before = [t.clone() for t in (P.master, P.m, P.v, P.grad, eng.step_t, eng.rng_offset)]
    x = eng.sample(5, generator=torch.Generator().manual_seed(5))
    after = (P.master, P.m, P.v, P.grad, eng.step_t, eng.rng_offset)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert x.shape == (5, 8) and x.dtype == torch.float32 and bool(torch.isfinite(x).all())
    u0 = torch.randn(5, 8, generator=torch.Generator().manual_seed(5))
    eng.data_override = x
    eng.forward()
    u = eng.X[cfg.n_layers]
    # fp64 reference of the same map and the fp32 error of the existing sequential sampler
    layers = []
    for l in range(cfg.n_layers):
        f = MAF(8, 12, 1, reverse=bool(l % 2), alpha_bound=cfg.alpha_bound)
        with torch.no_grad():
            for layer, (w, b) in zip(f.made.layers, (("W1", "b1"), ("W2", "b2"))):
                layer.weight.copy_(P.p(f"l{l}.{w}"))
                layer.bias.copy_(P.p(f"l{l}.{b}"))
        layers.append(f)

    def push(dtype):
        z = u0.to(dtype)
        with torch.no_grad():
            for f in reversed(layers):
                z, _ = f.to(dtype)(z)
            for f in layers:
                z, _ = f.inverse(z)
        return z

    u64 = push(torch.float64)
    err32 = err(push(torch.float32), u64)
    bound = 4 * max(err32, 8 * EPS32 * float(u64.abs().max()))
    print(f"engine round trip: err {err(u, u64):.3e}, bound {bound:.3e}")
    assert err(u64, u0.double()) < 1e-12
    assert err(u, u64) <= bound


def test_train_maf_density_sample_n(tmp_path):
    from vi_normflows_amd.train import main

    args = ["--config", "config5_maf64", "device=cpu", "iters=2", "batch=8", "dim=6", "hidden=10",
            "K=2", "log_every=1"]
    main(args + [f"out_dir={tmp_path / 'a'}"])
    assert not (tmp_path / "a" / "config5_maf64" / "samples.npy").exists()
    for impl in ("engine", "module"):
        out = tmp_path / impl
        main(args + [f"out_dir={out}", f"extra.impl={impl}", "extra.sample_n=4"])
        s = np.load(out / "config5_maf64" / "samples.npy")
        assert s.shape == (4, 6) and np.isfinite(s).all()
