"""The degree-sweep HIP kernel (csrc/kernels/made_sweep.hip) against the fp64 CPU sequential code
(``MAF.forward`` / ``IAF.inverse`` on CPU tensors: D MADE passes), and its wiring.

Bound, for x and for ldj: ``|kernel - ref64| <= K * max(err32, 8 eps32 max|ref64|)`` with
``err32`` the error of the existing fp32 sequential CPU path against the same fp64 result, so the
kernel may be K times as far off as the code it replaces. K = 2 x the worst ratio measured on the
MI355X over these cases, rounded up to a power of two (docs/PERF_NOTES.md, "Degree sweep"); a
kernel that needs K > 16 is wrong or uses a fast-math intrinsic. Weight recipe: test_made_sweep.py.
"""
import copy
import functools

import pytest
import torch

from test_made_sweep import EPS32, KINDS, err, make_flow, sequential
from vi_normflows_amd.flows.made import IAF, MAF
from vi_normflows_amd.ops import autoregressive as ar

pytestmark = pytest.mark.gpu

K = 2   # worst measured ratio 1.000 (maf_sample (12, 5, 3) ldj, B = 37)
assert K <= 16
B_FULL = 37
# (D, H, n_hidden, reverse, context_dim): (96, 160) has dot products wider than one wave,
# (256, 512) and (200, 96) many steps; D and H are multiples of nothing in particular
SHAPES = [(1, 4, 1, False, 0), (2, 3, 1, True, 0), (5, 7, 2, False, 0), (12, 5, 3, False, 3),
          (33, 70, 2, True, 4), (96, 160, 1, False, 0), (256, 512, 1, True, 0),
          (200, 96, 2, False, 8)]
_ids = lambda s: "-".join(str(int(v)) for v in s)   # noqa: E731


@functools.lru_cache(maxsize=None)
def _case(kind, shape):
    """CPU side of a case, computed once: the fp64 flow, its inputs (37 rows), the fp64
    sequential result, the fp32 sequential result and the kernel's fp32 inputs."""
    flow, v, ctx = make_flow(kind, *shape, batch=B_FULL)
    x64, l64 = sequential(flow, v, ctx)
    x32, l32 = sequential(flow.float(), v.float(), None if ctx is None else ctx.float())
    flow.double()
    made = flow.made
    with torch.no_grad():
        args = {"v": v.float(), "weights": [p.weight.float() for p in made.layers],
                "biases": [p.bias.float() for p in made.layers], "order": made.order.clone(),
                "ctx_bias": None if ctx is None else made.ctx(ctx).float()}
    kw = ({"bound": flow.bound} if kind == "maf_sample"
          else {"gate_bias": flow.gate_bias, "scale": flow.scale})
    return args, kw, (x64, l64), (x32, l32)


def _run(kind, shape, B):
    args, kw, _, _ = _case(kind, shape)
    dev = torch.device("cuda")
    cb = args["ctx_bias"]
    n0 = ar.sweep_launches()
    out = ar.made_sweep(args["v"][:B].to(dev), [w.to(dev) for w in args["weights"]],
                        [b.to(dev) for b in args["biases"]], args["order"], kind,
                        ctx_bias=None if cb is None else cb[:B].to(dev), **kw)
    assert ar.sweep_launches() == n0 + 1
    return out


@pytest.mark.parametrize("B", (1, B_FULL))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_kernel_matches_fp64_sequential(gpu, shape, kind, B):
    D, H, L = shape[:3]
    R = ar.kernel_rows(D, H, L)
    assert R >= 1 and (R == 1 or B_FULL % R)   # 37 rows leave a partial row tile
    _, _, (x64, l64), (x32, l32) = _case(kind, shape)
    x, l = _run(kind, shape, B)
    assert x.shape == (B, D) and l.shape == (B,) and x.dtype == l.dtype == torch.float32
    for name, got, r64, r32 in (("x", x, x64[:B], x32[:B]), ("ldj", l, l64[:B], l32[:B])):
        e, scale = err(got.cpu(), r64), max(err(r32, r64), 8 * EPS32 * float(r64.abs().max()))
        print(f"made_sweep {kind} {shape} B={B} {name}: err {e:.3e} ratio {e / scale:.3f}")
        assert e <= K * scale, (name, e, scale)


@pytest.mark.parametrize("kind,shape", [("maf_sample", SHAPES[4]), ("iaf_gated", SHAPES[5]),
                                        ("iaf_affine", SHAPES[7])])
def test_row_is_bitwise_independent_of_its_batch(gpu, kind, shape):
    x1, l1 = _run(kind, shape, 1)
    xb, lb = _run(kind, shape, B_FULL)
    assert torch.equal(x1[0], xb[0]) and torch.equal(l1[0], lb[0])


def _count_made(flow):
    calls = []
    flow.made.register_forward_hook(lambda *a: calls.append(1))
    return calls


@pytest.mark.parametrize("cls", (MAF, IAF))
def test_dispatch(gpu, cls):
    torch.manual_seed(0)
    flow = cls(64, 128, 1).to(gpu)
    run = flow.forward if cls is MAF else flow.inverse
    v = torch.randn(32, 64, device=gpu)
    calls = _count_made(flow)
    n0 = ar.sweep_launches()
    with torch.no_grad():
        x, ldj = run(v)
    assert not calls and ar.sweep_launches() == n0 + 1
    assert x.shape == v.shape and ldj.shape == (32,) and x.grad_fn is None
    # frozen parameters and a plain input need no graph either
    for p in flow.parameters():
        p.requires_grad_(False)
    run(v)
    assert not calls and ar.sweep_launches() == n0 + 2
    for p in flow.parameters():
        p.requires_grad_(True)
    xg, lg = run(v)   # grad mode on, parameters require grad: the differentiable loop
    assert len(calls) > 1 and ar.sweep_launches() == n0 + 2
    assert xg.grad_fn is not None and lg.grad_fn is not None


def test_density_round_trip(gpu):
    from vi_normflows_amd.models.maf_density import MAFConfig, MAFDensity

    torch.manual_seed(1)
    cfg = MAFConfig(dim=64, n_layers=3, hidden=128)
    model = MAFDensity(cfg).to(gpu)
    n0 = ar.sweep_launches()
    x = model.sample(32, generator=torch.Generator(device=gpu).manual_seed(9))
    assert ar.sweep_launches() == n0 + cfg.n_layers
    with torch.no_grad():
        assert bool(torch.isfinite(model.log_prob(x)).all())
    u0 = torch.randn(32, 64, generator=torch.Generator(device=gpu).manual_seed(9),
                     device=gpu).cpu()
    m64 = copy.deepcopy(model).cpu().double()
    m32 = copy.deepcopy(model).cpu().float()

    def back(xs):
        u = xs.double()
        with torch.no_grad():
            for f in m64.layers:
                u, _ = f.inverse(u)
        return u

    with torch.no_grad():   # the existing sequential sampler, fp32 on the CPU
        x32 = u0
        for f in reversed(m32.layers):
            x32, _ = f(x32)
    scale = max(err(back(x32), u0.double()), 8 * EPS32 * float(u0.abs().max()))
    e = err(back(x.cpu()), u0.double())
    print(f"made_sweep density round trip: err {e:.3e} ratio {e / scale:.3f}")
    assert e <= K * cfg.n_layers * scale


def test_supported_shapes_and_fallback(gpu):
    assert ar.kernel_supported(1024, 1024, 1) and ar.kernel_rows(1024, 1024, 1) >= 8
    assert ar.kernel_supported(256, 1024, 1) and ar.kernel_rows(256, 1024, 1) >= 8   # config 4 IAF
    assert not ar.kernel_supported(16384, 16384, 3) and ar.kernel_rows(16384, 16384, 3) == 0
    # a MADE whose state of one row exceeds the LDS budget keeps the sequential path
    flow = MAF(8, 30016, 1).to(gpu)
    assert not ar.kernel_supported(8, 30016, 1)
    v = torch.randn(32, 8, device=gpu)
    calls = _count_made(flow)
    n0 = ar.sweep_launches()
    with torch.no_grad():
        assert not ar.dispatch(flow, v, None)
        x, _ = flow(v)
    assert len(calls) > 1 and ar.sweep_launches() == n0 and bool(torch.isfinite(x).all())
    with pytest.raises(RuntimeError, match="LDS budget"):
        ar.made_sweep(v, [l.weight.detach() for l in flow.made.layers],
                      [l.bias.detach() for l in flow.made.layers], None, "maf_sample")
