"""The DSF degree sweep (ops/autoregressive.py, ``dsf_sweep``) on the CPU: the torch composite
against the sequential D-pass code of ``DSFAutoregressive.inverse``, plus the case helpers shared
with ``test_dsf_sweep_gpu.py``.

Weight recipe (the one of test_made_sweep.py): every weight entry, masked ones included, is
N(0, 1) * 0.7 / sqrt(fan_in) - this overwrites the 1e-2-scaled last layer, so the map is far from
the identity - biases N(0, 0.3), v = randn, seeded generators. Noise in the masked entries shows
that the sweep ignores them, as the module does (it multiplies by the mask).
"""
import copy
import functools

import pytest
import torch

from test_made_sweep import EPS32, err
from vi_normflows_amd.flows.naf import DSFAutoregressive
from vi_normflows_amd.ops import autoregressive as ar

B_FULL = 37
# (D, H, n_hidden, reverse, context_dim, units): all three register-array sizes (8, 16, 32) and
# unit counts that are no powers of two; (12, 5) has degrees without a hidden unit; (96, 160) and
# (256, 512) have dot products wider than one wave; (256, 512) many steps
SHAPES = [(1, 4, 1, False, 0, 1), (2, 3, 1, True, 0, 3), (5, 7, 2, False, 0, 4),
          (12, 5, 3, False, 3, 8), (33, 70, 2, True, 4, 5), (96, 160, 1, False, 0, 16),
          (40, 96, 2, False, 8, 32), (256, 512, 1, True, 0, 8)]
CPU_SHAPES = SHAPES[:5]
ids = lambda s: "-".join(str(int(v)) for v in s)   # noqa: E731


def make_dsf(D, H, n_hidden, reverse, C, U, seed=0, order=None, batch=B_FULL):
    """An fp64 ``DSFAutoregressive`` with the shared weight recipe, plus (v, context)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * D + H)
    flow = DSFAutoregressive(D, units=U, hidden=H, n_hidden=n_hidden, context_dim=C,
                             reverse=reverse).double()
    made = flow.made
    if order is not None:   # any permutation: rebuild the masks the way MADE.__init__ does
        from vi_normflows_amd.flows.made import made_degrees, made_masks

        d_in, hs = made_degrees(D, H, n_hidden, order)
        made.order.copy_(d_in)
        for layer, m in zip(made.layers, made_masks(d_in, hs, 3 * U)):
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


def sweep_args(flow, v, ctx, dtype):
    """The arguments of ``dsf_sweep`` for a flow, detached, in ``dtype``."""
    made = flow.made
    with torch.no_grad():
        return {"y": v.to(dtype), "weights": [p.weight.detach().to(dtype) for p in made.layers],
                "biases": [p.bias.detach().to(dtype) for p in made.layers],
                "order": made.order.clone(), "units": flow.units,
                "ctx_bias": None if ctx is None else made.ctx(ctx).to(dtype)}


@functools.lru_cache(maxsize=None)
def case(shape, order_seed=None):
    """CPU side of a case, computed once and never modified: the fp64 flow and its inputs (37
    rows), the fp64 sequential inverse, the fp32 sequential inverse (the existing CPU path) and
    the fp32 arguments of ``dsf_sweep``."""
    order = None
    if order_seed is not None:
        order = torch.randperm(shape[0], generator=torch.Generator().manual_seed(order_seed)) + 1
    flow, v, ctx = make_dsf(*shape, order=order)
    with torch.no_grad():
        z64, l64 = flow.inverse(v, ctx)
        z32, l32 = copy.deepcopy(flow).float().inverse(v.float(),
                                                       None if ctx is None else ctx.float())
    return flow, v, ctx, (z64, l64), (z32, l32), sweep_args(flow, v, ctx, torch.float32)


def run_sweep(args, B=None, device=None, **over):
    a = {**args, **over}
    mv = (lambda t: t if device is None else t.to(device))
    cb = a["ctx_bias"]
    return ar.dsf_sweep(mv(a["y"][:B]), [mv(w) for w in a["weights"]], [mv(b) for b in a["biases"]],
                        a["order"], a["units"], ctx_bias=None if cb is None else mv(cb[:B]))


def scale32(r32, r64):
    """max(err32, 8 eps32 max|ref|): the unit of the fp32 bounds."""
    return max(err(r32, r64), 8 * EPS32 * float(r64.abs().max()))


CPU_CASES = [(s, None) for s in CPU_SHAPES] + [((9, 14, 2, False, 2, 6), 3)]


@pytest.mark.parametrize("shape,order_seed", CPU_CASES, ids=lambda c: ids(c) if isinstance(c, tuple)
                         else str(c))
def test_composite_matches_sequential_fp64(shape, order_seed):
    """Both sides evaluate the same fp64 map and differ by summation order only; a wrong degree,
    prefix or plane index is off by 1e-2 or more."""
    flow, v, ctx, (z64, l64), _, _ = case(shape, order_seed)
    if order_seed is not None:
        assert not torch.equal(flow.made.order, torch.arange(1, shape[0] + 1))
    z, l = ar.dsf_sweep_flow(flow, v, ctx)
    assert z.dtype == torch.float64 and l.dtype == torch.float64
    assert z.shape == v.shape and l.shape == (v.shape[0],)
    assert err(z, v) > 1e-2   # not the identity
    assert err(z, z64) <= 1e-9 * max(1.0, float(z64.abs().max()))
    assert err(l, l64) <= 1e-9 * max(1.0, float(l64.abs().max()))
    # the same through the tensor interface
    z2, l2 = run_sweep(sweep_args(flow, v, ctx, torch.float64))
    assert torch.equal(z2, z) and torch.equal(l2, l)


@pytest.mark.parametrize("shape,order_seed", CPU_CASES, ids=lambda c: ids(c) if isinstance(c, tuple)
                         else str(c))
def test_composite_fp32_against_fp64(shape, order_seed):
    _, _, _, (z64, l64), (z32, l32), args = case(shape, order_seed)
    z, l = run_sweep(args)
    assert z.dtype == torch.float32 and l.dtype == torch.float32
    bz, bl = 4 * scale32(z32, z64), 4 * scale32(l32, l64)
    print(f"dsf_sweep composite {shape}: z err {err(z, z64):.3e} (bound {bz:.3e}), "
          f"ldj err {err(l, l64):.3e} (bound {bl:.3e})")
    assert err(z, z64) <= bz and err(l, l64) <= bl


def test_sweep_is_not_differentiable():
    flow, v, _ = make_dsf(5, 7, 1, False, 0, 4, batch=6)
    made = flow.made
    with pytest.raises(RuntimeError, match="not differentiable"):
        ar.dsf_sweep(v, [p.weight for p in made.layers], [p.bias for p in made.layers],
                     made.order, 4)
    with torch.no_grad():   # fine without a graph
        ar.dsf_sweep(v, [p.weight for p in made.layers], [p.bias for p in made.layers],
                     made.order, 4)


@pytest.mark.parametrize("units", (0, 33, 3))
def test_bad_units_raise(units):
    """Out of range, or not the unit count of the output layer (3 * 4 * D rows)."""
    flow, v, _ = make_dsf(5, 7, 1, False, 0, 4, batch=6)
    made = flow.made
    with pytest.raises(ValueError):
        ar.dsf_sweep(v, [p.weight.detach() for p in made.layers],
                     [p.bias.detach() for p in made.layers], made.order, units)


def test_cpu_module_keeps_the_sequential_path():
    """No CPU call dispatches to the sweep: the MADE runs D (+1) times."""
    flow, v, _ = make_dsf(5, 7, 1, False, 0, 4, batch=6)
    calls = []
    flow.made.register_forward_hook(lambda *a: calls.append(1))
    n0 = ar.sweep_launches()
    flow.inverse(v)
    assert len(calls) > 1 and ar.sweep_launches() == n0
