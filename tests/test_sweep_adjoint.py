"""The implicit gradient of the degree sweeps (ops/autoregressive.py) on the CPU, in fp64.

Two independent references: a dense implicit-function oracle built from the autograd Jacobians of
the one-pass direction (no recursion, no masks), and - for MAF / IAF, which have one - autograd
through the D-pass loop of the same module with ``implicit_grad`` off. Weight recipes and shapes
are those of test_made_sweep.py, test_dsf_sweep.py and test_rqs_sweep.py.
"""
import copy

import pytest
import torch
from torch.func import functional_call

from test_dsf_sweep import make_dsf
from test_made_sweep import KINDS, SHAPES, make_flow
from test_rqs_sweep import _two_moons, make_rqs
from vi_normflows_amd.flows import MaskedSplineFlow
from vi_normflows_amd.flows.made import MAF
from vi_normflows_amd.flows.naf import DSFAutoregressive, NeuralAutoregressiveFlow
from vi_normflows_amd.ops import autoregressive as ar

ROWS = 5
# (D, H, n_hidden, reverse, context_dim); the last entry carries the seed of a random order
STRUCT = [(1, 4, 1, False, 0), (2, 3, 1, True, 0), (5, 7, 2, False, 0), (12, 5, 1, False, 0),
          (12, 5, 3, False, 3), (9, 14, 2, False, 2, 3)]
FAMILIES = [("maf_sample", None), ("iaf_gated", None), ("iaf_affine", None), ("dsf", 1),
            ("dsf", 4), ("rqs", 2), ("rqs", 5)]
ids = lambda s: "-".join(str(v) for v in s) if isinstance(s, tuple) else str(s)   # noqa: E731


def build(family, n, shape, rows=ROWS):
    """An fp64 layer of ``family`` with the shared weight recipe and ``rows`` inputs."""
    D, H, L, reverse, C = shape[:5]
    order = None
    if len(shape) > 5:
        order = torch.randperm(D, generator=torch.Generator().manual_seed(shape[5])) + 1
    if family == "dsf":
        flow, v, ctx = make_dsf(D, H, L, reverse, C, n, order=order, batch=rows)
    elif family == "rqs":
        flow, _, ctx = make_rqs(D, H, L, reverse, C, n, 3.0, order=order, batch=rows)
        # inputs of our own: make_rqs plants values on the spline's boundary, where the
        # derivative of ldj jumps
        v = torch.randn(rows, D, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    else:
        flow, v, ctx = make_flow(family, D, H, L, reverse, C, order=order, batch=rows)
    return flow, v, ctx


def one_pass(flow, x, ctx):
    """``(T(x), ldj_T(x))``: the direction that is one MADE pass."""
    return flow.inverse(x, ctx) if isinstance(flow, MAF) else flow.forward(x, ctx)


def solve(flow, v, ctx):
    """``(x, -ldj_T(x))`` with ``T(x) = v``: the sequential direction."""
    return flow.forward(v, ctx) if isinstance(flow, MAF) else flow.inverse(v, ctx)


def cotangents(v, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(v.shape, generator=g, dtype=v.dtype),
            torch.randn(v.shape[0], generator=g, dtype=v.dtype))


def implicit_grads(flow, v, ctx, xbar, lbar, flag=True):
    """[v, context, *parameters] gradients of <xbar, x> + <lbar, l> through ``solve``."""
    f = copy.deepcopy(flow)
    f.implicit_grad = flag
    vv = v.clone().requires_grad_()
    cc = None if ctx is None else ctx.clone().requires_grad_()
    x, l = solve(f, vv, cc)
    ((x * xbar).sum() + (l * lbar).sum()).backward()
    return x.detach(), [vv.grad] + ([cc.grad] if cc is not None else []) \
        + [p.grad for p in f.parameters()]


class _OnePass(torch.nn.Module):
    def __init__(self, flow):
        super().__init__()
        self.flow = flow

    def forward(self, x, ctx):
        return one_pass(self.flow, x, ctx)


def dense_oracle(flow, x, ctx, xbar, lbar):
    """The same gradients from dense Jacobians of the one-pass direction, row by row:
    dx/dv = J_x^-1, dx/dtheta = -J_x^-1 J_theta, and l = -ldj_T(x) by the chain rule."""
    mod = _OnePass(flow)
    names = [n for n, _ in mod.named_parameters()]
    params = [p.detach() for _, p in mod.named_parameters()]
    has_ctx = ctx is not None
    gv = torch.zeros_like(x)
    gc = torch.zeros_like(ctx) if has_ctx else None
    gp = [torch.zeros_like(p) for p in params]
    for b in range(x.shape[0]):
        def f(xr, cr, *ps):
            y, ldj = functional_call(mod, dict(zip(names, ps)),
                                     (xr[None], cr[None] if has_ctx else None))
            return y[0], ldj[0]

        cr = ctx[b] if has_ctx else x.new_zeros(1)
        (Jv, Jl) = torch.autograd.functional.jacobian(f, (x[b], cr, *params))
        Jx, lx = Jv[0], Jl[0]
        w = torch.linalg.solve(Jx.T, xbar[b] - lbar[b] * lx)
        gv[b] = w
        if has_ctx:
            gc[b] = -(Jv[1].T @ w) - lbar[b] * Jl[1]
        for k in range(len(params)):
            gp[k] += -torch.tensordot(w, Jv[2 + k], dims=([0], [0])) - lbar[b] * Jl[2 + k]
    return [gv] + ([gc] if has_ctx else []) + gp


def assert_close(got, ref, what):
    assert len(got) == len(ref)
    for k, (a, r) in enumerate(zip(got, ref)):
        assert a is not None and a.shape == r.shape, (what, k)
        lim = 1e-9 * (1 + float(r.abs().max()))
        e = float((a - r).abs().max())
        assert e <= lim, f"{what}: gradient {k} off by {e:.3e} (limit {lim:.3e})"


@pytest.mark.parametrize("shape", STRUCT, ids=ids)
@pytest.mark.parametrize("family,n", FAMILIES, ids=ids)
def test_implicit_backward_matches_the_dense_oracle(family, n, shape):
    flow, v, ctx = build(family, n, shape)
    xbar, lbar = cotangents(v)
    x, got = implicit_grads(flow, v, ctx, xbar, lbar)
    ref = dense_oracle(flow, x, ctx, xbar, lbar)
    assert_close(got, ref, f"{family} {n} {shape}")


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("kind", KINDS)
def test_implicit_backward_matches_autograd_through_the_loop(kind, shape):
    flow, v, ctx = make_flow(kind, *shape, batch=ROWS)
    xbar, lbar = cotangents(v)
    x1, got = implicit_grads(flow, v, ctx, xbar, lbar, flag=True)
    x0, ref = implicit_grads(flow, v, ctx, xbar, lbar, flag=False)
    assert float((x1 - x0).abs().max()) <= 1e-12 * (1 + float(x0.abs().max()))
    assert_close(got, ref, f"{kind} {shape}")


@pytest.mark.parametrize("which", ["lbar_only", "xbar_only"])
@pytest.mark.parametrize("family,n", FAMILIES, ids=ids)
def test_single_cotangents(family, n, which):
    flow, v, ctx = build(family, n, (5, 7, 2, False, 0))
    xbar, lbar = cotangents(v, seed=9)
    if which == "lbar_only":
        xbar = torch.zeros_like(xbar)
    else:
        lbar = torch.zeros_like(lbar)
    x, got = implicit_grads(flow, v, ctx, xbar, lbar)
    assert_close(got, dense_oracle(flow, x, ctx, xbar, lbar), f"{family} {n} {which}")
    assert any(float(g.abs().max()) > 0 for g in got)


def test_flag_semantics():
    for family, n in (("dsf", 4), ("rqs", 5)):
        flow, v, ctx = build(family, n, (5, 7, 2, False, 0))
        z, l = flow.inverse(v)                      # flag off: the graph-less solve, as before
        assert z.grad_fn is None and l.grad_fn is None and not flow.implicit_grad
        flow.implicit_grad = True
        z, l = flow.inverse(v)
        assert z.grad_fn is not None and l.grad_fn is not None
        with torch.no_grad():                       # nothing needs a graph: as before
            z0, l0 = flow.inverse(v)
        assert z0.grad_fn is None and torch.equal(z0, flow._sequential_no_grad(v)[0]
                                                  if family == "rqs"
                                                  else flow._inverse_no_grad(v)[0])
    for kind in KINDS:
        flow, v, ctx = make_flow(kind, 5, 7, 1, False, 0)
        flow.implicit_grad = True
        calls = []
        flow.made.register_forward_hook(lambda *a: calls.append(1))
        x, l = solve(flow, v, ctx)
        assert x.grad_fn is not None and not calls   # the sweep, not D MADE passes
        with torch.no_grad():
            solve(flow, v, ctx)
        assert len(calls) > 1                        # CPU, no graph needed: the loop, as before


def test_plain_sweeps_still_raise_and_double_backward_raises():
    flow, v, _ = make_flow("maf_sample", 5, 7, 1, False, 0)
    W, b = [p.weight for p in flow.made.layers], [p.bias for p in flow.made.layers]
    with pytest.raises(RuntimeError, match="not differentiable"):
        ar.made_sweep(v, W, b, flow.made.order, "maf_sample")
    dsf, vd, _ = make_dsf(5, 7, 1, False, 0, 3, batch=4)
    with pytest.raises(RuntimeError, match="not differentiable"):
        ar.dsf_sweep(vd, [p.weight for p in dsf.made.layers], [p.bias for p in dsf.made.layers],
                     dsf.made.order, 3)
    rqs, vr, _ = make_rqs(5, 7, 1, False, 0, 4, 3.0, batch=4)
    with pytest.raises(RuntimeError, match="not differentiable"):
        ar.rqs_sweep(vr, [p.weight for p in rqs.made.layers], [p.bias for p in rqs.made.layers],
                     rqs.made.order, 4, 3.0)
    vv = v.clone().requires_grad_()
    x, l = ar.made_sweep_grad(vv, W, b, flow.made.order, "maf_sample")
    (g,) = torch.autograd.grad(x.sum() + l.sum(), vv, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    with pytest.raises(ValueError, match="conditioner"):
        NeuralAutoregressiveFlow(4, conditioner="coupling", implicit_grad=True)


def test_function_forms_match_the_flow_forms():
    dsf, v, ctx = make_dsf(5, 7, 2, False, 3, 4, batch=ROWS)
    made = dsf.made
    z0, l0 = ar.dsf_sweep_flow_grad(dsf, v, ctx)
    z1, l1 = ar.dsf_sweep_grad(v, [p.weight for p in made.layers], [p.bias for p in made.layers],
                               made.order, 4, ctx_bias=made.ctx(ctx))
    assert torch.equal(z0, z1) and torch.equal(l0, l1) and z1.grad_fn is not None
    assert isinstance(dsf, DSFAutoregressive)


def test_vi_training_is_the_same_with_and_without_the_flag():
    from vi_normflows_amd.inference.flow_vi import fit_flow_vi

    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        runs = [fit_flow_vi(target="U1", flow="maf", K=2, iters=5, lr=1e-2, n_samples=32,
                            optimizer="adam", hidden=16, implicit_grad=flag)
                for flag in (True, False)]
    finally:
        torch.set_default_dtype(prev)
    on, off = ({k: p.detach() for k, p in r.flow.named_parameters()} for r in runs)
    assert all(m.implicit_grad for m in runs[0].flow.modules() if isinstance(m, MAF))
    assert on.keys() == off.keys() and len(on) > 0
    moved = 0.0
    for k in on:
        assert on[k].dtype == torch.float64
        assert float((on[k] - off[k]).abs().max()) <= 1e-8, k
    torch.manual_seed(0)
    from vi_normflows_amd.inference.flow_vi import build_flow
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        fresh = {k: p.detach() for k, p in build_flow("maf", 2, 2, hidden=16).named_parameters()}
    finally:
        torch.set_default_dtype(prev)
    for k in on:
        moved = max(moved, float((on[k] - fresh[k]).abs().max()))
    assert moved > 1e-3    # the five steps did train


@pytest.mark.parametrize("which", ["nsf-ar", "naf"])
def test_density_training_that_had_no_gradient(which):
    from vi_normflows_amd.inference.flow_vi import fit_density

    data = _two_moons(256, torch.Generator().manual_seed(0))
    torch.manual_seed(0)
    if which == "nsf-ar":
        flow = MaskedSplineFlow(2, n_layers=2, bins=6, hidden=16, density=False,
                                implicit_grad=True)
    else:
        flow = NeuralAutoregressiveFlow(2, n_layers=2, units=4, hidden=16, implicit_grad=True)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)    # thousands of tiny ops: the thread pool's wake-ups would dominate
    try:
        trace = fit_density(flow, data, iters=30, lr=1e-2)
    finally:
        torch.set_num_threads(threads)
    print(f"{which} two moons: nll {trace[0]:.4f} -> {trace[-1]:.4f}")
    assert len(trace) == 30 and all(t == t for t in trace)
    assert trace[-1] < trace[0]


def test_build_flow_passes_the_flag_through():
    from vi_normflows_amd.flows.made import IAF
    from vi_normflows_amd.flows.spline import RQSAutoregressive
    from vi_normflows_amd.inference.flow_vi import build_flow

    for kind, cls in (("nsf-ar", RQSAutoregressive), ("naf", DSFAutoregressive), ("iaf", IAF),
                      ("maf", MAF)):
        for flag in (False, True):
            kw = {"implicit_grad": True} if flag else {}
            flow = build_flow(kind, 4, 3, hidden=8, **kw)
            layers = [m for m in flow.modules() if isinstance(m, cls)]
            assert len(layers) == 3 and all(m.implicit_grad is flag for m in layers), kind
    maf = build_flow("maf", 4, 2, hidden=8)
    x = torch.randn(6, 4)
    with torch.no_grad():
        y, ldj = maf(x)
        xb, ldj_inv = maf.inverse(y)
    assert float((xb - x).abs().max()) < 1e-4 and float((ldj + ldj_inv).abs().max()) < 1e-4
