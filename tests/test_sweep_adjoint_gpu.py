"""The adjoint degree-sweep HIP kernel (csrc/kernels/sweep_adjoint.hip) against the fp64 composite
on identical inputs, and the ``implicit_grad`` modules on the GPU against their fp64 CPU copies.

Bound, for every output: ``|kernel - ref64| <= KMUL * max(err32, 8 eps32 max|ref64|)`` with
``err32`` the error of the fp32 CPU composite (for the modules: the fp32 CPU implicit path)
against the same fp64 result - the project's unit for the sweeps. KMUL is 2 x the worst ratio
measured on the MI355X over these cases, rounded up to a power of two (docs/PERF_NOTES.md,
"Adjoint degree sweep"); a kernel that needs more than 16 is wrong. The kernel's inputs (hidden
activations, d, q, c, gx, weights) are computed once in fp64 and rounded to fp32, so the ReLU
states of the kernel and of the reference cannot differ.
"""
import copy
import functools

import pytest
import torch

from test_dsf import GRAD_TOL
from test_dsf_sweep import make_dsf, scale32
from test_made_sweep import err, make_flow
from test_rqs_sweep import module_copies
from test_spline import near_knot
from test_sweep_adjoint import build, cotangents, solve
from vi_normflows_amd.flows.made import IAF, MAF
from vi_normflows_amd.flows.naf import DSFAutoregressive
from vi_normflows_amd.flows.spline import RQSAutoregressive
from vi_normflows_amd.ops import autoregressive as ar

pytestmark = pytest.mark.gpu

KMUL = 4          # worst measured ratio 1.263 (a_3, (8, 3000, 4), B = 2); w at most 0.19, pbar 0.13
KMUL_MODULE = 8   # worst measured ratio 3.319 (spline module, output-layer weight gradient)
assert KMUL <= 16 and KMUL_MODULE <= 16
B_FULL = 37
# (family, count, (D, H, n_hidden, reverse, context_dim[, order seed])): P = 2, 3, 12, 5, 95
CASES = [("maf_sample", None, (1, 4, 1, False, 0)), ("dsf", 1, (2, 3, 1, True, 0)),
         ("dsf", 4, (5, 7, 2, False, 0)), ("rqs", 2, (12, 5, 1, False, 0)),
         ("rqs", 32, (12, 5, 3, False, 3)), ("iaf_gated", None, (9, 14, 2, False, 2, 3)),
         ("dsf", 4, (33, 70, 2, True, 4)), ("iaf_affine", None, (33, 70, 2, True, 4)),
         ("rqs", 2, (96, 160, 1, False, 0))]
# one shape per rows-per-block value (8 is every case above)
ROW_CASES = [(4, ("maf_sample", None, (8, 700, 4, False, 0))),
             (2, ("maf_sample", None, (8, 1500, 4, False, 0))),
             (1, ("maf_sample", None, (8, 3000, 4, False, 0)))]
ids = lambda c: "-".join(str(v) for v in (c[0], c[1], *c[2])) if len(c) == 3 else str(c)  # noqa


def _spec(family, n, flow):
    if family == "dsf":
        return ("dsf", n)
    if family == "rqs":
        return ("rqs", n, 3.0)
    return ("made", family, float(getattr(flow, "bound", 5.0)),
            float(getattr(flow, "gate_bias", 1.0)), float(getattr(flow, "scale", 1.0)))


@functools.lru_cache(maxsize=None)
def inputs(case, rows=B_FULL):
    """The kernel's inputs for a case, from the fp64 layer at its fp64 solution, rounded to fp32
    once; the fp64 and fp32 CPU composites on those values. Never modified."""
    family, n, shape = case
    flow, v, ctx = build(family, n, shape, rows=rows)
    made = flow.made
    spec = _spec(family, n, flow)
    P = ar._spec_planes(spec)
    xbar, lbar = cotangents(v, seed=17)
    with torch.no_grad():
        x, _ = solve(flow, v, ctx)
        W = [l.weight.detach() for l in made.layers]
        b = [l.bias.detach() for l in made.layers]
        masks = [l.mask for l in made.layers]
        cb = None if ctx is None else made.ctx(ctx)
        p, hidden = ar._masked_pass(x, W, b, masks, cb)
    le, d, q, c = ar._element_derivatives(spec, x, p, lbar)
    f32 = {"gx": (xbar - le).float(), "d": d.float(), "q": q.float().contiguous(),
           "c": c.float().contiguous(), "hidden": [h.float() for h in hidden],
           "weights": [w.float() for w in W], "order": made.order.clone()}
    assert f32["q"].shape == (rows, shape[0], P)

    def run(dtype):
        w, pbar, a = ar.sweep_adjoint_composite(
            f32["gx"].to(dtype), f32["d"].to(dtype), f32["q"].to(dtype), f32["c"].to(dtype),
            [h.to(dtype) for h in f32["hidden"]], [k.to(dtype) for k in f32["weights"]],
            f32["order"])
        return [w, pbar, *a]

    return f32, run(torch.float64), run(torch.float32)


def launch(f32, B=None, **over):
    a = {**f32, **over}
    dev = torch.device("cuda")
    n0 = ar.sweep_adjoint_launches()
    w, pbar, al = ar.sweep_adjoint(a["gx"][:B].to(dev), a["d"][:B].to(dev), a["q"][:B].to(dev),
                                   a["c"][:B].to(dev), [h[:B].to(dev) for h in a["hidden"]],
                                   [k.to(dev) for k in a["weights"]], a["order"])
    assert ar.sweep_adjoint_launches() == n0 + 1
    torch.cuda.synchronize()
    return [w.cpu(), pbar.cpu(), *[k.cpu() for k in al]]


@functools.lru_cache(maxsize=None)
def full(case):
    return launch(inputs(case)[0])


def check(case, got, B, rows=B_FULL, kmul=KMUL):
    _, r64, r32 = inputs(case, rows)
    names = ["w", "pbar"] + [f"a{l + 1}" for l in range(len(r64) - 2)]
    for name, g, ref, lo in zip(names, got, r64, r32):
        assert g.dtype == torch.float32 and g.shape == ref[:B].shape
        e, scale = err(g, ref[:B]), scale32(lo[:B], ref[:B])
        ratio = e / scale if scale > 0 else 0.0   # an all-zero reference (D = 1: no cotangent)
        print(f"sweep_adjoint {ids(case)} B={B} {name}: err {e:.3e} ratio {ratio:.3f}")
        assert e <= kmul * scale, (name, e, scale)


@pytest.mark.parametrize("B", (1, B_FULL))
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_kernel_matches_the_fp64_composite(gpu, case, B):
    D, H, L = case[2][:3]
    f32, r64, _ = inputs(case)
    assert ar.adjoint_kernel_rows(D, H, L, f32["q"].shape[2]) == 8   # 37 leaves a partial tile
    assert float(r64[0].abs().max()) > 1e-2 and float(r64[1].abs().max()) > 1e-3
    check(case, launch(f32, 1) if B == 1 else full(case), B)


@pytest.mark.parametrize("R,case", ROW_CASES,
                         ids=lambda v: ids(v) if isinstance(v, tuple) else str(v))
def test_every_rows_per_block_value(gpu, R, case):
    D, H, L = case[2][:3]
    assert ar.adjoint_kernel_rows(D, H, L, 2) == R
    f32, _, _ = inputs(case, R + 1)
    got = launch(f32)
    check(case, got, R + 1, rows=R + 1)
    one = launch(f32, 1)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(one, got))   # the place in the tile


@pytest.mark.parametrize("case", [CASES[4], CASES[6], CASES[8]], ids=ids)
def test_rows_are_bitwise_independent(gpu, case):
    f32 = inputs(case)[0]
    ref = full(case)
    one, again = launch(f32, 1), launch(f32)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(one, ref))
    assert all(torch.equal(a, b) for a, b in zip(again, ref))
    gx = f32["gx"].clone()
    row = 5
    gx[row, case[2][0] // 3] = float("nan")
    bad = launch(f32, gx=gx)
    keep = torch.arange(B_FULL) != row
    assert all(torch.equal(a[keep], b[keep]) for a, b in zip(bad, ref))
    assert not bool(torch.isfinite(bad[0][row]).all())


@pytest.mark.parametrize("family,n", [("dsf", 4), ("rqs", 5)])
def test_pbar_is_the_element_backward_at_w(gpu, family, n):
    """``pbar = q w + lbar r`` against the shipped element backward called with
    ``(gy = w, gldj = lbar)`` at the same fp32 parameters, within that kernel's own limit."""
    from vi_normflows_amd.ops.dsf import dsf_bwd
    from vi_normflows_amd.ops.spline import rqs_bwd

    shape = (33, 70, 2, True, 4)
    flow, v, ctx = build(family, n, shape, rows=B_FULL)
    spec = _spec(family, n, flow)
    xbar, lbar = cotangents(v, seed=23)
    f = copy.deepcopy(flow).float().to(gpu)
    made = f.made
    with torch.no_grad():
        vg, cg = v.float().to(gpu), ctx.float().to(gpu)
        x, _ = solve(f, vg, cg)
        W = [l.weight.detach() for l in made.layers]
        p, hidden = ar._masked_pass(x, W, [l.bias.detach() for l in made.layers],
                                    [l.mask for l in made.layers], made.ctx(cg))
        lb = lbar.float().to(gpu)
        le, d, q, c = ar._element_derivatives(spec, x, p, lb)
        w, pbar, _ = ar.sweep_adjoint(xbar.float().to(gpu) - le, d, q, c, hidden, W, made.order)
        if family == "dsf":
            dparams, _ = dsf_bwd(p.contiguous(), x, w, lb, n, False)
        else:
            dparams, _ = rqs_bwd(p.contiguous(), x, w, lb, n, 3.0, False)
    got = pbar.transpose(1, 2).reshape(B_FULL, -1).double().cpu()
    ref = dparams.double().cpu()
    e, lim = float((got - ref).abs().max()), GRAD_TOL * (1 + float(ref.abs().max()))
    print(f"pbar vs {family}_bwd: err {e:.3e} (limit {lim:.3e})")
    assert float(ref.abs().max()) > 1e-3 and e <= lim


def _preacts(flow, x, ctx):
    """Hidden pre-activations of the masked pass at ``x`` (fp64)."""
    made = flow.made
    h, out = x, []
    for l, layer in enumerate(made.layers[:-1]):
        h = torch.nn.functional.linear(h, layer.weight * layer.mask, layer.bias)
        if l == 0 and ctx is not None:
            h = h + made.ctx(ctx)
        out.append(h)
        h = torch.relu(h)
    return out


def _module_case(which):
    if which == "maf":
        return make_flow("maf_sample", 33, 70, 2, True, 4, batch=B_FULL)
    if which == "iaf_gated":
        return make_flow("iaf_gated", 33, 70, 2, True, 4, batch=B_FULL)
    if which == "dsf":
        return make_dsf(33, 70, 2, True, 4, 4, batch=B_FULL)
    ref, _, x, _, _ = module_copies()       # spline: inputs that keep clear of the knots
    with torch.no_grad():
        v, _ = ref(x.double())
    return ref, v, None


def _grads(flow, v, ctx, xbar, lbar):
    vv = v.clone().requires_grad_()
    cc = None if ctx is None else ctx.clone().requires_grad_()
    x, l = solve(flow, vv, cc)
    assert x.grad_fn is not None
    ((x * xbar).sum() + (l * lbar).sum()).backward()
    return [x.detach(), l.detach(), vv.grad] + ([cc.grad] if cc is not None else []) \
        + [p.grad for p in flow.parameters()]


@pytest.mark.parametrize("which", ["maf", "iaf_gated", "dsf", "rqs"])
def test_module_gradients_against_the_fp64_cpu_module(gpu, which):
    flow, v, ctx = _module_case(which)
    flow.implicit_grad = True
    assert isinstance(flow, (MAF, IAF, DSFAutoregressive, RQSAutoregressive))
    # rows whose ReLU state fp32 rounding could flip are decided here, in fp64, and leave both runs
    with torch.no_grad():
        x64, _ = solve(flow, v, ctx)
        pre = _preacts(flow, x64, ctx)
        if which == "rqs":
            assert not bool(near_knot(flow._params(x64, None), x64, flow.bins, flow.bound).any())
    keep = torch.stack([p.abs().min(1).values for p in pre]).min(0).values >= 1e-4
    removed = int((~keep).sum())
    print(f"{which}: {removed} of {B_FULL} rows within the ReLU margin")
    assert removed <= 3
    v = v[keep]
    ctx = None if ctx is None else ctx[keep]
    xbar, lbar = cotangents(v, seed=29)
    ref = _grads(copy.deepcopy(flow), v, ctx, xbar, lbar)
    c32 = None if ctx is None else ctx.float()
    lo = _grads(copy.deepcopy(flow).float(), v.float(), c32, xbar.float(), lbar.float())
    dev = copy.deepcopy(flow).float().to(gpu)
    n0, m0 = ar.sweep_launches(), ar.sweep_adjoint_launches()
    got = _grads(dev, v.float().to(gpu), None if ctx is None else c32.to(gpu),
                 xbar.float().to(gpu), lbar.float().to(gpu))
    assert ar.sweep_launches() == n0 + 1 and ar.sweep_adjoint_launches() == m0 + 1
    assert len(got) == len(ref) == len(lo)
    for k, (g, r, l32) in enumerate(zip(got, ref, lo)):
        assert g is not None and g.shape == r.shape
        e, scale = err(g.cpu(), r), scale32(l32, r)
        ratio = e / scale if scale > 0 else 0.0
        print(f"module {which} tensor {k} {tuple(r.shape)}: err {e:.3e} ratio {ratio:.3f}")
        assert e <= KMUL_MODULE * scale, (which, k, e, scale)


def test_outside_the_lds_budget(gpu):
    """With the flag on and a graph needed, a DSF / spline layer outside the kernels' limits
    raises (it has no other differentiable path); MAF keeps its D-pass loop."""
    assert not ar.adjoint_kernel_supported(8, 30016, 1, 6)
    y = torch.randn(4, 8, device=gpu)
    m0 = ar.sweep_adjoint_launches()
    for flow in (DSFAutoregressive(8, units=2, hidden=30016, implicit_grad=True),
                 RQSAutoregressive(8, bins=2, hidden=30016, implicit_grad=True)):
        flow = flow.to(gpu)
        with pytest.raises(RuntimeError, match="LDS budget"):
            flow.inverse(y)
        with torch.no_grad():                # nothing needs a graph: as before
            z, _ = flow.inverse(y)
        assert z.grad_fn is None
    maf = MAF(8, 30016, implicit_grad=True).to(gpu)
    calls = []
    maf.made.register_forward_hook(lambda *a: calls.append(1))
    x, _ = maf(y)
    assert len(calls) > 1 and x.grad_fn is not None and ar.sweep_adjoint_launches() == m0
    with pytest.raises(RuntimeError, match="LDS budget"):
        ar.sweep_adjoint(torch.zeros(2, 8, device=gpu), torch.ones(2, 8, device=gpu),
                         torch.zeros(2, 8, 2, device=gpu), torch.zeros(2, 8, 2, device=gpu),
                         [torch.zeros(2, 30016, device=gpu)],
                         [torch.zeros(30016, 8, device=gpu), torch.zeros(16, 30016, device=gpu)],
                         None)
    with pytest.raises(RuntimeError, match="fp32"):
        ar.sweep_adjoint(torch.zeros(2, 8, device=gpu).double(), torch.ones(2, 8, device=gpu),
                         torch.zeros(2, 8, 2, device=gpu), torch.zeros(2, 8, 2, device=gpu),
                         [torch.zeros(2, 16, device=gpu)],
                         [torch.zeros(16, 8, device=gpu), torch.zeros(16, 16, device=gpu)], None)


def test_row_helpers(gpu):
    rows, ok = ar.adjoint_kernel_rows, ar.adjoint_kernel_supported
    assert rows(256, 512, 1, 2) == 8 and rows(1024, 1024, 1, 2) == 8
    assert rows(16384, 16384, 3, 2) == 0
    assert rows(64, 128, 1, 0) == 0 and rows(64, 128, 1, 97) == 0
    assert ok(64, 128, 4, 96) and not ok(64, 128, 5, 2)
