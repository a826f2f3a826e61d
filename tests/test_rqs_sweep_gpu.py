"""The RQS degree-sweep HIP kernel (csrc/kernels/rqs_sweep.hip) against the fp64 CPU sequential
code (the sequential direction of ``RQSAutoregressive`` on CPU tensors: D MADE passes and spline
inverses), its wiring, and the fused one-pass node of ``ops/made_fused.py``.

Bound, for z and for ldj: ``|kernel - ref64| <= KMUL * max(err32, 8 eps32 max|ref64|)`` with
``err32`` the error of the fp32 sequential CPU path against the same fp64 result, so the kernel
may be KMUL times as far off as the code it replaces. KMUL = 2 x the worst ratio measured on the
MI355X over these 16 cases, rounded up to a power of two (docs/PERF_NOTES.md, "RQS degree sweep");
a kernel that needs KMUL > 16 is wrong or needs the accurate math forms. Weight recipe and cases:
test_rqs_sweep.py.
"""
import copy
import functools

import pytest
import torch

from test_dsf import GRAD_TOL, LDJ_RTOL, Y_ATOL, Y_RTOL, ldj_atol
from test_dsf_sweep import ids, scale32
from test_made_sweep import err
from test_rqs_sweep import (B_FULL, SHAPES, case, make_rqs, module_copies, recipe_, run_sweep)
from test_spline import near_knot
from vi_normflows_amd.flows import MaskedSplineFlow, RQSAutoregressive
from vi_normflows_amd.ops import autoregressive as ar

pytestmark = pytest.mark.gpu

# worst measured ratio 2.256 (ldj, (1, 4, 1, K = 2), B = 1: err 2.5e-7 on the 8 eps32 floor); z at
# most 1.08 ((96, 160, 1, K = 16), B = 1)
KMUL = 8
assert KMUL <= 16
# one shape per register-array size (8, 16, 32 bins)
KMAX_SHAPES = [SHAPES[4], SHAPES[5], SHAPES[6]]


def _launch(shape, B, **over):
    _, _, _, _, _, args = case(shape)
    n0 = ar.sweep_launches()
    out = run_sweep(args, B, torch.device("cuda"), **over)
    assert ar.sweep_launches() == n0 + 1
    return out


@functools.lru_cache(maxsize=None)
def _full(shape):
    """The kernel's (z, ldj) of the 37-row launch of a case, on the CPU; never modified."""
    z, l = _launch(shape, B_FULL)
    return z.cpu(), l.cpu()


@pytest.mark.parametrize("B", (1, B_FULL))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_kernel_matches_fp64_sequential(gpu, shape, B):
    D, H, L, _, _, K, bound = shape
    R = ar.rqs_kernel_rows(D, H, L, K)
    assert R >= 1 and (R == 1 or B_FULL % R)   # 37 rows leave a partial row tile
    _, v, _, (z64, l64), (z32, l32), _ = case(shape)
    z, l = _launch(shape, B) if B != B_FULL else _full(shape)
    assert z.shape == (B, D) and l.shape == (B,) and z.dtype == l.dtype == torch.float32
    assert err(z64, v) > 1e-2   # not the identity
    if D >= 5 and B == B_FULL:   # the planted tails are the identity, bitwise
        zc = z.cpu()
        assert zc[0, 0] == bound and zc[1, D // 2] == -bound
        assert zc[2, D - 1] == 1.5 * bound and zc[3, 1] == -2 * bound
    for name, got, r64, r32 in (("z", z, z64[:B], z32[:B]), ("ldj", l, l64[:B], l32[:B])):
        e, scale = err(got.cpu(), r64), scale32(r32, r64)
        print(f"rqs_sweep {shape} B={B} {name}: err {e:.3e} ratio {e / scale:.3f}")
        assert e <= KMUL * scale, (name, e, scale)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_round_trip_through_the_fp64_one_pass_direction(gpu, shape):
    """Reference-free: the fp64 CPU one-pass direction of the kernel's z returns y, and the
    kernel's ldj is minus its ldj at that z, within the project's limits for the row-wise
    kernels."""
    flow, v, ctx, _, _, _ = case(shape)
    z, l = _full(shape)
    with torch.no_grad():
        y_back, l_fwd = flow(z.double(), ctx)
    assert bool(((y_back - v).abs() <= Y_ATOL + Y_RTOL * v.abs()).all()), err(y_back, v)
    assert bool(((l.double() + l_fwd).abs() <= ldj_atol(shape[0]) + LDJ_RTOL * l_fwd.abs()).all())


@pytest.mark.parametrize("shape", KMAX_SHAPES, ids=ids)
def test_row_is_bitwise_independent_of_its_batch(gpu, shape):
    z1, l1 = _launch(shape, 1)
    zb, lb = _launch(shape, B_FULL)
    zc, lc = _full(shape)
    assert torch.equal(z1[0], zb[0]) and torch.equal(l1[0], lb[0])
    assert torch.equal(zb.cpu(), zc) and torch.equal(lb.cpu(), lc)   # two identical launches


@pytest.mark.parametrize("bad", (float("nan"), 1e4))
@pytest.mark.parametrize("shape", (SHAPES[4], SHAPES[6]), ids=ids)
def test_rows_are_independent(gpu, shape, bad):
    """One coordinate of one row is replaced: the launch returns and every other row is bitwise
    what it was. The NaN goes into a coordinate of middle degree, so it spreads through the
    conditioner to every later step of its row; the 1e4 goes into the coordinate of the highest
    degree, which feeds no conditioner input: it lies in the linear tail, so it comes back as
    1e4 and the row stays finite."""
    flow, _, _, _, _, args = case(shape)
    row = 5
    order = flow.made.order
    col = int(torch.argsort(order)[shape[0] // 2]) if bad != bad else int(torch.argmax(order))
    y = args["y"].clone()
    y[row, col] = bad
    z, l = _launch(shape, B_FULL, y=y)
    torch.cuda.synchronize()
    z, l = z.cpu(), l.cpu()
    z0, l0 = _full(shape)
    keep = torch.arange(B_FULL) != row
    assert torch.equal(z[keep], z0[keep]) and torch.equal(l[keep], l0[keep])
    if bad == 1e4:
        assert bool(torch.isfinite(z[row]).all()) and bool(torch.isfinite(l[row]))
        assert float(z[row, col]) == 1e4
    else:
        assert z[row, col] != z[row, col]   # a NaN is the identity of its own element


def _count_made(flow):
    calls = []
    for m in flow.modules():
        if isinstance(m, RQSAutoregressive):
            m.made.register_forward_hook(lambda *a: calls.append(1))
    return calls


def test_dispatch_layer_and_stack(gpu):
    torch.manual_seed(0)
    flow = RQSAutoregressive(64, bins=8, hidden=128).to(gpu)
    y = torch.randn(32, 64, device=gpu)
    calls = _count_made(flow)
    n0 = ar.sweep_launches()
    z, ldj = flow.inverse(y)
    assert not calls and ar.sweep_launches() == n0 + 1
    assert z.shape == y.shape and ldj.shape == (32,) and z.grad_fn is None
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(ldj).all())
    with torch.no_grad():
        assert ar.dispatch(flow, y, None)
    stack = MaskedSplineFlow(64, n_layers=3, bins=8, hidden=128).to(gpu)
    calls = _count_made(stack)
    n0 = ar.sweep_launches()
    z, ldj = stack.inverse(y)
    assert not calls and ar.sweep_launches() == n0 + 3
    # density=True: the sweep is forward, the one-pass direction inverse
    dens = RQSAutoregressive(64, bins=8, hidden=128, density=True).to(gpu)
    calls = _count_made(dens)
    n0 = ar.sweep_launches()
    x, ldj = dens(y)
    assert not calls and ar.sweep_launches() == n0 + 1 and x.grad_fn is None
    u, ldj_u = dens.inverse(y)   # one pass (the fused node, which does not call MADE.forward)
    assert ar.sweep_launches() == n0 + 1 and u.grad_fn is not None and ldj_u.grad_fn is not None
    xb, ldj_b = dens(u.detach())   # the sweep undoes the one-pass direction
    assert float((xb - y).abs().max()) <= 1e-3 and float((ldj_b + ldj_u).abs().max()) <= 1e-2


def test_log_prob_of_a_masked_spline_posterior(gpu):
    """``FlowDistribution.log_prob`` on GPU points runs one sweep per layer and agrees with the
    fp64 CPU copy of the model within the KMUL-bound scaled by the layer count."""
    from vi_normflows_amd.distributions.base import StdNormal
    from vi_normflows_amd.flows import FlowDistribution

    D, n_layers = 16, 3
    torch.manual_seed(2)
    flow = MaskedSplineFlow(D, n_layers=n_layers, bins=8, hidden=32)
    g = torch.Generator().manual_seed(21)
    for f in flow.layers:   # the shared recipe instead of the near-identity initialisation
        if isinstance(f, RQSAutoregressive):
            recipe_(f.made, g, torch.float32)
    x = torch.randn(B_FULL, D, generator=g)
    with torch.no_grad():
        ref = FlowDistribution(StdNormal(D), copy.deepcopy(flow).double()).log_prob(x.double())
        lp32 = FlowDistribution(StdNormal(D), copy.deepcopy(flow)).log_prob(x)
        n0 = ar.sweep_launches()
        got = FlowDistribution(StdNormal(D), flow.to(gpu)).log_prob(x.to(gpu))
    assert ar.sweep_launches() == n0 + n_layers
    assert got.shape == (B_FULL,) and bool(torch.isfinite(got).all())
    e, scale = err(got.cpu(), ref), scale32(lp32, ref)
    print(f"rqs_sweep log_prob ({n_layers} layers): err {e:.3e} ratio {e / scale:.3f}")
    assert e <= KMUL * n_layers * scale


def test_outside_the_lds_budget(gpu):
    """A MADE whose state of one row exceeds the LDS budget keeps the loop; a direct call raises."""
    assert not ar.rqs_kernel_supported(8, 30016, 1, 2)
    flow = RQSAutoregressive(8, bins=2, hidden=30016).to(gpu)
    y = torch.randn(16, 8, device=gpu)
    calls = _count_made(flow)
    n0 = ar.sweep_launches()
    with torch.no_grad():
        assert not ar.dispatch(flow, y, None)
    z, _ = flow.inverse(y)
    assert len(calls) > 1 and ar.sweep_launches() == n0 and bool(torch.isfinite(z).all())
    with pytest.raises(RuntimeError, match="LDS budget"):
        ar.rqs_sweep(y, [l.weight.detach() for l in flow.made.layers],
                     [l.bias.detach() for l in flow.made.layers], None, 2, 3.0)
    assert ar.sweep_launches() == n0


def test_row_helpers(gpu):
    assert ar.rqs_kernel_rows(256, 1024, 1, 8) >= 1 and ar.rqs_kernel_supported(256, 1024, 1, 8)
    assert ar.rqs_kernel_rows(1024, 1024, 1, 8) >= 1
    assert ar.rqs_kernel_rows(16384, 16384, 3, 8) == 0
    assert not ar.rqs_kernel_supported(16384, 16384, 3, 8)
    assert ar.rqs_kernel_rows(64, 128, 1, 1) == 0 and ar.rqs_kernel_rows(64, 128, 1, 33) == 0
    assert not ar.rqs_kernel_supported(64, 128, 1, 1)
    # the other sweeps' helpers are unchanged (the shapes of test_dsf_sweep_gpu.py)
    assert ar.dsf_kernel_rows(256, 1024, 1, 8) >= 1 and ar.dsf_kernel_supported(256, 1024, 1, 8)
    assert ar.dsf_kernel_rows(1024, 1024, 1, 8) >= 1
    assert ar.dsf_kernel_rows(16384, 16384, 3, 8) == 0
    assert ar.dsf_kernel_rows(64, 128, 1, 0) == 0 and ar.dsf_kernel_rows(64, 128, 1, 33) == 0
    assert ar.kernel_rows(1024, 1024, 1) >= 8 and ar.kernel_rows(256, 1024, 1) >= 8
    assert ar.kernel_rows(16384, 16384, 3) == 0 and not ar.kernel_supported(8, 30016, 1)


def test_bindings_reject_bad_arguments(gpu):
    """Host checks of ``torch.ops.vinf.rqs_sweep``: nothing is launched."""
    from vi_normflows_amd.ops._ext import native

    ops = native()
    D, H, K, B = 6, 10, 4, 5
    flow, v, _ = make_rqs(D, H, 1, False, 0, K, 3.0, batch=B)
    made = flow.float().to(gpu).made
    plan = ar.plan_for(D, H, 1, made.order.cpu())
    perm, ubeg = plan.on(gpu)
    W = [l.weight.detach() for l in made.layers]
    b = [l.bias.detach() for l in made.layers]
    y = v.float().to(gpu)
    z, ldj = torch.empty_like(y), torch.empty(B, device=gpu)

    def call(y=y, W=W, b=b, perm=perm, ubeg=ubeg, bins=K, bound=3.0, z=z, ldj=ldj):
        ops.rqs_sweep(y, W, b, perm, ubeg, bins, bound, None, z, ldj)

    call()   # the good call goes through
    torch.cuda.synchronize()
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(ldj).all())
    with pytest.raises(RuntimeError, match="bins"):
        call(bins=1)
    with pytest.raises(RuntimeError, match="bins"):
        call(bins=33)
    with pytest.raises(RuntimeError, match="bound"):
        call(bound=0.0)
    with pytest.raises(RuntimeError, match="bound"):
        call(bound=-3.0)
    Wr = torch.randn(12 * D, H, device=gpu)
    with pytest.raises(RuntimeError, match="output weight"):   # 3 U D rows: the DSF layout
        call(W=[W[0], Wr], b=[b[0], Wr[:, 0].contiguous()])
    with pytest.raises(RuntimeError, match="output weight"):   # 2 D rows: the affine layout
        call(W=[W[0], W[1][:2 * D]], b=[b[0], b[1][:2 * D]])
    with pytest.raises(RuntimeError, match="fp32"):
        call(W=[W[0].bfloat16(), W[1]])
    with pytest.raises(RuntimeError, match="ubeg"):
        call(ubeg=ubeg.flatten()[:-1])
    with pytest.raises(RuntimeError, match="unit inner stride"):
        call(y=y.t().contiguous().t())
    with pytest.raises(RuntimeError, match="LDS budget"):
        ops.rqs_sweep(torch.zeros(2, 8, device=gpu),
                      [torch.zeros(30016, 8, device=gpu), torch.zeros(40, 30016, device=gpu)],
                      [torch.zeros(30016, device=gpu), torch.zeros(40, device=gpu)],
                      torch.arange(8, device=gpu, dtype=torch.int32),
                      torch.zeros(10, device=gpu, dtype=torch.int32), 2, 3.0, None,
                      torch.zeros(2, 8, device=gpu), torch.zeros(2, device=gpu))


# ---------------------------------------------------------------- the one-pass direction

def _close(got, ref, atol, rtol, what):
    e = (got.double().cpu() - ref).abs()
    lim = atol + rtol * ref.abs()
    print(f"{what}: max err {float(e.max()):.3e}, worst err/limit {float((e / lim).max()):.3f}")
    assert (e <= lim).all(), what


def test_rqs_autoregressive_module_matches_fp64_cpu_fp32_params(gpu):
    """A shape the fused MADE does not take (dim 10, 37 rows): the masked layers run as fp32
    linears and fp32 params reach the kernels. Forward outputs and parameter gradients against
    the fp64 CPU module with the same weights, then the sweep's round trip through it."""
    from vi_normflows_amd.ops import made_fused

    ref, dev, x, gy, gl = module_copies(gpu)
    assert not made_fused.supported(dev.made, x.to(gpu), None)
    with torch.no_grad():
        assert not bool(near_knot(ref._params(x.double(), None), x.double(), 5, 3.0).any())
    yr, lr = ref(x.double())
    ((yr * gy.double()).sum() + (lr * gl.double()).sum()).backward()
    yd, ld = dev(x.to(gpu))
    ((yd * gy.to(gpu)).sum() + (ld * gl.to(gpu)).sum()).backward()
    assert (yr - x.double()).abs().max() > 1e-2
    _close(yd.detach(), yr.detach(), Y_ATOL, Y_RTOL, "forward y")
    _close(ld.detach(), lr.detach(), ldj_atol(10), LDJ_RTOL, "forward ldj")
    for (n, pr), pd in zip(ref.named_parameters(), dev.parameters()):
        e = (pd.grad.double().cpu() - pr.grad).abs().max()
        lim = GRAD_TOL * (1 + float(pr.grad.abs().max()))
        print(f"forward grad {n}: max err {float(e):.3e}, limit {lim:.3e}")
        assert e <= lim, n
    # the sequential direction of the GPU module (one sweep), checked through the fp64 module
    n0 = ar.sweep_launches()
    xd, ld_inv = dev.inverse(yd.detach())
    assert ar.sweep_launches() == n0 + 1 and not xd.requires_grad
    with torch.no_grad():
        y_back, l_back = ref(xd.double().cpu())
    _close(y_back, yd.detach().double().cpu(), Y_ATOL, Y_RTOL, "f64(inverse(y)) vs y")
    _close(ld_inv, -l_back, ldj_atol(10), LDJ_RTOL, "inverse ldj vs -L(x)")


def test_fused_node_matches_the_two_existing_nodes(gpu):
    """``made_fused.rqs_autoregressive`` against the composition of the two existing autograd
    nodes on the same module (``made_forward`` then ``rqs_transform``): both run the same
    kernels on the same bf16 MADE output, so y, ldj and every weight and bias gradient are
    bitwise equal; dx differs by a few fp32 roundings, because the node adds the MADE path onto
    the direct path inside the GEMM epilogue instead of afterwards."""
    from vi_normflows_amd.ops import made_fused
    from vi_normflows_amd.ops.spline import rqs_transform

    N, D, K, bound = 64, 32, 4, 3.0
    torch.manual_seed(4)
    layer = RQSAutoregressive(D, bins=K, bound=bound, hidden=64).to(gpu)
    g = torch.Generator().manual_seed(9)
    recipe_(layer.made, g, torch.float32)
    x0 = (torch.randn(N, D, generator=g) * 1.5).to(gpu)
    gy, gl = torch.randn(N, D, generator=g).to(gpu), torch.randn(N, generator=g).to(gpu)
    assert made_fused.supported(layer.made, x0, None)

    def run(fn):
        layer.zero_grad()
        x = x0.clone().requires_grad_(True)
        y, ldj = fn(x)
        ((y * gy).sum() + (ldj * gl).sum()).backward()
        return (y.detach(), ldj.detach(), x.grad.clone(),
                [p.grad.clone() for p in layer.parameters()])

    ya, la, dxa, ga = run(lambda x: made_fused.rqs_autoregressive(layer, x))
    yb, lb, dxb, gb = run(lambda x: rqs_transform(made_fused.made_forward(layer.made, x), x, K,
                                                  bound))
    assert float((ya - x0).abs().max()) > 1e-2
    assert torch.equal(ya, yb) and torch.equal(la, lb)
    assert len(ga) == len(gb) == 4
    for (n, _), a, b in zip(layer.named_parameters(), ga, gb):
        assert torch.equal(a, b), n
    e = float((dxa - dxb).abs().max())
    lim = 1e-6 * (1 + float(dxb.abs().max()))
    print(f"fused node dx: max diff {e:.3e}, limit {lim:.3e}")
    assert e <= lim
    # the layer's forward takes the node
    yc, lc, _, _ = run(lambda x: layer(x))
    assert torch.equal(yc, ya) and torch.equal(lc, la)
