"""The DSF degree-sweep HIP kernel (csrc/kernels/dsf_sweep.hip) against the fp64 CPU sequential
code (``DSFAutoregressive.inverse`` on CPU tensors: D MADE passes and root solves), and its wiring.

Bound, for z and for ldj: ``|kernel - ref64| <= K * max(err32, 8 eps32 max|ref64|)`` with
``err32`` the error of the existing fp32 sequential CPU path against the same fp64 result, so the
kernel may be K times as far off as the code it replaces. K = 2 x the worst ratio measured on the
MI355X over these cases, rounded up to a power of two (docs/PERF_NOTES.md, "DSF degree sweep"); a
kernel that needs K > 16 is wrong or needs the accurate math forms. Weight recipe and cases:
test_dsf_sweep.py.
"""
import copy
import functools

import pytest
import torch

from test_dsf import LDJ_RTOL, Y_ATOL, Y_RTOL, ldj_atol
from test_dsf_sweep import B_FULL, SHAPES, case, ids, make_dsf, run_sweep, scale32
from test_made_sweep import err
from vi_normflows_amd.flows.naf import DSFAutoregressive, NeuralAutoregressiveFlow
from vi_normflows_amd.ops import autoregressive as ar

pytestmark = pytest.mark.gpu

K = 8   # worst measured ratio 2.163 (ldj, (40, 96, 2, U = 32), B = 37); z at most 0.28
assert K <= 16
# one shape per register-array size (8, 16, 32 units)
UMAX_SHAPES = [SHAPES[4], SHAPES[5], SHAPES[6]]


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
    D, H, L, _, _, U = shape
    R = ar.dsf_kernel_rows(D, H, L, U)
    assert R >= 1 and (R == 1 or B_FULL % R)   # 37 rows leave a partial row tile
    _, v, _, (z64, l64), (z32, l32), _ = case(shape)
    z, l = _launch(shape, B) if B != B_FULL else _full(shape)
    assert z.shape == (B, D) and l.shape == (B,) and z.dtype == l.dtype == torch.float32
    assert err(z64, v) > 1e-2   # not the identity
    for name, got, r64, r32 in (("z", z, z64[:B], z32[:B]), ("ldj", l, l64[:B], l32[:B])):
        e, scale = err(got.cpu(), r64), scale32(r32, r64)
        print(f"dsf_sweep {shape} B={B} {name}: err {e:.3e} ratio {e / scale:.3f}")
        assert e <= K * scale, (name, e, scale)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_round_trip_through_the_fp64_forward(gpu, shape):
    """Reference-free: the fp64 CPU forward of the kernel's z returns y, and the kernel's ldj is
    minus the forward's ldj at that z, within the project's limits for the row-wise kernels."""
    flow, v, ctx, _, _, _ = case(shape)
    z, l = _full(shape)
    with torch.no_grad():
        y_back, l_fwd = flow(z.double(), ctx)
    assert bool(((y_back - v).abs() <= Y_ATOL + Y_RTOL * v.abs()).all()), err(y_back, v)
    assert bool(((l.double() + l_fwd).abs() <= ldj_atol(shape[0]) + LDJ_RTOL * l_fwd.abs()).all())


@pytest.mark.parametrize("shape", UMAX_SHAPES, ids=ids)
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
    what it was; a row holding 1e4 stays finite.

    The NaN goes into a coordinate of middle degree, so it spreads through the conditioner to
    every later step of its row. The 1e4 goes into the coordinate of the highest degree, which
    feeds no conditioner input: its root is about 1e4 / a ~ 1.5e4, and with these weights such a
    value in an earlier coordinate drives later raw slopes to about -1e4, where a = softplus
    underflows to the clamp 1e-38 and the root (y - b) / a overflows in the map itself - the
    fp64 CPU sequential inverse of such a row is not finite either (12982 then inf / NaN at
    degree 22 of (33, 70); 14711 at degree 14 of (40, 96)). Whether the row stays finite is
    then a property of the element solve alone, which is what the kernel controls."""
    flow, _, _, _, _, args = case(shape)
    row = 5
    col = shape[0] // 3 if bad != bad else int(torch.argmax(flow.made.order))
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
        assert float(z[row, col].abs()) > 1e3 and not torch.equal(l[row], l0[row])
    else:
        assert not bool(torch.isfinite(z[row]).all())


def _count_made(flow):
    calls = []
    for m in flow.modules():
        if isinstance(m, DSFAutoregressive):
            m.made.register_forward_hook(lambda *a: calls.append(1))
    return calls


def test_dispatch_layer_and_stack(gpu):
    torch.manual_seed(0)
    flow = DSFAutoregressive(64, units=8, hidden=128).to(gpu)
    y = torch.randn(32, 64, device=gpu)
    calls = _count_made(flow)
    n0 = ar.sweep_launches()
    z, ldj = flow.inverse(y)
    assert not calls and ar.sweep_launches() == n0 + 1
    assert z.shape == y.shape and ldj.shape == (32,) and z.grad_fn is None
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(ldj).all())
    with torch.no_grad():
        assert ar.dispatch(flow, y, None)
    stack = NeuralAutoregressiveFlow(64, n_layers=3, units=8, hidden=128,
                                     conditioner="made").to(gpu)
    calls = _count_made(stack)
    n0 = ar.sweep_launches()
    z, ldj = stack.inverse(y)
    assert not calls and ar.sweep_launches() == n0 + 3


def test_log_prob_of_a_naf_posterior(gpu):
    """``FlowDistribution.log_prob`` on GPU points runs one sweep per layer and agrees with the
    fp64 CPU copy of the model within the K-bound scaled by the layer count."""
    from vi_normflows_amd.distributions.base import StdNormal
    from vi_normflows_amd.flows import FlowDistribution

    D, n_layers = 16, 3
    torch.manual_seed(2)
    flow = NeuralAutoregressiveFlow(D, n_layers=n_layers, units=8, hidden=32, conditioner="made")
    g = torch.Generator().manual_seed(21)
    with torch.no_grad():   # the shared recipe instead of the near-identity initialisation
        for f in flow.layers:
            if isinstance(f, DSFAutoregressive):
                for layer in f.made.layers:
                    layer.weight.copy_(torch.randn(layer.weight.shape, generator=g)
                                       * 0.7 / layer.weight.shape[1] ** 0.5)
                    layer.bias.copy_(torch.randn(layer.bias.shape, generator=g) * 0.3)
    x = torch.randn(B_FULL, D, generator=g)
    with torch.no_grad():
        ref = FlowDistribution(StdNormal(D), copy.deepcopy(flow).double()).log_prob(x.double())
        lp32 = FlowDistribution(StdNormal(D), copy.deepcopy(flow)).log_prob(x)
        n0 = ar.sweep_launches()
        got = FlowDistribution(StdNormal(D), flow.to(gpu)).log_prob(x.to(gpu))
    assert ar.sweep_launches() == n0 + n_layers
    assert got.shape == (B_FULL,) and bool(torch.isfinite(got).all())
    e, scale = err(got.cpu(), ref), scale32(lp32, ref)
    print(f"dsf_sweep log_prob ({n_layers} layers): err {e:.3e} ratio {e / scale:.3f}")
    assert e <= K * n_layers * scale


def test_outside_the_lds_budget(gpu):
    """A MADE whose state of one row exceeds the LDS budget keeps the loop; a direct call raises."""
    assert not ar.dsf_kernel_supported(8, 30016, 1, 2)
    flow = DSFAutoregressive(8, units=2, hidden=30016).to(gpu)
    y = torch.randn(16, 8, device=gpu)
    calls = _count_made(flow)
    n0 = ar.sweep_launches()
    with torch.no_grad():
        assert not ar.dispatch(flow, y, None)
    z, _ = flow.inverse(y)
    assert len(calls) > 1 and ar.sweep_launches() == n0 and bool(torch.isfinite(z).all())
    with pytest.raises(RuntimeError, match="LDS budget"):
        ar.dsf_sweep(y, [l.weight.detach() for l in flow.made.layers],
                     [l.bias.detach() for l in flow.made.layers], None, 2)
    assert ar.sweep_launches() == n0


def test_row_helpers(gpu):
    assert ar.dsf_kernel_rows(256, 1024, 1, 8) >= 1 and ar.dsf_kernel_supported(256, 1024, 1, 8)
    assert ar.dsf_kernel_rows(1024, 1024, 1, 8) >= 1
    assert ar.dsf_kernel_rows(16384, 16384, 3, 8) == 0
    assert not ar.dsf_kernel_supported(16384, 16384, 3, 8)
    assert ar.dsf_kernel_rows(64, 128, 1, 0) == 0 and ar.dsf_kernel_rows(64, 128, 1, 33) == 0
    # the affine sweep's helper is unchanged (the shapes of test_made_sweep_gpu.py)
    assert ar.kernel_rows(1024, 1024, 1) >= 8 and ar.kernel_rows(256, 1024, 1) >= 8
    assert ar.kernel_rows(16384, 16384, 3) == 0 and not ar.kernel_supported(8, 30016, 1)


def test_bindings_reject_bad_arguments(gpu):
    """Host checks of ``torch.ops.vinf.dsf_sweep``: nothing is launched."""
    from vi_normflows_amd.ops._ext import native

    ops = native()
    D, H, U, B = 6, 10, 4, 5
    flow, v, _ = make_dsf(D, H, 1, False, 0, U, batch=B)
    made = flow.float().to(gpu).made
    plan = ar.plan_for(D, H, 1, made.order.cpu())
    perm, ubeg = plan.on(gpu)
    W = [l.weight.detach() for l in made.layers]
    b = [l.bias.detach() for l in made.layers]
    y = v.float().to(gpu)
    z, ldj = torch.empty_like(y), torch.empty(B, device=gpu)

    def call(y=y, W=W, b=b, perm=perm, ubeg=ubeg, units=U, z=z, ldj=ldj):
        ops.dsf_sweep(y, W, b, perm, ubeg, units, None, z, ldj)

    call()   # the good call goes through
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="units"):
        call(units=0)
    with pytest.raises(RuntimeError, match="units"):
        call(units=33)
    with pytest.raises(RuntimeError, match="output weight"):   # 2D rows: the affine layout
        call(W=[W[0], W[1][:2 * D]], b=[b[0], b[1][:2 * D]])
    with pytest.raises(RuntimeError, match="fp32"):
        call(W=[W[0].bfloat16(), W[1]])
    with pytest.raises(RuntimeError, match="ubeg"):
        call(ubeg=ubeg.flatten()[:-1])
    with pytest.raises(RuntimeError, match="unit inner stride"):
        call(y=y.t().contiguous().t())
    with pytest.raises(RuntimeError, match="LDS budget"):
        ops.dsf_sweep(torch.zeros(2, 8, device=gpu),
                      [torch.zeros(30016, 8, device=gpu), torch.zeros(48, 30016, device=gpu)],
                      [torch.zeros(30016, device=gpu), torch.zeros(48, device=gpu)],
                      torch.arange(8, device=gpu, dtype=torch.int32),
                      torch.zeros(10, device=gpu, dtype=torch.int32), 2, None,
                      torch.zeros(2, 8, device=gpu), torch.zeros(2, device=gpu))
