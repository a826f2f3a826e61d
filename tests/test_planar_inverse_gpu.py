"""Fused planar / radial inverse kernels (fp32, GPU) against the fp64 composites on the CPU.

Shapes cover every PER dispatch edge (D = 1, 2, 5, 16 lane-per-row; 17, 64, 65, 1000
wave-per-row), a partial last block in both row mappings and a tail element at D = 1000, each
with shared and per-sample parameters. Limits are those of test_flow_kernels_gpu.py /
test_dsf_gpu.py: atol 2e-4 (radial ldj 5e-4), rtol 1e-4, gradients 2e-3 (1 + max|ref|).

* residual: the kernel's x pushed through the fp64 forward must give y back; this holds whatever
  the conditioning, so it is checked on well-conditioned and on raw parameters.
* x and ldj against the oracle: the limits are multiplied per row by the oracle's own
  amplification of an input error, prod_k 1 / min(1, psi_k) for planar (1 / psi is the largest
  singular direction of a layer's inverse Jacobian along u_hat) and prod_k 1 / min(1, q1_k, q2_k)
  for radial (q1 = 1 + beta h and q2 = 1 + beta alpha h^2 are the eigenvalues of the forward
  Jacobian).
* gradients: well-conditioned parameters only.
"""
import copy
import functools
import math

import pytest
import torch

from vi_normflows_amd.distributions.base import StdNormal
from vi_normflows_amd.flows import (FlowDistribution, FlowSequence, PlanarStack, RadialStack,
                                    get_uhat, planar_stack_inverse,
                                    planar_stack_inverse_reference, planar_stack_reference,
                                    radial_params, radial_stack_inverse,
                                    radial_stack_inverse_reference, radial_stack_reference)

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 1), (257, 2, 3), (63, 5, 3), (257, 16, 1), (5, 17, 3), (6, 64, 1), (5, 65, 3),
         (3, 1000, 2)]
ATOL, RTOL, ATOL_RADIAL_LDJ = 2e-4, 1e-4, 5e-4


def _planar_psi(x, W, U, B):
    """psi of every layer at the forward states from x: [K, N]."""
    _, _, states = planar_stack_reference(x, W, U, B, return_states=True)
    out = []
    for k, z in enumerate(states):
        a = (z * W[k]).sum(-1) + B[k]
        c = (W[k] * get_uhat(U[k], W[k])).sum(-1)
        out.append((1.0 + (1.0 - torch.tanh(a) ** 2) * c).expand(x.shape[0]))
    return torch.stack(out)


def _radial_q(x, Z0, al, be):
    """min(q1, q2) of every layer at the forward states from x: [K, N]."""
    out, z = [], x
    for k in range(Z0.shape[0]):
        d = z - Z0[k]
        h = 1.0 / (al[k] + torch.sqrt((d * d).sum(-1)))
        out.append(torch.minimum(1 + be[k] * h, 1 + be[k] * al[k] * h * h))
        z = z + (be[k] * h).unsqueeze(-1) * d
    return torch.stack(out)


@functools.lru_cache(maxsize=None)
def _case(kind, N, D, K, per_sample, cond):
    """Seeded fp32 inputs and their fp64 CPU oracle (x, ldj, amplification, gradients), computed
    once per case and shared by the tests; nothing here is modified afterwards."""
    g = torch.Generator().manual_seed(1000 * N + 10 * D + K + 7 * per_sample + (cond == "raw"))
    shp = (K, N, D) if per_sample else (K, D)
    std = (1.0 if cond == "well" else 1.5) / math.sqrt(D)
    y = torch.randn(N, D, generator=g)
    if kind == "planar":
        W, U = torch.randn(*shp, generator=g) * std, torch.randn(*shp, generator=g) * std
        if cond == "well":   # w.u >= 0: c = m(w.u) >= ln 2 - 1 and psi >= 1 + c >= ln 2
            U = U * torch.where((W * U).sum(-1, keepdim=True) < 0, -1.0, 1.0)
        params = (W, U, torch.randn(*shp[:-1], generator=g))
        inverse, forward = planar_stack_inverse_reference, planar_stack_reference
    else:
        a_raw, b_raw = torch.randn(*shp[:-1], generator=g), torch.randn(*shp[:-1], generator=g)
        if cond == "well":   # beta >= 0: q1, q2 >= 1
            al, be = torch.nn.functional.softplus(a_raw), torch.nn.functional.softplus(b_raw)
        else:
            al, be = radial_params(1.5 * a_raw, 1.5 * b_raw)
        params = (torch.randn(*shp, generator=g) * std, al, be)
        inverse, forward = radial_stack_inverse_reference, radial_stack_reference
    gx, gl = torch.randn(N, D, generator=g), torch.randn(N, generator=g)
    leaves = [t.double().requires_grad_(True) for t in (y, *params)]
    x, ldj = inverse(*leaves)
    grads = torch.autograd.grad((x * gx.double()).sum() + (ldj * gl.double()).sum(), leaves)
    x, ldj = x.detach(), ldj.detach()
    pd = [t.double() for t in params]
    stab = _planar_psi(x, *pd) if kind == "planar" else _radial_q(x, *pd)
    amp = (1.0 / stab.clamp(max=1.0)).prod(0)
    return dict(y=y, params=params, gx=gx, gl=gl, x=x, ldj=ldj, grads=grads, stab=stab, amp=amp,
                forward=forward)


def _run(kind, c, dev, grads=False):
    fn = planar_stack_inverse if kind == "planar" else radial_stack_inverse
    leaves = [t.to(dev).requires_grad_(grads) for t in (c["y"], *c["params"])]
    x, ldj = fn(*leaves)
    if not grads:
        return x, ldj
    g = torch.autograd.grad((x * c["gx"].to(dev)).sum() + (ldj * c["gl"].to(dev)).sum(), leaves)
    return x.detach(), ldj.detach(), g


@pytest.mark.parametrize("N,D,K", CASES)
@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("cond", ["well", "raw"])
@pytest.mark.parametrize("kind", ["planar", "radial"])
def test_inverse_kernel_values(gpu, kind, cond, per_sample, N, D, K):
    c = _case(kind, N, D, K, per_sample, cond)
    if cond == "well":
        assert c["stab"].min() >= (0.69 if kind == "planar" else 1.0)
    x, ldj = _run(kind, c, gpu)
    assert x.dtype == torch.float32 and ldj.dtype == torch.float32
    x, ldj = x.cpu().double(), ldj.cpu().double()
    assert torch.isfinite(x).all() and torch.isfinite(ldj).all()
    y = c["y"].double()
    back = c["forward"](x, *[t.double() for t in c["params"]])[0]
    res = (back - y).abs()
    ex, el = (x - c["x"]).abs(), (ldj - c["ldj"]).abs()
    atol_l = ATOL if kind == "planar" else ATOL_RADIAL_LDJ
    lim_x = c["amp"][:, None] * (ATOL + RTOL * c["x"].abs())
    lim_l = c["amp"] * (atol_l + RTOL * c["ldj"].abs())
    print(f"residual {float(res.max()):.2e}  |dx| {float(ex.max()):.2e} (limit used "
          f"{float((ex / lim_x).max()):.3f})  |dldj| {float(el.max()):.2e} (limit used "
          f"{float((el / lim_l).max()):.3f})  max amp {float(c['amp'].max()):.1f}")
    assert (res <= ATOL + RTOL * y.abs()).all()
    assert (ex <= lim_x).all()
    assert (el <= lim_l).all()


@pytest.mark.parametrize("N,D,K", CASES)
@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("kind", ["planar", "radial"])
def test_inverse_kernel_gradients(gpu, kind, per_sample, N, D, K):
    c = _case(kind, N, D, K, per_sample, "well")
    _, _, g = _run(kind, c, gpu, grads=True)
    for name, ga, gb in zip(("gy", "p0", "p1", "p2"), g, c["grads"]):
        err = float((ga.cpu().double() - gb).abs().max())
        print(f"{name}: |d| {err:.2e}, limit {2e-3 * (1 + float(gb.abs().max())):.2e}")
        assert ga.shape == gb.shape
        assert err <= 2e-3 * (1 + float(gb.abs().max()))


@pytest.mark.parametrize("kind", ["planar", "radial"])
@pytest.mark.parametrize("per_sample", [False, True])
def test_two_launches_bitwise_equal(gpu, kind, per_sample):
    for N, D, K in ((257, 2, 3), (5, 65, 3)):
        c = _case(kind, N, D, K, per_sample, "raw")
        a, b = _run(kind, c, gpu, grads=True), _run(kind, c, gpu, grads=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for ga, gb in zip(a[2], b[2]):
            assert torch.equal(ga, gb)


@pytest.mark.parametrize("D", [2, 65])
def test_noncontiguous_inputs_and_encoder_slices(gpu, D):
    """y as a strided view, and W / U / B (Z0 / alpha / beta) as slices of one encoder output
    [N, K (2 D + 1)], give bitwise the result of contiguous copies."""
    N, K = 63, 3
    g = torch.Generator().manual_seed(D)
    y = torch.randn(N, 2 * D, generator=g).to(gpu)[:, ::2]
    enc = (torch.randn(N, K * (2 * D + 1), generator=g) / math.sqrt(D)).to(gpu)
    W = enc[:, :K * D].view(N, K, D).permute(1, 0, 2)
    U = enc[:, K * D:2 * K * D].view(N, K, D).permute(1, 0, 2)
    B = enc[:, 2 * K * D:].t()
    assert not (y.is_contiguous() or W.is_contiguous() or U.is_contiguous() or B.is_contiguous())
    for fn, params in ((planar_stack_inverse, (W, U, B)),
                       (radial_stack_inverse, (W, *radial_params(B, U[..., 0])))):
        out = []
        for args in ((y, *params), tuple(t.contiguous() for t in (y, *params))):
            leaves = [t.detach().requires_grad_(True) for t in args]
            x, ldj = fn(*leaves)
            out.append((x, ldj, *torch.autograd.grad(x.sum() + 0.5 * ldj.sum(), leaves)))
        for a, b in zip(*out):
            assert a.shape == b.shape and torch.equal(a, b)
        fwd = planar_stack_reference if fn is planar_stack_inverse else radial_stack_reference
        yd = y.cpu().double()
        back = fwd(out[0][0].cpu().double(), *[t.cpu().double() for t in params])[0]
        assert ((back - yd).abs() <= ATOL + RTOL * yd.abs()).all()


@pytest.mark.parametrize("per_sample", [False, True])
def test_planar_inverse_psi_zero_is_guarded(gpu, per_sample):
    """w.u_hat = -1 and a = 0 at the preimage give psi = 0: x, the guarded inverse log-det and
    every gradient stay finite (cf. test_planar_psi_zero_is_guarded)."""
    N, D = 64, 2
    y = torch.zeros(N, D, device=gpu, requires_grad=True)
    shp = (1, N, D) if per_sample else (1, D)
    W = torch.zeros(*shp, device=gpu)
    W[..., 0] = 1.0
    U = torch.zeros(*shp, device=gpu)
    U[..., 0] = -30.0            # m(w.u) = -1 + softplus(-30) == -1 in fp32 -> w.u_hat = -1
    W.requires_grad_(True)
    U.requires_grad_(True)
    B = torch.zeros(*shp[:-1], device=gpu, requires_grad=True)
    assert float((W * get_uhat(U, W)).sum(-1).flatten()[0].detach()) == -1.0
    x, ldj = planar_stack_inverse(y, W, U, B)
    # a triple root: s - tanh(s) = 0 holds to fp32 for |s| up to ~1e-2, so x is 0 only to that
    # accuracy, while its image under the forward map is y = 0 to well below the limit
    assert torch.isfinite(x).all() and float(x.abs().max()) < 2e-2
    back = planar_stack_reference(x.detach().cpu().double(), W.detach().cpu().double(),
                                  U.detach().cpu().double(), B.detach().cpu().double())[0]
    assert float(back.abs().max()) <= ATOL
    # psi = tanh^2(s) <= 4e-4 there: -log(4e-4 + 1e-7) <= ldj <= -log(1e-7)
    assert torch.isfinite(ldj).all()
    assert -math.log(4e-4 + 1e-7) <= float(ldj.min()) and float(ldj.max()) <= -math.log(1e-7) + 1e-3
    for t in torch.autograd.grad(ldj.sum() + x.sum(), [y, W, U, B]):
        assert torch.isfinite(t).all()


def test_bindings_reject_bad_arguments(gpu):
    from vi_normflows_amd.ops._ext import native

    ops = native()
    N, D, K = 4, 3, 2

    def bufs(D=D, dtype=torch.float32):
        y = torch.randn(N, D, device=gpu, dtype=dtype)
        W = torch.randn(K, D, device=gpu, dtype=dtype) * 0.3
        return (y, W, W.clone(), torch.zeros(K, device=gpu, dtype=dtype), torch.empty_like(y),
                torch.empty(N, device=gpu, dtype=dtype), torch.empty(K, N, D, device=gpu, dtype=dtype))

    y, W, U, B, x, ldj, saved = bufs()
    ops.planar_stack_inv(y, W, U, B, False, False, x, ldj, saved)       # the accepted call
    with pytest.raises(RuntimeError, match="broadcast"):
        ops.planar_stack_inv(y, W, U, B, False, True, x, ldj, saved)
    with pytest.raises(RuntimeError, match="broadcast"):
        ops.planar_stack_inv_bwd(saved, W, U, B, False, True, y, ldj, x, saved.clone(),
                                 saved.clone(), torch.empty(K, N, device=gpu))
    with pytest.raises(RuntimeError, match="fp32"):
        ops.planar_stack_inv(*bufs(dtype=torch.float64)[:4], False, False, x, ldj, saved)
    with pytest.raises(RuntimeError, match="fp32"):
        y64, Z64, _, a64, *_ = bufs(dtype=torch.float64)
        ops.radial_stack_inv(y64, Z64, a64, a64, False, x, ldj, saved)
    yb, Wb, Ub, Bb, xb, lb, sb = bufs(D=1025)
    with pytest.raises(RuntimeError, match="1024"):
        ops.planar_stack_inv(yb, Wb, Ub, Bb, False, False, xb, lb, sb)
    with pytest.raises(RuntimeError, match="1024"):
        ops.radial_stack_inv(yb, Wb, torch.ones(K, device=gpu), Bb, False, xb, lb, sb)
    with pytest.raises(RuntimeError, match="1024"):
        ops.planar_stack_inv_bwd(sb, Wb, Ub, Bb, False, False, yb, lb, xb, sb.clone(), sb.clone(),
                                 torch.empty(K, N, device=gpu))
    with pytest.raises(RuntimeError, match="shapes"):
        ops.planar_stack_inv(y, W[:, :2].contiguous(), U[:, :2].contiguous(), B, False, False, x,
                             ldj, saved)


@pytest.mark.parametrize("kind", ["planar", "radial", "planar+radial"])
def test_module_log_prob_gpu_matches_cpu_fp64(gpu, kind):
    """log_prob = log N(x) + ldj: the ldj limit plus the x limit carried through
    -|x|^2 / 2 to first order (sum_j |x_j| dx_j), times the oracle's amplification."""
    g = torch.Generator().manual_seed(4)
    N, D, K = 257, 2, 3
    planar, radial = PlanarStack(D, K, init="random", generator=g), RadialStack(D, K, generator=g)
    with torch.no_grad():
        planar.W.mul_(6.0)
        planar.U.mul_(6.0)
    flow = {"planar": planar, "radial": radial, "planar+radial": FlowSequence([planar, radial])}[kind]
    assert flow.invertible
    y = 2.0 * torch.randn(N, D, generator=g)
    ref_flow = copy.deepcopy(flow).double()
    with torch.no_grad():
        x, ldj = ref_flow.inverse(y.double())
        ref = FlowDistribution(StdNormal(D), ref_flow).log_prob(y.double())
        amp = torch.ones(N, dtype=torch.float64)
        mid = x
        if "planar" in kind:
            P = [t.detach().double() for t in (planar.W, planar.U, planar.B)]
            amp = amp * (1.0 / _planar_psi(x, *P).clamp(max=1.0)).prod(0)
            mid = planar_stack_reference(x, *P)[0]
        if "radial" in kind:
            R = [t.detach().double() for t in radial.params()]
            amp = amp * (1.0 / _radial_q(mid, *R).clamp(max=1.0)).prod(0)
        got = FlowDistribution(StdNormal(D), flow.to(gpu)).log_prob(y.to(gpu))
    assert got.is_cuda and got.dtype == torch.float32
    atol_l = ATOL * ("planar" in kind) + ATOL_RADIAL_LDJ * ("radial" in kind)   # the stacks' add up
    lim = amp * (atol_l + RTOL * ldj.abs() + (x.abs() * (ATOL + RTOL * x.abs())).sum(-1))
    err = (got.cpu().double() - ref).abs()
    print(f"|d log p| {float(err.max()):.2e}, limit used {float((err / lim).max()):.3f}")
    assert (err <= lim).all()
