"""Deep sigmoidal flow (neural autoregressive flow): the torch composite against the definition,
the flow modules, the VI / CLI plumbing (CPU, fp64 unless said), and the input helper, oracle
and limits shared with ``test_dsf_gpu.py``."""
import functools
import math
import os
import subprocess
import sys

import pytest
import torch

from vi_normflows_amd.ops import reference
from vi_normflows_amd.ops.dsf import dsf_transform
from vi_normflows_amd.ops.reference import dsf_units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "vi_normflows_amd", "_native", "libvinf_hip.so")

# (B, D, H) of the GPU tests: one row and one column; B no multiple of the 4 rows of a block; D
# on either side of the wave width and past two lane strides; H at and just past each
# register-array size (8, 16, 32); the headline half-width.
GPU_CASES = [(1, 1, 1), (5, 3, 4), (7, 63, 5), (6, 64, 8), (9, 65, 9), (257, 130, 8),
             (33, 7, 16), (12, 20, 17), (10, 24, 32), (64, 392, 8)]
SEED = 5
PARAM_SCALE = 0.5    # std of the raw parameters of the GPU cases
X_SCALE = 1.5        # std of the input of either direction

# The project's limits for the row-wise flow kernels (test_spline_gpu.py).
Y_ATOL, Y_RTOL = 2e-4, 1e-4
LDJ_RTOL = 1e-4
GRAD_TOL = 2e-3
BF16_ROUND = 2.0 ** -8   # output rounding of a bf16 dparams, per element


def ldj_atol(D):
    return 2e-4 + 2e-6 * D


def make_inputs(B, D, H, seed=SEED):
    """fp32 ``params`` [B, 3H D] and ``x`` [B, D] (the input of either direction), seeded on the
    CPU generator (one stream per shape)."""
    g = torch.Generator().manual_seed(seed * 1_000_003 + (B * 1009 + D) * 37 + H)
    params = torch.randn(B, 3 * H * D, generator=g) * PARAM_SCALE
    x = torch.randn(B, D, generator=g) * X_SCALE
    return params, x


def make_robust_inputs(B=16, D=70, H=8, seed=17):
    """fp32 inputs far outside the comfortable range: raw parameters of scale 4 and |x| up to
    1e4 (both ends present)."""
    g = torch.Generator().manual_seed(seed)
    params = torch.randn(B, 3 * H * D, generator=g) * 4.0
    x = (torch.randn(B, D, generator=g) * 3e3).clamp(-1e4, 1e4)
    x[0, 0], x[0, 1], x[0, 2] = 1e4, -1e4, 0.0
    return params, x, H


def envelope(params64, x64, H):
    """[min_h p_h, max_h p_h] of every element, in fp64."""
    a, b, _ = dsf_units(params64, H)
    pj = a * x64.unsqueeze(1) + b
    return pj.amin(1), pj.amax(1)


@functools.lru_cache(maxsize=None)
def oracle(case, dtype, inverse):
    """Inputs of one case and the fp64 composite's outputs and gradients on them (computed
    once, shared by the tests of both files, never modified). ``x`` is the input of the
    direction; for bf16 the oracle is fed the bf16-rounded params."""
    B, D, H = case
    p32, x = make_inputs(B, D, H)
    p_in = p32.to(dtype)
    g = torch.Generator().manual_seed(B * 7919 + D * 31 + H)
    g_out = torch.randn(B, D, generator=g)
    g_ldj = torch.randn(B, generator=g)
    p64 = p_in.double().requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    out, ldj = reference.dsf_transform(p64, x64, H, inverse)
    dp, gx = torch.autograd.grad((out * g_out.double()).sum() + (ldj * g_ldj.double()).sum(),
                                 (p64, x64))
    return dict(B=B, D=D, H=H, params=p_in, x=x, g_out=g_out, g_ldj=g_ldj, out=out.detach(),
                ldj=ldj.detach(), dparams=dp, gx=gx)


def _ratio(got, ref, atol, rtol):
    err = (got.double().cpu() - ref).abs()
    return float((err / (atol + rtol * ref.abs())).max()), float(err.max())


def check_outputs(out, ldj, o, inverse, frac=1.0):
    """The direction's outputs against the fp64 composite, at ``frac`` of the limits. Forward: y
    and ldj themselves. Inverse: an fp32 root is only determined to ulp(y) / y', so what is well
    conditioned is compared: the fp64 forward map applied to the recovered x reproduces y, and
    ldj equals -L of the fp64 composite at that same x. No element is left out."""
    D, H = o["D"], o["H"]
    out64, p64 = out.double().cpu(), o["params"].double()
    if inverse:
        y_back, L = reference.dsf_transform(p64, out64, H)
        pairs = [("f64(x) vs y", y_back, o["x"].double(), Y_ATOL, Y_RTOL),
                 ("ldj vs -L(x)", ldj, -L, ldj_atol(D), LDJ_RTOL)]
    else:
        pairs = [("y", out, o["out"], Y_ATOL, Y_RTOL), ("ldj", ldj, o["ldj"], ldj_atol(D), LDJ_RTOL)]
    for what, got, ref, atol, rtol in pairs:
        r, e = _ratio(got, ref, atol, rtol)
        print(f"{what}: max err {e:.3e}, worst err/limit {r:.4f} (allowed {frac})")
        assert r <= frac, what


def check_grads(dparams, gx, o, frac=1.0):
    """|delta| <= frac * 2e-3 (1 + max|ref|); a bf16 dparams gets 2^-8 |ref| per element on top
    for its output rounding, which is the format's and not the arithmetic's (not scaled)."""
    bf16 = o["params"].dtype == torch.bfloat16
    for what, got, ref, rel in (("gx", gx, o["gx"], 0.0),
                                ("dparams", dparams, o["dparams"], BF16_ROUND if bf16 else 0.0)):
        err = (got.double().cpu() - ref).abs()
        base = GRAD_TOL * (1 + float(ref.abs().max()))
        r = float(((err - rel * ref.abs()).clamp_min(0) / base).max())
        print(f"{what}: max err {float(err.max()):.3e}, max|ref| {float(ref.abs().max()):.3e}, "
              f"worst err/limit {r:.4f} (allowed {frac})")
        assert r <= frac, what


# ------------------------------------------------------------------ the fp64 composite
def _rand(B, D, H, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(B, 3 * H * D, generator=g, dtype=torch.float64) * scale
    x = torch.randn(B, D, generator=g, dtype=torch.float64) * 1.5
    return p, x


SHAPES = [(1, 1, 1), (6, 5, 8), (9, 7, 17), (4, 3, 32)]


@pytest.mark.parametrize("B,D,H", SHAPES)
def test_ldj_is_log_of_jacobian_diagonal(B, D, H):
    p, x = _rand(B, D, H, seed=2)
    for inv in (False, True):
        xx = x.clone().requires_grad_(True)
        y, ldj = dsf_transform(p, xx, H, inverse=inv)
        (dy,) = torch.autograd.grad(y.sum(), xx)   # element-wise map: the Jacobian diagonal
        assert (dy > 0).all()
        assert (dy.log().sum(1) - ldj).abs().max() <= 1e-10


@pytest.mark.parametrize("B,D,H", SHAPES)
def test_zero_params_is_identity(B, D, H):
    _, x = _rand(B, D, H)
    for dtype, ytol, ltol in ((torch.float64, 1e-12, 1e-12), (torch.float32, 1e-6, 1e-5)):
        p = torch.zeros(B, 3 * H * D, dtype=dtype)
        for inv in (False, True):
            y, ldj = dsf_transform(p, x.to(dtype), H, inverse=inv)
            assert y.dtype == dtype and ldj.shape == (B,)
            assert (y - x.to(dtype)).abs().max() <= ytol
            assert ldj.abs().max() <= ltol


@pytest.mark.parametrize("B,D,H", SHAPES)
def test_units_and_envelope(B, D, H):
    p, x = _rand(B, D, H, seed=1, scale=1.5)
    a, b, logw = dsf_units(p, H)
    assert a.shape == b.shape == logw.shape == (B, H, D)
    assert (a > 0).all() and (logw.exp().sum(1) - 1).abs().max() <= 1e-12
    assert torch.equal(b, p.view(B, 3 * H, D)[:, H:2 * H])
    y, _ = dsf_transform(p, x, H)
    lo, hi = envelope(p, x, H)
    assert (y >= lo - 1e-12).all() and (y <= hi + 1e-12).all()


def test_strictly_increasing_on_a_sorted_grid():
    H, n = 8, 4001
    p, _ = _rand(1, 3, H, seed=6, scale=1.5)
    grid = torch.linspace(-12.0, 12.0, n, dtype=torch.float64)
    x = grid[:, None].expand(n, 3).contiguous()
    for inv in (False, True):
        y, _ = dsf_transform(p.expand(n, -1), x, H, inverse=inv)
        assert (y[1:] - y[:-1] > 0).all()


@pytest.mark.parametrize("B,D,H", SHAPES + [(64, 40, 8)])
def test_inverse_round_trip(B, D, H):
    p, x = _rand(B, D, H, seed=3)
    y, ldj = dsf_transform(p, x, H)
    xr, ldj_inv = dsf_transform(p, y, H, inverse=True)
    assert (xr - x).abs().max() <= 1e-8
    assert (ldj + ldj_inv).abs().max() <= 1e-8


@pytest.mark.parametrize("B,D,H", [(1, 1, 1), (2, 2, 3), (2, 1, 8)])
def test_inverse_gradients_are_the_implicit_function_gradients(B, D, H):
    """The re-attached inverse against torch.autograd.functional.jacobian of the forward map,
    inverted by hand: dx/dy = 1 / f_x, dx/dp = -f_p / f_x (element-wise map: row r, column d of
    x depends on y[r, d] and on params row r only), and d ldj_inv = -(L_p dp + L_x dx)."""
    from torch.autograd.functional import jacobian

    p, y = _rand(B, D, H, seed=4)
    pp, yy = p.clone().requires_grad_(True), y.clone().requires_grad_(True)
    x, ldj = dsf_transform(pp, yy, H, inverse=True)
    xs = x.detach()
    Jp_y, Jx_y = jacobian(lambda q, v: dsf_transform(q, v, H)[0], (p, xs))    # [B,D,B,P], [B,D,B,D]
    Jp_L, Jx_L = jacobian(lambda q, v: dsf_transform(q, v, H)[1], (p, xs))    # [B,B,P], [B,B,D]
    for r in range(B):
        for d in range(D):
            gp, gy = torch.autograd.grad(x[r, d], (pp, yy), retain_graph=True)
            fx = Jx_y[r, d, r, d]
            want_p = torch.zeros_like(p)
            want_p[r] = -Jp_y[r, d, r] / fx
            want_y = torch.zeros_like(y)
            want_y[r, d] = 1.0 / fx
            assert (gp - want_p).abs().max() <= 1e-9 and (gy - want_y).abs().max() <= 1e-9
        gp, gy = torch.autograd.grad(ldj[r], (pp, yy), retain_graph=True)
        dxdy = 1.0 / torch.diagonal(Jx_y[r, :, r, :])                          # [D]
        dxdp = -Jp_y[r, :, r] * dxdy[:, None]                                  # [D, P]
        want_p = torch.zeros_like(p)
        want_p[r] = -(Jp_L[r, r] + Jx_L[r, r] @ dxdp)
        want_y = torch.zeros_like(y)
        want_y[r] = -Jx_L[r, r] * dxdy
        assert (gp - want_p).abs().max() <= 1e-9 and (gy - want_y).abs().max() <= 1e-9


def test_float32_composite_and_shape_errors():
    p, x = make_inputs(6, 5, 8)
    y, ldj = dsf_transform(p, x, 8)
    assert y.dtype == torch.float32 and ldj.dtype == torch.float32 and ldj.shape == (6,)
    y64, ldj64 = dsf_transform(p.double(), x.double(), 8)
    assert (y - y64).abs().max() <= 1e-5 and (ldj - ldj64).abs().max() <= 1e-4
    with pytest.raises(ValueError):
        dsf_transform(p[:, :-1], x, 8)
    with pytest.raises(ValueError):
        dsf_transform(torch.zeros(2, 0), torch.zeros(2, 1), 0)
    with pytest.raises(ValueError):
        dsf_transform(torch.zeros(2, 99), torch.zeros(2, 1), 33)
    with pytest.raises(ValueError):
        dsf_transform(torch.zeros(3, 24), torch.zeros(2, 1), 8)


def test_robust_to_large_inputs_and_parameters():
    """fp32, |x| up to 1e4, raw parameters of scale 4: everything finite, y inside the envelope
    (up to the rounding of p_h itself)."""
    p, x, H = make_robust_inputs()
    assert float(x.abs().max()) == 1e4
    pp, xx = p.clone().requires_grad_(True), x.clone().requires_grad_(True)
    y, ldj = dsf_transform(pp, xx, H)
    gp, gx = torch.autograd.grad(y.sum() + ldj.sum(), (pp, xx))
    for t in (y, ldj, gp, gx):
        assert torch.isfinite(t).all()
    lo, hi = envelope(p.double(), x.double(), H)
    slack = 1e-6 * torch.maximum(lo.abs(), hi.abs()) + 1e-6
    assert (y.double() >= lo - slack).all() and (y.double() <= hi + slack).all()
    xr, ldj_inv = dsf_transform(p, y.detach(), H, inverse=True)
    assert torch.isfinite(xr).all() and torch.isfinite(ldj_inv).all()


# ------------------------------------------------------------------------- modules
def _randomise_last_layers(flow, std, seed):
    """Draw the last conditioner layer of every DSF layer (masked for a MADE)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for layer in getattr(flow, "layers", [flow]):
            if hasattr(layer, "net"):
                last = layer.net[-1]
            elif hasattr(layer, "made"):
                last = layer.made.layers[-1]
            else:
                continue
            last.weight.copy_(torch.randn(last.weight.shape, generator=g) * std)
            last.bias.copy_(torch.randn(last.bias.shape, generator=g) * std)
            if hasattr(last, "mask"):
                last.weight.mul_(last.mask)


def test_modules_start_at_the_identity():
    from vi_normflows_amd.flows import DSFAutoregressive, DSFCoupling

    torch.manual_seed(0)
    x = torch.randn(32, 5, dtype=torch.float64) * 2
    for parity in (0, 1):
        f = DSFCoupling(5, units=4, hidden=8, parity=parity).double()
        assert f.invertible and f.net[-1].out_features == 3 * 4 * f.d_b
        y, ldj = f(x)
        assert (y - x).abs().max() <= 1e-12 and ldj.abs().max() <= 1e-12
    f = DSFAutoregressive(5, units=4, hidden=16).double()
    assert f.invertible and f.made.out_mult == 12
    y, ldj = f(x)
    assert (y - x).abs().max() <= 0.1 and ldj.abs().max() <= 0.25   # 1e-2-scaled last layer
    with pytest.raises(ValueError):
        DSFCoupling(4, units=33)
    with pytest.raises(ValueError):
        DSFAutoregressive(4, units=0)


@pytest.mark.parametrize("reverse", [False, True])
def test_autoregressive_jacobian_is_triangular_in_the_made_order(reverse):
    from torch.autograd.functional import jacobian
    from vi_normflows_amd.flows import DSFAutoregressive

    torch.manual_seed(1)
    f = DSFAutoregressive(5, units=3, hidden=16, reverse=reverse).double()
    _randomise_last_layers(f, 0.5, seed=3)
    x = torch.randn(5, dtype=torch.float64)
    J = jacobian(lambda v: f(v[None])[0][0], x)
    order = f.made.order
    later = order[None, :] > order[:, None]          # input j comes after output i
    assert (J[later] == 0).all()
    assert (torch.diagonal(J) > 0).all()
    assert abs(float(torch.diagonal(J).log().sum() - f(x[None])[1][0].detach())) <= 1e-10
    earlier = order[None, :] < order[:, None]
    assert (J[earlier] != 0).any()


def test_modules_invert():
    from vi_normflows_amd.flows import DSFAutoregressive, NeuralAutoregressiveFlow

    torch.manual_seed(2)
    x = torch.randn(24, 5, dtype=torch.float64) * 2
    ctx = torch.randn(24, 2, dtype=torch.float64)
    flow = NeuralAutoregressiveFlow(5, n_layers=3, units=4, hidden=8, conditioner="coupling",
                                    context_dim=2).double()
    assert flow.uses_context and flow.invertible
    assert [f.parity for f in flow.layers] == [0, 1, 0]
    _randomise_last_layers(flow, 0.5, seed=8)
    y, ldj = flow(x, ctx)
    xr, ldj_inv = flow.inverse(y, ctx)
    assert (y - x).abs().max() > 1e-2
    assert (xr - x).abs().max() <= 1e-8 and (ldj + ldj_inv).abs().max() <= 1e-8
    for reverse in (False, True):
        f = DSFAutoregressive(5, units=4, hidden=16, reverse=reverse, context_dim=2).double()
        _randomise_last_layers(f, 0.5, seed=9)
        y, ldj = f(x, ctx)
        xr, ldj_inv = f.inverse(y, ctx)
        assert (y - x).abs().max() > 1e-2 and not xr.requires_grad
        assert (xr - x).abs().max() <= 1e-8 and (ldj + ldj_inv).abs().max() <= 1e-8
    flow = NeuralAutoregressiveFlow(4, n_layers=2, units=3, hidden=8).double()
    _randomise_last_layers(flow, 0.5, seed=10)
    y, ldj = flow(x[:, :4])
    xr, ldj_inv = flow.inverse(y)
    assert (xr - x[:, :4]).abs().max() <= 1e-8 and (ldj + ldj_inv).abs().max() <= 1e-8


def test_build_flow_naf_and_state_dict_round_trip():
    import normflows.flows as shim
    from vi_normflows_amd import flows
    from vi_normflows_amd.flows.base import Reverse
    from vi_normflows_amd.inference.flow_vi import build_flow

    for name in ("DSFCoupling", "DSFAutoregressive", "NeuralAutoregressiveFlow"):
        assert getattr(shim, name) is getattr(flows, name) and name in flows.__all__
    a = build_flow("naf", 2, 4)
    assert isinstance(a, flows.NeuralAutoregressiveFlow) and a.conditioner == "made"
    assert [type(f) for f in a.layers] == [flows.DSFAutoregressive, Reverse] * 3 + \
        [flows.DSFAutoregressive]
    assert a.layers[0].units == 8
    c = build_flow("naf", 3, 4, conditioner="coupling", units=5, hidden=8)
    assert [f.parity for f in c.layers] == [0, 1, 0, 1] and c.layers[0].units == 5
    with pytest.raises(ValueError):
        build_flow("naf", 2, 2, conditioner="dense")
    for kw in (dict(), dict(conditioner="coupling")):
        a, b = build_flow("naf", 2, 3, **kw), build_flow("naf", 2, 3, **kw)
        _randomise_last_layers(a, 0.5, seed=9)
        b.load_state_dict(a.state_dict())
        x = torch.randn(16, 2)
        (ya, la), (yb, lb) = a(x), b(x)
        assert torch.equal(ya, yb) and torch.equal(la, lb) and (ya - x).abs().max() > 1e-3


def test_train_cli_naf(tmp_path):
    from vi_normflows_amd.train import main

    out = main(["--config", "config1_two_moons_cpu", "flow=naf", "K=2", "iters=20",
                "log_every=10", "extra.units=4", "extra.conditioner=coupling",
                f"out_dir={tmp_path}"])
    assert math.isfinite(out["free_energy"])
    sd = torch.load(tmp_path / "config1_two_moons_cpu" / "flow.pt")
    assert sd["layers.0.net.2.weight"].shape[0] == 3 * 4   # extra.units reached the flow


def test_naf_density_normalises():
    """exp(log_prob) of a non-trivial 2-D coupling NAF integrates to 1 on a 601^2 grid over
    [-8, 8]^2, within 2e-3 (as test_neural_spline_flow_density_normalises). The same sum for
    the base density alone gives the grid's own error, which has to stay at least 10x below
    that bound so that the bound tests the flow and not the grid. The last layers are drawn
    with std 0.1: the flow then moves points by up to 6 units with |ldj| up to 1.9; the ReLU
    conditioners are unbounded, and from std 0.15 on the slopes at the far corners of the grid
    get so small (1e-145 at std 0.3) that three stacked layers leave the range of fp64 and the
    sum is NaN; at std 0.1 it is within 1e-6 of 1."""
    from vi_normflows_amd.distributions.base import StdNormal
    from vi_normflows_amd.flows import FlowDistribution, NeuralAutoregressiveFlow

    torch.manual_seed(0)
    flow = NeuralAutoregressiveFlow(2, n_layers=3, units=4, hidden=16,
                                    conditioner="coupling").double()
    _randomise_last_layers(flow, 0.1, seed=7)
    dist = FlowDistribution(StdNormal(2), flow)
    n = 601
    ax = torch.linspace(-8.0, 8.0, n, dtype=torch.float64)
    hstep = float(ax[1] - ax[0])
    pts = torch.cartesian_prod(ax, ax)
    with torch.no_grad():
        z, ldj = flow(pts[::97])
        assert (z - pts[::97]).abs().max() > 0.1 and ldj.abs().max() > 0.1   # not the identity
        total = float(dist.log_prob(pts).exp().sum()) * hstep * hstep
        grid_err = abs(float(StdNormal(2).log_prob(pts).exp().sum()) * hstep * hstep - 1.0)
    print(f"integral {total:.6f}, grid error for the base {grid_err:.2e}")
    assert 10 * grid_err <= 2e-3
    assert abs(total - 1.0) <= 2e-3


@functools.lru_cache(maxsize=None)
def _planar_u1_kl():
    from vi_normflows_amd.inference.flow_vi import fit_flow_vi

    return fit_flow_vi("U1", "planar", K=8, iters=300, lr=5e-3, n_samples=512, optimizer="adam",
                       init="random").final["kl_estimate"]


U1_MEASURED = {"coupling": 0.144, "made": 0.053}   # kl_estimate of a CPU run of this test


@pytest.mark.parametrize("conditioner", ["coupling", "made"])
def test_naf_vi_beats_planar_on_u1(conditioner):
    """KL(q || p) = F + log Z on U1, 4 DSF layers of 8 units, Adam lr 5e-3, 300 iterations, 512
    samples: above the project's floor tolerance (-0.05), below a random-init planar stack of
    K = 8 trained here on the same budget (0.83), and below twice what a CPU run of this
    implementation reached: 0.144 with coupling conditioners (one hidden layer of 64), 0.053
    with MADE conditioners."""
    from vi_normflows_amd.inference.flow_vi import fit_flow_vi

    kl = fit_flow_vi("U1", "naf", K=4, iters=300, lr=5e-3, n_samples=512, optimizer="adam",
                     units=8, conditioner=conditioner).final["kl_estimate"]
    kl_planar = _planar_u1_kl()
    print(f"U1 kl_estimate: naf/{conditioner} {kl:.4f}, planar {kl_planar:.4f}")
    assert kl > -0.05
    assert kl < kl_planar
    assert kl < 2 * U1_MEASURED[conditioner]


@pytest.mark.skipif(not os.path.exists(LIB), reason="native library not built")
def test_native_library_registers_dsf_ops():
    code = ("import torch; torch.ops.load_library(%r); "
            "print('HAVE', hasattr(torch.ops.vinf, 'dsf_fwd'), hasattr(torch.ops.vinf, 'dsf_bwd'))"
            % LIB)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       cwd="/tmp")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "HAVE True True" in r.stdout, r.stdout


# ---------------------------------------------------------------- input helper
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", GPU_CASES, ids=["%dx%dh%d" % c for c in GPU_CASES])
def test_gpu_inputs_leave_the_tolerances_to_the_kernel(case, dtype, inverse):
    """The fp32 composite on exactly the GPU tests' inputs sits within 0.25 of every GPU limit
    against the fp64 composite, outputs and all gradients, both directions: the limits then
    test the kernel and not the conditioning of the inputs. The factor 4 left over is for the
    device's fast exp / log / rcp, a few ulp looser than libm."""
    B, D, H = case
    o = oracle(case, dtype, inverse)
    assert make_inputs(B, D, H)[1].equal(o["x"])     # seeded
    p = o["params"].clone().requires_grad_(True)
    x = o["x"].clone().requires_grad_(True)
    out, ldj = reference.dsf_transform(p, x, H, inverse)
    assert out.dtype == torch.float32
    ((out * o["g_out"]).sum() + (ldj * o["g_ldj"]).sum()).backward()
    assert p.grad.dtype == dtype
    check_outputs(out.detach(), ldj.detach(), o, inverse, frac=0.25)
    check_grads(p.grad, x.grad, o, frac=0.25)
