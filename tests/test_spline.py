"""Rational-quadratic spline coupling: the torch composite against the definition, the flow
modules, the VI / CLI plumbing (CPU, fp64 unless said), and the input helper shared with
``test_spline_gpu.py``."""
import math
import os
import subprocess
import sys

import pytest
import torch

from vi_normflows_amd.ops.reference import RQS_MIN, rqs_knots
from vi_normflows_amd.ops.spline import rqs_transform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "vi_normflows_amd", "_native", "libvinf_hip.so")

# (B, Dh, K) of the GPU tests: one row and one column; B no multiple of 4; Dh on either side of
# the wave width; more than two lane strides; K at and just past each register-array size
# (8, 16, 32); the headline half-width.
GPU_CASES = [(1, 1, 2), (5, 3, 4), (7, 63, 5), (6, 64, 8), (9, 65, 9), (257, 130, 8),
             (33, 7, 16), (12, 20, 17), (10, 24, 32), (64, 392, 8)]
SEED = 3
KNOT_EPS = 1e-4   # in units of bound


def case_bound(K):
    return 5.0 if K == 16 else 3.0


def make_inputs(B, Dh, K, bound, seed=SEED):
    """fp32 ``params`` [B, (3K-1) Dh] and ``x`` [B, Dh], seeded on the CPU generator (one
    stream per shape)."""
    g = torch.Generator().manual_seed(seed * 1_000_003 + (B * 1009 + Dh) * 37 + K)
    params = torch.randn(B, (3 * K - 1) * Dh, generator=g) * 0.5
    x = torch.randn(B, Dh, generator=g) * (1.6 * bound / 3)
    return params, x


def near_knot(params64, v64, K, bound, inverse=False):
    """[B, Dh] mask: v within KNOT_EPS * bound of a knot (the fp64 x-knots, or y-knots for the
    inverse direction). The gradient of ldj jumps there, and an fp32 knot can land on the
    other side of v."""
    xk, _, yk, _, _ = rqs_knots(params64, K, bound)
    kn = yk if inverse else xk
    return ((v64.unsqueeze(1) - kn).abs() <= KNOT_EPS * bound).any(1)


def _rand(B, Dh, K, bound, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(B, (3 * K - 1) * Dh, generator=g, dtype=torch.float64) * scale
    x = torch.randn(B, Dh, generator=g, dtype=torch.float64) * (1.6 * bound / 3)
    return p, x


SHAPES = [(1, 1, 2, 3.0), (6, 5, 8, 3.0), (9, 7, 17, 5.0), (4, 3, 32, 3.0)]


@pytest.mark.parametrize("B,Dh,K,bound", SHAPES)
def test_zero_params_is_identity(B, Dh, K, bound):
    _, x = _rand(B, Dh, K, bound)
    p = torch.zeros(B, (3 * K - 1) * Dh, dtype=torch.float64)
    for inv in (False, True):
        y, ldj = rqs_transform(p, x, K, bound, inverse=inv)
        assert (y - x).abs().max() <= 1e-12
        assert ldj.abs().max() <= 1e-12


@pytest.mark.parametrize("B,Dh,K,bound", SHAPES)
def test_spline_passes_through_its_knots(B, Dh, K, bound):
    """Against the definition, not against itself: x_k maps to y_k with slope d_k."""
    p, _ = _rand(B, Dh, K, bound, seed=1)
    xk, w, yk, h, d = rqs_knots(p, K, bound)
    assert xk.shape == (B, K + 1, Dh) and w.shape == (B, K, Dh)
    assert (xk[:, 0] == -bound).all() and (xk[:, -1] == bound).all()
    assert (yk[:, 0] == -bound).all() and (yk[:, -1] == bound).all()
    assert (d[:, 0] == 1).all() and (d[:, -1] == 1).all()
    assert w.min() >= 2 * bound * RQS_MIN and h.min() >= 2 * bound * RQS_MIN and d.min() >= RQS_MIN
    assert (w.sum(1) - 2 * bound).abs().max() <= 1e-12
    for k in range(K + 1):
        x = xk[:, k].clone().requires_grad_(True)
        y, _ = rqs_transform(p, x, K, bound)
        (dy,) = torch.autograd.grad(y.sum(), x)
        assert (y - yk[:, k]).abs().max() <= 1e-10, k
        assert (dy - d[:, k]).abs().max() <= 1e-10, k


@pytest.mark.parametrize("B,Dh,K,bound", SHAPES)
def test_ldj_is_log_of_jacobian_diagonal(B, Dh, K, bound):
    p, x = _rand(B, Dh, K, bound, seed=2)
    for inv in (False, True):
        xx = x.clone().requires_grad_(True)
        y, ldj = rqs_transform(p, xx, K, bound, inverse=inv)
        (dy,) = torch.autograd.grad(y.sum(), xx)   # element-wise map: the Jacobian diagonal
        assert (dy > 0).all()
        assert (dy.log().sum(1) - ldj).abs().max() <= 1e-10


@pytest.mark.parametrize("B,Dh,K,bound", SHAPES + [(64, 392, 8, 3.0)])
def test_inverse_round_trip(B, Dh, K, bound):
    p, x = _rand(B, Dh, K, bound, seed=3)
    y, ldj = rqs_transform(p, x, K, bound)
    xr, ldj_inv = rqs_transform(p, y, K, bound, inverse=True)
    assert (xr - x).abs().max() <= 1e-8
    assert (ldj + ldj_inv).abs().max() <= 1e-8


def test_tails_are_identity_with_zero_parameter_gradient():
    B, Dh, K, bound = 4, 6, 5, 2.0
    p, _ = _rand(B, Dh, K, bound, seed=4)
    g = torch.Generator().manual_seed(5)
    x = bound + torch.rand(B, Dh, generator=g, dtype=torch.float64) * 3.0
    x[:, ::2] *= -1
    x[0, 0], x[0, 1] = bound, -bound       # the end knots belong to the tails
    for inv in (False, True):
        pp, xx = p.clone().requires_grad_(True), x.clone().requires_grad_(True)
        y, ldj = rqs_transform(pp, xx, K, bound, inverse=inv)
        assert torch.equal(y, xx) and (ldj == 0).all()
        gy = torch.randn(B, Dh, generator=g, dtype=torch.float64)
        gl = torch.randn(B, generator=g, dtype=torch.float64)
        gp, gx = torch.autograd.grad((y * gy).sum() + (ldj * gl).sum(), (pp, xx))
        assert (gp == 0).all() and torch.equal(gx, gy)


def test_strictly_increasing_on_a_sorted_grid():
    K, bound, n = 8, 3.0, 4001
    p, _ = _rand(1, 3, K, bound, seed=6, scale=1.5)
    grid = torch.linspace(-1.2 * bound, 1.2 * bound, n, dtype=torch.float64)
    x = grid[:, None].expand(n, 3).contiguous()
    for inv in (False, True):
        y, _ = rqs_transform(p.expand(n, -1), x, K, bound, inverse=inv)
        assert (y[1:] - y[:-1] > 0).all()


def test_float32_composite_and_shape_errors():
    p, x = make_inputs(6, 5, 8, 3.0)
    y, ldj = rqs_transform(p, x, 8, 3.0)
    assert y.dtype == torch.float32 and ldj.dtype == torch.float32 and ldj.shape == (6,)
    y64, ldj64 = rqs_transform(p.double(), x.double(), 8, 3.0)
    assert (y - y64).abs().max() <= 1e-5 and (ldj - ldj64).abs().max() <= 1e-4
    with pytest.raises(ValueError):
        rqs_transform(p[:, :-1], x, 8, 3.0)
    with pytest.raises(ValueError):
        rqs_transform(torch.zeros(2, 2), torch.zeros(2, 1), 1, 3.0)
    with pytest.raises(ValueError):
        rqs_transform(torch.zeros(2, 98), torch.zeros(2, 1), 33, 3.0)
    with pytest.raises(ValueError):
        rqs_transform(p, x, 8, 0.0)


@pytest.mark.parametrize("B,Dh,K", GPU_CASES)
def test_gpu_input_helper_conditions(B, Dh, K):
    """What the GPU tests rely on, verified without a GPU: few elements sit next to a knot
    (they are left out of the gradient comparison), and both the tails and the interval get
    their share of elements."""
    bound = case_bound(K)
    p, x = make_inputs(B, Dh, K, bound)
    n = B * Dh
    for inv in (False, True):
        near = int(near_knot(p.double(), x.double(), K, bound, inv).sum())
        assert near <= 0.01 * n, (near, n)
        if n < 100:
            assert near == 0
    tail = float(((x <= -bound) | (x >= bound)).float().mean())
    if n >= 1000:
        assert 0.02 <= tail <= 0.15, tail
    # bf16-rounded params (the bf16 kernels' oracle input) obey the same cap
    pb = p.to(torch.bfloat16).double()
    for inv in (False, True):
        assert int(near_knot(pb, x.double(), K, bound, inv).sum()) <= 0.01 * n


def _randomise_last_layers(flow, std, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for layer in getattr(flow, "layers", [flow]):
            last = layer.net[-1]
            last.weight.copy_(torch.randn(last.weight.shape, generator=g) * std)
            last.bias.copy_(torch.randn(last.bias.shape, generator=g) * std)


def test_neural_spline_flow_density_normalises():
    """exp(log_prob) of a non-trivial 2-D spline flow integrates to 1 on a 601^2 grid over
    [-6, 6]^2, within 2e-3. The same sum for the base density alone gives the grid's own error
    (truncation at 6 sigma plus quadrature), which has to stay at least 10x below that bound
    so that the bound tests the flow and not the grid. The last layers are drawn with std 0.4:
    the flow then moves points by several units with |ldj| up to ~9, while its density is
    still resolved by the 0.02 spacing (the sum is within 4e-5 of 1, and closer on finer
    grids; std 0.7 gives bins so narrow that the 601^2 sum is 4e-3 off and only converges to 1
    under refinement)."""
    from vi_normflows_amd.distributions.base import StdNormal
    from vi_normflows_amd.flows import FlowDistribution, NeuralSplineFlow

    torch.manual_seed(0)
    flow = NeuralSplineFlow(2, n_layers=3, bins=6, bound=3.0, hidden=16).double()
    _randomise_last_layers(flow, 0.4, seed=7)
    dist = FlowDistribution(StdNormal(2), flow)
    n = 601
    ax = torch.linspace(-6.0, 6.0, n, dtype=torch.float64)
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


def test_module_identity_at_init_and_inverse():
    from vi_normflows_amd.flows import NeuralSplineFlow, RQSCoupling

    torch.manual_seed(0)
    x = torch.randn(32, 5, dtype=torch.float64) * 2
    for parity in (0, 1):
        f = RQSCoupling(5, bins=5, hidden=8, parity=parity).double()
        assert f.invertible and f.net[-1].out_features == (3 * 5 - 1) * f.d_b
        y, ldj = f(x)
        assert (y - x).abs().max() <= 1e-12 and ldj.abs().max() <= 1e-12
    flow = NeuralSplineFlow(5, n_layers=3, bins=5, hidden=8, context_dim=2).double()
    assert flow.uses_context and flow.invertible
    _randomise_last_layers(flow, 0.5, seed=8)
    ctx = torch.randn(32, 2, dtype=torch.float64)
    y, ldj = flow(x, ctx)
    xr, ldj_inv = flow.inverse(y, ctx)
    assert (y - x).abs().max() > 1e-2
    assert (xr - x).abs().max() <= 1e-8 and (ldj + ldj_inv).abs().max() <= 1e-8


def test_build_flow_nsf_and_state_dict_round_trip():
    import normflows.flows as shim
    from vi_normflows_amd.flows import NeuralSplineFlow
    from vi_normflows_amd.inference.flow_vi import build_flow

    assert shim.NeuralSplineFlow is NeuralSplineFlow
    a = build_flow("nsf", 2, 4)
    assert isinstance(a, NeuralSplineFlow) and len(a.layers) == 4
    assert a.layers[0].bins == 8 and a.layers[0].bound == 4.0
    assert [f.parity for f in a.layers] == [0, 1, 0, 1]
    _randomise_last_layers(a, 0.5, seed=9)
    b = build_flow("nsf", 2, 4)
    b.load_state_dict(a.state_dict())
    x = torch.randn(16, 2)
    (ya, la), (yb, lb) = a(x), b(x)
    assert torch.equal(ya, yb) and torch.equal(la, lb) and (ya - x).abs().max() > 1e-3
    c = build_flow("nsf", 2, 2, bins=4, bound=2.5, hidden=8)
    assert c.layers[0].bins == 4 and c.layers[0].bound == 2.5


def test_nsf_vi_reaches_the_u1_floor():
    """KL(q || p) = F + log Z: above the project's floor tolerance (-0.05, as in
    test_flow_vi_respects_kl_floor_on_normalised_gmm) and below 0.15, 3x what a prototype with
    plain linear conditioners reached on U1 (0.024 - 0.029)."""
    from vi_normflows_amd.inference.flow_vi import fit_flow_vi

    r = fit_flow_vi("U1", "nsf", K=4, iters=300, lr=5e-3, n_samples=512, optimizer="adam",
                    bins=8, bound=4.0)
    kl = r.final["kl_estimate"]
    print(f"U1 nsf kl_estimate {kl:.4f}")
    assert kl > -0.05
    assert kl < 0.15


def test_train_cli_nsf(tmp_path):
    from vi_normflows_amd.train import main

    out = main(["--config", "config1_two_moons_cpu", "flow=nsf", "K=2", "iters=20",
                "log_every=10", "extra.bins=4", f"out_dir={tmp_path}"])
    assert math.isfinite(out["free_energy"])
    sd = torch.load(tmp_path / "config1_two_moons_cpu" / "flow.pt")
    assert sd["layers.0.net.4.weight"].shape[0] == 3 * 4 - 1   # extra.bins reached the flow


@pytest.mark.skipif(not os.path.exists(LIB), reason="native library not built")
def test_native_library_registers_spline_ops():
    code = ("import torch; torch.ops.load_library(%r); "
            "print('HAVE', hasattr(torch.ops.vinf, 'rqs_fwd'), hasattr(torch.ops.vinf, 'rqs_bwd'))"
            % LIB)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       cwd="/tmp")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "HAVE True True" in r.stdout, r.stdout
