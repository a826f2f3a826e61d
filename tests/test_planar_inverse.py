"""Inverses of the planar and radial stacks on the CPU (fp64 composites): round trips, the
independent ``planar_pushforward`` density, gradients, normalisation, module flags, and
maximum-likelihood recovery of the known planar flow."""
import importlib.util
import math
import sys
from pathlib import Path

import pytest
import torch

from vi_normflows_amd.distributions.base import StdNormal
from vi_normflows_amd.distributions.energies import planar_pushforward
from vi_normflows_amd.flows import (AmortizedPlanar, AmortizedRadial, FlowDistribution,
                                    FlowSequence, Planar, PlanarStack, Radial, RadialStack,
                                    planar_stack_inverse, planar_stack_inverse_reference,
                                    planar_stack_reference, radial_params, radial_stack_inverse,
                                    radial_stack_inverse_reference, radial_stack_reference)
from vi_normflows_amd.inference.flow_vi import build_flow, fit_density

F64 = torch.float64
EX = Path(__file__).resolve().parents[1] / "examples"


def _planar_params(K, N, D, per_sample, g):
    shp = (K, N, D) if per_sample else (K, D)
    std = 1.5 / math.sqrt(D)
    return (torch.randn(*shp, dtype=F64, generator=g) * std,
            torch.randn(*shp, dtype=F64, generator=g) * std,
            torch.randn(*shp[:-1], dtype=F64, generator=g) * std)


def _radial_params(K, N, D, per_sample, g):
    shp = (K, N, D) if per_sample else (K, D)
    std = 1.5 / math.sqrt(D)
    al, be = radial_params(torch.randn(*shp[:-1], dtype=F64, generator=g) * std,
                           torch.randn(*shp[:-1], dtype=F64, generator=g) * std)
    return torch.randn(*shp, dtype=F64, generator=g) * std, al, be


@pytest.mark.parametrize("D", [1, 2, 5])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("kind", ["planar", "radial", "planar+radial"])
def test_round_trip(kind, per_sample, K, D):
    N = 33
    g = torch.Generator().manual_seed(100 * D + 10 * K + per_sample)
    x = torch.randn(N, D, dtype=F64, generator=g)
    P, R = _planar_params(K, N, D, per_sample, g), _radial_params(K, N, D, per_sample, g)
    y, lf = x, torch.zeros(N, dtype=F64)
    if "planar" in kind:
        y, l = planar_stack_reference(y, *P)
        lf = lf + l
    if "radial" in kind:
        y, l = radial_stack_reference(y, *R)
        lf = lf + l
    assert (y - x).abs().max() > 1e-3      # not the identity
    xi, li = y, torch.zeros(N, dtype=F64)
    if "radial" in kind:
        xi, l = radial_stack_inverse(xi, *R)
        li = li + l
    if "planar" in kind:
        xi, l = planar_stack_inverse(xi, *P)
        li = li + l
    print(f"|dx| {float((xi - x).abs().max()):.2e}  |ldj_f + ldj_i| {float((lf + li).abs().max()):.2e}")
    assert (xi - x).abs().max() <= 1e-10
    assert (lf + li).abs().max() <= 1e-10


def test_modules_round_trip_and_amortized_context():
    g = torch.Generator().manual_seed(3)
    N, D, K = 33, 2, 3
    x = torch.randn(N, D, dtype=F64, generator=g)
    for flow in (PlanarStack(D, K, init="random", generator=g), Planar(D, init="random", generator=g),
                 RadialStack(D, K, generator=g), Radial(D, generator=g), build_flow("planar+radial", D, K)):
        flow = flow.double()
        with torch.no_grad():
            y, lf = flow(x)
            xi, li = flow.inverse(y)
        assert (xi - x).abs().max() <= 1e-10 and (lf + li).abs().max() <= 1e-10
    P = _planar_params(K, N, D, True, g)
    ap = AmortizedPlanar(D, K)
    y, lf = ap(x, P)
    xi, li = ap.inverse(y, P)
    assert (xi - x).abs().max() <= 1e-10 and (lf + li).abs().max() <= 1e-10
    ctx = (torch.randn(K, N, D, dtype=F64, generator=g), torch.randn(K, N, dtype=F64, generator=g),
           torch.randn(K, N, dtype=F64, generator=g))
    ar = AmortizedRadial(D, K)
    y, lf = ar(x, ctx)
    xi, li = ar.inverse(y, ctx)
    assert (xi - x).abs().max() <= 1e-10 and (lf + li).abs().max() <= 1e-10


def test_log_prob_matches_planar_pushforward():
    """FlowDistribution.log_prob through the planar inverse against the independently solved
    exact density (80 fp64 bisections, unguarded log): they differ by the 1e-7 guard only."""
    flow = PlanarStack(2, 1).double()
    with torch.no_grad():
        flow.W.copy_(torch.tensor([[-5.0, 1.0]]))
        flow.U.copy_(torch.tensor([[-2.0, 1.0]]))
        flow.B.zero_()
    dist = FlowDistribution(StdNormal(2), flow)
    g = torch.Generator().manual_seed(0)
    y = 3.0 * torch.randn(500, 2, dtype=F64, generator=g)
    with torch.no_grad():
        lp = dist.log_prob(y)
    ref = planar_pushforward()(y)
    err = float((lp - ref).abs().max())
    print(f"max |d log p| {err:.2e}")
    assert lp.dtype == F64 and err <= 1e-6


@pytest.mark.parametrize("per_sample", [False, True])
def test_gradcheck_planar_inverse(per_sample):
    N, D, K = 3, 2, 2
    g = torch.Generator().manual_seed(11 + per_sample)
    y = torch.randn(N, D, dtype=F64, generator=g).requires_grad_(True)
    W, U, B = (t.requires_grad_(True) for t in _planar_params(K, N, D, per_sample, g))
    assert torch.autograd.gradcheck(planar_stack_inverse_reference, (y, W, U, B))


@pytest.mark.parametrize("per_sample", [False, True])
def test_gradcheck_radial_inverse(per_sample):
    N, D, K = 3, 2, 2
    g = torch.Generator().manual_seed(21 + per_sample)
    y = torch.randn(N, D, dtype=F64, generator=g).requires_grad_(True)
    Z0, al, be = (t.detach().requires_grad_(True) for t in _radial_params(K, N, D, per_sample, g))
    assert torch.autograd.gradcheck(radial_stack_inverse_reference, (y, Z0, al, be))


def test_planar_radial_density_normalises():
    """exp(log_prob) of a seeded 2-D K = 3 planar-then-radial flow integrates to 1 on an 801^2
    grid over [-8, 8]^2 within 2e-3; the same sum for the base alone (the grid's own error) has
    to stay 10x below that bound so that the bound tests the flow and not the grid."""
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(5)
    planar = PlanarStack(2, 3, init="random", generator=g)
    radial = RadialStack(2, 3, generator=g)
    with torch.no_grad():
        planar.W.mul_(8.0)
        planar.U.mul_(8.0)
        radial.b_raw.copy_(torch.tensor([1.0, -1.0, 0.5]))
    flow = FlowSequence([planar, radial]).double()
    dist = FlowDistribution(StdNormal(2), flow)
    n = 801
    ax = torch.linspace(-8.0, 8.0, n, dtype=F64)
    hstep = float(ax[1] - ax[0])
    pts = torch.cartesian_prod(ax, ax)
    with torch.no_grad():
        z, ldj = flow(pts[::97])
        assert (z - pts[::97]).abs().max() > 0.1 and ldj.abs().max() > 0.1   # not the identity
        total = float(dist.log_prob(pts).exp().sum()) * hstep * hstep
        grid_err = abs(float(StdNormal(2).log_prob(pts).exp().sum()) * hstep * hstep - 1.0)
    print(f"integral {total:.7f}, grid error for the base {grid_err:.2e}")
    assert 10 * grid_err <= 2e-3
    assert abs(total - 1.0) <= 2e-3


def test_invertible_flags():
    assert PlanarStack(2, 2).invertible and Planar(2).invertible and AmortizedPlanar(2, 2).invertible
    assert RadialStack(2, 2).invertible and Radial(2).invertible and AmortizedRadial(2, 2).invertible
    assert build_flow("planar+radial", 2, 2).invertible
    for kw in ({"variant": "reference"}, {"uhat_norm": "l2"}, {"ldj": "reference"}):
        assert not PlanarStack(2, 2, **kw).invertible
        assert not AmortizedPlanar(2, 2, **kw).invertible
    assert not build_flow("planar", 2, 2, variant="reference").invertible


@pytest.mark.parametrize("kw,word", [({"variant": "reference"}, "variant"),
                                     ({"uhat_norm": "l2"}, "uhat_norm"),
                                     ({"ldj": "reference"}, "ldj")])
def test_inverse_rejects_compat_options(kw, word):
    y = torch.randn(4, 2)
    with pytest.raises(NotImplementedError, match=word):
        PlanarStack(2, 2, **kw).inverse(y)
    P = (torch.randn(2, 4, 2), torch.randn(2, 4, 2), torch.randn(2, 4))
    with pytest.raises(NotImplementedError, match=word):
        AmortizedPlanar(2, 2, **kw).inverse(y, P)


def _known_flow_samples(n, g):
    z = torch.randn(n, 2, dtype=F64, generator=g)
    return planar_stack_reference(z, torch.tensor([[-5.0, 1.0]], dtype=F64),
                                  torch.tensor([[-2.0, 1.0]], dtype=F64),
                                  torch.zeros(1, dtype=F64))[0]


def test_fit_density_recovers_known_planar_flow():
    """Maximum likelihood on 4000 samples of the known flow (w = (-5, 1), u = (-2, 1), b = 0),
    K = 1 from a 0.1 randn initialisation, Adam at 0.02, 600 full-batch steps. The yardstick is
    the exact density (``planar_pushforward``) on 2000 held-out samples: the held-out NLL falls,
    cannot beat the exact NLL by more than 3 standard errors, and closes at least half of the
    gap from the initial to the exact NLL."""
    g = torch.Generator().manual_seed(0)
    train, held = _known_flow_samples(4000, g), _known_flow_samples(2000, g)
    exact_lp = planar_pushforward()(held)
    exact = float(-exact_lp.mean())
    flow = PlanarStack(2, 1, init="random", generator=g).double()
    dist = FlowDistribution(StdNormal(2), flow)
    with torch.no_grad():
        nll0 = float(-dist.log_prob(held).mean())
    trace = fit_density(flow, train, iters=600, lr=0.02)
    with torch.no_grad():
        lp = dist.log_prob(held)
    nll = float(-lp.mean())
    se = float((lp - exact_lp).std() / math.sqrt(held.shape[0]))   # of the NLL difference
    share = (nll0 - nll) / (nll0 - exact)
    print(f"held-out NLL {nll0:.4f} -> {nll:.4f}, exact {exact:.4f}, se {se:.4f}, "
          f"share of the gap closed {share:.3f}")
    assert len(trace) == 600 and trace[-1] < trace[0]
    assert nll < nll0
    assert nll >= exact - 3 * se
    assert share >= 0.5


def test_fit_density_minibatch_and_base():
    g = torch.Generator().manual_seed(1)
    data = _known_flow_samples(512, g)
    flow = RadialStack(2, 2, generator=g).double()
    trace = fit_density(flow, data, base=StdNormal(2), iters=20, lr=0.02, batch=128, generator=g)
    assert len(trace) == 20 and all(math.isfinite(v) for v in trace)


def test_plot_flow_density(tmp_path):
    from vi_normflows_amd.viz import plot_flow_density

    dist = FlowDistribution(StdNormal(2), build_flow("planar+radial", 2, 2))
    plot_flow_density(dist, lims=(-4, 4), n=40, path=tmp_path / "d.png")
    assert (tmp_path / "d.png").exists()


def test_example_runs_reduced(tmp_path):
    sys.path.insert(0, str(EX))
    spec = importlib.util.spec_from_file_location("planar_density_estimation",
                                                  EX / "planar_density_estimation.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    s = mod.main(["--iters", "60", "--train", "500", "--heldout", "300", "--out", str(tmp_path)])
    assert s["heldout_nll"] < s["heldout_nll_init"] and math.isfinite(s["exact_nll"])
    assert (tmp_path / "density.png").exists()
