"""The GLM likelihood HIP kernel (csrc/kernels/glm.hip) against the fp64 CPU composite.

The oracle is glm_logp_grad_reference of ops/reference.py in fp64 on the fp32 inputs. The limit is
per element, against the oracle's own abs-sums

    A_i  = scale sum_n |ll_in| + |log prior_i|                                           (logp)
    G_ic = scale sum_n |r_in x_nc| + |prec_c theta_ic|                                   (grad)

as |logp - ref| <= 1e-4 A_i and |grad - ref| <= 1e-4 G_ic. 1e-4 is the project's row-kernel rtol
(tests/test_stein_gpu.py): above the worst-case fp32 bound for these shapes (recursive summation
at most N 2^-24 ~ 6.6e-5 at N = 1100, the rounding of eta through ll and r a few D 2^-24, the
hardware exp / log / rcp 1 ulp each). A tolerance cannot see one dropped data row at N = 1100, so
the indexing is pinned separately, bitwise, with exactly representable operands.
"""
import functools
import math

import pytest
import torch

from vi_normflows_amd.distributions.base import StdNormal
from vi_normflows_amd.distributions.energies import get_target
from vi_normflows_amd.flows.planar import PlanarStack
from vi_normflows_amd.inference.elbo import free_energy
from vi_normflows_amd.inference.flow_vi import FlowVI
from vi_normflows_amd.inference.svgd import SVGD, flow_ksd
from vi_normflows_amd.ops import glm
from vi_normflows_amd.ops._ext import native
from vi_normflows_amd.ops.reference import glm_logp_grad_reference, svgd_direction_reference

pytestmark = pytest.mark.gpu

RTOL = 1e-4
FAMILIES = ("bernoulli", "poisson", "gaussian")
PRIORS = ("scalar", "vector", None)
SCALES = (1.0, 3.5)
NOISE_VAR = 0.7
CASES = [(1, 1, 1), (2, 3, 2), (glm.TILE_B + 1, glm.TILE_N + 1, 3), (130, 2 * glm.TILE_N - 1, 17),
         (129, 300, 64), (257, 1100, 5), (64, 513, 16), (100, 260, 40)]
SPLITS = (1, 2, 3, 7, None)


@functools.lru_cache(maxsize=None)
def _inputs(family, B, N, D):
    """Seeded fp32 CPU inputs of a case: theta ~ 0.5 N(0, 1) / sqrt(D), X ~ N(0, 1) (so eta is
    O(1)), y drawn from the family at a seeded theta_true; the Poisson theta is scaled so that
    eta <= 5."""
    g = torch.Generator().manual_seed(100000 * B + 100 * N + D)
    theta = 0.5 * torch.randn(B, D, generator=g) / math.sqrt(D)
    X = torch.randn(N, D, generator=g)
    eta = X @ (torch.randn(D, generator=g) / math.sqrt(D))
    if family == "bernoulli":
        y = torch.bernoulli(torch.sigmoid(eta), generator=g)
    elif family == "poisson":
        y = torch.poisson(torch.exp(eta.clamp_max(3.0)), generator=g)
        theta = theta * min(1.0, 5.0 / (theta @ X.T).abs().max().item())
    else:
        y = eta + math.sqrt(NOISE_VAR) * torch.randn(N, generator=g)
    return theta, X, y


@functools.lru_cache(maxsize=None)
def _prior(kind, D):
    if kind == "vector":   # one flat coordinate where there is room for it
        p = 0.5 + 1.5 * torch.rand(D, generator=torch.Generator().manual_seed(D))
        if D > 1:
            p[D // 2] = 0.0
        return p
    return 0.8 if kind == "scalar" else None


@functools.lru_cache(maxsize=None)
def _oracle(family, B, N, D, prior, scale):
    """fp64 CPU composite on the fp32 inputs: logp, grad, A, G (shared, never modified)."""
    theta, X, y = _inputs(family, B, N, D)
    return glm_logp_grad_reference(theta.double(), X.double(), y.double(), family,
                                   _prior(prior, D), NOISE_VAR, scale, return_abs=True)


def _within(got_lp, got_g, oracle, tag):
    lp, g, A, G = oracle
    e_lp, e_g = (got_lp.double().cpu() - lp).abs(), (got_g.double().cpu() - g).abs()
    tiny = torch.finfo(torch.float64).tiny
    print(f"{tag}: logp {(e_lp / A.clamp_min(tiny)).max().item():.2e} A, "
          f"grad {(e_g / G.clamp_min(tiny)).max().item():.2e} G")
    assert torch.isfinite(got_lp).all() and torch.isfinite(got_g).all(), tag
    assert (e_lp <= RTOL * A).all(), tag
    assert (e_g <= RTOL * G).all(), tag


def _check_case(family, B, N, D, prior, scale, n_splits=None):
    theta, X, y = _inputs(family, B, N, D)
    p = _prior(prior, D)
    p = p.cuda() if isinstance(p, torch.Tensor) else p
    lp, g = glm.glm_logp_grad(theta.cuda(), X.cuda(), y.cuda(), family, p, NOISE_VAR, scale,
                              impl="kernel", n_splits=n_splits)
    assert lp.shape == (B,) and g.shape == (B, D) and lp.dtype == g.dtype == torch.float32
    _within(lp, g, _oracle(family, B, N, D, prior, scale),
            f"{family} B={B} N={N} D={D} prior={prior} scale={scale} n_splits={n_splits}")
    return lp, g


@pytest.mark.parametrize("B,N,D", CASES)
def test_kernel_against_fp64_oracle(gpu, B, N, D):
    n0 = glm.glm_launches()
    for family in FAMILIES:
        for prior in PRIORS:
            for scale in SCALES:
                _check_case(family, B, N, D, prior, scale)
    assert glm.glm_launches() == n0 + len(FAMILIES) * len(PRIORS) * len(SCALES)


@pytest.mark.parametrize("B,N,D", [(glm.TILE_B + 1, 2 * glm.TILE_N + 1, 5), (130, 1100, 17),
                                   (129, 300, 64)])
def test_exact_indexing(gpu, B, N, D):
    """Gaussian family, inv_var = 1, no prior, integer X in [-2, 2], theta in {-1, -0.5, .., 1},
    integer y in [-3, 3]: |eta| <= 128, r is a multiple of 0.5 with |r| <= 131 and every partial
    sum of r x stays below 3e5 < 2^23, so every fp32 operation of the gradient is exact and a
    dropped, doubled or misplaced row, column or split changes bits."""
    g = torch.Generator().manual_seed(B + N + D)
    theta = torch.randint(-2, 3, (B, D), generator=g).float() / 2
    X = torch.randint(-2, 3, (N, D), generator=g).float()
    y = torch.randint(-3, 4, (N,), generator=g).float()
    for scale in (1.0, 2.0):
        lp, grad, A, G = glm_logp_grad_reference(theta.double(), X.double(), y.double(),
                                                 "gaussian", None, 1.0, scale, return_abs=True)
        assert G.max() < 3e5 * scale and torch.equal(grad.float().double(), grad)
        for ns in SPLITS:
            got_lp, got = glm.glm_logp_grad(theta.cuda(), X.cuda(), y.cuda(), "gaussian", None,
                                            1.0, scale, impl="kernel", n_splits=ns)
            assert torch.equal(got.cpu(), grad.float()), (scale, ns)
            assert ((got_lp.double().cpu() - lp).abs() <= RTOL * A).all(), (scale, ns)


@pytest.mark.parametrize("B,N,D", [(300, 1100, 3), (129, 513, 40)])
def test_split_n(gpu, B, N, D):
    for ns in SPLITS:
        a = _check_case("bernoulli", B, N, D, "scalar", 1.0, n_splits=ns)
        b = _check_case("bernoulli", B, N, D, "scalar", 1.0, n_splits=ns)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), ns


def test_row_independence_and_strides(gpu):
    B, N, D = 257, 300, 17
    for family in FAMILIES:
        theta, X, y = (t.cuda() for t in _inputs(family, B, N, D))
        prec = _prior("vector", D).cuda()

        def run(th, XX=X, yy=y):
            return glm.glm_logp_grad(th, XX, yy, family, prec, NOISE_VAR, 3.5, impl="kernel",
                                     n_splits=2)
        lp, g = run(theta)
        for i in (0, 1, glm.TILE_B - 1, glm.TILE_B, B - 1):   # alone: B = 1, first lane
            lp1, g1 = run(theta[i:i + 1])
            assert torch.equal(lp1[0], lp[i]) and torch.equal(g1[0], g[i]), (family, i)
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).cuda()
        lp_p, g_p = run(theta[perm])
        assert torch.equal(lp_p, lp[perm]) and torch.equal(g_p, g[perm]), family
        # views: a column slice of a wider theta, a column slice of a wider X, a row offset
        wide_t = torch.randn(B, D + 5, device=gpu)
        wide_t[:, 2:2 + D] = theta
        wide_x = torch.randn(N + 100, D + 3, device=gpu)
        wide_x[100:, 1:1 + D] = X
        tv, xv = wide_t[:, 2:2 + D], wide_x[:, 1:1 + D][100:]
        assert tv.stride() == (D + 5, 1) and xv.stride() == (D + 3, 1) and xv.storage_offset() > 0
        n0 = glm.glm_launches()
        for got in (run(tv), run(theta, xv), run(tv, xv)):
            assert torch.equal(got[0], lp) and torch.equal(got[1], g), family
        yw = torch.cat([torch.zeros(100, device=gpu), y])
        got = run(tv, wide_x[:, 1:1 + D][100:], yw[100:])
        assert torch.equal(got[0], lp) and torch.equal(got[1], g), family
        assert glm.glm_launches() == n0 + 4


def test_bernoulli_range(gpu):
    B, N, D = 64, 513, 16
    theta, X, y = _inputs("bernoulli", B, N, D)
    theta = theta * (1e4 / (theta @ X.T).abs().max().item())
    eta = (theta.double() @ X.double().T).abs()
    assert eta.max() > 9.9e3 and (eta > 100).float().mean() > 0.9
    for prior in PRIORS:
        p = _prior(prior, D)
        lp, g = glm.glm_logp_grad(theta.cuda(), X.cuda(), y.cuda(), "bernoulli",
                                  p.cuda() if isinstance(p, torch.Tensor) else p, impl="kernel")
        _within(lp, g, glm_logp_grad_reference(theta.double(), X.double(), y.double(), "bernoulli",
                                               p, return_abs=True), f"range prior={prior}")


def test_autograd(gpu):
    B, N, D = 130, 300, 17
    for family in FAMILIES:
        theta, X, y = (t.cuda() for t in _inputs(family, B, N, D))
        gout = torch.randn(B, device=gpu)
        lp0, grad = glm.glm_logp_grad(theta, X, y, family, 0.8, NOISE_VAR, 3.5, impl="kernel",
                                      const=1.25)
        th = theta.clone().requires_grad_(True)
        n0 = glm.glm_launches()
        lp = glm.glm_log_prob(th, X, y, family, 0.8, NOISE_VAR, 3.5, impl="kernel", const=1.25)
        assert glm.glm_launches() == n0 + 1 and lp.requires_grad and torch.equal(lp, lp0)
        lp.backward(gout)
        assert glm.glm_launches() == n0 + 1
        assert torch.equal(th.grad, gout[:, None] * grad)
        with pytest.raises(RuntimeError, match="X requires grad"):
            glm.glm_log_prob(th, X.clone().requires_grad_(True), y, family)


def test_errors(gpu):
    ops = native()
    th, X, y = torch.randn(8, 3, device=gpu), torch.randn(9, 3, device=gpu), torch.randn(9, device=gpu)
    lp, g = torch.empty(8, device=gpu), torch.empty(8, 3, device=gpu)
    assert ops.glm_workspace(8, 9, 3, 1) == 8 * 4 and ops.glm_workspace(8, 200, 3, 2) == 2 * 8 * 4
    work = torch.empty(ops.glm_workspace(8, 9, 3, 1), device=gpu)

    def raw(th=th, X=X, y=y, prec=None, prec_host=1.0, has_prior=True, family=0, inv_var=1.0,
            scale=1.0, ns=1, lp=lp, g=g, work=work):
        ops.glm_logp_grad(th, X, y, prec, prec_host, has_prior, family, inv_var, scale, ns, lp, g,
                          work)
    raw()
    t65 = torch.randn(4, 65, device=gpu)
    with pytest.raises(RuntimeError, match="D <= 64"):
        raw(th=t65, X=t65, y=torch.randn(4, device=gpu))
    with pytest.raises(RuntimeError, match="impl='kernel'.*D = 65"):
        glm.glm_logp_grad(t65, t65, torch.randn(4, device=gpu), impl="kernel")
    with pytest.raises(RuntimeError, match="theta must be fp32"):
        raw(th=th.double())
    with pytest.raises(RuntimeError, match="X must be fp32"):
        raw(X=X.double())
    with pytest.raises(RuntimeError, match="y must be fp32"):
        raw(y=y.double())
    with pytest.raises(RuntimeError, match="impl='kernel'.*float64"):
        glm.glm_logp_grad(th.double(), X.double(), y.double(), impl="kernel")
    with pytest.raises(RuntimeError, match="y has shape"):
        raw(y=y[:-1])
    with pytest.raises(ValueError, match="y must have one entry per row"):
        glm.glm_logp_grad(th, X, y[:-1], impl="kernel")
    with pytest.raises(RuntimeError, match="scale must be positive"):
        raw(scale=0.0)
    with pytest.raises(ValueError, match="scale must be positive"):
        glm.glm_logp_grad(th, X, y, scale=-1.0, impl="kernel")
    with pytest.raises(RuntimeError, match="inv_var must be positive"):
        raw(family=2, inv_var=0.0)
    with pytest.raises(RuntimeError, match="theta must have unit inner stride"):
        raw(th=torch.randn(8, 6, device=gpu)[:, ::2])
    with pytest.raises(RuntimeError, match="X must have unit inner stride"):
        raw(X=torch.randn(9, 6, device=gpu)[:, ::2])
    with pytest.raises(RuntimeError, match="unknown family 3"):
        raw(family=3)
    with pytest.raises(RuntimeError, match="prec_host = -1"):
        raw(prec_host=-1.0)
    raw(prec_host=-1.0, has_prior=False)   # not read without a prior
    with pytest.raises(RuntimeError, match="prec_dev must be"):
        raw(prec=torch.ones(4, device=gpu))
    with pytest.raises(RuntimeError, match="work has"):
        raw(work=work[:-1])
    with pytest.raises(RuntimeError, match="grad has"):
        raw(g=torch.empty(8, 4, device=gpu))
    with pytest.raises(RuntimeError, match="logp has"):
        raw(lp=torch.empty(9, device=gpu))
    with pytest.raises(RuntimeError, match="n_splits"):
        raw(ns=-1)
    # the wrapper copies what the kernel cannot stride over, instead of raising
    tt = torch.randn(8, 6, device=gpu)[:, ::2]
    assert torch.equal(glm.glm_logp_grad(tt, X, y, impl="kernel")[1],
                       glm.glm_logp_grad(tt.contiguous(), X, y, impl="kernel")[1])


def test_auto_falls_back_beyond_64_dimensions(gpu):
    th, X = torch.randn(33, 65, device=gpu) / 8, torch.randn(40, 65, device=gpu)
    y = torch.bernoulli(torch.full((40,), 0.5, device=gpu))
    assert not glm.kernel_supported(th, X, y) and glm.kernel_supported(th[:, :64], X[:, :64], y)
    n0 = glm.glm_launches()
    got, want = glm.glm_logp_grad(th, X, y), glm_logp_grad_reference(th, X, y)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert glm.glm_launches() == n0
    glm.glm_logp_grad(th[:, :64], X[:, :64], y)
    assert glm.glm_launches() == n0 + 1


# ------------------------------------------------------------------ wiring
@functools.lru_cache(maxsize=None)
def _logreg():
    return get_target("logreg", dim=3, n=200, seed=11)


def _oracle_at(tgt, z):
    """fp64 CPU composite of a GLM target at the fp32 samples z: logp (with the target's
    constant), grad, A, G."""
    d = tgt.meta["glm"]
    lp, g, A, G = glm_logp_grad_reference(z.detach().double().cpu(), d.X.double(), d.y.double(),
                                          d.family, d.prec, d.noise_var, return_abs=True)
    return lp + d.const, g, A, G


def test_free_energy_backpropagates_through_the_kernel(gpu):
    """One free-energy evaluation and backward of a planar flow on a logreg target, the kernel
    against impl="composite" on the same device and samples. F differs by the mean difference of
    log p; a flow-parameter gradient is J^T (dF/dz) with dF/dz = -grad / B, so it differs by at
    most sum_ic |e_ic| |dz_ic / dp| / B where e is the difference of the two scores. Each of the
    two is bounded against the fp64 oracle: the kernel by the limit (1e-4 A_i, 1e-4 G_ic), the
    composite by its own measured error. The Jacobians are those of an fp64 CPU copy of the flow.
    Rounding of the two fp32 backward passes themselves (they are the same kernels on inputs that
    differ in the last bits) gets 64 x 2^-24 of the abs-sum of the terms of each gradient: a
    loose count of the rounding steps along the K = 2 chain and the 512-row reduction."""
    tgt, B, K = _logreg(), 512, 2
    data = tgt.meta["glm"]
    flow = PlanarStack(3, K, init="random", generator=torch.Generator().manual_seed(3)).to(gpu)
    base = StdNormal(3).to(gpu)
    out = {}
    for impl in ("kernel", "composite"):
        data.impl = impl
        seen = {}

        def log_target(z):
            seen["z"] = z.detach()
            seen["lp"] = tgt.log_prob(z)
            return seen["lp"]
        flow.zero_grad()
        n0 = glm.glm_launches()
        r = free_energy(base, flow, log_target, B,
                        generator=torch.Generator(device=gpu).manual_seed(5))
        r.F.backward()
        assert glm.glm_launches() == n0 + (impl == "kernel")
        out[impl] = (r.F.detach().double().cpu(), seen["z"], seen["lp"].detach().double().cpu(),
                     data.score(seen["z"]).double().cpu(),
                     [p.grad.detach().double().cpu().clone() for p in flow.parameters()])
    data.impl = "auto"
    (Fk, zk, lpk, sk, gk), (Fc, zc, lpc, sc, gc) = out["kernel"], out["composite"]
    assert torch.equal(zk, zc)
    lp, g, A, G = _oracle_at(tgt, zk)
    assert ((lpk - lp).abs() <= RTOL * A).all()
    assert ((sk - g).abs() <= RTOL * G).all()
    lim_F = (RTOL * A + (lpc - lp).abs()).mean() + 64 * 2.0 ** -24 * lp.abs().mean()
    print(f"F kernel {Fk.item():.6f} composite {Fc.item():.6f} limit {lim_F.item():.2e}")
    assert all(q.abs().max() > 0 for q in gk) and torch.isfinite(Fk)
    assert (Fk - Fc).abs() <= lim_F

    # Jacobians of z_K and of the log-det w.r.t. the flow parameters, fp64 CPU
    cpu = PlanarStack(3, K)
    cpu.load_state_dict({k: v.detach().cpu() for k, v in flow.state_dict().items()})
    cpu = cpu.double()
    z0 = base.rsample(B, torch.Generator(device=gpu).manual_seed(5)).double().cpu()
    names = [n for n, _ in cpu.named_parameters()]

    def f(*ps):
        return torch.func.functional_call(cpu, dict(zip(names, ps)), (z0,))
    Jz, Jl = torch.autograd.functional.jacobian(f, tuple(cpu.parameters()), vectorize=True)
    assert (f(*cpu.parameters())[0] - zk.double().cpu()).abs().max() < 1e-5
    E = RTOL * G + (sc - g).abs()
    for jz, jl, a, b, name in zip(Jz, Jl, gk, gc, names):
        jz = jz.reshape(B, 3, -1).abs()
        lim = torch.einsum("ic,icp->p", E, jz) / B
        terms = (torch.einsum("ic,icp->p", g.abs(), jz) + jl.reshape(B, -1).abs().sum(0)) / B
        lim = (lim + 64 * 2.0 ** -24 * terms).reshape(a.shape)
        print(f"{name}: max |dk - dc| / limit = {((a - b).abs() / lim).max().item():.3f}")
        assert ((a - b).abs() <= lim).all(), name


def test_svgd_direction_with_kernel_scores(gpu):
    tgt, N, h = _logreg(), 257, 0.5
    x = (0.5 * torch.randn(N, 3, generator=torch.Generator().manual_seed(8))).cuda()
    n0 = glm.glm_launches()
    sv = SVGD(tgt, x.clone(), 0.1, optimizer="sgd", bandwidth=h)
    phi = sv.direction()
    assert glm.glm_launches() == n0 + 1
    s = tgt.score(x)
    _, g, _, G = _oracle_at(tgt, x)
    assert ((s.double().cpu() - g).abs() <= RTOL * G).all()
    want, A = svgd_direction_reference(x.double().cpu(), s.double().cpu(), h, "rbf",
                                       return_abs=True)
    err = (phi.double().cpu() - want).abs()
    print(f"max |phi - ref| / A = {(err / A).max().item():.2e}")
    assert (err <= RTOL * A).all()


def test_flow_ksd_launches_the_kernel_once(gpu):
    tgt = _logreg()
    model = FlowVI(tgt, PlanarStack(3, 2)).to(gpu)
    n0 = glm.glm_launches()
    v = flow_ksd(model, 300, torch.Generator(device=gpu).manual_seed(2))
    assert glm.glm_launches() == n0 + 1
    assert v.dtype == torch.float64 and math.isfinite(float(v))
