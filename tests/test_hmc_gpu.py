"""The HMC trajectory kernel (csrc/kernels/glm_hmc.hip) on the GPU.

The kernel is pinned from three sides, none of which needs an end-to-end tolerance:

1. one leapfrog step against the fp64 composite on the fp32 inputs, with limits derived from the
   number of fp32 roundings (and the GLM kernel's own 1e-4 abs-sum limit for the pass inside);
2. L steps in one launch bitwise equal to L launches of one step;
3. a two-step trajectory on exactly representable operands, bitwise equal to the fp64 oracle.

Together with (lp_L, g_L) being bitwise glm_logp_grad(theta_prop, n_splits=1) this fixes every
intermediate pass. The rest checks the independence of a chain from its neighbours and from the
row tile, the accept step, the wiring into inference.HMC and the binding's argument checks.
"""
import functools
import math

import pytest
import torch

from vi_normflows_amd.distributions.energies import get_target
from vi_normflows_amd.inference.bbvi import linreg_posterior
from vi_normflows_amd.inference.hmc import HMC
from vi_normflows_amd.ops import glm, hmc
from vi_normflows_amd.ops._ext import native
from vi_normflows_amd.ops.reference import glm_logp_grad_reference

pytestmark = pytest.mark.gpu

RTOL = 1e-4   # the project's row-kernel rtol (tests/test_glm_gpu.py)
U = 2.0 ** -24
FAMILIES = ("bernoulli", "poisson", "gaussian")
PRIORS = ("scalar", "vector", None)
NOISE_VAR = 0.7
ROWS = hmc.ROW_TILES
CASES = ([(1, 1, 1), (2, 3, 2)] + [(r + 1, glm.TILE_N + 1, 3) for r in ROWS]
         + [(130, 2 * glm.TILE_N - 1, 17), (129, 300, 64), (64, 513, 16), (100, 260, 40)])
NINF, PINF = float("-inf"), float("inf")


@functools.lru_cache(maxsize=None)
def _inputs(family, B, N, D):
    """Seeded fp32 CPU inputs: theta0 ~ 0.5 N(0, 1) / sqrt(D), X ~ N(0, 1), y from the family at a
    seeded theta_true, p0 ~ N(0, 1), eps = U(0.5, 1.5) x base with base = 0.5 / sqrt(N) (0.2 /
    sqrt(N) for Poisson, whose curvature carries exp(eta)): a step moves theta by about a
    posterior standard deviation, so |eta| stays O(1). The Poisson theta0 is scaled to eta <= 4,
    and the one-step test asserts eta <= 5 at the proposal."""
    g = torch.Generator().manual_seed(100000 * B + 100 * N + D + 7)
    theta = 0.5 * torch.randn(B, D, generator=g) / math.sqrt(D)
    X = torch.randn(N, D, generator=g)
    eta = X @ (torch.randn(D, generator=g) / math.sqrt(D))
    if family == "bernoulli":
        y = torch.bernoulli(torch.sigmoid(eta), generator=g)
    elif family == "poisson":
        y = torch.poisson(torch.exp(eta.clamp_max(3.0)), generator=g)
        theta = theta * min(1.0, 4.0 / (theta @ X.T).abs().max().item())
    else:
        y = eta + math.sqrt(NOISE_VAR) * torch.randn(N, generator=g)
    p = torch.randn(B, D, generator=g)
    base = (0.2 if family == "poisson" else 0.5) / math.sqrt(N)
    eps = base * (0.5 + torch.rand(B, generator=g))
    return theta, X, y, p, eps


@functools.lru_cache(maxsize=None)
def _prior(kind, D):
    if kind == "vector":   # one flat coordinate where there is room for it
        p = 0.5 + 1.5 * torch.rand(D, generator=torch.Generator().manual_seed(D))
        if D > 1:
            p[D // 2] = 0.0
        return p
    return 0.8 if kind == "scalar" else None


@functools.lru_cache(maxsize=None)
def _minv(kind, D):
    if kind is None:
        return None
    return 0.5 + 1.5 * torch.rand(D, generator=torch.Generator().manual_seed(1000 + D))


def _dev(t):
    return t.cuda() if isinstance(t, torch.Tensor) else t


def _state(family, B, N, D, prior, scale=1.0):
    """GPU inputs of a case and the kernel's own (logp0, grad0) at theta0."""
    theta, X, y, p, eps = (t.cuda() for t in _inputs(family, B, N, D))
    prec = _dev(_prior(prior, D))
    lp0, g0 = glm.glm_logp_grad(theta, X, y, family, prec, NOISE_VAR, scale, impl="kernel",
                                n_splits=1)
    return theta, X, y, p, eps, prec, lp0, g0


def _run(theta, lp, g, p, log_u, eps, L, X, y, family, prec, minv, scale=1.0, rows=None):
    return hmc.glm_hmc_step(theta, lp, g, p, log_u, eps, L, X, y, family, prec, NOISE_VAR, scale,
                            minv, impl="kernel", rows=rows)


def _same(a, b, fields=hmc.HMCStep._fields):
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in fields)


# ------------------------------------------------------------------ 1. one step, derived limits
@pytest.mark.parametrize("B,N,D", CASES)
def test_one_step_against_fp64_composite(gpu, B, N, D):
    """L = 1, log_u = -inf, every family, prior and mass, against the fp64 composite on the fp32
    inputs (theta0, p0, eps, minv and the kernel's own fp32 logp0 / grad0).

    theta_prop = fma(eps minv, fma(h, g0, p0), theta0) is three fp32 roundings (eps minv, the kick,
    the drift), each at most 2^-24 of a term bounded by |theta0| + |eps minv| (|p0| + |h g0|): the
    limit is 4 x 2^-24 of that. (logp_out, grad_out) must be bitwise glm_logp_grad(theta_prop,
    n_splits=1), which test_glm_gpu.py holds within 1e-4 of the oracle's abs-sums A, G. p_prop is
    two fma roundings on top of that pass, so with the oracle evaluated at the kernel's own
    theta_prop its limit is 2^-23 (|p0| + |h g0| + |h g1|) + |h| 1e-4 G_1. dH = (kin_1 - kin_0) +
    (logp0 - lp_1): the kinetic energy inherits sum_c minv_c (|p1_c| dp_c + dp_c^2 / 2) from
    the limit dp of p_prop plus (D + 3) 2^-24 of each sum of D terms; lp_1 has 1e-4 A_1; the three
    final operations add 3 x 2^-24 of the magnitudes involved."""
    n0 = hmc.hmc_launches()
    runs = 0
    for family in FAMILIES:
        for prior in PRIORS:
            for mk in (None, "seeded"):
                theta, X, y, p, eps, prec, lp0, g0 = _state(family, B, N, D, prior)
                minv = _dev(_minv(mk, D))
                log_u = torch.full((B,), NINF, device=gpu)
                r = _run(theta, lp0, g0, p, log_u, eps, 1, X, y, family, prec, minv)
                runs += 1
                tag = f"{family} B={B} N={N} D={D} prior={prior} minv={mk}"
                assert r.theta_prop.shape == (B, D) and r.dH.shape == (B,), tag
                assert torch.equal(r.accept, torch.ones(B, device=gpu)), tag
                assert torch.equal(r.theta, r.theta_prop), tag
                # the pass inside is the GLM kernel's, bitwise
                lp1, g1 = glm.glm_logp_grad(r.theta_prop, X, y, family, prec, NOISE_VAR, 1.0,
                                            impl="kernel", n_splits=1)
                assert torch.equal(r.logp, lp1) and torch.equal(r.grad, g1), tag
                # fp64 composite
                t0, p0, e, g0d, lp0d = (t.double().cpu() for t in (theta, p, eps, g0, lp0))
                mi = torch.ones(D, dtype=torch.float64) if minv is None else minv.double().cpu()
                h = 0.5 * e[:, None]
                em = e[:, None] * mi
                ph = p0 + h * g0d
                th1 = t0 + em * ph
                lim_t = 4 * U * (t0.abs() + em.abs() * (p0.abs() + (h * g0d).abs()))
                err_t = (r.theta_prop.double().cpu() - th1).abs()
                assert (err_t <= lim_t).all(), tag
                thk = r.theta_prop.double().cpu()
                pr64 = _prior(prior, D)
                lp1d, g1d, A1, G1 = glm_logp_grad_reference(thk, X.double().cpu(),
                                                            y.double().cpu(), family, pr64,
                                                            NOISE_VAR, 1.0, return_abs=True)
                if family == "poisson":
                    assert (thk @ X.double().cpu().T).max() <= 5.0, tag
                assert ((r.logp.double().cpu() - lp1d).abs() <= RTOL * A1).all(), tag
                assert ((r.grad.double().cpu() - g1d).abs() <= RTOL * G1).all(), tag
                p1 = ph + h * g1d
                lim_p = 2 * U * (p0.abs() + (h * g0d).abs() + (h * g1d).abs()) + h.abs() * RTOL * G1
                err_p = (r.p_prop.double().cpu() - p1).abs()
                assert (err_p <= lim_p).all(), tag
                kin0, kin1 = 0.5 * (mi * p0 * p0).sum(1), 0.5 * (mi * p1 * p1).sum(1)
                dH = (kin1 - kin0) + (lp0d - lp1d)
                lim_kin = (mi * (p1.abs() * lim_p + 0.5 * lim_p * lim_p)).sum(1) \
                    + (D + 3) * U * (kin0 + kin1)
                lim_dH = lim_kin + RTOL * A1 + 3 * U * (kin0 + kin1 + lp0d.abs() + lp1d.abs())
                err_dH = (r.dH.double().cpu() - dH).abs()
                print(f"{tag}: theta {(err_t / lim_t.clamp_min(1e-300)).max().item():.2f} "
                      f"p {(err_p / lim_p.clamp_min(1e-300)).max().item():.2f} "
                      f"dH {(err_dH / lim_dH.clamp_min(1e-300)).max().item():.2f} of the limits")
                assert (err_dH <= lim_dH).all(), tag
    assert hmc.hmc_launches() == n0 + runs


# ------------------------------------------------------------------ 2. composition, bitwise
@pytest.mark.parametrize("B,N,D", CASES)
def test_L_steps_equal_L_launches(gpu, B, N, D):
    for family in FAMILIES:
        theta, X, y, p, eps, prec, lp0, g0 = _state(family, B, N, D, "vector")
        minv = _minv("seeded", D).cuda()
        log_u = torch.full((B,), NINF, device=gpu)
        for L in (2, 5):
            one = _run(theta, lp0, g0, p, log_u, eps, L, X, y, family, prec, minv)
            th, lp, g, pp = theta, lp0, g0, p
            for _ in range(L):
                r = _run(th, lp, g, pp, log_u, eps, 1, X, y, family, prec, minv)
                th, lp, g, pp = r.theta_prop, r.logp, r.grad, r.p_prop
            assert torch.isfinite(one.theta_prop).all() and torch.isfinite(one.dH).all()
            assert _same(one, r, ("theta_prop", "p_prop", "logp", "grad")), (family, L)


# ------------------------------------------------------------------ 3. exact arithmetic
@pytest.mark.parametrize("B,N,D", [(ROWS[-1] + 1, glm.TILE_N + 3, 3),
                                   (ROWS[0] + 1, 2 * glm.TILE_N + 2, 5),
                                   (ROWS[1] + 1, glm.TILE_N + 3, 17)])
def test_exact_two_steps(gpu, B, N, D):
    """Gaussian family, inv_var = 1, no prior, X in {-1, 0, 1}, theta0 and p0 in {-1, -0.5, .., 1},
    integer y in [-2, 2], eps in {1/4, 1/8}, minv in {1, 2}, N > TILE_N. Every theta, gradient and
    momentum of the two-step fp64 trajectory is then a multiple of a per-chain power of two u
    (down to 2^-19 for the last momentum) with few enough leading bits to be an fp32 number, and
    the abs-sums of each pass (sum_c |theta_c x_c| for eta, sum_n |r_n x_nc| for the gradient) stay
    below 2^24 u, so every fp32 operation on the way is exact whatever the order of the tiles. The
    oracle is checked for exactly that before the kernel's theta_prop, p_prop and grad are
    compared bitwise; a dropped, doubled or misplaced row, column or tile of either pass changes
    bits."""
    g = torch.Generator().manual_seed(B + N + D)
    theta = torch.randint(-2, 3, (B, D), generator=g).double() / 2
    p = torch.randint(-2, 3, (B, D), generator=g).double() / 2
    X = torch.randint(-1, 2, (N, D), generator=g).double()
    y = torch.randint(-2, 3, (N,), generator=g).double()
    eps = torch.pow(2.0, -torch.randint(2, 4, (B,), generator=g).double())
    minv = torch.pow(2.0, torch.randint(0, 2, (D,), generator=g).double())

    def exact32(t):
        return torch.equal(t.float().double(), t)

    def unit(row):   # the largest power of two that divides every entry
        k = 0
        while not torch.equal((row * 2.0 ** k).round(), row * 2.0 ** k):
            k += 1
        return 2.0 ** -k

    def oracle_pass(th):
        lp, gr, _, G = glm_logp_grad_reference(th, X, y, "gaussian", None, 1.0, 1.0,
                                               return_abs=True)
        ug = torch.tensor([unit(gr[i]) for i in range(B)], dtype=torch.float64)
        ut = torch.tensor([unit(th[i]) for i in range(B)], dtype=torch.float64)
        assert exact32(th) and exact32(gr)
        assert (G.max(1).values < 2.0 ** 24 * ug).all()
        assert ((th.abs() @ X.abs().T).max(1).values < 2.0 ** 24 * ut).all()
        return lp, gr

    lp0, g0 = oracle_pass(theta)
    h, th, pp, gr = 0.5 * eps[:, None], theta, p, g0
    for _ in range(2):
        pp = pp + h * gr
        assert exact32(pp)
        th = th + eps[:, None] * minv * pp
        _, gr = oracle_pass(th)
        pp = pp + h * gr
        assert exact32(pp)
    f = lambda t: t.float().cuda()   # noqa: E731
    for rows in (None,) + ROWS:
        r = hmc.glm_hmc_step(f(theta), f(lp0), f(g0), f(p), torch.full((B,), NINF, device=gpu),
                             f(eps), 2, f(X), f(y), "gaussian", None, 1.0, 1.0, f(minv),
                             impl="kernel", rows=rows)
        assert torch.equal(r.theta_prop.cpu(), th.float()), rows
        assert torch.equal(r.p_prop.cpu(), pp.float()), rows
        assert torch.equal(r.grad.cpu(), gr.float()), rows


# ------------------------------------------------------------------ 4. row tiles and independence
def test_row_tiles_independence_and_strides(gpu):
    B, N, D, L = 2 * ROWS[-1] + 1, 300, 17, 3
    for family in FAMILIES:
        theta, X, y, p, eps, prec, lp0, g0 = _state(family, B, N, D, "vector", scale=3.5)
        minv = _minv("seeded", D).cuda()
        log_u = torch.full((B,), NINF, device=gpu)

        def run(sel=slice(None), rows=None, th=None, XX=X):
            th = theta[sel] if th is None else th
            return _run(th, lp0[sel], g0[sel], p[sel], log_u[sel], eps[sel], L, XX, y, family,
                        prec, minv, scale=3.5, rows=rows)
        # log_u around -dH, so that both branches of the accept step are taken
        shift = torch.randn(B, generator=torch.Generator().manual_seed(4)).cuda()
        log_u = -run().dH + 0.5 * shift
        ref = run()
        assert 0 < ref.accept.sum() < B
        for rows in ROWS:                        # every row tile, and twice the same
            assert _same(run(rows=rows), ref), (family, rows)
        assert _same(run(), ref)
        for i in (0, 1, ROWS[0] - 1, ROWS[0], ROWS[-1] - 1, ROWS[-1], B - 1):   # alone: B = 1
            one = run(slice(i, i + 1))
            for fld in hmc.HMCStep._fields:
                assert torch.equal(getattr(one, fld)[0], getattr(ref, fld)[i]), (family, i, fld)
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).cuda()
        pr = run(perm)
        for fld in hmc.HMCStep._fields:
            assert torch.equal(getattr(pr, fld), getattr(ref, fld)[perm]), (family, fld)
        # views: theta0 a column slice of a wider tensor, X a row-offset column slice
        wide_t = torch.randn(B, D + 5, device=gpu)
        wide_t[:, 2:2 + D] = theta
        wide_x = torch.randn(N + 100, D + 3, device=gpu)
        wide_x[100:, 1:1 + D] = X
        tv, xv = wide_t[:, 2:2 + D], wide_x[:, 1:1 + D][100:]
        assert tv.stride() == (D + 5, 1) and xv.stride() == (D + 3, 1) and xv.storage_offset() > 0
        n0 = hmc.hmc_launches()
        for got in (run(th=tv), run(XX=xv), run(th=tv, XX=xv)):
            assert _same(got, ref), family
        assert hmc.hmc_launches() == n0 + 3


# ------------------------------------------------------------------ 5. accept step
def test_accept_step(gpu):
    B, N, D, L = 130, 2 * glm.TILE_N - 1, 17, 4
    for family in FAMILIES:
        theta, X, y, p, eps, prec, lp0, g0 = _state(family, B, N, D, "scalar")
        args = (eps, L, X, y, family, prec, None)
        rej = _run(theta, lp0, g0, p, torch.full((B,), PINF, device=gpu), *args)
        assert torch.equal(rej.theta, theta) and torch.equal(rej.logp, lp0)
        assert torch.equal(rej.grad, g0) and torch.equal(rej.accept, torch.zeros(B, device=gpu))
        acc = _run(theta, lp0, g0, p, torch.full((B,), NINF, device=gpu), *args)
        assert torch.equal(acc.theta, acc.theta_prop) and torch.equal(acc.accept,
                                                                      torch.ones(B, device=gpu))
        assert torch.equal(acc.theta_prop, rej.theta_prop) and torch.equal(acc.p_prop, rej.p_prop)
        assert torch.equal(acc.dH, rej.dH) and torch.isfinite(acc.dH).all()
        # mixed: log_u placed around -dH so that both outcomes occur
        shift = torch.randn(B, generator=torch.Generator().manual_seed(2)).cuda()
        log_u = -acc.dH + 0.5 * shift
        mix = _run(theta, lp0, g0, p, log_u, *args)
        want = torch.isfinite(mix.dH) & (log_u < -mix.dH)
        assert 0 < want.sum() < B and torch.equal(mix.accept, want.float())
        assert torch.equal(mix.dH, acc.dH)
        assert torch.equal(mix.theta, torch.where(want[:, None], acc.theta, theta))
        assert torch.equal(mix.grad, torch.where(want[:, None], acc.grad, g0))
        assert torch.equal(mix.logp, torch.where(want, acc.logp, lp0))


def test_diverged_chain_is_rejected_alone(gpu):
    B, N, D, L = 130, 2 * glm.TILE_N - 1, 17, 4
    theta, X, y, p, eps, prec, lp0, g0 = _state("poisson", B, N, D, "scalar")
    log_u = torch.full((B,), NINF, device=gpu)
    ref = _run(theta, lp0, g0, p, log_u, eps, L, X, y, "poisson", prec, None)
    bad = 37
    eps_bad = eps.clone()
    eps_bad[bad] = 1e6
    r = _run(theta, lp0, g0, p, log_u, eps_bad, L, X, y, "poisson", prec, None)
    assert not torch.isfinite(r.dH[bad]) and r.accept[bad] == 0
    assert torch.equal(r.theta[bad], theta[bad]) and torch.equal(r.logp[bad], lp0[bad])
    assert torch.equal(r.grad[bad], g0[bad])
    keep = torch.arange(B, device=gpu) != bad
    for fld in hmc.HMCStep._fields:
        assert torch.equal(getattr(r, fld)[keep], getattr(ref, fld)[keep]), fld
    assert ref.accept.sum() == B


# ------------------------------------------------------------------ 6. wiring
def test_hmc_class_launches(gpu):
    tgt, L = get_target("logreg", dim=3, n=200, seed=11), 5
    theta0 = (0.1 * torch.randn(64, 3, generator=torch.Generator().manual_seed(0))).cuda()
    g0, h0 = glm.glm_launches(), hmc.hmc_launches()
    s = HMC(tgt, theta0, 0.05, L, jitter=0.1, generator=torch.Generator(device=gpu).manual_seed(1),
            impl="kernel")
    assert glm.glm_launches() == g0 + 1 and hmc.hmc_launches() == h0      # the initial score
    for t in range(3):
        s.step()
        assert hmc.hmc_launches() == h0 + t + 1 and glm.glm_launches() == g0 + 1
    assert s.theta.is_cuda and s.theta.dtype == torch.float32 and s.last.accept.mean() > 0.5
    # the kept state is the target's density and score at the kept positions
    d = tgt.meta["glm"]
    lp, gr, A, G = glm_logp_grad_reference(s.theta.double().cpu(), d.X.double(), d.y.double(),
                                           d.family, d.prec, d.noise_var, return_abs=True)
    assert ((s.logp.double().cpu() - (lp + d.const)).abs() <= RTOL * A).all()
    assert ((s.grad.double().cpu() - gr).abs() <= RTOL * G).all()
    # stepwise: L likelihood launches per iteration and no trajectory launch; auto is whichever of
    # the two the benchmark decided for (ops.hmc.auto_takes_kernel)
    s3 = HMC(tgt, theta0, 0.05, L, generator=torch.Generator(device=gpu).manual_seed(1))
    g1, h1 = glm.glm_launches(), hmc.hmc_launches()
    s3.step()
    fused = hmc.auto_takes_kernel(64, 200, 3, L)
    assert hmc.hmc_launches() == h1 + fused and glm.glm_launches() == g1 + (0 if fused else L)
    s2 = HMC(tgt, theta0, 0.05, L, generator=torch.Generator(device=gpu).manual_seed(1),
             impl="stepwise")
    g1, h1 = glm.glm_launches(), hmc.hmc_launches()
    s2.step()
    assert glm.glm_launches() == g1 + L and hmc.hmc_launches() == h1


def test_falls_back_beyond_64_dimensions(gpu):
    tgt = get_target("logreg", dim=65, n=50, seed=3)
    theta0 = torch.zeros(8, 65, device=gpu)
    s = HMC(tgt, theta0, 0.02, 3, generator=torch.Generator(device=gpu).manual_seed(1))
    g0, h0 = glm.glm_launches(), hmc.hmc_launches()
    s.step()
    assert glm.glm_launches() == g0 and hmc.hmc_launches() == h0
    assert torch.isfinite(s.theta).all() and s.last.accept.sum() > 0
    with pytest.raises(RuntimeError, match="impl='kernel'.*D = 65"):
        HMC(tgt, theta0, 0.02, 3, impl="kernel").step()


def test_linreg_invariance_through_the_kernel(gpu):
    """The invariance test of tests/test_hmc.py (same C, T, step size and derived 5-sigma limits)
    with fp32 GPU chains through the fused kernel: chains started at exact posterior draws stay
    posterior-distributed, and the acceptance rate lies strictly inside (0.5, 0.95) so that
    rejections take part."""
    C, T, L, step = 4096, 10, 4, 0.2
    tgt = get_target("linreg", dim=4, n=60, seed=5)
    d = tgt.meta["glm"]
    m, S = linreg_posterior(d.X.double(), d.y.double(), torch.eye(4, dtype=torch.float64),
                            d.noise_var)
    gen = torch.Generator().manual_seed(123)
    theta0 = m + torch.randn(C, 4, generator=gen, dtype=torch.float64) @ torch.linalg.cholesky(S).T
    h0 = hmc.hmc_launches()
    s = HMC(tgt, theta0.float().cuda(), step, L,
            generator=torch.Generator(device=gpu).manual_seed(7), impl="kernel")
    acc = 0.0
    for _ in range(T):
        acc += float(s.step().accept.mean()) / T
    assert hmc.hmc_launches() == h0 + T
    th = s.theta.double().cpu()
    var = torch.diagonal(S)
    print(f"acceptance {acc:.3f}; mean gap / limit "
          f"{((th.mean(0) - m).abs() / (5 * (var / C).sqrt())).max().item():.2f}; var gap / limit "
          f"{((th.var(0) / var - 1).abs() / (5 * math.sqrt(2 / (C - 1)))).max().item():.2f}")
    assert 0.5 < acc < 0.95
    assert ((th.mean(0) - m).abs() <= 5 * (var / C).sqrt()).all()
    assert ((th.var(0) / var - 1).abs() <= 5 * math.sqrt(2 / (C - 1))).all()


# ------------------------------------------------------------------ 7. binding errors
def test_errors(gpu):
    ops = native()
    B, N, D = 8, 9, 3
    th, X, y = torch.randn(B, D, device=gpu), torch.randn(N, D, device=gpu), torch.randn(N, device=gpu)
    v = lambda: torch.zeros(B, device=gpu)        # noqa: E731
    m = lambda: torch.zeros(B, D, device=gpu)     # noqa: E731
    base = dict(theta0=th, p0=m(), logp0=v(), grad0=m(), eps=torch.full((B,), 0.01, device=gpu),
                minv=None, log_u=v(), L=2, X=X, y=y, prec=None, prec_host=1.0, has_prior=True,
                family=0, inv_var=1.0, scale=1.0, rows=0, theta_prop=m(), p_prop=m(),
                theta_out=m(), logp_out=v(), grad_out=m(), accept=v(), dH=v())

    def raw(**kw):
        a = {**base, **kw}
        ops.glm_hmc_trajectory(*a.values())
    raw()
    t65 = torch.randn(4, 65, device=gpu)
    for kw, msg in [
            (dict(theta0=t65, X=t65), "D <= 64"),
            (dict(L=0), "1 <= L <= 1024"),
            (dict(L=1025), "1 <= L <= 1024"),
            (dict(theta0=th.double()), "theta0 must be fp32"),
            (dict(X=X.double()), "X must be fp32"),
            (dict(X=X.cpu()), "X must be on the device"),
            (dict(X=torch.randn(N, D + 1, device=gpu)), "X has shape"),
            (dict(theta0=torch.randn(B, 2 * D, device=gpu)[:, ::2]),
             "theta0 must have unit inner stride"),
            (dict(X=torch.randn(N, 2 * D, device=gpu)[:, ::2]), "X must have unit inner stride"),
            (dict(y=y.double()), "y must be fp32"),
            (dict(y=y[:-1]), "y has shape"),
            (dict(family=3), "unknown family 3"),
            (dict(family=2, inv_var=0.0), "inv_var must be positive"),
            (dict(scale=0.0), "scale must be positive"),
            (dict(prec_host=-1.0), "prec_host = -1"),
            (dict(prec=torch.ones(D + 1, device=gpu)), "prec_dev has shape"),
            (dict(minv=torch.ones(D + 1, device=gpu)), "minv has shape"),
            (dict(eps=torch.zeros(B + 1, device=gpu)), "eps has shape"),
            (dict(log_u=torch.zeros(B, 1, device=gpu)), "log_u has shape"),
            (dict(logp0=torch.zeros(2 * B, device=gpu)[::2]), "logp0 has shape.*not contiguous"),
            (dict(grad0=torch.zeros(B, D + 1, device=gpu)), "grad0 has shape"),
            (dict(p0=torch.zeros(B, 2 * D, device=gpu)[:, :D]), "p0 has shape.*not contiguous"),
            (dict(p0=m().double()), "p0 must be an fp32"),
            (dict(theta_prop=torch.zeros(B, D + 1, device=gpu)), "theta_prop has shape"),
            (dict(p_prop=torch.zeros(B + 1, D, device=gpu)), "p_prop has shape"),
            (dict(theta_out=torch.zeros(B * D, device=gpu)), "theta_out has shape"),
            (dict(logp_out=torch.zeros(B + 1, device=gpu)), "logp_out has shape"),
            (dict(grad_out=torch.zeros(B, 2 * D, device=gpu)[:, :D]),
             "grad_out has shape.*not contiguous"),
            (dict(accept=torch.zeros(B - 1, device=gpu)), "accept has shape"),
            (dict(dH=torch.zeros(B, device=gpu).double()), "dH must be an fp32"),
            (dict(theta_out=th), "shares storage"),
            (dict(rows=48), "rows must be 0"),
            (dict(rows=-1), "rows must be 0")]:
        with pytest.raises(RuntimeError, match=msg):
            raw(**kw)
    raw(prec_host=-1.0, has_prior=False)   # not read without a prior
    # the launcher's row tile: the smallest until its grid covers the card a few times over, and
    # every built size as an override
    assert [ops.glm_hmc_rows(b, d, 0) in ROWS for b, d in [(1, 1), (4096, 64), (1 << 20, 8)]] \
        == [True] * 3
    assert ops.glm_hmc_rows(256, 8, 0) == hmc.kernel_rows(256, 8) == 64
    assert [ops.glm_hmc_rows(b, d, 0) for b, d in [(256, 16), (16384, 16), (256, 64), (256, 17)]] \
        == [32, 64, 128, 128]
    assert ops.glm_hmc_rows(1 << 20, 16, 0) == 128
    for r in ROWS:
        assert ops.glm_hmc_rows(1000, 16, r) == r
    with pytest.raises(RuntimeError, match="rows must be 0"):
        ops.glm_hmc_rows(1000, 16, 100)
    with pytest.raises(RuntimeError, match="1 <= D <= 64"):
        ops.glm_hmc_rows(1000, 65, 0)
    # the Python layer raises before the binding where it can name the argument
    with pytest.raises(ValueError, match="rows must be None or one of"):
        hmc.glm_hmc_step(th, v(), m(), m(), v(), 0.01, 2, X, y, rows=48)
    with pytest.raises(RuntimeError, match="impl='kernel'.*float64"):
        hmc.glm_hmc_step(th.double(), v().double(), m().double(), m().double(), v().double(), 0.01,
                         2, X.double(), y.double(), impl="kernel")
