"""The GLM Newton-statistics HIP kernel (csrc/kernels/glm_hess.hip) against the fp64 CPU composite.

The oracle is glm_hessian_reference of ops/reference.py in fp64 on the fp32 inputs. The limits are
per element, against the oracle's own abs-sums

    A_b   = scale sum_n |ll_bn| + |log prior_b|                                          (logp)
    G_bc  = scale sum_n |r_bn x_nc| + |prec_c theta_bc|                                  (grad)
    W_bjk = scale sum_n |w_bn x_nj x_nk| + prec_j delta_jk                               (H)

as |logp - ref| <= 1e-4 A, |grad - ref| <= 1e-4 G and |H - ref| <= 1e-4 W: the project's
row-kernel rtol (tests/test_glm_gpu.py), above the worst-case fp32 bound for these shapes
(recursive summation at most N 2^-24 ~ 6.6e-5 at N = 1100). A tolerance cannot see one dropped
data row at N = 1100, so the indexing is pinned separately, bitwise, with exactly representable
operands.
"""
import functools
import math

import pytest
import torch

from vi_normflows_amd.distributions.energies import get_target
from vi_normflows_amd.inference.laplace import laplace
from vi_normflows_amd.ops import glm
from vi_normflows_amd.ops._ext import native
from vi_normflows_amd.ops.reference import glm_hessian_reference

pytestmark = pytest.mark.gpu

RTOL = 1e-4
FAMILIES = ("bernoulli", "poisson", "gaussian")
PRIORS = ("scalar", "vector", None)
SCALES = (1.0, 3.5)
NOISE_VAR = 0.7
CASES = [(1, 1, 1), (2, 3, 2), (3, glm.TILE_N + 1, 3), (5, 2 * glm.TILE_N - 1, 17), (2, 300, 64),
         (3, 1100, 5), (4, 513, 16), (3, 200, 32), (3, 200, 33), (2, 260, 40)]
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


def _dev(p):
    return p.cuda() if isinstance(p, torch.Tensor) else p


@functools.lru_cache(maxsize=None)
def _oracle(family, B, N, D, prior, scale):
    """fp64 CPU composite on the fp32 inputs: logp, grad, H, A, G, W (shared, never modified)."""
    theta, X, y = _inputs(family, B, N, D)
    return glm_hessian_reference(theta.double(), X.double(), y.double(), family, _prior(prior, D),
                                 NOISE_VAR, scale, return_abs=True)


def _within(got, oracle, tag):
    """Assert the three limits; returns the worst ratios (logp / A, grad / G, H / W)."""
    lp, g, H, A, G, W = oracle
    tiny = torch.finfo(torch.float64).tiny
    errs = [(a.double().cpu() - b).abs() for a, b in zip(got, (lp, g, H))]
    ratios = [(e / s.clamp_min(tiny)).max().item() for e, s in zip(errs, (A, G, W))]
    print(f"{tag}: logp {ratios[0]:.2e} A, grad {ratios[1]:.2e} G, H {ratios[2]:.2e} W")
    assert all(torch.isfinite(t).all() for t in got), tag
    for e, s in zip(errs, (A, G, W)):
        assert (e <= RTOL * s).all(), tag
    assert torch.equal(got[2], got[2].mT), tag
    return ratios


def _check_case(family, B, N, D, prior, scale, n_splits=None):
    theta, X, y = _inputs(family, B, N, D)
    got = glm.glm_logp_grad_hess(theta.cuda(), X.cuda(), y.cuda(), family, _dev(_prior(prior, D)),
                                 NOISE_VAR, scale, impl="kernel", n_splits=n_splits)
    assert got[0].shape == (B,) and got[1].shape == (B, D) and got[2].shape == (B, D, D)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in got)
    _within(got, _oracle(family, B, N, D, prior, scale),
            f"{family} B={B} N={N} D={D} prior={prior} scale={scale} n_splits={n_splits}")
    return got


@pytest.mark.parametrize("B,N,D", CASES)
def test_kernel_against_fp64_oracle(gpu, B, N, D):
    n0 = glm.glm_launches()
    for family in FAMILIES:
        for prior in PRIORS:
            for scale in SCALES:
                _check_case(family, B, N, D, prior, scale)
    assert glm.glm_launches() == n0 + len(FAMILIES) * len(PRIORS) * len(SCALES)


@pytest.mark.parametrize("B,N,D", [(2, 2 * glm.TILE_N + 1, 5), (2, 1100, 17), (2, 300, 64)])
def test_exact_indexing(gpu, B, N, D):
    """Gaussian family, noise_var = 0.5 (inv_var = 2), no prior, integer X in [-2, 2]: every term
    2 x_nj x_nk and every partial sum of H is an integer of at most 8 N < 2^23, so every fp32
    operation is exact and H must equal scale 2 X^T X bit for bit: a dropped, doubled or misplaced
    row, column, micro-tile or split changes bits. X^T X is not symmetric in its inputs' roles
    (column j against column k of a random X), so a transposed write shows as well."""
    g = torch.Generator().manual_seed(B + N + D)
    theta = torch.randint(-2, 3, (B, D), generator=g).float() / 2
    X = torch.randint(-2, 3, (N, D), generator=g).float()
    y = torch.randint(-3, 4, (N,), generator=g).float()
    XtX = X.double().T @ X.double()
    assert 8 * N < 2 ** 23
    for scale in (1.0, 2.0):
        want = (scale * 2.0 * XtX).float()
        assert torch.equal(want.double(), scale * 2.0 * XtX)
        for ns in SPLITS:
            lp, gr, H = glm.glm_logp_grad_hess(theta.cuda(), X.cuda(), y.cuda(), "gaussian", None,
                                               0.5, scale, impl="kernel", n_splits=ns)
            for b in range(B):
                assert torch.equal(H[b].cpu(), want), (scale, ns, b)


@pytest.mark.parametrize("B,N,D", [(3, 1100, 3), (2, 513, 40)])
def test_split_n(gpu, B, N, D):
    ops = native()
    E = D * D + D + 1
    nt = -(-N // glm.TILE_N)
    assert ops.glm_hess_workspace(B, N, D, 7) == 7 * B * E
    assert ops.glm_hess_workspace(B, N, D, 1000) == nt * B * E   # never more than data tiles
    assert ops.glm_hess_workspace(1, 1 << 20, D, 0) >= 256 * E   # B = 1 fills the card
    assert ops.glm_hess_workspace(1, 100, D, 0) == 2 * E
    for ns in SPLITS:
        a = _check_case("bernoulli", B, N, D, "scalar", 1.0, n_splits=ns)
        b = _check_case("bernoulli", B, N, D, "scalar", 1.0, n_splits=ns)
        assert all(torch.equal(u, v) for u, v in zip(a, b)), ns


def test_row_independence_and_strides(gpu):
    B, N, D = 7, 300, 17
    for family in FAMILIES:
        theta, X, y = (t.cuda() for t in _inputs(family, B, N, D))
        prec = _prior("vector", D).cuda()

        def run(th, XX=X, yy=y):
            return glm.glm_logp_grad_hess(th, XX, yy, family, prec, NOISE_VAR, 3.5, impl="kernel",
                                          n_splits=2)
        ref = run(theta)
        assert torch.equal(ref[2], ref[2].mT)
        for i in (0, 3, B - 1):   # alone: B = 1
            one = run(theta[i:i + 1])
            assert all(torch.equal(u[0], v[i]) for u, v in zip(one, ref)), (family, i)
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).cuda()
        got = run(theta[perm])
        assert all(torch.equal(u, v[perm]) for u, v in zip(got, ref)), family
        # views: a column slice of a wider theta, a column slice of a wider X, a row offset
        wide_t = torch.randn(B, D + 5, device=gpu)
        wide_t[:, 2:2 + D] = theta
        wide_x = torch.randn(N + 100, D + 3, device=gpu)
        wide_x[100:, 1:1 + D] = X
        tv, xv = wide_t[:, 2:2 + D], wide_x[:, 1:1 + D][100:]
        assert tv.stride() == (D + 5, 1) and xv.stride() == (D + 3, 1) and xv.storage_offset() > 0
        n0 = glm.glm_launches()
        for got in (run(tv), run(theta, xv), run(tv, xv)):
            assert all(torch.equal(u, v) for u, v in zip(got, ref)), family
        yw = torch.cat([torch.zeros(100, device=gpu), y])
        got = run(tv, xv, yw[100:])
        assert all(torch.equal(u, v) for u, v in zip(got, ref)), family
        assert glm.glm_launches() == n0 + 4


def test_bernoulli_range(gpu):
    B, N, D = 4, 513, 16
    theta, X, y = _inputs("bernoulli", B, N, D)
    theta = theta * (1e4 / (theta @ X.T).abs().max().item())
    eta = (theta.double() @ X.double().T).abs()
    assert eta.max() > 9.9e3 and (eta > 100).float().mean() > 0.9
    for prior in PRIORS:
        p = _prior(prior, D)
        got = glm.glm_logp_grad_hess(theta.cuda(), X.cuda(), y.cuda(), "bernoulli", _dev(p),
                                     impl="kernel")
        _within(got, glm_hessian_reference(theta.double(), X.double(), y.double(), "bernoulli", p,
                                           return_abs=True), f"range prior={prior}")
        diag = got[2].diagonal(dim1=1, dim2=2).cpu()
        floor = p if isinstance(p, torch.Tensor) else torch.full((D,), float(p or 0.0))
        assert (diag >= floor).all(), prior


def test_errors(gpu):
    ops = native()
    th, X, y = torch.randn(8, 3, device=gpu), torch.randn(9, 3, device=gpu), torch.randn(9, device=gpu)
    lp, g, H = (torch.empty(8, device=gpu), torch.empty(8, 3, device=gpu),
                torch.empty(8, 3, 3, device=gpu))
    assert ops.glm_hess_workspace(8, 9, 3, 1) == 8 * 13
    assert ops.glm_hess_workspace(8, 200, 3, 2) == 2 * 8 * 13
    work = torch.empty(ops.glm_hess_workspace(8, 9, 3, 1), device=gpu)

    def raw(th=th, X=X, y=y, prec=None, prec_host=1.0, has_prior=True, family=0, inv_var=1.0,
            scale=1.0, ns=1, lp=lp, g=g, H=H, work=work):
        ops.glm_logp_grad_hess(th, X, y, prec, prec_host, has_prior, family, inv_var, scale, ns,
                               lp, g, H, work)
    raw()
    t65 = torch.randn(4, 65, device=gpu)
    with pytest.raises(RuntimeError, match="D <= 64"):
        raw(th=t65, X=t65, y=torch.randn(4, device=gpu))
    with pytest.raises(RuntimeError, match="D <= 64"):
        ops.glm_hess_workspace(4, 4, 65, 0)
    with pytest.raises(RuntimeError, match="impl='kernel'.*D = 65"):
        glm.glm_logp_grad_hess(t65, t65, torch.randn(4, device=gpu), impl="kernel")
    with pytest.raises(RuntimeError, match="theta must be a GPU tensor"):
        raw(th=th.cpu())
    with pytest.raises(RuntimeError, match="theta \\[B, D\\] expected"):
        raw(th=th[0])
    with pytest.raises(RuntimeError, match="theta must be fp32"):
        raw(th=th.double())
    with pytest.raises(RuntimeError, match="X must be fp32"):
        raw(X=X.double())
    with pytest.raises(RuntimeError, match="X must be on the device"):
        raw(X=X.cpu())
    with pytest.raises(RuntimeError, match="X has shape"):
        raw(X=torch.randn(9, 4, device=gpu))
    with pytest.raises(RuntimeError, match="y must be fp32"):
        raw(y=y.double())
    with pytest.raises(RuntimeError, match="y must be on the device"):
        raw(y=y.cpu())
    with pytest.raises(RuntimeError, match="impl='kernel'.*float64"):
        glm.glm_logp_grad_hess(th.double(), X.double(), y.double(), impl="kernel")
    with pytest.raises(RuntimeError, match="y has shape"):
        raw(y=y[:-1])
    with pytest.raises(ValueError, match="y must have one entry per row"):
        glm.glm_logp_grad_hess(th, X, y[:-1], impl="kernel")
    with pytest.raises(RuntimeError, match="scale must be positive"):
        raw(scale=0.0)
    with pytest.raises(ValueError, match="scale must be positive"):
        glm.glm_logp_grad_hess(th, X, y, scale=-1.0, impl="kernel")
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
    with pytest.raises(RuntimeError, match="hess has"):
        raw(H=torch.empty(8, 3, 4, device=gpu))
    with pytest.raises(RuntimeError, match="hess must be a contiguous"):
        raw(H=torch.empty(8, 3, 6, device=gpu)[:, :, ::2])
    with pytest.raises(RuntimeError, match="grad has"):
        raw(g=torch.empty(8, 4, device=gpu))
    with pytest.raises(RuntimeError, match="logp has"):
        raw(lp=torch.empty(9, device=gpu))
    with pytest.raises(RuntimeError, match="n_splits"):
        raw(ns=-1)
    with pytest.raises(RuntimeError, match="n_splits"):
        raw(ns=65536)
    with pytest.raises(RuntimeError, match="n_splits"):
        ops.glm_hess_workspace(8, 9, 3, -1)
    # the wrapper copies what the kernel cannot stride over, instead of raising
    tt = torch.randn(8, 6, device=gpu)[:, ::2]
    assert torch.equal(glm.glm_logp_grad_hess(tt, X, y, impl="kernel")[2],
                       glm.glm_logp_grad_hess(tt.contiguous(), X, y, impl="kernel")[2])


def test_auto_falls_back_beyond_64_dimensions(gpu):
    th, X = torch.randn(5, 65, device=gpu) / 8, torch.randn(40, 65, device=gpu)
    y = torch.bernoulli(torch.full((40,), 0.5, device=gpu))
    n0 = glm.glm_launches()
    got, want = glm.glm_logp_grad_hess(th, X, y), glm_hessian_reference(th, X, y)
    assert all(torch.equal(u, v) for u, v in zip(got, want))
    assert glm.glm_launches() == n0
    glm.glm_logp_grad_hess(th[:, :64], X[:, :64], y)
    assert glm.glm_launches() == n0 + 1


def test_laplace_end_to_end(gpu):
    """laplace on GPU fp32: one kernel launch per call of the Newton statistics, and a mode that
    the fp64 oracle agrees is one. At the returned mode, with the oracle's g, G, H and its Newton
    step delta = H^-1 g:

        |delta_c| <= sum_k |H^-1|_ck 1e-4 G_k + xtol (1 + |theta_c|)

    A converged iterate's own (kernel) step is at most xtol-scale, and it differs from the true
    step by at most |H^-1| times the gradient limit; the Hessian's own error enters at second
    order."""
    tgt = get_target("logreg", dim=8, n=500, seed=11)
    d = tgt.meta["glm"]
    n0 = glm.glm_launches()
    res = laplace(tgt, device=gpu)
    nr = res.newton
    assert nr.theta.is_cuda and nr.theta.dtype == torch.float32 and res.converged.all()
    assert glm.glm_launches() == n0 + nr.n_evals
    assert nr.n_evals == 1 + int(nr.n_iter.max()) + nr.n_backtracks
    xtol = math.sqrt(torch.finfo(torch.float32).eps)   # newton_map's default
    mode = res.mode[None]
    lp, g, H, A, G, W = glm_hessian_reference(mode, d.X.double(), d.y.double(), d.family, d.prec,
                                              d.noise_var, return_abs=True)
    Hinv = torch.linalg.inv(H[0])
    delta = Hinv @ g[0]
    lim = Hinv.abs() @ (RTOL * G[0]) + xtol * (1 + mode[0].abs())
    print(f"iterations {nr.n_iter.tolist()}, max |delta| / limit = {(delta.abs() / lim).max():.3e}")
    assert (delta.abs() <= lim).all()
    cpu = laplace(tgt, dtype=torch.float64)
    print(f"log evidence GPU fp32 {res.log_evidence:.6f}, CPU fp64 {cpu.log_evidence:.6f}, "
          f"limit {RTOL * float(A[0]):.2e}")
    assert abs(res.log_evidence - cpu.log_evidence) <= RTOL * float(A[0])
