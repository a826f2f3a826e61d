"""The fused Sylvester stack kernels (csrc/kernels/sylvester.hip) against the fp64 CPU composite
on the same fp32 values, for shared and per-sample parameters.

Tolerances: z atol 2e-4, rtol 1e-4 (the project's flow-kernel tolerance); a row's ldj atol
2e-4 + 2e-6 D K (the spline test's per-log-term allowance times the D K terms of a row), rtol
1e-4; gradients |delta| <= 2e-3 (1 + max|ref|) per tensor, as in test_planar_stack_kernel. The
fp32 composite stays under 1 % of each limit on these inputs (asserted to be inside them
without a GPU in test_sylvester.py)."""
import pytest
import torch

from test_sylvester import (GPU_CASES, PARAM_NAMES, grad_ratio, make_cotangents, make_inputs,
                            oracle, output_limits, run_stack, worst_ratio)
from vi_normflows_amd.ops import sylvester as syl

pytestmark = pytest.mark.gpu

IDS = ["%dx%dk%dh%d" % c for c in GPU_CASES]
MODES = pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per_sample"])
CASES = pytest.mark.parametrize("case", GPU_CASES, ids=IDS)


def _to(dev, o):
    z = o["z"].to(dev).requires_grad_(True)
    params = [p.to(dev).requires_grad_(True) for p in o["params"]]
    return z, params


def _run(dev, o, impl="kernel"):
    """Forward + backward on the GPU: (zK, ldj, {name: grad})."""
    z, params = _to(dev, o)
    zK, ldj = run_stack(z, params, o["flips"], impl)
    ((zK * o["gz"].to(dev)).sum() + (ldj * o["gl"].to(dev)).sum()).backward()
    grads = {"z": z.grad, **{n: p.grad for n, p in zip(PARAM_NAMES, params)}}
    return zK.detach(), ldj.detach(), grads


@MODES
@CASES
def test_kernel_outputs_match_fp64(gpu, case, per_sample):
    N, D, K, H = case
    o = oracle(case, per_sample)
    z, params = _to(gpu, o)
    with torch.no_grad():
        zK, ldj = run_stack(z, params, o["flips"], "kernel")
    assert zK.dtype == torch.float32 and zK.shape == (N, D) and ldj.shape == (N,)
    for name, got in (("zK", zK), ("ldj", ldj)):
        atol, rtol = output_limits(o, D, K)[name]
        r = worst_ratio(got, o[name], atol, rtol)
        print(f"{name}: worst err / limit {r:.4f}")
        assert r <= 1.0, name


@MODES
@CASES
def test_kernel_gradients_match_fp64(gpu, case, per_sample):
    o = oracle(case, per_sample)
    _, _, grads = _run(gpu, o)
    for name, ref in o["grads"].items():
        got = grads[name]
        if got is None:                      # an empty tensor (D = 1: R, H = 0: V)
            assert ref.numel() == 0, name
            continue
        assert got.shape == ref.shape and got.dtype == torch.float32, name
        r = grad_ratio(got, ref)
        print(f"d{name}: err / limit {r:.4f}")
        assert r <= 1.0, name


def _packed(dev, case, pad=3):
    """Per-sample raw parameters as column slices of one [N, Dout] buffer (``pad`` unused
    columns in front of, between and behind them), plus dense copies."""
    N, D, K, H = case
    z, params, flips = make_inputs(N, D, K, H, True)
    widths = [p[0].numel() for p in params]
    buf = torch.full((N, sum(widths) + pad * 7), 7.0)
    views, spans, o = [], [], pad
    for p, w in zip(params, widths):
        buf[:, o:o + w] = p.reshape(N, w)
        spans.append((o, o + w))
        o += w + pad
    buf = buf.to(dev).requires_grad_(True)
    for p, (a, b) in zip(params, spans):
        views.append(buf[:, a:b].unflatten(1, tuple(p.shape[1:])))
    dense = [p.to(dev).requires_grad_(True) for p in params]
    return z.to(dev), buf, views, spans, dense, flips


@pytest.mark.parametrize("case", [(40, 40, 4, 8), (33, 63, 2, 1), (64, 5, 3, 5)],
                         ids=["40x40k4h8", "33x63k2h1", "64x5k3h5"])
def test_strided_views_equal_dense_copies(gpu, case):
    N, D, K, H = case
    z, buf, views, spans, dense, flips = _packed(gpu, case)
    gz, gl = (t.to(gpu) for t in make_cotangents(N, D, K, H, True))
    # R1, R2, b, V reach the op as the strided views themselves (the diagonals pass through
    # tanh first): the op must see the buffer's row stride
    assert all(v.stride(0) == buf.shape[1] and v.data_ptr() != d.data_ptr()
               for v, d in zip(views, dense))
    zs, ls = run_stack(z, views, flips, "kernel")
    ((zs * gz).sum() + (ls * gl).sum()).backward()
    zd, ld = run_stack(z, dense, flips, "kernel")
    ((zd * gz).sum() + (ld * gl).sum()).backward()
    assert torch.equal(zs, zd) and torch.equal(ls, ld)
    inside = torch.zeros(buf.shape[1], dtype=torch.bool, device=gpu)
    for (a, b), d in zip(spans, dense):
        inside[a:b] = True
        assert torch.equal(buf.grad[:, a:b], d.grad.reshape(N, -1))
    assert bool((buf.grad[:, ~inside] == 0).all())
    assert bool((buf.grad[:, inside] != 0).any())


def test_op_rejects_a_non_dense_inner_dimension(gpu):
    N, D, K, H = 6, 5, 2, 1
    z, params, flips = make_inputs(N, D, K, H, True)
    z = z.to(gpu)
    R1, R2, d1, d2, b, V = (p.to(gpu) for p in params)
    wide = torch.randn(N, K, 2 * R1.shape[2], device=gpu)
    with pytest.raises(RuntimeError, match="dense inner"):
        syl.sylvester_fwd(z, wide[:, :, ::2], R2, d1, d2, b, V, flips)
    kt = torch.randn(K, N, D, device=gpu).transpose(0, 1)       # [N, K, D], layer-major memory
    with pytest.raises(RuntimeError, match="dense inner"):
        syl.sylvester_fwd(z, R1, R2, d1, d2, kt, V, flips)
    with pytest.raises(RuntimeError, match="flips"):
        syl.sylvester_fwd(z, R1, R2, d1, d2, b, V, flips[:1])
    with pytest.raises(RuntimeError, match="packed"):
        syl.sylvester_fwd(z, R1[:, :, :-1], R2, d1, d2, b, V, flips)
    with pytest.raises(RuntimeError, match="fp32"):
        syl.sylvester_fwd(z, R1.double(), R2, d1, d2, b, V, flips)
    # the autograd wrapper makes such a tensor dense itself
    zk, _ = syl.sylvester_stack(z, R1, R2, d1, d2, kt, V, flips, impl="kernel")
    zr, _ = syl.sylvester_stack(z, R1, R2, d1, d2, kt.contiguous(), V, flips, impl="kernel")
    assert torch.equal(zk, zr)


@MODES
def test_two_runs_are_bitwise_equal(gpu, per_sample):
    o = oracle((130, 33, 3, 4), per_sample)
    a, b = _run(gpu, o), _run(gpu, o)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


def test_shared_gradient_sum_does_not_depend_on_the_chunking(gpu, monkeypatch):
    """1000 rows of shared parameters: one chunk under the default budget, four chunks (one
    block of rows each) under a budget below one block."""
    N, D, K, H = 1000, 5, 3, 2
    z, params, flips = make_inputs(N, D, K, H, False)
    gz, gl = make_cotangents(N, D, K, H, False)
    o = dict(z=z, params=params, flips=flips, gz=gz, gl=gl)
    calls = []
    real = syl.sylvester_bwd

    def counting(*a, **k):
        calls.append(a[0].shape[0])
        return real(*a, **k)

    monkeypatch.setattr(syl, "sylvester_bwd", counting)
    whole = _run(gpu, o)
    assert calls == [N]
    monkeypatch.setattr(syl, "SHARED_GRAD_BUDGET_BYTES", 1024)
    del calls[:]
    split = _run(gpu, o)
    assert calls == [256, 256, 256, 232]
    for n in whole[2]:
        assert torch.equal(whole[2][n], split[2][n]), n
    # and the sum is the right one
    ref = oracle_grads_fp64(o)
    for n, g in ref.items():
        assert grad_ratio(whole[2][n], g) <= 1.0, n


def oracle_grads_fp64(o):
    zz = o["z"].double().requires_grad_(True)
    pp = [p.double().requires_grad_(True) for p in o["params"]]
    zK, ldj = run_stack(zz, pp, o["flips"])
    grads = torch.autograd.grad((zK * o["gz"].double()).sum() + (ldj * o["gl"].double()).sum(),
                                [zz, *pp])
    return dict(zip(("z",) + PARAM_NAMES, grads))


def test_limits_raise_from_the_op_and_auto_falls_back(gpu, monkeypatch):
    used = []
    real = syl.reference.sylvester_stack_reference

    def spy(*a, **k):
        used.append(1)
        return real(*a, **k)

    monkeypatch.setattr(syl.reference, "sylvester_stack_reference", spy)
    for (N, D, K, H), what in (((3, 65, 1, 1), "D <= 64"), ((3, 4, 1, 17), "H <= 16")):
        z, params, flips = make_inputs(N, D, K, H, False)
        z = z.to(gpu)
        R1, R2, d1, d2, b, V = (p.to(gpu) for p in params)
        with pytest.raises(RuntimeError, match=what):
            syl.sylvester_fwd(z, R1, R2, d1, d2, b, V, flips)
        with pytest.raises(RuntimeError, match=what):
            syl.sylvester_stack(z, R1, R2, d1, d2, b, V, flips, impl="kernel")
        del used[:]
        zK, ldj = syl.sylvester_stack(z, R1, R2, d1, d2, b, V, flips)      # auto
        assert used and zK.is_cuda and zK.shape == (N, D)
    z, params, flips = make_inputs(4, 3, 2, 1, False, dtype=torch.float64)
    del used[:]
    zK, _ = syl.sylvester_stack(z.to(gpu), *(p.to(gpu) for p in params), flips)
    assert used and zK.dtype == torch.float64
    del used[:]
    z, params, flips = make_inputs(4, 3, 2, 1, False)
    syl.sylvester_stack(z.to(gpu), *(p.to(gpu) for p in params), flips)
    assert not used                                   # fp32 inside the limits: the kernel


def test_vae_module_path_matches_fp64(gpu, monkeypatch):
    """SylvesterVAE (dz 40, K 2, H 4, width 64, N 16): per-sample free-energy terms
    log q0 - ldj - log p on the GPU against the same weights and noise in fp64 on the CPU. The
    kernel path may err at most 4x what the fp32 composite path on the GPU errs against that
    oracle. Measured on an MI355X (profiles/r8/sylvester_gpu_tests.txt): composite 8.8e-5,
    kernel 8.8e-5, on terms of up to 546; both are the error of the fp32 GPU encoder and
    decoder, which the two paths share."""
    from vi_normflows_amd.inference import elbo
    from vi_normflows_amd.models.sylvester_vae import SylvesterVAE
    from vi_normflows_amd.models.vae import VAEConfig

    cfg = VAEConfig(dim_x=784, dim_z=40, K=2, width=64, hidden_layers=3)
    N = 16
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(N, cfg.dim_x, generator=g) < 0.3).float()
    eps = torch.randn(N, cfg.dim_z, generator=g)

    def terms(vae, x, eps):
        mu, lv, fp = vae.encode(x)
        z0 = mu + torch.exp(0.5 * lv) * eps
        lq0 = (-0.5 * cfg.dim_z * elbo.LOG2PI - 0.5 * lv.sum(1) - 0.5 * (eps * eps).sum(1))
        zK, ldj = vae.flow(z0, fp)
        return (lq0 - ldj - vae.log_joint(x, zK)).detach().double().cpu()

    def build(impl, dtype, dev):
        vae = SylvesterVAE(cfg, householders=4, impl=impl)
        vae.init_reference(scale=0.05, generator=torch.Generator().manual_seed(3))
        return vae.to(dtype).to(dev)

    ref = terms(build("composite", torch.float64, "cpu"), x.double(), eps.double())
    calls = []
    real = syl.sylvester_fwd

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(syl, "sylvester_fwd", counting)
    with torch.no_grad():
        comp = terms(build("composite", torch.float32, gpu), x.to(gpu), eps.to(gpu))
        assert not calls
        kern = terms(build("auto", torch.float32, gpu), x.to(gpu), eps.to(gpu))
    assert calls == [1]                               # the kernel op ran
    e_comp = float((comp - ref).abs().max())
    e_kern = float((kern - ref).abs().max())
    print(f"free-energy terms vs fp64: composite {e_comp:.3e}, kernel {e_kern:.3e}, "
          f"max|ref| {float(ref.abs().max()):.3e}")
    assert e_comp > 0
    assert e_kern <= 4 * e_comp
