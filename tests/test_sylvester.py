"""Sylvester flows: the torch composite against the definition, the packing, the flow modules,
the VAE and the VI / CLI plumbing (CPU), and the seeded input helper shared with
``test_sylvester_gpu.py``."""
import functools
import math
import os
import subprocess
import sys

import pytest
import torch

from vi_normflows_amd.ops.reference import SYL_EPS, sylvester_basis_apply
from vi_normflows_amd.ops.sylvester import sylvester_stack, tri_index, tri_pack, tri_unpack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "vi_normflows_amd", "_native", "libvinf_hip.so")

# (N, D, K, H) of the GPU tests: D = 1 (empty R), a partly filled wave, a full wave, the H limit,
# a single row; each with shared and with per-sample parameters
GPU_CASES = [(257, 1, 3, 0), (300, 2, 4, 2), (64, 5, 3, 5), (40, 40, 4, 8), (17, 64, 2, 16),
             (33, 63, 2, 1), (1, 3, 2, 0), (130, 33, 3, 4)]
PARAM_NAMES = ("R1", "R2", "d1_raw", "d2_raw", "b", "V")


def make_inputs(N, D, K, H, per_sample, seed=0, dtype=torch.float32):
    """Seeded inputs of one case: ``z`` [N, D], the six parameters (raw diagonals; shared
    [K, ...] or per-sample [N, K, ...]) and the flips k mod 2. R ~ N(0, (1.5 / sqrt D)^2), raw
    diagonals ~ N(0, 0.8^2), b, V, z ~ N(0, 1)."""
    g = torch.Generator().manual_seed(
        seed * 1_000_003 + ((N * 1009 + D) * 67 + K) * 37 + H * 2 + int(per_sample))
    lead = (N, K) if per_sample else (K,)
    P = D * (D - 1) // 2

    def rn(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(dtype)

    z = rn(N, D)
    R1, R2 = rn(*lead, P, scale=1.5 / math.sqrt(D)), rn(*lead, P, scale=1.5 / math.sqrt(D))
    d1_raw, d2_raw = rn(*lead, D, scale=0.8), rn(*lead, D, scale=0.8)
    b, V = rn(*lead, D), rn(*lead, H, D)
    return z, [R1, R2, d1_raw, d2_raw, b, V], [k % 2 for k in range(K)]


def make_cotangents(N, D, K, H, per_sample):
    g = torch.Generator().manual_seed(N * 7919 + D * 31 + K * 5 + H + 100 * int(per_sample))
    return torch.randn(N, D, generator=g), torch.randn(N, generator=g)


def run_stack(z, params, flips, impl="composite"):
    """The stack on raw diagonals: tanh squashing in torch, as the modules do."""
    R1, R2, d1_raw, d2_raw, b, V = params
    return sylvester_stack(z, R1, R2, torch.tanh(d1_raw), torch.tanh(d2_raw), b, V, flips,
                           impl=impl)


@functools.lru_cache(maxsize=None)
def oracle(case, per_sample, dtype=torch.float64):
    """Outputs and gradients of sum(z_K g) + sum(ldj c) from the CPU composite in ``dtype`` on
    the fp32 inputs of one case (computed once, shared, never modified)."""
    N, D, K, H = case
    z, params, flips = make_inputs(N, D, K, H, per_sample)
    gz, gl = make_cotangents(N, D, K, H, per_sample)
    zz = z.to(dtype).requires_grad_(True)
    pp = [p.to(dtype).requires_grad_(True) for p in params]
    zK, ldj = run_stack(zz, pp, flips)
    grads = torch.autograd.grad((zK * gz.to(dtype)).sum() + (ldj * gl.to(dtype)).sum(),
                                [zz, *pp], allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, [zz, *pp])]
    return dict(z=z, params=params, flips=flips, gz=gz, gl=gl, zK=zK.detach(),
                ldj=ldj.detach(), grads=dict(zip(("z",) + PARAM_NAMES, grads)))


def output_limits(o, D, K):
    """(atol, rtol) per output: the project's flow-kernel tolerance for z; for ldj the spline
    test's per-log-term allowance times the D K terms of a row."""
    return {"zK": (2e-4, 1e-4), "ldj": (2e-4 + 2e-6 * D * K, 1e-4)}


def worst_ratio(got, ref, atol, rtol):
    err = (got.double().cpu() - ref.double()).abs()
    lim = atol + rtol * ref.double().abs()
    return float((err / lim).max()) if err.numel() else 0.0


def grad_ratio(got, ref):
    """|delta| / (2e-3 (1 + max|ref|)), the bound of test_planar_stack_kernel."""
    if ref.numel() == 0:
        return 0.0
    err = float((got.double().cpu() - ref.double()).abs().max())
    return err / (2e-3 * (1.0 + float(ref.abs().max())))


# ------------------------------------------------------------------ definition
def _jac_logdet(z, params, flips, n):
    """slogdet of the autograd Jacobian of row n."""
    per = params[2].dim() == 3
    row = [p[n:n + 1] if per else p for p in params]

    def f(x):
        return run_stack(x.unsqueeze(0), row, flips)[0].squeeze(0)

    return torch.linalg.slogdet(torch.autograd.functional.jacobian(f, z[n]))[1]


@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per_sample"])
@pytest.mark.parametrize("D,K,H", [(5, 3, 0), (5, 3, 2), (1, 2, 0), (7, 2, 2)])
def test_ldj_is_the_log_det_of_the_jacobian(D, K, H, per_sample):
    N = 4
    z, params, flips = make_inputs(N, D, K, H, per_sample, seed=1, dtype=torch.float64)
    _, ldj = run_stack(z, params, flips)
    ref = torch.stack([_jac_logdet(z, params, flips, n) for n in range(N)])
    # the guard adds at most log(1 + 1e-7 / |psi|) per term; |psi| > 1 - tanh(.)^2 here
    print("ldj vs slogdet:", float((ldj - ref).abs().max()))
    assert (ldj - ref).abs().max() <= 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per_sample"])
def test_zero_parameters_are_the_identity(dtype, per_sample):
    """z' = z bit for bit. The definition's guard makes a layer's ldj D log(1 + 1e-7), not 0:
    the test asserts exactly that value, i.e. zero up to the size of the guard."""
    N, D, K, H = 6, 5, 3, 2
    z, params, flips = make_inputs(N, D, K, H, per_sample, dtype=dtype)
    zero = [torch.zeros_like(p) for p in params]
    zero[5] = params[5]                       # any reflections: Q Q^T y with y = 0
    zK, ldj = run_stack(z, zero, flips)
    assert torch.equal(zK, z)
    guard = D * K * math.log1p(SYL_EPS)
    assert (ldj - guard).abs().max() <= (2e-7 if dtype == torch.float32 else 1e-15) * D * K
    assert ldj.abs().max() <= 1.3e-7 * D * K


def test_zero_v_is_the_identity_reflection_with_zero_gradient():
    N, D, K, H = 5, 4, 2, 2
    z, params, flips = make_inputs(N, D, K, H, True, dtype=torch.float64)
    noref = [p.clone() for p in params]
    noref[5] = params[5][:, :, :0]            # H = 0
    params[5] = torch.zeros_like(params[5]).requires_grad_(True)
    zK, ldj = run_stack(z, params, flips)
    zK0, ldj0 = run_stack(z, noref, flips)
    assert torch.equal(zK, zK0) and torch.equal(ldj, ldj0)
    (zK.sum() + ldj.sum()).backward()
    assert torch.equal(params[5].grad, torch.zeros_like(params[5]))


@pytest.mark.parametrize("flip", [False, True])
def test_basis_is_orthogonal(flip):
    D, H = 9, 4
    g = torch.Generator().manual_seed(5)
    Vk = torch.randn(H, D, generator=g, dtype=torch.float64)
    eye = torch.eye(D, dtype=torch.float64)
    Q = sylvester_basis_apply(eye, Vk, flip, transpose=False).t()     # columns Q e_i
    Qt = sylvester_basis_apply(eye, Vk, flip, transpose=True).t()
    assert (Q.t() @ Q - eye).abs().max() <= 1e-12
    assert (Qt - Q.t()).abs().max() <= 1e-12
    assert flip == bool((Q - sylvester_basis_apply(eye, Vk, False, False).t()).abs().max() > 0.1)


@pytest.mark.parametrize("D", [1, 2, 5, 64])
def test_tri_pack_round_trip_and_index_formula(D):
    P = D * (D - 1) // 2
    g = torch.Generator().manual_seed(D)
    A = torch.randn(3, D, D, generator=g, dtype=torch.float64)
    upper = torch.triu(A, 1)
    p = tri_pack(A)
    assert p.shape == (3, P)
    assert torch.equal(tri_unpack(p, D), upper)
    assert torch.equal(tri_pack(tri_unpack(p, D)), p)
    rows, cols = tri_index(D)
    assert bool((rows < cols).all()) and rows.numel() == P
    for i in range(D):
        for j in range(i + 1, D):
            assert float(p[1, j * (j - 1) // 2 + i]) == float(A[1, i, j])
    with pytest.raises(ValueError):
        tri_unpack(torch.zeros(P + 1), D)


# --------------------------------------------------------------------- modules
def test_stack_module_shapes_init_and_variants():
    from vi_normflows_amd.flows import SylvesterStack

    f = SylvesterStack(5, 4, householders=3)
    assert f.R1.shape == (4, 10) and f.V.shape == (4, 3, 5) and f.flips == [0, 0, 0, 0]
    assert float(f.R1.detach().std()) < 0.03 and float(f.d1_raw.detach().abs().max()) < 0.1
    assert 0.5 < float(f.V.detach().std()) < 1.5
    t = SylvesterStack(5, 4, householders=3, basis="triangular")
    assert t.V.shape == (4, 0, 5) and t.flips == [0, 1, 0, 1]
    x = torch.randn(7, 5)
    for fl in (f, t):
        y, ldj = fl(x)
        assert y.shape == x.shape and ldj.shape == (7,) and (y - x).abs().max() < 0.2
    with pytest.raises(ValueError):
        SylvesterStack(5, 2, basis="orthogonal")
    with pytest.raises(ValueError):
        SylvesterStack(5, 2, householders=17)


def test_amortized_split_returns_views_of_the_block():
    from vi_normflows_amd.flows import AmortizedSylvester

    D, K, H, N = 6, 3, 2, 5
    fl = AmortizedSylvester(D, K, H)
    assert fl.uses_context
    P = D * (D - 1) // 2
    assert fl.param_width() == K * (2 * P + 3 * D + H * D)
    phi = torch.randn(N, 2 * D + fl.param_width())
    parts = fl.split(phi[:, 2 * D:])
    lo, hi = phi.data_ptr(), phi.data_ptr() + phi.numel() * phi.element_size()
    shapes = [(N, K, P), (N, K, P), (N, K, D), (N, K, D), (N, K, D), (N, K, H, D)]
    for p, s in zip(parts, shapes):
        assert p.shape == s and lo <= p.data_ptr() < hi and p._base is not None
        assert p.stride(0) == phi.shape[1] and p[0].is_contiguous()
    cols = torch.cat([p.reshape(N, -1) for p in parts], 1)
    assert torch.equal(cols, phi[:, 2 * D:])                  # in order, nothing skipped
    tr = AmortizedSylvester(D, K, H, basis="triangular")
    assert tr.param_width() == K * (2 * P + 3 * D) and tr.flips == [0, 1, 0]


def _small_vae(K=2, H=2, dz=6, basis="householder"):
    from vi_normflows_amd.models.sylvester_vae import SylvesterVAE
    from vi_normflows_amd.models.vae import VAEConfig

    cfg = VAEConfig(dim_x=20, dim_z=dz, K=K, width=16, hidden_layers=2)
    vae = SylvesterVAE(cfg, householders=H, basis=basis).double()
    vae.init_reference(scale=0.3, generator=torch.Generator().manual_seed(2))
    return vae, cfg


@pytest.mark.parametrize("basis", ["householder", "triangular"])
def test_vae_every_encoder_column_gets_a_gradient(basis):
    vae, cfg = _small_vae(basis=basis)
    x = (torch.rand(9, cfg.dim_x, generator=torch.Generator().manual_seed(1)) < 0.5).double()
    assert vae.encoder.Dout == 2 * cfg.dim_z + vae.flow.param_width()
    vae.loss(x, generator=torch.Generator().manual_seed(4)).F.backward()
    gb = vae.encoder.linears[-1].bias.grad
    assert gb.shape == (vae.encoder.Dout,)
    assert bool((gb != 0).all()), (gb == 0).nonzero().flatten().tolist()


def test_vae_with_a_zero_flow_block_is_the_flowless_planar_vae():
    from vi_normflows_amd.models.vae import PlanarVAE, VAEConfig

    vae, cfg = _small_vae()
    dz = cfg.dim_z
    with torch.no_grad():
        vae.encoder.linears[-1].weight[2 * dz:].zero_()
        vae.encoder.linears[-1].bias[2 * dz:].zero_()
    base = PlanarVAE(VAEConfig(dim_x=cfg.dim_x, dim_z=dz, K=0, width=cfg.width,
                               hidden_layers=cfg.hidden_layers)).double()
    with torch.no_grad():
        for a, b in zip(base.encoder.linears[:-1], vae.encoder.linears[:-1]):
            a.weight.copy_(b.weight)
            a.bias.copy_(b.bias)
        base.encoder.linears[-1].weight.copy_(vae.encoder.linears[-1].weight[:2 * dz])
        base.encoder.linears[-1].bias.copy_(vae.encoder.linears[-1].bias[:2 * dz])
        base.decoder.load_state_dict(vae.decoder.state_dict())
    x = (torch.rand(9, cfg.dim_x, generator=torch.Generator().manual_seed(1)) < 0.5).double()
    Fs = float(vae.loss(x, generator=torch.Generator().manual_seed(4)).F)
    Fp = float(base.loss(x, generator=torch.Generator().manual_seed(4)).F)
    # identity flow; its ldj is the guard's dz K log(1 + 1e-7)
    assert abs((Fp - Fs) - dz * cfg.K * math.log1p(SYL_EPS)) <= 1e-12 * max(1.0, abs(Fp))


# ------------------------------------------------------------- build_flow, CLI
def test_build_flow_sylvester_and_state_dict_round_trip():
    import normflows.flows as shim
    from vi_normflows_amd.flows import AmortizedSylvester, SylvesterStack
    from vi_normflows_amd.inference.flow_vi import build_flow

    assert shim.SylvesterStack is SylvesterStack and shim.AmortizedSylvester is AmortizedSylvester
    a = build_flow("sylvester", 3, 4)
    assert isinstance(a, SylvesterStack) and a.householders == 1 and a.basis == "householder"
    b = build_flow("sylvester", 3, 4)
    b.load_state_dict(a.state_dict())
    x = torch.randn(16, 3)
    (ya, la), (yb, lb) = a(x), b(x)
    assert torch.equal(ya, yb) and torch.equal(la, lb) and (ya - x).abs().max() > 1e-5
    c = build_flow("sylvester", 3, 4, householders=2, basis="triangular")
    assert c.householders == 0 and c.flips == [0, 1, 0, 1]
    assert build_flow("sylvester", 3, 2, householders=3).V.shape == (2, 3, 3)


def test_train_cli_sylvester(tmp_path):
    from vi_normflows_amd.train import main

    out = main(["--config", "config1_two_moons_cpu", "flow=sylvester", "K=2", "iters=20",
                "log_every=10", "extra.householders=2", f"out_dir={tmp_path}"])
    assert math.isfinite(out["free_energy"])
    sd = torch.load(tmp_path / "config1_two_moons_cpu" / "flow.pt")
    assert sd["V"].shape == (2, 2, 2)          # extra.householders reached the flow


def test_train_cli_sylvester_vae(tmp_path):
    from vi_normflows_amd.train import main

    out = main(["--config", "mnist_planar_vae", "extra.flow=sylvester", "extra.householders=2",
                "K=2", "iters=5", "device=cpu", "log_every=5", "extra.n_data=64", "batch=32",
                f"out_dir={tmp_path}"])
    assert out["engine"] == "module" and math.isfinite(out["free_energy_per_sample"])


def test_sylvester_vi_beats_planar_on_u1():
    """KL(q || p) = F + log Z on U1, 8 layers, one reflection, Adam lr 1e-2, 300 iterations, 512
    samples: above the project's floor tolerance (-0.05), below 0.45 (2x what a prototype of
    this definition and initialisation reached, 0.20 - 0.24), and below a random-init planar
    stack of K = 8 on the same budget (0.86 in the prototype)."""
    from vi_normflows_amd.inference.flow_vi import fit_flow_vi

    kw = dict(K=8, iters=300, lr=1e-2, n_samples=512, optimizer="adam")
    kl = fit_flow_vi("U1", "sylvester", householders=1, **kw).final["kl_estimate"]
    kl_planar = fit_flow_vi("U1", "planar", init="random", **kw).final["kl_estimate"]
    print(f"U1 kl_estimate: sylvester {kl:.4f}, planar {kl_planar:.4f}")
    assert -0.05 < kl < 0.45
    assert kl < kl_planar


@pytest.mark.skipif(not os.path.exists(LIB), reason="native library not built")
def test_native_library_registers_sylvester_ops():
    code = ("import torch; torch.ops.load_library(%r); "
            "print('HAVE', hasattr(torch.ops.vinf, 'sylvester_fwd'), "
            "hasattr(torch.ops.vinf, 'sylvester_bwd'))" % LIB)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       cwd="/tmp")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "HAVE True True" in r.stdout, r.stdout


# ---------------------------------------------------------------- input helper
@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per_sample"])
@pytest.mark.parametrize("case", GPU_CASES, ids=["%dx%dk%dh%d" % c for c in GPU_CASES])
def test_gpu_inputs_leave_the_tolerances_to_the_kernel(case, per_sample):
    """The fp32 composite on the GPU tests' inputs against the fp64 composite: far inside every
    GPU tolerance (under 1 % of each limit on a CPU), so those limits test the kernel, not the
    conditioning of the inputs."""
    N, D, K, H = case
    ref = oracle(case, per_sample)
    f32 = oracle(case, per_sample, torch.float32)
    assert make_inputs(N, D, K, H, per_sample)[1][0].equal(ref["params"][0])     # seeded
    worst = 0.0
    for name, (atol, rtol) in output_limits(ref, D, K).items():
        r = worst_ratio(f32[name], ref[name], atol, rtol)
        print(f"{name}: err / limit {r:.4f}")
        worst = max(worst, r)
    for name, g in ref["grads"].items():
        r = grad_ratio(f32["grads"][name], g)
        print(f"d{name}: err / limit {r:.4f}")
        worst = max(worst, r)
    assert worst <= 1.0
