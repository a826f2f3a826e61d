"""In-kernel Gaussian noise against a bit-exact, element-addressable reference (MI355X only).

vinf::reparam_sample, vinf::normal_fill (csrc/kernels/sampling.hip) and the Philox branch of
vinf::vae_step (csrc/kernels/vae.hip) are compared element by element with tests/philox_ref.py:
Philox4x32-10 in exact integer arithmetic (pinned to the published known-answer vectors by
tests/test_philox_ref.py) and Box-Muller in float64, laid out by the documented counter layouts.

Tolerance of one normal draw. F = max |box_muller32 - box_muller64| over the very uniforms of a
case, from the reference alone, is what evaluating the formula in float32 costs; the kernels
use the hardware log / sin / cos paths (a few float32 ulp, not correctly rounded), so a draw
may be 16 F away, and 16 F <= 1e-4 keeps a broken helper from inflating the bound. A wrong
counter word, key, lane or offset moves a draw by O(1).
"""
import math

import numpy as np
import pytest
import torch

import philox_ref as pr

pytestmark = pytest.mark.gpu

SEEDS = [7, (3 << 32) | 5]
OFFSETS = [0, 5, (1 << 32) + 2]
STREAMS = [0, 1, 5]


def _draw_tol(layout_fn, *args):
    F = pr.rounding_floor(layout_fn, *args)
    tol = 16.0 * F
    assert 0.0 < tol <= 1e-4, tol
    return tol


def _check_draws(got, want, tol, what):
    """|got - want| <= tol per element; prints the observed maximum before asserting."""
    got = got.detach().cpu().double().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    print(f"[noise] {what}: max |gpu - ref64| = {err.max():.3e} (bound 16 F = {tol:.3e})")
    assert err.max() <= tol, (what, float(err.max()), tol, np.unravel_index(err.argmax(), err.shape))


def _mu_lv(D, gpu):
    return torch.linspace(-1, 1, D, device=gpu), torch.linspace(-1, 0.5, D, device=gpu)


def _reparam(gpu, B, D, seed, offset, stream, mu=None, lv=None, zdtype=torch.bfloat16, nbf=0,
             zb_width=None, device_offset=False, z=None, with_zbf=True):
    """One vinf::reparam_sample call; outputs start from sentinels so an unwritten element shows."""
    z = torch.full((B, D), float("nan"), device=gpu) if z is None else z
    eps = torch.full((B, D), float("nan"), device=gpu)
    lq = torch.full((B,), float("nan"), device=gpu)
    zb = None
    if with_zbf:
        zb = torch.full((B, nbf + 3 if zb_width is None else zb_width), 7.0, device=gpu, dtype=zdtype)
    off_t = torch.tensor(offset, dtype=torch.int64, device=gpu) if device_offset else None
    torch.ops.vinf.reparam_sample(mu, lv, seed, off_t, 0 if device_offset else offset, stream, z,
                                  eps, zb, nbf, lq)
    torch.cuda.synchronize()
    return dict(z=z, eps=eps, lq=lq, zb=zb)


def _check_reparam(out, B, D, seed, offset, stream, mu, lv, nbf, what):
    """Every output of reparam_sample against float64: eps within 16 F of the reference draw, z
    and logq0 from the REFERENCE eps (atol 1e-5 + rtol 1e-5, and rtol 1e-5 + atol 1e-3: the
    bounds test_reparam_sample_statistics_and_logq0 uses), the compute copy exactly."""
    eps_ref = pr.reparam_eps(B, D, seed, offset, stream)
    _check_draws(out["eps"], eps_ref, _draw_tol(pr.reparam_eps, B, D, seed, offset, stream), what)
    mu64 = np.zeros(D) if mu is None else mu.cpu().double().numpy()
    lv64 = np.zeros(D) if lv is None else lv.cpu().double().numpy()
    z_ref = mu64 + np.exp(0.5 * lv64) * eps_ref
    z = out["z"].cpu().double().numpy()
    assert np.allclose(z, z_ref, rtol=1e-5, atol=1e-5), (what, np.abs(z - z_ref).max())
    lq_ref = -0.5 * D * math.log(2 * math.pi) - 0.5 * lv64.sum() - 0.5 * (eps_ref * eps_ref).sum(1)
    lq = out["lq"].cpu().double().numpy()
    assert np.allclose(lq, lq_ref, rtol=1e-5, atol=1e-3), (what, np.abs(lq - lq_ref).max())
    zb = out["zb"]
    if zb is not None:
        assert torch.equal(zb[:, :nbf], out["z"][:, :nbf].to(zb.dtype)), what
        assert (zb[:, nbf:] == 0).all(), what


@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("seed", SEEDS)
# (5, 260): B not a multiple of the 4 rows per block, 65 float4 groups (lane 0 loops twice);
# (3, 7) and (2, 1): D % 4 != 0, the scalar path with a partial last group
@pytest.mark.parametrize("B,D", [(5, 260), (3, 7), (2, 1)])
def test_reparam_sample_matches_reference(gpu, B, D, seed, offset, stream):
    """Every output at every (seed, offset, stream) word, the offset passed by value and read
    from device memory (bitwise the same).

    Observed on the MI355X: max |eps - ref64| = 1.30e-6 over these 54 cases, whose bounds 16 F
    run from 2.2e-7 (the two draws of (2, 1) at seed 7, offset 0) to 2.5e-5; the case closest
    to its bound, that (2, 1) one, is at 1.14e-7 of 2.25e-7."""
    mu, lv = _mu_lv(D, gpu)
    nbf = min(5, D)
    host = _reparam(gpu, B, D, seed, offset, stream, mu, lv, nbf=nbf)
    _check_reparam(host, B, D, seed, offset, stream, mu, lv, nbf,
                   f"reparam B={B} D={D} seed={seed:#x} off={offset:#x} stream={stream}")
    dev = _reparam(gpu, B, D, seed, offset, stream, mu, lv, nbf=nbf, device_offset=True)
    for k in ("z", "eps", "lq", "zb"):
        assert torch.equal(host[k], dev[k]), k


@pytest.mark.parametrize("use_mu,use_lv", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("B,D", [(5, 260), (3, 7)])
def test_reparam_sample_optional_mu_logvar(gpu, B, D, use_mu, use_lv):
    mu, lv = _mu_lv(D, gpu)
    mu, lv = (mu if use_mu else None), (lv if use_lv else None)
    seed, offset, stream = SEEDS[1], OFFSETS[2], 1
    out = _reparam(gpu, B, D, seed, offset, stream, mu, lv, with_zbf=False)
    _check_reparam(out, B, D, seed, offset, stream, mu, lv, 0, f"reparam mu={use_mu} lv={use_lv} D={D}")
    if not use_mu and not use_lv:
        assert torch.equal(out["z"], out["eps"])


@pytest.mark.parametrize("zdtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B,D,nbf", [(5, 260, 0), (5, 260, 5), (5, 260, 260), (3, 7, 0), (3, 7, 5),
                                     (3, 7, 7)])
def test_reparam_sample_compute_copy(gpu, B, D, nbf, zdtype):
    """zbf (bf16 and the fp32 instantiation) is z rounded once, nbf columns wide, zero beyond,
    for a copy wider than nbf (and than D) and one exactly nbf wide."""
    mu, lv = _mu_lv(D, gpu)
    seed, offset, stream = SEEDS[0], OFFSETS[1], 0
    what = f"reparam zbf {zdtype} D={D} nbf={nbf}"
    for width in (nbf + 3, max(nbf, 1)):
        out = _reparam(gpu, B, D, seed, offset, stream, mu, lv, zdtype=zdtype, nbf=nbf, zb_width=width)
        assert out["zb"].shape == (B, width)
        _check_reparam(out, B, D, seed, offset, stream, mu, lv, nbf, what)


def test_reparam_sample_unaligned_rows_take_scalar_path(gpu):
    """z as a column view of a (4, 11) buffer: the row stride is no multiple of 4, so the float4
    path is off at an aligned D = 8. Same reference, bitwise the contiguous (float4) result,
    and the buffer's other columns are untouched."""
    B, D = 4, 8
    mu, lv = _mu_lv(D, gpu)
    seed, offset, stream = SEEDS[1], OFFSETS[2], 5
    buf = torch.full((B, 11), 3.0, device=gpu)
    view = _reparam(gpu, B, D, seed, offset, stream, mu, lv, nbf=5, z=buf[:, :D])
    _check_reparam(view, B, D, seed, offset, stream, mu, lv, 5, "reparam ldz=11")
    assert (buf[:, D:] == 3.0).all()
    cont = _reparam(gpu, B, D, seed, offset, stream, mu, lv, nbf=5)
    _check_reparam(cont, B, D, seed, offset, stream, mu, lv, 5, "reparam ldz=8")
    for k in ("z", "eps", "lq", "zb"):
        assert torch.equal(view[k], cont[k]), k


def _fill(gpu, n, seed, offset, stream, device_offset=False):
    out = torch.full((n,), float("nan"), device=gpu)
    off_t = torch.tensor(offset, dtype=torch.int64, device=gpu) if device_offset else None
    torch.ops.vinf.normal_fill(out, seed, off_t, 0 if device_offset else offset, stream)
    torch.cuda.synchronize()
    return out


# 4_500_001: 1 125 001 groups > 4096 blocks x 256 threads, the smallest size whose tail enters
# the grid-stride second pass
@pytest.mark.parametrize("n,seed,offset,stream", [
    (1, 7, 3, 0), (6, 7, 3, 0), (1027, 7, 3, 0), (4_500_001, 7, 3, 0),
    (1027, (3 << 32) | 5, 3, 0),            # 64-bit seed
    (1027, 7, (1 << 32) + 2, 0),            # high-word offset
    (1027, 7, 3, 5),                        # non-zero stream
    (1027, (3 << 32) | 5, (1 << 32) + 2, 1),
])
def test_normal_fill_matches_reference(gpu, n, seed, offset, stream):
    """The whole array, the offset by value and from device memory.

    Observed on the MI355X: max |out - ref64| = 1.77e-6 at n = 4 500 001 (16 F = 2.7e-5), at
    most 1.1e-6 at n = 1027 (16 F >= 1.3e-5), 6.5e-8 at n = 1 (16 F = 8.6e-7)."""
    want = pr.normal_fill_ref(n, seed, offset, stream)
    host = _fill(gpu, n, seed, offset, stream)
    _check_draws(host, want, _draw_tol(pr.normal_fill_ref, n, seed, offset, stream),
                 f"normal_fill n={n} seed={seed:#x} off={offset:#x} stream={stream}")
    assert torch.equal(host, _fill(gpu, n, seed, offset, stream, device_offset=True))


def test_graph_replay_draws_fresh_reference_noise(gpu):
    """offset.add_(1); normal_fill; reparam_sample captured as one chain: every replay reads the
    bumped offset from device memory, so replays 1, 2, 3 give the reference at offsets 1, 2, 3."""
    n, B, D, seed, stream = 1027, 5, 260, SEEDS[1], 1
    mu, lv = _mu_lv(D, gpu)
    off = torch.zeros((), dtype=torch.int64, device=gpu)
    out = torch.empty(n, device=gpu)
    z, eps, lq = torch.empty(B, D, device=gpu), torch.empty(B, D, device=gpu), torch.empty(B, device=gpu)

    def step():
        off.add_(1)
        torch.ops.vinf.normal_fill(out, seed, off, 0, stream)
        torch.ops.vinf.reparam_sample(mu, lv, seed, off, 0, stream, z, eps, None, 0, lq)

    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream(gpu).wait_stream(s)
    torch.cuda.synchronize()
    off.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for k in (1, 2, 3):
        g.replay()
        torch.cuda.synchronize()
        assert off.item() == k
        _check_draws(out, pr.normal_fill_ref(n, seed, k, stream),
                     _draw_tol(pr.normal_fill_ref, n, seed, k, stream), f"graph replay {k} normal_fill")
        _check_reparam(dict(z=z, eps=eps, lq=lq, zb=None), B, D, seed, k, stream, mu, lv, 0,
                       f"graph replay {k} reparam")


# ---------------------------------------------------------------- VAE step, Philox branch
def _vae_engine(gpu, B, dz, K, scale=4.0):
    from vi_normflows_amd.models.vae import VAEConfig, synthetic_binary_images
    from vi_normflows_amd.models.vae_engine import PlanarVAEEngine

    cfg = VAEConfig(dim_x=784, dim_z=dz, K=K, width=64, hidden_layers=3)
    assert PlanarVAEEngine.supported(cfg)
    eng = PlanarVAEEngine(cfg, batch=B, device=gpu, seed=1)
    with torch.no_grad():   # as test_vae_step_matches_autograd: larger weights than the init
        eng.params.master.mul_(scale)
    eng.set_batch(synthetic_binary_images(B, 784, seed=1).to(gpu))
    eng.beta.fill_(0.7)
    eng.zk_out = torch.zeros(B, dz, device=gpu)
    eng.ldj_out = torch.zeros(B, device=gpu)
    return eng


def _vae_run(eng):
    eng.forward_backward()
    torch.cuda.synchronize()
    return dict(loss=eng.loss.clone(), frow=eng.frow.clone(), zk=eng.zk_out.clone(),
                ldj=eng.ldj_out.clone(), grad=eng.params.grad.clone())


def _vae_philox_vs_injected(gpu, B, dz, K, seed, offset, scale=4.0):
    """The same kernel twice: in-kernel Philox noise, then the reference noise injected."""
    eng = _vae_engine(gpu, B, dz, K, scale)
    eng.seed = seed
    eng.rng_offset.fill_(offset)
    eng.eps_override = None
    got = _vae_run(eng)
    eps = pr.vae_eps(B, dz, seed, offset)
    _draw_tol(pr.vae_eps, B, dz, seed, offset)
    eng.eps_override = torch.from_numpy(eps).to(torch.float32).to(gpu)
    ref = _vae_run(eng)
    assert eng.rng_offset.item() == offset
    assert torch.isfinite(got["grad"]).all() and torch.isfinite(ref["grad"]).all()
    err = abs(got["loss"].item() - ref["loss"].item())
    print(f"[noise] vae B={B} dz={dz} seed={seed:#x} off={offset:#x} weights x {scale}: loss err "
          f"{err:.3e} (|ref| {abs(ref['loss'].item()):.3e})")
    assert err <= 1e-4 * abs(ref["loss"].item()) + 1e-4, err
    for k in ("frow", "zk", "ldj"):
        err = (got[k] - ref[k]).abs().max().item()
        print(f"[noise]   {k} max err {err:.3e} (max |ref| {ref[k].abs().max().item():.3e})")
        assert err <= 1e-4 * ref[k].abs().max().item() + 1e-4, (k, err)
    for name in eng.layout.order:
        a, r = eng.layout.view(got["grad"], name), eng.layout.view(ref["grad"], name)
        err = (a - r).abs().max().item()
        assert err <= 2e-4 * r.abs().max().item() + 1e-6, (name, err, r.abs().max().item())
    return got


def _rank_seeds():
    from vi_normflows_amd.utils.config import rank_seed

    return rank_seed(0, 0), rank_seed(0, 1)


# B = 100 is not a multiple of the rows per block (the global row index matters); (37, 12, 2):
# a second width; ((5 << 32) | 9): vae_step keeps the low seed word only. Weights x 4 as in
# test_vae_step_matches_autograd make |z_K| ~ 1e3, so its relative bound is loose on most
# elements; at the plain 0.05 init z_K is O(1) and the same bound binds every element.
@pytest.mark.parametrize("B,dz,K,seed,offset,scale", [
    (100, 40, 4, "rank0", (1 << 32) + 3, 4.0),
    (100, 40, 4, "rank1", (1 << 32) + 3, 4.0),
    (100, 40, 4, "rank1", 2, 4.0),
    (100, 40, 4, "rank1", (1 << 32) + 3, 1.0),
    (37, 12, 2, "rank0", 0, 4.0),
    (37, 12, 2, (5 << 32) | 9, (1 << 32) + 3, 1.0),
])
def test_vae_step_philox_matches_injected_reference_noise(gpu, B, dz, K, seed, offset, scale):
    """forward_backward() with in-kernel noise == forward_backward() fed vae_eps(...): loss,
    per-row free energies, z_K, log-det and every named gradient, within the bounds of
    test_vae_step_matches_autograd (both runs are the same kernel, only the noise differs).

    Observed on the MI355X, weights x 4: z_K within 1.3e-3 at |z_K| up to 2.9e3 (bound 0.29),
    log-det within 7.6e-5, loss within 1.6e-2 at 1e5; weights x 1: z_K within 1.2e-6 at
    |z_K| up to 3.6 (bound 4.6e-4), log-det within 2.4e-7, frow within 6.1e-5 at 367, loss equal."""
    r0, r1 = _rank_seeds()
    seed = {"rank0": r0, "rank1": r1}.get(seed, seed)
    _vae_philox_vs_injected(gpu, B, dz, K, seed, offset, scale)


def test_vae_step_rank_seeds_draw_different_noise(gpu):
    r0, r1 = _rank_seeds()
    assert r0 != r1
    B, dz, K, offset = 100, 40, 4, (1 << 32) + 3
    zk = []
    for seed in (r0, r1):
        eng = _vae_engine(gpu, B, dz, K)
        eng.seed = seed
        eng.rng_offset.fill_(offset)
        zk.append(_vae_run(eng)["zk"])
    assert (zk[0] != zk[1]).all()
    e0, e1 = pr.vae_eps(B, dz, r0, offset), pr.vae_eps(B, dz, r1, offset)
    assert (e0 != e1).all()


def test_vae_step_odd_dz(gpu):
    """An odd dz leaves the last lane pair half used (the even lane's n0 only). The HIP step
    takes multiples of 4 only, so today no odd dz is supported and vinf::vae_step refuses one;
    should the gate ever open, the comparison runs at the first odd dz it accepts."""
    from vi_normflows_amd.models.vae import VAEConfig, synthetic_binary_images
    from vi_normflows_amd.models.vae_engine import PlanarVAEEngine

    odd = [dz for dz in range(1, 65, 2) if PlanarVAEEngine.supported(
        VAEConfig(dim_x=784, dim_z=dz, K=2, width=64, hidden_layers=3))]
    if odd:
        _vae_philox_vs_injected(gpu, 37, odd[0], 2, _rank_seeds()[1], (1 << 32) + 3)
        return
    eng = PlanarVAEEngine(VAEConfig(dim_x=784, dim_z=39, K=2, width=64, hidden_layers=3), batch=16,
                          device=gpu, seed=0)
    eng.set_batch(synthetic_binary_images(16, 784, seed=0).to(gpu))
    with pytest.raises(RuntimeError, match="multiple of 4"):
        eng.forward_backward()
