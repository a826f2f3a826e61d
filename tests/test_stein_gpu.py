"""The all-pairs Stein HIP kernels (csrc/kernels/stein.hip) against the fp64 CPU composite.

The oracle is the composite of ops/reference.py in fp64 on the fp32 inputs. The limit is per
element, against the oracle's own abs-sums

    A_i = (1/N) sum_j (|f_ij s_j| + |2 f'_ij (x_i - x_j)|)                         (phi, elementwise)
    B_i = sum_j (|f s_i.s_j| + |2 f' (s_j - s_i).(x_i - x_j)| + |2 D f'| + |4 f'' r2|)      (rows)

as |got - ref| <= 1e-4 A_i (B_i). 1e-4 is the project's row-kernel rtol. It sits above the
worst-case fp32 bound for these shapes (recursive summation at most N 2^-24 ~ 6.6e-5 at N = 1100,
the exponent's argument error at most 87 2^-24 ~ 5e-6) and below the effect of one dropped or
doubled pair at the wide bandwidth (about A_i / N >= 9e-4 A_i), where every pair carries about
equal weight: that bandwidth is the one that checks the indexing.
"""
import functools

import pytest
import torch

from vi_normflows_amd.distributions.energies import get_target
from vi_normflows_amd.inference.svgd import SVGD, score_fn
from vi_normflows_amd.ops import fused, stein
from vi_normflows_amd.ops._ext import native
from vi_normflows_amd.ops.reference import (ksd_rows_reference, stein_kernel_terms_reference,
                                            svgd_direction_reference)

pytestmark = pytest.mark.gpu

RTOL = 1e-4
KINDS = ("rbf", "imq")
CASES = [(1, 1), (2, 2), (257, 2), (300, 3), (1000, 5), (513, 16), (130, 17), (260, 40), (129, 64),
         (1100, 2), (stein.TILE_I + 1, 2), (2 * stein.TILE_J + 1, 5), (stein.TILE_J - 1, 3)]


@functools.lru_cache(maxsize=None)
def _inputs(N, D):
    """Seeded fp32 CPU inputs of a case and its two bandwidths (median heuristic, 100 x that)."""
    g = torch.Generator().manual_seed(1000 * N + D)
    x = 1.5 * torch.randn(N, D, generator=g)
    s = -x + 0.3 * torch.randn(N, D, generator=g)
    h = float(stein.median_bandwidth(x))
    return x, s, (h, 100.0 * h)


@functools.lru_cache(maxsize=None)
def _oracle(N, D, kind, h):
    """fp64 CPU composite on the fp32 inputs: phi, A, rows, diag, B (shared, never modified)."""
    x, s, _ = _inputs(N, D)
    phi, A = svgd_direction_reference(x.double(), s.double(), h, kind, return_abs=True)
    rows, diag, B = ksd_rows_reference(x.double(), s.double(), h, kind, return_abs=True)
    return phi, A, rows, diag, B


def _diag_scale(s, h, kind, D):
    f, fp, _ = stein_kernel_terms_reference(torch.zeros((), dtype=torch.float64), h, kind)
    return f.abs() * (s.double() ** 2).sum(1) + 2.0 * D * fp.abs()


def _check_case(N, D, kind, h, j_splits=None, tag=""):
    x, s, _ = _inputs(N, D)
    phi, A, rows, diag, B = _oracle(N, D, kind, h)
    xg, sg = x.cuda(), s.cuda()
    got_phi = stein.svgd_direction(xg, sg, h, kind, impl="kernel", j_splits=j_splits)
    got_rows, got_diag = stein.ksd_rows(xg, sg, h, kind, impl="kernel", j_splits=j_splits)
    e_phi = ((got_phi.double().cpu() - phi).abs() / A).max().item()
    e_rows = ((got_rows.double().cpu() - rows).abs() / B).max().item()
    e_diag = ((got_diag.double().cpu() - diag).abs() / _diag_scale(s, h, kind, D)).max().item()
    print(f"N={N} D={D} {kind} h={h:.4g} {tag}: phi {e_phi:.2e} A, rows {e_rows:.2e} B, "
          f"diag {e_diag:.2e}")
    assert got_phi.shape == (N, D) and got_rows.shape == (N,) and got_diag.shape == (N,)
    assert e_phi <= RTOL, (N, D, kind, h, j_splits)
    assert e_rows <= RTOL, (N, D, kind, h, j_splits)
    assert e_diag <= RTOL, (N, D, kind, h, j_splits)
    return got_phi, got_rows, got_diag


@pytest.mark.parametrize("N,D", CASES)
def test_kernels_against_fp64_oracle(gpu, N, D):
    n0 = stein.stein_launches()
    for kind in KINDS:
        for h in _inputs(N, D)[2]:
            _check_case(N, D, kind, h)
    assert stein.stein_launches() == n0 + 8


@pytest.mark.parametrize("N,D", [(300, 3), (1100, 2)])
def test_split_j(gpu, N, D):
    h = _inputs(N, D)[2][1]
    for kind in KINDS:
        for js in (1, 2, 3, 7, None):
            a = _check_case(N, D, kind, h, j_splits=js, tag=f"j_splits={js}")
            b = _check_case(N, D, kind, h, j_splits=js, tag=f"j_splits={js} again")
            assert all(torch.equal(u, v) for u, v in zip(a, b)), (kind, js)


def test_strided_inputs_and_device_bandwidth(gpu):
    N, D = 300, 5
    g = torch.Generator().manual_seed(7)
    wide = (1.5 * torch.randn(N, 2 * D + 3, generator=g)).cuda()
    x, s = wide[:, 1:1 + D], wide[:, D + 2:2 * D + 2]
    assert not x.is_contiguous() and x.stride(1) == 1
    h_dev = stein.median_bandwidth(x)
    assert h_dev.is_cuda and h_dev.shape == (1,)
    h = float(h_dev)
    for kind in KINDS:
        want_phi = stein.svgd_direction(x.contiguous(), s.contiguous(), h, kind, impl="kernel")
        want_rows = stein.ksd_rows(x.contiguous(), s.contiguous(), h, kind, impl="kernel")
        assert torch.equal(stein.svgd_direction(x, s, h, kind, impl="kernel"), want_phi)
        assert torch.equal(stein.svgd_direction(x, s, h_dev, kind, impl="kernel"), want_phi)
        for got in (stein.ksd_rows(x, s, h, kind, impl="kernel"),
                    stein.ksd_rows(x, s, h_dev, kind, impl="kernel")):
            assert torch.equal(got[0], want_rows[0]) and torch.equal(got[1], want_rows[1])


@pytest.mark.parametrize("N,D", [(300, 3), (1000, 5)])
def test_ksd_statistics(gpu, N, D):
    x, s, (h, _) = _inputs(N, D)
    for kind in KINDS:
        _, _, rows, diag, B = _oracle(N, D, kind, h)
        lim = RTOL * B.sum().item() / N ** 2
        want = {"u": (rows.sum() - diag.sum()) / (N * (N - 1)), "v": rows.sum() / N ** 2}
        for stat in ("u", "v"):
            got = stein.ksd(x.cuda(), s.cuda(), h, kind, stat, impl="kernel")
            print(f"N={N} D={D} {kind} {stat}: {got.item():.8f} vs {want[stat].item():.8f}, "
                  f"limit {lim:.2e}")
            assert got.dtype == torch.float64 and abs(got.item() - want[stat].item()) <= lim


def test_one_svgd_step_on_u1(gpu):
    N, eps, h = 257, 0.1, 0.8
    tgt = get_target("U1")
    g = torch.Generator().manual_seed(5)
    x0 = (1.5 * torch.randn(N, 2, generator=g)).cuda()
    n_stein, n_energy = stein.stein_launches(), fused.energy2d_launches()
    sv = SVGD(tgt, x0.clone(), eps, optimizer="sgd", mass=0.0, bandwidth=h)
    sv.step()
    assert stein.stein_launches() > n_stein and fused.energy2d_launches() > n_energy
    x1 = sv.particles
    move = (x1.double() - x0.double()).cpu()
    # oracle: fp64 composite fed fp64 autograd scores of the target's torch definition
    xd = x0.double().cpu()
    s64 = score_fn(tgt)(xd)
    phi, A = svgd_direction_reference(xd, s64, h, "rbf", return_abs=True)
    # the score kernel's own error enters phi weighted by f_ij
    ds = (score_fn(tgt)(x0).double().cpu() - s64).abs()
    f, _, _ = stein_kernel_terms_reference(((xd[:, None] - xd[None]) ** 2).sum(-1),
                                           torch.tensor(h, dtype=torch.float64), "rbf")
    slack = f @ ds / N
    big = torch.maximum(x0.abs(), x1.abs())
    ulp = (torch.nextafter(big, torch.full_like(big, float("inf"))) - big).double().cpu()
    err = (move - eps * phi).abs()
    lim = eps * (RTOL * A + slack) + ulp
    print(f"max |move - eps phi| / limit = {(err / lim).max().item():.3f}, "
          f"max |move| = {move.abs().max().item():.4f}")
    assert move.abs().max() > 1e-3
    assert (err <= lim).all()


def test_binding_errors(gpu):
    ops = native()
    x, s = torch.randn(8, 3, device=gpu), torch.randn(8, 3, device=gpu)
    phi, rows, diag = torch.empty(8, 3, device=gpu), torch.empty(8, device=gpu), torch.empty(8, device=gpu)
    work = torch.empty(ops.stein_workspace(8, 3, 2, 0), device=gpu)
    assert work.numel() == 2 * 8 * 3 and ops.stein_workspace(8, 3, 2, 1) == 2 * 8
    ops.stein_svgd(x, s, None, 1.0, 0, 2, phi, work)
    ops.stein_ksd_rows(x, s, None, 1.0, 1, 2, rows, diag, work)
    with pytest.raises(RuntimeError, match="D <= 64"):
        x65 = torch.randn(4, 65, device=gpu)
        ops.stein_svgd(x65, x65, None, 1.0, 0, 1, torch.empty(4, 65, device=gpu), work)
    with pytest.raises(RuntimeError, match="must be fp32"):
        ops.stein_svgd(x.double(), s, None, 1.0, 0, 2, phi, work)
    with pytest.raises(RuntimeError, match="must be fp32"):
        ops.stein_ksd_rows(x, s.double(), None, 1.0, 1, 2, rows, diag, work)
    with pytest.raises(RuntimeError, match="unit inner stride"):
        ops.stein_svgd(torch.randn(8, 6, device=gpu)[:, ::2], s, None, 1.0, 0, 2, phi, work)
    with pytest.raises(RuntimeError, match="work has"):
        ops.stein_svgd(x, s, None, 1.0, 0, 2, phi, work[:-1])
    with pytest.raises(RuntimeError, match="work has"):
        ops.stein_ksd_rows(x, s, None, 1.0, 1, 2, rows, diag, work[:15])
    with pytest.raises(RuntimeError, match="phi has"):
        ops.stein_svgd(x, s, None, 1.0, 0, 2, phi[:-1], work)
    with pytest.raises(RuntimeError, match="unknown kind 9"):
        ops.stein_svgd(x, s, None, 1.0, 9, 2, phi, work)
    with pytest.raises(RuntimeError, match="must be positive"):
        ops.stein_svgd(x, s, None, 0.0, 0, 2, phi, work)
    with pytest.raises(RuntimeError, match="impl='kernel'"):
        stein.svgd_direction(torch.randn(4, 65, device=gpu), torch.randn(4, 65, device=gpu), 1.0,
                             impl="kernel")


def test_auto_falls_back_beyond_64_dimensions(gpu):
    x, s = torch.randn(33, 65, device=gpu), torch.randn(33, 65, device=gpu)
    n0 = stein.stein_launches()
    assert torch.equal(stein.svgd_direction(x, s, 50.0), svgd_direction_reference(x, s, 50.0))
    rows, diag = stein.ksd_rows(x, s, 50.0)
    want = ksd_rows_reference(x, s, 50.0)
    assert torch.equal(rows, want[0]) and torch.equal(diag, want[1])
    assert stein.stein_launches() == n0
