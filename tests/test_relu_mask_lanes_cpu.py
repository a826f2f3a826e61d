"""The lane-private ReLU mask flags (ops.gemm.linear_fwd mask_lanes / linear_dgrad bits_lanes,
KernelPaths.relu_mask_lanes) off the MFMA path: CPU tensors and the oracle take the flags and
compute exactly what they compute without them (they use ``relu_of``, never the mask)."""
import pytest
import torch

from vi_normflows_amd.ops import gemm
from vi_normflows_amd.utils.config import KernelPaths


def _inputs(M=24, N=16, K=8):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g)
    b = torch.randn(N, generator=g)
    dy = torch.randn(M, N, generator=g)
    return x, W, b, dy


@pytest.mark.parametrize("use_oracle", [False, True])
def test_cpu_wrappers_take_the_flags(use_oracle):
    x, W, b, dy = _inputs()
    M, N = x.shape[0], W.shape[0]

    def run(lanes):
        y = torch.empty(M, N)
        mask = torch.full((M, N // 8), 0x5A, dtype=torch.uint8)
        gemm.linear_fwd(x, W, b, y, relu=True, mask_out=mask, mask_lanes=lanes)
        dx = torch.empty(M, W.shape[1])
        gemm.linear_dgrad(dy * (y > 0), W, dx)
        dh = torch.empty(M, N)
        gemm.linear_dgrad(torch.ones(M, N), torch.eye(N), dh, relu_of=y, relu_bits=mask,
                          bits_lanes=lanes)
        return y, mask, dx, dh

    if use_oracle:
        with gemm.oracle():
            a, b_ = run(True), run(False)
    else:
        a, b_ = run(True), run(False)
    for u, v in zip(a, b_):
        assert torch.equal(u, v)
    y, mask, _, dh = a
    assert torch.equal(y, (x @ W.t() + b).relu())
    assert (mask == 0x5A).all(), "the torch path never writes the mask"
    assert torch.equal(dh, (y > 0).float())


def test_kernel_paths_switch(monkeypatch):
    assert KernelPaths().relu_mask_lanes is True
    monkeypatch.setenv("VINF_KERNEL_PATHS", "relu_mask_lanes=0")
    p = KernelPaths.from_env()
    assert p.relu_mask_lanes is False and p.cpl_fuse is True
    monkeypatch.setenv("VINF_KERNEL_PATHS", "relu_mask_lanes=1,dgrad_nt=0")
    p = KernelPaths.from_env()
    assert p.relu_mask_lanes is True and p.dgrad_nt is False


def test_cpu_engine_ignores_the_switch():
    """A CPU engine has no bitmask at all: the switch changes nothing, step for step."""
    from vi_normflows_amd.models.realnvp import RealNVPConfig, RealNVPVI

    out = []
    for lanes in (True, False):
        paths = KernelPaths()
        paths.relu_mask_lanes = lanes
        cfg = RealNVPConfig(dim=8, n_layers=2, hidden=256, anneal="none", paths=paths)
        eng = RealNVPVI(cfg, batch=256, device="cpu", lr=1e-3, seed=1)
        eng.eps_override = torch.randn(256, 8, generator=torch.Generator().manual_seed(2))
        eng.train_step()
        eng.train_step()
        assert eng.Mk is None and not any(eng.mk_lanes)
        out.append((eng.loss.clone(), eng.params.grad.clone(), eng.params.master.clone()))
    for u, v in zip(*out):
        assert torch.equal(u, v)
