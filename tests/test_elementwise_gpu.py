"""The shared autograd.Function of the element-wise transforms (ops/_elementwise.py) when only
one of its two outputs carries a gradient: a loss on y alone and a loss on ldj alone. Autograd
then hands the backward zeros for the other output (gradients are materialised), which the
backward passes to the kernel as they are. Gradients against the fp64 composite on the inputs
and with the limits of test_spline_gpu.py / test_dsf.py: |delta| <= 2e-3 (1 + max|ref|)."""
import pytest
import torch

import test_dsf
import test_spline_gpu
from vi_normflows_amd.ops import dsf as ds
from vi_normflows_amd.ops import reference
from vi_normflows_amd.ops import spline as sp

pytestmark = pytest.mark.gpu

CASE = (5, 3, 4)
LOSSES = {"y": lambda out, ldj, o: (out * o["g_out"].to(out)).sum(),
          "ldj": lambda out, ldj, o: (ldj * o["g_ldj"].to(ldj)).sum()}


def _grads(transform, o, loss, device, dtype):
    p = o["params"].to(device=device, dtype=dtype).requires_grad_(True)
    x = o["x"].to(device=device, dtype=dtype).requires_grad_(True)
    out, ldj = transform(p, x)
    loss(out, ldj, o).backward()
    return p.grad, x.grad


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("loss", list(LOSSES), ids=list(LOSSES))
def test_rqs_transform_gradients_of_one_output(gpu, loss, inverse):
    o = test_spline_gpu.oracle(CASE, torch.float32, inverse)
    K, bound, keep = o["K"], o["bound"], o["keep"]
    assert keep.any()

    def transform(p, x):
        return sp.rqs_transform(p, x, K, bound, inverse)

    dp64, gx64 = _grads(lambda p, x: reference.rqs_transform(p, x, K, bound, inverse), o,
                        LOSSES[loss], "cpu", torch.float64)
    dp, gx = _grads(transform, o, LOSSES[loss], gpu, torch.float32)
    B, Dh = o["B"], o["Dh"]
    for what, got, ref in (("gx", gx, gx64), ("dparams", dp, dp64)):
        if what == "dparams":   # [B, (3K-1) Dh] -> [B, Dh, 3K-1], so the [B, Dh] mask applies
            got, ref = (t.view(B, 3 * K - 1, Dh).permute(0, 2, 1) for t in (got, ref))
        err, r = (got.double().cpu() - ref).abs()[keep], ref[keep]
        lim = 2e-3 * (1 + float(r.abs().max()))
        print(f"{what}: max err {float(err.max()):.3e}, limit {lim:.3e}")
        assert (err <= lim).all(), what


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("loss", list(LOSSES), ids=list(LOSSES))
def test_dsf_transform_gradients_of_one_output(gpu, loss, inverse):
    o = test_dsf.oracle(CASE, torch.float32, inverse)
    H = o["H"]
    dp64, gx64 = _grads(lambda p, x: reference.dsf_transform(p, x, H, inverse), o, LOSSES[loss],
                        "cpu", torch.float64)
    dp, gx = _grads(lambda p, x: ds.dsf_transform(p, x, H, inverse), o, LOSSES[loss], gpu,
                    torch.float32)
    test_dsf.check_grads(dp, gx, dict(o, dparams=dp64, gx=gx64))
