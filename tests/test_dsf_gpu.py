"""The fused deep sigmoidal flow kernels (csrc/kernels/dsf.hip) against the fp64 CPU composite on
the same values; for bf16 params the oracle is fed the bf16-rounded values.

Limits (the project's, from test_spline_gpu.py; helpers in test_dsf.py): y atol 2e-4, rtol 1e-4;
a row's ldj atol 2e-4 + 2e-6 D, rtol 1e-4; gradients |delta| <= 2e-3 (1 + max|ref|), plus
2^-8 |ref| per element of a bf16 dparams for its output rounding. The map is smooth: no element
is left out anywhere. In the inverse direction an fp32 root is only determined to ulp(y) / y',
so the recovered x is checked through the fp64 forward map and ldj against -L at that same x;
the gradients are compared with the fp64 composite's re-attached inverse. test_dsf.py asserts
without a GPU that the fp32 composite sits within a quarter of each limit on these inputs."""
import pytest
import torch

from test_dsf import (GPU_CASES, LDJ_RTOL, Y_ATOL, Y_RTOL, _randomise_last_layers, check_grads,
                      check_outputs, envelope, ldj_atol, make_inputs, make_robust_inputs, oracle)
from vi_normflows_amd.ops import dsf as ds
from vi_normflows_amd.ops import reference
from vi_normflows_amd.ops.reference import dsf_units

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = [f"{b}x{d}h{h}" for b, d, h in GPU_CASES]


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", GPU_CASES, ids=IDS)
def test_dsf_kernel_matches_fp64(gpu, case, dtype, inverse):
    o = oracle(case, dtype, inverse)
    out, ldj = ds.dsf_fwd(o["params"].to(gpu), o["x"].to(gpu), o["H"], inverse)
    assert out.dtype == torch.float32 and out.shape == o["x"].shape and ldj.shape == (o["B"],)
    check_outputs(out, ldj, o, inverse)


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", GPU_CASES, ids=IDS)
def test_dsf_transform_gradients_match_fp64(gpu, case, dtype, inverse):
    o = oracle(case, dtype, inverse)
    p = o["params"].to(gpu).requires_grad_(True)
    x = o["x"].to(gpu).requires_grad_(True)
    out, ldj = ds.dsf_transform(p, x, o["H"], inverse)
    ((out * o["g_out"].to(gpu)).sum() + (ldj * o["g_ldj"].to(gpu)).sum()).backward()
    assert p.grad.dtype == dtype and p.grad.shape == p.shape and x.grad.dtype == torch.float32
    check_grads(p.grad, x.grad, o)


REPEAT_CASES = [(257, 130, 8), (33, 7, 16), (10, 24, 32), (64, 392, 8)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", REPEAT_CASES, ids=[f"{b}x{d}h{h}" for b, d, h in REPEAT_CASES])
def test_two_launches_are_bitwise_equal(gpu, case, dtype):
    for inverse in (False, True):
        o = oracle(case, dtype, inverse)
        p, x = o["params"].to(gpu), o["x"].to(gpu)
        go, gl = o["g_out"].to(gpu), o["g_ldj"].to(gpu)
        a = ds.dsf_fwd(p, x, o["H"], inverse)
        b = ds.dsf_fwd(p, x, o["H"], inverse)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        xs = a[0] if inverse else x          # the backward takes the x-side value
        c = ds.dsf_bwd(p, xs, go, gl, o["H"], inverse)
        d = ds.dsf_bwd(p, xs, go, gl, o["H"], inverse)
        assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1])


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
def test_init_false_accumulates(gpu, inverse):
    o = oracle((9, 65, 9), torch.float32, inverse)
    p, x = o["params"].to(gpu), o["x"].to(gpu)
    _, fresh = ds.dsf_fwd(p, x, o["H"], inverse)
    pre = torch.linspace(-3.0, 5.0, o["B"], device=gpu)
    acc = pre.clone()
    _, out = ds.dsf_fwd(p, x, o["H"], inverse, ldj=acc)
    assert out is acc
    assert torch.equal(acc, pre + fresh)   # one fp32 add of the same row sum


ZERO_CASES = [(5, 3, 4), (9, 65, 9), (10, 24, 32), (64, 392, 8)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", ZERO_CASES, ids=[f"{b}x{d}h{h}" for b, d, h in ZERO_CASES])
def test_zero_params_is_identity_on_gpu(gpu, case, dtype):
    """The limits of the fp32 composite's identity test (test_dsf.py) and of the spline's: with
    zero params the kernel's y is x up to one rounding of logsigmoid(-|x|) - |x| and a row's
    ldj is a sum of such roundings."""
    B, D, H = case
    x = make_inputs(B, D, H)[1].to(gpu)
    p = torch.zeros(B, 3 * H * D, device=gpu, dtype=dtype)
    for inverse in (False, True):
        y, ldj = ds.dsf_fwd(p, x, H, inverse)
        print(f"inverse={inverse}: max |y - x| {float((y - x).abs().max()):.3e}, "
              f"max |ldj| {float(ldj.abs().max()):.3e}")
        assert (y - x).abs().max() <= 1e-6
        assert ldj.abs().max() <= 1e-5


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_robust_to_large_inputs_and_parameters_on_gpu(gpu, dtype):
    """The robustness inputs of test_dsf.py (|x| up to 1e4, raw parameters of scale 4):
    everything finite, y inside [min p_h, max p_h] and the inverse's x inside its bracket, both
    up to the fp32 rounding of their ends."""
    p32, x, H = make_robust_inputs()
    pin = p32.to(dtype)
    p = pin.to(gpu).requires_grad_(True)
    xg = x.to(gpu).requires_grad_(True)
    y, ldj = ds.dsf_transform(p, xg, H)
    (y.sum() + ldj.sum()).backward()
    for t in (y, ldj, p.grad, xg.grad):
        assert torch.isfinite(t).all()
    lo, hi = envelope(pin.double(), x.double(), H)
    slack = 1e-6 * torch.maximum(lo.abs(), hi.abs()) + 1e-6
    yc = y.detach().double().cpu()
    assert (yc >= lo - slack).all() and (yc <= hi + slack).all()
    xr, ldj_inv = ds.dsf_fwd(pin.to(gpu), x.to(gpu), H, inverse=True)
    assert torch.isfinite(xr).all() and torch.isfinite(ldj_inv).all()
    a, b, _ = dsf_units(pin.double(), H)
    r = (x.double().unsqueeze(1) - b) / a
    lo, hi = r.amin(1), r.amax(1)
    slack = 1e-5 * torch.maximum(lo.abs(), hi.abs()) + 1e-6
    xc = xr.double().cpu()
    assert (xc >= lo - slack).all() and (xc <= hi + slack).all()


def _close(got, ref, atol, rtol, what):
    err = (got.double().cpu() - ref).abs()
    lim = atol + rtol * ref.abs()
    print(f"{what}: max err {float(err.max()):.3e}, worst err/limit {float((err / lim).max()):.3f}")
    assert (err <= lim).all(), what


def _copies(make, std, seed, gpu, prepare=None):
    torch.manual_seed(0)
    mod = make()
    _randomise_last_layers(mod, std, seed=seed)
    if prepare is not None:
        with torch.no_grad():
            prepare(mod)
    ref = make().double()
    ref.load_state_dict(mod.state_dict())
    dev = make().to(gpu)
    dev.load_state_dict(mod.state_dict())
    return ref, dev


def _run_both(ref, dev, name, x, gy, gl, gpu):
    ref.zero_grad()
    dev.zero_grad()
    yr, lr = getattr(ref, name)(x.double())
    ((yr * gy.double()).sum() + (lr * gl.double()).sum()).backward()
    yd, ld = getattr(dev, name)(x.to(gpu))
    ((yd * gy.to(gpu)).sum() + (ld * gl.to(gpu)).sum()).backward()
    assert (yr - x.double()).abs().max() > 1e-2
    return yr.detach(), lr.detach(), yd, ld


def _check_param_grads(ref, dev, name, tol):
    for (n, pr), pd in zip(ref.named_parameters(), dev.parameters()):
        err = (pd.grad.double().cpu() - pr.grad).abs().max()
        lim = tol * (1 + float(pr.grad.abs().max()))
        print(f"{name} grad {n}: max err {float(err):.3e}, limit {lim:.3e}")
        assert err <= lim, n


def test_dsf_coupling_module_matches_fp64_cpu(gpu):
    """Outputs of forward / inverse and the parameter gradients of a scalar loss against the
    fp64 CPU module with the same weights. The conditioner runs on MfmaLinear in its default
    fp32 precision (<= 1e-5 against fp64, test_module_mfma_gpu.py), so fp32 params reach the
    kernels. The inverse's x is checked through the fp64 module's forward, its ldj against
    minus the fp64 ldj at that same x."""
    from vi_normflows_amd.flows import DSFCoupling

    ref, dev = _copies(lambda: DSFCoupling(dim=10, units=5, hidden=32), 0.3, 11, gpu)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(37, 10, generator=g) * 1.5
    gy, gl = torch.randn(37, 10, generator=g), torch.randn(37, generator=g)
    for name in ("forward", "inverse"):
        yr, lr, yd, ld = _run_both(ref, dev, name, x, gy, gl, gpu)
        if name == "forward":
            _close(yd, yr, Y_ATOL, Y_RTOL, "forward y")
            _close(ld, lr, ldj_atol(5), LDJ_RTOL, "forward ldj")
        else:
            with torch.no_grad():
                y_back, l_back = ref(yd.detach().double().cpu())
            _close(y_back, x.double(), Y_ATOL, Y_RTOL, "f64(inverse(y)) vs y")
            _close(ld, -l_back, ldj_atol(5), LDJ_RTOL, "inverse ldj vs -L(x)")
        _check_param_grads(ref, dev, name, 2e-3)


def test_dsf_autoregressive_module_matches_fp64_cpu_fp32_params(gpu):
    """A shape the fused MADE does not take (dim 10, 37 rows): the masked layers run as fp32
    linears and fp32 params reach the kernels. Forward outputs, parameter gradients and the
    sequential inverse's round trip against the fp64 CPU module with the same weights."""
    from vi_normflows_amd.flows import DSFAutoregressive
    from vi_normflows_amd.ops import made_fused

    ref, dev = _copies(lambda: DSFAutoregressive(dim=10, units=5, hidden=24), 0.3, 13, gpu)
    g = torch.Generator().manual_seed(14)
    x = torch.randn(37, 10, generator=g) * 1.5
    gy, gl = torch.randn(37, 10, generator=g), torch.randn(37, generator=g)
    assert not made_fused.supported(dev.made, x.to(gpu), None)
    yr, lr, yd, ld = _run_both(ref, dev, "forward", x, gy, gl, gpu)
    _close(yd, yr, Y_ATOL, Y_RTOL, "forward y")
    _close(ld, lr, ldj_atol(10), LDJ_RTOL, "forward ldj")
    _check_param_grads(ref, dev, "forward", 2e-3)
    # the sequential inverse of the GPU module, checked through the fp64 module's forward
    xd, ld_inv = dev.inverse(yd.detach())
    assert not xd.requires_grad
    with torch.no_grad():
        y_back, l_back = ref(xd.double().cpu())
    _close(y_back, yd.detach().double().cpu(), Y_ATOL, Y_RTOL, "f64(inverse(y)) vs y")
    _close(ld_inv, -l_back, ldj_atol(10), LDJ_RTOL, "inverse ldj vs -L(x)")


def test_dsf_autoregressive_module_matches_fp64_cpu_bf16_params(gpu):
    """A shape the fused MADE takes (64 rows, dim 32, hidden 64, 4 units): its bf16 output goes
    straight into the kernels and their bf16 dparams straight into the masked GEMMs.

    Against the fp64 CPU module the conditioner's own bf16 arithmetic has to be allowed for. A
    bf16 rounding is 2^-9 relative, and a path from x to an output o_k of the one-hidden-layer
    MADE crosses five of them (x, W1, the stored hidden activation, W2, the stored output; the
    biases are rounded too), accumulated in fp32, so to first order
    |delta o_k| <= 5 * 2^-9 * S_k with S = |W2 M2| (|W1 M1| |x| + |b1|) + |b2|. The transformer
    is element-wise, so the fp64 composite's own derivatives carry that to the outputs:
    y[r, d] gets sum_k |dy[r, d] / do[r, k, d]| |delta o[r, k, d]| and a row's ldj the sum over k
    and d, each on top of the kernel's usual limit. The parameter gradients are sums of
    products of such values, with the bf16 dparams and the stored activations as GEMM operands
    (eight roundings along a path): 8 * 2^-9 = 2^-6 in the project's gradient form
    |delta| <= tol (1 + max|ref|). A first-order bound needs every ReLU to fall the same way in
    bf16 and fp64 (one that flips adds or drops a whole sample's term of a weight gradient), so
    the hidden layer's bias is set to 4: every pre-activation is above 1 (asserted)."""
    from vi_normflows_amd.flows import DSFAutoregressive
    from vi_normflows_amd.ops import made_fused

    H, D = 4, 32
    ref, dev = _copies(lambda: DSFAutoregressive(dim=D, units=H, hidden=64), 0.05, 15, gpu,
                       prepare=lambda m: m.made.layers[0].bias.fill_(4.0))
    g = torch.Generator().manual_seed(16)
    x = torch.randn(64, D, generator=g) * 1.5
    gy, gl = torch.randn(64, D, generator=g), torch.randn(64, generator=g)
    assert made_fused.supported(dev.made, x.to(gpu), None)
    yr, lr, yd, ld = _run_both(ref, dev, "forward", x, gy, gl, gpu)
    with torch.no_grad():
        l1, l2 = ref.made.layers
        assert (x.double() @ (l1.weight * l1.mask).T + l1.bias).min() > 1.0
        S = ((x.double().abs() @ (l1.weight * l1.mask).abs().T + l1.bias.abs())
             @ (l2.weight * l2.mask).abs().T + l2.bias.abs())
        do = (5 * 2.0 ** -9 * S).view(64, 3 * H, D)
    o64 = ref.made(x.double()).detach().requires_grad_(True)
    y2, l2_ = reference.dsf_transform(o64.reshape(64, -1), x.double(), H)
    (dy_do,) = torch.autograd.grad(y2.sum(), o64, retain_graph=True)
    (dl_do,) = torch.autograd.grad(l2_.sum(), o64)
    extra_y = (dy_do.abs() * do).sum(1)
    extra_l = (dl_do.abs() * do).sum((1, 2))
    for what, got, want, lim in (
            ("forward y", yd, yr, Y_ATOL + Y_RTOL * yr.abs() + extra_y),
            ("forward ldj", ld, lr, ldj_atol(D) + LDJ_RTOL * lr.abs() + extra_l)):
        err = (got.detach().double().cpu() - want).abs()
        print(f"{what}: max err {float(err.max()):.3e}, worst err/limit "
              f"{float((err / lim).max()):.3f}, largest limit {float(lim.max()):.3e}")
        assert (err <= lim).all(), what
    _check_param_grads(ref, dev, "forward", 2.0 ** -6)


def test_bindings_reject_bad_arguments(gpu):
    """Host-side checks; nothing is launched."""
    ops = torch.ops.vinf
    B, D, H = 4, 6, 4
    x = torch.zeros(B, D, device=gpu)
    y, ldj = torch.empty_like(x), torch.empty(B, device=gpu)

    def params(h, d=D, b=B):
        return torch.zeros(b, 3 * h * d, device=gpu)

    with pytest.raises(RuntimeError, match="1 <= H <= 32"):
        ops.dsf_fwd(params(1), x, 0, False, True, y, ldj)
    with pytest.raises(RuntimeError, match="1 <= H <= 32"):
        ops.dsf_fwd(params(33), x, 33, False, True, y, ldj)
    with pytest.raises(RuntimeError, match="columns"):
        ops.dsf_fwd(params(H, D + 1), x, H, False, True, y, ldj)
    with pytest.raises(RuntimeError, match="rows"):
        ops.dsf_fwd(params(H, D, B + 1), x, H, False, True, y, ldj)
    with pytest.raises(RuntimeError, match="ldj"):
        ops.dsf_fwd(params(H), x, H, False, True, y, torch.empty(B + 1, device=gpu))
    xt = torch.zeros(D, B, device=gpu).t()
    assert not xt.is_contiguous()
    with pytest.raises(RuntimeError, match="x must be a contiguous"):
        ops.dsf_fwd(params(H), xt, H, False, True, y, ldj)
    g = torch.zeros(B, D, device=gpu)
    with pytest.raises(RuntimeError, match="x must be a contiguous"):
        ops.dsf_bwd(params(H), xt, g, ldj, H, False, params(H), torch.empty_like(x))
    with pytest.raises(RuntimeError, match="1 <= H <= 32"):
        ops.dsf_bwd(params(33), x, g, ldj, 33, False, params(33), torch.empty_like(x))
    with pytest.raises(RuntimeError, match="dparams"):
        ops.dsf_bwd(params(H), x, g, ldj, H, False, params(H).bfloat16(), torch.empty_like(x))
    with pytest.raises(RuntimeError, match="g_ldj"):
        ops.dsf_bwd(params(H), x, g, torch.empty(B + 1, device=gpu), H, False, params(H),
                    torch.empty_like(x))
    with pytest.raises(RuntimeError, match="params must be a contiguous fp32 or bf16"):
        ops.dsf_fwd(params(H).half(), x, H, False, True, y, ldj)
