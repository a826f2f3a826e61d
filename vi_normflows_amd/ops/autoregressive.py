"""Degree sweep: the sequential direction of a MADE-conditioned flow in one masked pass.

MAF sampling (u -> x) and the IAF inverse (y -> z) solve, coordinate by coordinate in degree
order, ``x_i = T(v_i; m_i, s_i)`` with ``[m, s] = MADE(x)``. ``made_degrees`` gives every hidden
layer sorted, non-decreasing degrees, so for the coordinate of degree ``t`` (``i = perm[t - 1]``)

* ``m_i, s_i`` read a prefix ``h_L[:c(t)]`` of the last hidden layer (units of degree < t);
* the hidden units of degree ``t`` are a contiguous range per layer; layer 1 reads the first ``t``
  coordinates in degree order, layer ``l`` a prefix of layer ``l - 1`` (degrees <= t).

Walking ``t = 1 .. D`` is a forward substitution that uses every in-mask weight once per row: one
masked MADE pass instead of ``D`` full ones. Entries outside the masks are never read, so the
weights need not be pre-multiplied by the masks.

fp32 GPU tensors run ``csrc/kernels/made_sweep.hip`` (one launch per flow layer, a tile of rows per
block with its state in LDS; a row's result is bitwise independent of the batch around it).
:func:`made_sweep_composite` is the same sweep in torch: the CPU path and the test oracle. A GPU
call never falls back to it: a missing native library or a shape outside the kernel's LDS budget
raises (callers that have another path ask :func:`supported` first).

The inverse of a MADE-conditioned deep sigmoidal flow layer (``DSFAutoregressive.inverse``) is the
same walk with ``3 units`` outputs per coordinate and the DSF root solve as the transform:
:func:`dsf_sweep` (``csrc/kernels/dsf_sweep.hip``), :func:`dsf_sweep_composite`,
:func:`dsf_sweep_flow`.

The sequential direction of a MADE-conditioned rational-quadratic spline layer
(``RQSAutoregressive``) is the walk with ``3 bins - 1`` outputs per coordinate and the closed-form
spline inverse as the transform: :func:`rqs_sweep` (``csrc/kernels/rqs_sweep.hip``),
:func:`rqs_sweep_composite`, :func:`rqs_sweep_flow`.

Not differentiable: ``MAF.forward`` / ``IAF.inverse`` take this path only when nothing needs a
graph (:func:`dispatch`); ``DSFAutoregressive.inverse`` and the sequential direction of
``RQSAutoregressive`` never build one.
"""
from __future__ import annotations

import torch

from ._ext import native

KINDS = {"maf_sample": 0, "iaf_gated": 1, "iaf_affine": 2}
MAX_HIDDEN = 4   # NF_MADE_SWEEP_MAX_HIDDEN of csrc/include/launchers.h

_sweep_launches = 0
_plans: dict = {}


def sweep_launches(reset: bool = False) -> int:
    """Number of sweep kernel launches so far (evidence that the HIP path ran)."""
    global _sweep_launches
    n = _sweep_launches
    if reset:
        _sweep_launches = 0
    return n


class SweepPlan:
    """Host-side ranges of one (D, H, L, order): ``perm`` [D] (coordinate of degree t is
    ``perm[t - 1]``) and ``ubeg`` [L, D + 2] with ``ubeg[l][t]`` = number of layer-l units of
    degree < t, so the units of degree t are ``ubeg[l][t] : ubeg[l][t + 1]`` and
    ``c(t) = ubeg[L - 1][t]``. Device copies (int32) are made once per device."""

    def __init__(self, dim: int, hidden: int, n_hidden: int, order):
        from ..flows.made import made_degrees

        d_in, hs = made_degrees(dim, hidden, n_hidden, None if order is None else order.cpu())
        if sorted(d_in.tolist()) != list(range(1, dim + 1)):
            raise ValueError("made_sweep: order must be a permutation of 1 .. D")
        self.perm = torch.argsort(d_in).to(torch.int32)
        t = torch.arange(dim + 2)
        self.ubeg = torch.stack([torch.searchsorted(h.contiguous(), t) for h in hs]).to(torch.int32)
        self._dev: dict = {}

    def on(self, device):
        d = self._dev.get(device)
        if d is None:
            d = self._dev[device] = (self.perm.to(device), self.ubeg.to(device).contiguous())
        return d


def plan_for(dim: int, hidden: int, n_hidden: int, order) -> SweepPlan:
    """Cached :class:`SweepPlan` (``order`` None = degrees 1 .. D in place)."""
    key = (dim, hidden, n_hidden, None if order is None else tuple(order.tolist()))
    p = _plans.get(key)
    if p is None:
        if len(_plans) >= 64:
            _plans.clear()
        p = _plans[key] = SweepPlan(dim, hidden, n_hidden, order)
    return p


def _transform(kind, v, m, s, bound, gate_bias, scale):
    """One coordinate: (x, log-det share)."""
    if kind == "maf_sample":
        a = bound * torch.tanh(s / bound)
        return v * torch.exp(a) + m, a
    if kind == "iaf_gated":
        g = torch.sigmoid(s + gate_bias)
        return (v - (1 - g) * m) / g, -torch.nn.functional.logsigmoid(s + gate_bias)
    c = scale * torch.tanh(s)
    return (v - m) * torch.exp(-c), -c


def made_sweep_composite(v, weights, biases, order, kind, *, ctx_bias=None, bound=5.0,
                         gate_bias=1.0, scale=1.0, plan=None):
    """The sweep in torch, in the dtype of ``v`` (weights are cast to it)."""
    B, D = v.shape
    L, H = len(weights) - 1, weights[0].shape[0]
    plan = plan or plan_for(D, H, L, order)
    perm, ubeg = plan.perm.tolist(), plan.ubeg.tolist()
    Ws = [w.detach().to(v.dtype) for w in weights]
    bs = [b.detach().to(v.dtype) for b in biases]
    idx = plan.perm.to(v.device, torch.long)
    x = torch.empty_like(v)
    ldj = v.new_zeros(B)
    h = [v.new_zeros(B, H) for _ in range(L)]
    for t in range(1, D + 1):
        i, c = perm[t - 1], ubeg[L - 1][t]
        m = bs[L][i] + h[L - 1][:, :c] @ Ws[L][i, :c]
        s = bs[L][i + D] + h[L - 1][:, :c] @ Ws[L][i + D, :c]
        x[:, i], share = _transform(kind, v[:, i], m, s, bound, gate_bias, scale)
        ldj = ldj + share
        _hidden_step(x, h, Ws, bs, ubeg, idx, t, ctx_bias)
    return x, ldj


def kernel_supported(D: int, H: int, L: int) -> bool:
    """``made_sweep_supported`` of the native library: the (D, H, L) state of at least one row
    fits the LDS budget the launcher requests."""
    return bool(native().made_sweep_supported(int(D), int(H), int(L)))


def kernel_rows(D: int, H: int, L: int) -> int:
    """Rows per block the launcher picks for (D, H, L); 0 when unsupported."""
    return int(native().made_sweep_rows(int(D), int(H), int(L)))


def made_sweep(v, weights, biases, order, kind, *, ctx_bias=None, bound=5.0, gate_bias=1.0,
               scale=1.0, plan=None):
    """``(x, ldj)`` of the sequential direction of one autoregressive flow layer; no-grad.

    ``weights`` / ``biases``: the MADE's hidden layers then its output layer ([2D, H]: rows i = m,
    i + D = s), fp32 and unmasked. ``order``: input degrees (a permutation of 1 .. D) or None for
    1 .. D in place. ``kind``: ``maf_sample`` (x = v exp(a) + m, a = bound tanh(s / bound),
    ldj = sum a), ``iaf_gated`` (inverse of y = g z + (1 - g) m, g = sigmoid(s + gate_bias),
    ldj = -sum log g) or ``iaf_affine`` (inverse of y = z exp(c) + m, c = scale tanh(s),
    ldj = -sum c). ``ctx_bias`` [B, H] is added to the first hidden layer's pre-activation.
    ``plan``: the :class:`SweepPlan` of (D, H, L, order) when the caller keeps one.
    GPU tensors run the HIP kernel (fp32 only, raising outside its limits), CPU tensors the
    composite."""
    if kind not in KINDS:
        raise ValueError(f"made_sweep: kind must be one of {sorted(KINDS)}, got {kind!r}")
    _check_sweep_inputs("made_sweep", v, weights, biases, ctx_bias)
    if not v.is_cuda:
        return made_sweep_composite(v, weights, biases, order, kind, ctx_bias=ctx_bias,
                                    bound=bound, gate_bias=gate_bias, scale=scale, plan=plan)
    global _sweep_launches
    ops = native()
    B, D = v.shape
    L, H = len(weights) - 1, weights[0].shape[0]
    if v.dtype != torch.float32 or any(t.dtype != torch.float32 for t in (*weights, *biases)):
        raise RuntimeError("made_sweep: the HIP kernel takes fp32 tensors only")
    if not ops.made_sweep_supported(D, H, L):
        raise RuntimeError(f"made_sweep: (D, H, L) = ({D}, {H}, {L}) is outside the kernel's LDS "
                           "budget")
    perm, ubeg = (plan or plan_for(D, H, L, order)).on(v.device)

    param = {"maf_sample": bound, "iaf_gated": gate_bias, "iaf_affine": scale}[kind]
    x = torch.empty(B, D, device=v.device, dtype=torch.float32)
    ldj = torch.empty(B, device=v.device, dtype=torch.float32)
    ops.made_sweep(_rows(v), [_rows(w) for w in weights],
                   [b.detach().contiguous() for b in biases], perm, ubeg, KINDS[kind], float(param),
                   None if ctx_bias is None else _rows(ctx_bias.float()), x, ldj)
    _sweep_launches += 1
    return x, ldj


def _check_sweep_inputs(name, v, weights, biases, ctx_bias):
    if v.dim() != 2 or len(weights) < 2 or len(weights) != len(biases):
        raise ValueError(f"{name}: v [B, D] and at least one hidden plus the output layer")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad
                                       for t in (v, ctx_bias, *weights, *biases)):
        raise RuntimeError(f"{name} is not differentiable: detach the inputs or call it under "
                           "torch.no_grad()")


def _rows(t):   # unit inner stride
    t = t.detach()
    return t if t.shape[1] == 1 or t.stride(1) == 1 else t.contiguous()


def _hidden_step(x, h, Ws, bs, ubeg, idx, t, ctx_bias):
    """The hidden units of degree ``t`` of every layer, in place in ``h``."""
    for l in range(len(h)):
        u0, u1 = ubeg[l][t], ubeg[l][t + 1]
        if u1 == u0:
            continue
        if l == 0:
            pre = x[:, idx[:t]] @ Ws[0][u0:u1][:, idx[:t]].T
            if ctx_bias is not None:
                pre = pre + ctx_bias[:, u0:u1].to(x.dtype)
        else:
            n = ubeg[l - 1][t + 1]
            pre = h[l - 1][:, :n] @ Ws[l][u0:u1, :n].T
        h[l][:, u0:u1] = torch.relu(pre + bs[l][u0:u1])


def _check_units(units) -> int:
    if not 1 <= int(units) <= 32:
        raise ValueError(f"dsf_sweep: need 1 <= units <= 32, got {units}")
    return int(units)


def dsf_sweep_composite(y, weights, biases, order, units, *, ctx_bias=None, plan=None):
    """The DSF sweep in torch, in the dtype of ``y`` (weights are cast to it): per coordinate the
    ``3 units`` outputs over the prefix ``h_L[:c(t)]``, then ``ops.reference.dsf_transform(...,
    inverse=True)`` of that one coordinate."""
    from .reference import dsf_transform

    U = _check_units(units)
    B, D = y.shape
    L, H = len(weights) - 1, weights[0].shape[0]
    if weights[L].shape[0] != 3 * U * D:
        raise ValueError(f"dsf_sweep: the output layer has {weights[L].shape[0]} rows, expected "
                         f"3 units D = {3 * U * D}")
    plan = plan or plan_for(D, H, L, order)
    perm, ubeg = plan.perm.tolist(), plan.ubeg.tolist()
    Ws = [w.detach().to(y.dtype) for w in weights]
    bs = [b.detach().to(y.dtype) for b in biases]
    idx = plan.perm.to(y.device, torch.long)
    planes = torch.arange(3 * U, device=y.device) * D
    z = torch.empty_like(y)
    ldj = y.new_zeros(B)
    h = [y.new_zeros(B, H) for _ in range(L)]
    with torch.no_grad():
        for t in range(1, D + 1):
            i, c = perm[t - 1], ubeg[L - 1][t]
            p = bs[L][planes + i] + h[L - 1][:, :c] @ Ws[L][planes + i, :c].T     # [B, 3U]
            zi, share = dsf_transform(p, y[:, i:i + 1], U, inverse=True)
            z[:, i] = zi[:, 0]
            ldj = ldj + share
            _hidden_step(z, h, Ws, bs, ubeg, idx, t, ctx_bias)
    return z, ldj


def dsf_kernel_supported(D: int, H: int, L: int, units: int) -> bool:
    """``dsf_sweep_supported`` of the native library: 1 <= units <= 32 and the (D, H, L, units)
    state of at least one row fits the LDS budget the launcher requests."""
    return bool(native().dsf_sweep_supported(int(D), int(H), int(L), int(units)))


def dsf_kernel_rows(D: int, H: int, L: int, units: int) -> int:
    """Rows per block the DSF launcher picks for (D, H, L, units); 0 when unsupported."""
    return int(native().dsf_sweep_rows(int(D), int(H), int(L), int(units)))


def dsf_sweep(y, weights, biases, order, units, *, ctx_bias=None, plan=None):
    """``(z, ldj)`` of the inverse of one MADE-conditioned DSF layer; no-grad.

    ``weights`` / ``biases``: the MADE's hidden layers then its output layer ([3 units D, H],
    plane-major: row k D + i is plane k of coordinate i; planes [0, units) raw slopes, then
    shifts, then mixture logits), fp32 and unmasked. ``z_i`` solves
    ``logit(sum_h w_h sigmoid(a_h z + b_h)) = y_i`` and ``ldj = -sum_i log dy_i/dz_i`` at z.
    ``order`` / ``ctx_bias`` / ``plan`` as in :func:`made_sweep`. GPU tensors run the HIP kernel
    (fp32 only, raising outside its limits), CPU tensors the composite."""
    U = _check_units(units)
    _check_sweep_inputs("dsf_sweep", y, weights, biases, ctx_bias)
    if not y.is_cuda:
        return dsf_sweep_composite(y, weights, biases, order, U, ctx_bias=ctx_bias, plan=plan)
    global _sweep_launches
    ops = native()
    B, D = y.shape
    L, H = len(weights) - 1, weights[0].shape[0]
    if y.dtype != torch.float32 or any(t.dtype != torch.float32 for t in (*weights, *biases)):
        raise RuntimeError("dsf_sweep: the HIP kernel takes fp32 tensors only")
    if not ops.dsf_sweep_supported(D, H, L, U):
        raise RuntimeError(f"dsf_sweep: (D, H, L, units) = ({D}, {H}, {L}, {U}) is outside the "
                           "kernel's LDS budget")
    perm, ubeg = (plan or plan_for(D, H, L, order)).on(y.device)
    z = torch.empty(B, D, device=y.device, dtype=torch.float32)
    ldj = torch.empty(B, device=y.device, dtype=torch.float32)
    ops.dsf_sweep(_rows(y), [_rows(w) for w in weights], [b.detach().contiguous() for b in biases],
                  perm, ubeg, U, None if ctx_bias is None else _rows(ctx_bias.float()), z, ldj)
    _sweep_launches += 1
    return z, ldj


def _check_bins(bins, bound) -> tuple:
    if not 2 <= int(bins) <= 32:
        raise ValueError(f"rqs_sweep: need 2 <= bins <= 32, got {bins}")
    if not float(bound) > 0:
        raise ValueError(f"rqs_sweep: need bound > 0, got {bound}")
    return int(bins), float(bound)


def _check_rqs_rows(weights, K, D):
    if weights[-1].shape[0] != (3 * K - 1) * D:
        raise ValueError(f"rqs_sweep: the output layer has {weights[-1].shape[0]} rows, expected "
                         f"(3 bins - 1) D = {(3 * K - 1) * D}")


def rqs_sweep_composite(y, weights, biases, order, bins, bound, *, ctx_bias=None, plan=None):
    """The spline sweep in torch, in the dtype of ``y`` (weights are cast to it): per coordinate
    the ``3 bins - 1`` outputs over the prefix ``h_L[:c(t)]``, then
    ``ops.reference.rqs_transform(..., inverse=True)`` of that one coordinate."""
    from .reference import rqs_transform

    K, bound = _check_bins(bins, bound)
    B, D = y.shape
    L, H = len(weights) - 1, weights[0].shape[0]
    _check_rqs_rows(weights, K, D)
    plan = plan or plan_for(D, H, L, order)
    perm, ubeg = plan.perm.tolist(), plan.ubeg.tolist()
    Ws = [w.detach().to(y.dtype) for w in weights]
    bs = [b.detach().to(y.dtype) for b in biases]
    idx = plan.perm.to(y.device, torch.long)
    planes = torch.arange(3 * K - 1, device=y.device) * D
    z = torch.empty_like(y)
    ldj = y.new_zeros(B)
    h = [y.new_zeros(B, H) for _ in range(L)]
    with torch.no_grad():
        for t in range(1, D + 1):
            i, c = perm[t - 1], ubeg[L - 1][t]
            p = bs[L][planes + i] + h[L - 1][:, :c] @ Ws[L][planes + i, :c].T     # [B, 3K - 1]
            zi, share = rqs_transform(p, y[:, i:i + 1], K, bound, inverse=True)
            z[:, i] = zi[:, 0]
            ldj = ldj + share
            _hidden_step(z, h, Ws, bs, ubeg, idx, t, ctx_bias)
    return z, ldj


def rqs_kernel_supported(D: int, H: int, L: int, bins: int) -> bool:
    """``rqs_sweep_supported`` of the native library: 2 <= bins <= 32 and the (D, H, L, bins)
    state of at least one row fits the LDS budget the launcher requests."""
    return bool(native().rqs_sweep_supported(int(D), int(H), int(L), int(bins)))


def rqs_kernel_rows(D: int, H: int, L: int, bins: int) -> int:
    """Rows per block the spline launcher picks for (D, H, L, bins); 0 when unsupported."""
    return int(native().rqs_sweep_rows(int(D), int(H), int(L), int(bins)))


def rqs_sweep(y, weights, biases, order, bins, bound, *, ctx_bias=None, plan=None):
    """``(z, ldj)`` of the sequential direction of one MADE-conditioned spline layer; no-grad.

    ``weights`` / ``biases``: the MADE's hidden layers then its output layer ([(3 bins - 1) D, H],
    plane-major: row k D + i is plane k of coordinate i; planes [0, bins) unnormalised widths,
    then heights, then the bins - 1 interior derivatives), fp32 and unmasked. ``z_i`` solves
    ``RQS(z_i; p_i(z)) = y_i`` on (-bound, bound) and is ``y_i`` outside;
    ``ldj = -sum_i log dy_i/dz_i`` at z. ``order`` / ``ctx_bias`` / ``plan`` as in
    :func:`made_sweep`. GPU tensors run the HIP kernel (fp32 only, raising outside its limits),
    CPU tensors the composite."""
    K, bound = _check_bins(bins, bound)
    _check_sweep_inputs("rqs_sweep", y, weights, biases, ctx_bias)
    _check_rqs_rows(weights, K, y.shape[1])
    if not y.is_cuda:
        return rqs_sweep_composite(y, weights, biases, order, K, bound, ctx_bias=ctx_bias,
                                   plan=plan)
    global _sweep_launches
    ops = native()
    B, D = y.shape
    L, H = len(weights) - 1, weights[0].shape[0]
    if y.dtype != torch.float32 or any(t.dtype != torch.float32 for t in (*weights, *biases)):
        raise RuntimeError("rqs_sweep: the HIP kernel takes fp32 tensors only")
    if not ops.rqs_sweep_supported(D, H, L, K):
        raise RuntimeError(f"rqs_sweep: (D, H, L, bins) = ({D}, {H}, {L}, {K}) is outside the "
                           "kernel's LDS budget")
    perm, ubeg = (plan or plan_for(D, H, L, order)).on(y.device)
    z = torch.empty(B, D, device=y.device, dtype=torch.float32)
    ldj = torch.empty(B, device=y.device, dtype=torch.float32)
    ops.rqs_sweep(_rows(y), [_rows(w) for w in weights], [b.detach().contiguous() for b in biases],
                  perm, ubeg, K, bound, None if ctx_bias is None else _rows(ctx_bias.float()),
                  z, ldj)
    _sweep_launches += 1
    return z, ldj


def supported(made, v, context, out_mult: int = 2) -> bool:
    """A MADE and input the sweep handles: ReLU, 1 .. 4 hidden layers, ``out_mult`` outputs per
    input (2: MAF / IAF; 3 units: a DSF layer; 3 bins - 1: a spline layer - never a multiple of 3,
    and 2 stays the affine case), fp32 everywhere, a context exactly when the MADE
    projects one, and (GPU) a shape inside the kernel's LDS budget."""
    L = len(made.layers) - 1
    if not (isinstance(made.act, torch.nn.ReLU) and 1 <= L <= MAX_HIDDEN
            and made.out_mult == out_mult):
        return False
    if v.dim() != 2 or v.dtype != torch.float32 or v.shape[1] != made.dim or v.shape[0] < 1:
        return False
    if any(l.weight.dtype != torch.float32 or l.bias is None for l in made.layers):
        return False
    if (made.ctx is not None) != (context is not None):
        return False
    if context is not None and (context.dim() != 2 or context.shape[0] != v.shape[0]):
        return False
    if not v.is_cuda:
        return True
    H = made.layers[0].weight.shape[0]
    if out_mult == 2:
        return kernel_supported(made.dim, H, L)
    if out_mult % 3 == 2 and out_mult >= 5:
        return rqs_kernel_supported(made.dim, H, L, (out_mult + 1) // 3)
    return out_mult % 3 == 0 and dsf_kernel_supported(made.dim, H, L, out_mult // 3)


def dispatch(flow, v, context) -> bool:
    """True when ``MAF.forward`` / ``IAF.inverse`` / ``DSFAutoregressive.inverse`` / the sequential
    direction of ``RQSAutoregressive`` take the sweep: GPU tensors, a supported MADE (two outputs
    per input, ``3 units`` for the DSF layer, ``3 bins - 1`` for the spline layer), and
    nothing that needs a graph (grad mode off, or neither the input, the context nor any
    parameter of the flow requires grad)."""
    if not v.is_cuda or not supported(flow.made, v, context, flow.made.out_mult):
        return False
    if not torch.is_grad_enabled():
        return True
    return not (v.requires_grad or (context is not None and context.requires_grad)
                or any(p.requires_grad for p in flow.parameters()))


def _plan_of(made) -> SweepPlan:
    plan = made.__dict__.get("_sweep_plan")   # cached on the module, like ops.masked.MaskPlan
    if plan is None:
        plan = made.__dict__["_sweep_plan"] = plan_for(
            made.dim, made.layers[0].weight.shape[0], len(made.layers) - 1, made.order)
    return plan


def dsf_sweep_flow(flow, y, context=None):
    """The sweep of a ``DSFAutoregressive`` layer (inverse, y -> z): the ``(z, -ldj)`` that
    ``DSFAutoregressive.inverse`` returns."""
    made = flow.made
    with torch.no_grad():
        ctx_bias = None
        if made.ctx is not None and context is not None:
            ctx_bias = made.ctx(context)
        return dsf_sweep(y, [l.weight for l in made.layers], [l.bias for l in made.layers],
                         made.order, flow.units, ctx_bias=ctx_bias, plan=_plan_of(made))


def rqs_sweep_flow(layer, y, context=None):
    """The sweep of an ``RQSAutoregressive`` layer (y -> z with T(z) = y): the ``(z, -ldj_T(z))``
    its sequential direction returns."""
    made = layer.made
    with torch.no_grad():
        ctx_bias = None
        if made.ctx is not None and context is not None:
            ctx_bias = made.ctx(context)
        return rqs_sweep(y, [l.weight for l in made.layers], [l.bias for l in made.layers],
                         made.order, layer.bins, layer.bound, ctx_bias=ctx_bias,
                         plan=_plan_of(made))


def made_sweep_flow(flow, v, context=None):
    """The sweep of a ``MAF`` (sampling, u -> x) or ``IAF`` (inverse, y -> z) layer: the
    ``(x, ldj)`` that ``MAF.forward`` / ``IAF.inverse`` return."""
    from ..flows.made import IAF, MAF

    made = flow.made
    if isinstance(flow, MAF):
        kind, kw = "maf_sample", {"bound": flow.bound}
    elif isinstance(flow, IAF):
        kind = "iaf_gated" if flow.mode == "gated" else "iaf_affine"
        kw = {"gate_bias": flow.gate_bias, "scale": flow.scale}
    else:
        raise TypeError(f"made_sweep_flow: expected a MAF or IAF layer, got {type(flow).__name__}")
    with torch.no_grad():
        ctx_bias = None
        if made.ctx is not None and context is not None:
            ctx_bias = made.ctx(context)
        return made_sweep(v, [l.weight for l in made.layers], [l.bias for l in made.layers],
                          made.order, kind, ctx_bias=ctx_bias, plan=_plan_of(made), **kw)
