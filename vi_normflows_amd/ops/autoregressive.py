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

The three sweeps themselves are not differentiable: ``MAF.forward`` / ``IAF.inverse`` take them
only when nothing needs a graph (:func:`dispatch`); ``DSFAutoregressive.inverse`` and the
sequential direction of ``RQSAutoregressive`` build none by default.

Implicit gradient (opt-in: ``implicit_grad=True`` on the modules, or the ``*_sweep_grad``
functions). A sweep solves ``T(x) = v`` for a map that is triangular in degree order,
``v_i = tau(x_i; p_i)``, ``p_i = MADE_i(x_{<i})`` in R^P, and returns ``l = -sum_i log dtau/dx_i``.
With ``d = dtau/dx``, ``q = dtau/dp``, ``e = dlog d/dx``, ``r = dlog d/dp`` at the solution and
cotangents ``(xbar, lbar)``, the cotangent ``w`` of ``v`` and ``pbar`` of ``p`` solve the transpose
of the forward substitution, walking the degrees downwards: :func:`sweep_adjoint`
(``csrc/kernels/sweep_adjoint.hip`` for fp32 GPU tensors, :func:`sweep_adjoint_composite`
elsewhere and as the oracle). ``q``, ``c = lbar r`` and ``pbar`` are COORDINATE-major [B, D, P]:
the P values of one coordinate are contiguous, since a step of the walk touches exactly those.
The backward of the one ``autograd.Function`` behind :func:`made_sweep_grad`,
:func:`dsf_sweep_grad` and :func:`rqs_sweep_grad` is one fp32 masked MADE pass at ``x``, the
element derivatives, the adjoint sweep and L + 1 weight-gradient products; no MADE input-gradient
chain is run. It is differentiable once.
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
        self._degrees = (d_in, hs)
        self._masks: dict = {}

    def on(self, device):
        d = self._dev.get(device)
        if d is None:
            d = self._dev[device] = (self.perm.to(device), self.ubeg.to(device).contiguous())
        return d

    def masks(self, out_mult: int, device, dtype):
        """The MADE's weight masks (hidden layers, then the output layer with ``out_mult`` rows
        per coordinate), as ``flows.made.made_masks`` builds them."""
        key = (int(out_mult), device, dtype)
        m = self._masks.get(key)
        if m is None:
            from ..flows.made import made_masks

            if len(self._masks) >= 8:
                self._masks.clear()
            m = self._masks[key] = [k.to(device=device, dtype=dtype)
                                    for k in made_masks(*self._degrees, int(out_mult))]
        return m


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


# ---- the implicit gradient of the sweeps ---------------------------------------------------------

_adjoint_launches = 0


def sweep_adjoint_launches(reset: bool = False) -> int:
    """Number of adjoint-sweep kernel launches so far (evidence that the HIP path ran)."""
    global _adjoint_launches
    n = _adjoint_launches
    if reset:
        _adjoint_launches = 0
    return n


def adjoint_kernel_supported(D: int, H: int, L: int, P: int) -> bool:
    """``sweep_adjoint_supported`` of the native library: 1 <= P <= 96 and the (D, H, L, P) state
    of at least one row fits the LDS budget the launcher requests."""
    return bool(native().sweep_adjoint_supported(int(D), int(H), int(L), int(P)))


def adjoint_kernel_rows(D: int, H: int, L: int, P: int) -> int:
    """Rows per block the adjoint launcher picks for (D, H, L, P); 0 when unsupported."""
    return int(native().sweep_adjoint_rows(int(D), int(H), int(L), int(P)))


def _check_adjoint_inputs(gx, d, q, c, hidden, weights):
    if gx.dim() != 2 or d.shape != gx.shape or q.dim() != 3 or q.shape[:2] != gx.shape \
            or c.shape != q.shape:
        raise ValueError("sweep_adjoint: gx, d [B, D] and q, c [B, D, P] (coordinate-major)")
    L = len(weights) - 1
    if L < 1 or len(hidden) != L:
        raise ValueError("sweep_adjoint: at least one hidden plus the output layer, and one "
                         "activation per hidden layer")
    if weights[L].shape[0] != q.shape[2] * gx.shape[1]:
        raise ValueError(f"sweep_adjoint: the output layer has {weights[L].shape[0]} rows, "
                         f"expected P D = {q.shape[2] * gx.shape[1]}")


def sweep_adjoint_composite(gx, d, q, c, hidden, weights, order, *, plan=None):
    """The adjoint sweep in torch, in the dtype of ``gx`` (weights are cast to it): the recursion
    of :func:`sweep_adjoint`, degree by degree. The CPU path and the oracle."""
    _check_adjoint_inputs(gx, d, q, c, hidden, weights)
    B, D = gx.shape
    P = q.shape[2]
    L, H = len(weights) - 1, weights[0].shape[0]
    plan = plan or plan_for(D, H, L, order)
    perm, ubeg = plan.perm.tolist(), plan.ubeg.tolist()
    Ws = [w.detach().to(gx.dtype) for w in weights]
    idx = plan.perm.to(gx.device, torch.long)
    planes = torch.arange(P, device=gx.device) * D
    xhat = gx.new_zeros(B, D)                      # degree order
    hbar = [gx.new_zeros(B, H) for _ in range(L)]
    a = [gx.new_zeros(B, H) for _ in range(L)]
    w = torch.empty_like(gx)
    pbar = torch.empty_like(q)
    for t in range(D, 0, -1):
        i = perm[t - 1]
        for l in range(L - 1, -1, -1):
            u0, u1 = ubeg[l][t], ubeg[l][t + 1]
            if u1 == u0:
                continue
            al = torch.where(hidden[l][:, u0:u1] > 0, hbar[l][:, u0:u1],
                             torch.zeros((), dtype=gx.dtype, device=gx.device))
            a[l][:, u0:u1] = al
            if l == 0:
                xhat[:, :t] += al @ Ws[0][u0:u1][:, idx[:t]]
            else:
                n = ubeg[l - 1][t + 1]
                hbar[l - 1][:, :n] += al @ Ws[l][u0:u1, :n]
        wi = (gx[:, i] - xhat[:, t - 1]) / d[:, i]
        w[:, i] = wi
        pb = q[:, i] * wi[:, None] + c[:, i]
        pbar[:, i] = pb
        cc = ubeg[L - 1][t]
        hbar[L - 1][:, :cc] += pb @ Ws[L][planes + i, :cc]
    return w, pbar, a


def sweep_adjoint(gx, d, q, c, hidden, weights, order, *, plan=None):
    """``(w, pbar, [a_l])``: the transpose of a degree sweep's forward substitution; no-grad.

    ``gx = xbar - lbar e`` and ``d`` are [B, D]; ``q`` and ``c = lbar r`` are [B, D, P],
    COORDINATE-major (``q[:, i]`` holds the P derivatives of coordinate i; the conditioner's
    plane-major output [B, P D] maps to it by ``.view(B, P, D).transpose(1, 2)``); ``hidden``
    are the L hidden activations [B, H] at the solution, used only for ``> 0``; ``weights`` the
    MADE's hidden layers then its output layer [P D, H] (plane-major rows), unmasked. Walking
    ``t = D .. 1`` with ``i = perm[t - 1]``: the hidden units of degree t get
    ``a_l = hbar_l [h_l > 0]`` and push it into the prefix below them (layer 1: into ``xhat[:t]``);
    ``w_i = (gx_i - xhat_t) / d_i``; ``pbar_i = q_i w_i + c_i``;
    ``hbar_L[:c(t)] += pbar_i Wo[planes of i, :c(t)]``. Returns ``w`` [B, D] (the cotangent of
    ``v``), ``pbar`` [B, D, P] and the ``a_l`` [B, H] (the cotangents of the hidden
    pre-activations). GPU tensors run the HIP kernel (fp32 only, raising outside its limits), CPU
    tensors the composite."""
    _check_adjoint_inputs(gx, d, q, c, hidden, weights)
    if not gx.is_cuda:
        return sweep_adjoint_composite(gx, d, q, c, hidden, weights, order, plan=plan)
    global _adjoint_launches
    ops = native()
    B, D = gx.shape
    P = q.shape[2]
    L, H = len(weights) - 1, weights[0].shape[0]
    if any(t.dtype != torch.float32 for t in (gx, d, q, c, *hidden, *weights)):
        raise RuntimeError("sweep_adjoint: the HIP kernel takes fp32 tensors only")
    if not ops.sweep_adjoint_supported(D, H, L, P):
        raise RuntimeError(f"sweep_adjoint: (D, H, L, P) = ({D}, {H}, {L}, {P}) is outside the "
                           "kernel's LDS budget")
    perm, ubeg = (plan or plan_for(D, H, L, order)).on(gx.device)
    w = torch.empty(B, D, device=gx.device, dtype=torch.float32)
    pbar = torch.empty(B, D, P, device=gx.device, dtype=torch.float32)
    a = [torch.zeros(B, H, device=gx.device, dtype=torch.float32) for _ in range(L)]
    ops.sweep_adjoint(_rows(gx), _rows(d), q.detach().contiguous(), c.detach().contiguous(),
                      [_rows(h) for h in hidden], [_rows(k) for k in weights], perm, ubeg,
                      w, pbar, a)
    _adjoint_launches += 1
    return w, pbar, a


def _spec_planes(spec) -> int:
    if spec[0] == "made":
        return 2
    return 3 * spec[1] if spec[0] == "dsf" else 3 * spec[1] - 1


def _run_sweep(spec, v, weights, biases, order, ctx_bias, plan):
    if spec[0] == "made":
        _, kind, bound, gate_bias, scale = spec
        return made_sweep(v, weights, biases, order, kind, ctx_bias=ctx_bias, bound=bound,
                          gate_bias=gate_bias, scale=scale, plan=plan)
    if spec[0] == "dsf":
        return dsf_sweep(v, weights, biases, order, spec[1], ctx_bias=ctx_bias, plan=plan)
    return rqs_sweep(v, weights, biases, order, spec[1], spec[2], ctx_bias=ctx_bias, plan=plan)


def _masked_pass(x, weights, biases, masks, ctx_bias):
    """One masked MADE pass at ``x`` in its dtype: the plane-major output [B, P D] and the hidden
    activations. GPU: the exact-fp32 MFMA products of ``ops/linear.py`` on ``weight * mask``."""
    from .linear import linear

    h, hidden = x, []
    for l, (W, b, m) in enumerate(zip(weights, biases, masks)):
        h = linear(h, (W * m).to(x.dtype), b.to(x.dtype), precision="fp32" if x.is_cuda else None)
        if l == 0 and ctx_bias is not None:
            h = h + ctx_bias.to(x.dtype)
        if l < len(weights) - 1:
            h = torch.relu(h)
            hidden.append(h)
    return h, hidden


def _coord_major(t, P):   # plane-major [B, P D] -> coordinate-major [B, D, P]
    return t.view(t.shape[0], P, -1).transpose(1, 2).contiguous()


def _element_derivatives(spec, x, p, lbar):
    """``(lbar e, d, q, c = lbar r)`` of ``v = tau(x; p)`` at ``(x, p)``; ``q`` and ``c`` are
    coordinate-major [B, D, P]."""
    B, D = x.shape
    if spec[0] == "made":
        _, kind, bound, gate_bias, scale = spec
        m, s = p[:, :D], p[:, D:]
        if kind == "maf_sample":          # v = (x - m) exp(-a), a = bound tanh(s / bound)
            th = torch.tanh(s / bound)
            d = torch.exp(-bound * th)
            da = 1 - th * th
            qm, qs, rs = -d, -(x - m) * d * da, -da
        elif kind == "iaf_gated":         # v = g x + (1 - g) m, g = sigmoid(s + gate_bias)
            d = torch.sigmoid(s + gate_bias)
            qm, qs, rs = 1 - d, (x - m) * d * (1 - d), 1 - d
        else:                             # v = x exp(c) + m, c = scale tanh(s)
            th = torch.tanh(s)
            d = torch.exp(scale * th)
            dc = scale * (1 - th * th)
            qm, qs, rs = torch.ones_like(d), x * d * dc, dc
        q = torch.stack([qm, qs], 2)
        c = torch.stack([torch.zeros_like(rs), lbar[:, None] * rs], 2)
        return torch.zeros_like(x), d, q, c
    P = _spec_planes(spec)
    if x.is_cuda:   # the element backward is linear in (gy, gldj): q is the gy = 1 call
        from .dsf import dsf_bwd
        from .spline import rqs_bwd

        def bwd(gy, gl):
            if spec[0] == "dsf":
                return dsf_bwd(p, x, gy, gl, spec[1], False)
            return rqs_bwd(p, x, gy, gl, spec[1], spec[2], False)

        p, x = p.contiguous(), x.contiguous()
        q, d = bwd(torch.ones_like(x), torch.zeros_like(lbar))
        c, le = bwd(torch.zeros_like(x), lbar.contiguous())
        return le, d, _coord_major(q, P), _coord_major(c, P)
    from . import reference

    with torch.enable_grad():
        pg, xg = p.detach().requires_grad_(), x.detach().requires_grad_()
        if spec[0] == "dsf":
            y, ldj = reference.dsf_transform(pg, xg, spec[1])
        else:
            y, ldj = reference.rqs_transform(pg, xg, spec[1], spec[2])
        q, d = torch.autograd.grad(y.sum(), (pg, xg), retain_graph=True)
        c, le = torch.autograd.grad((ldj * lbar).sum(), (pg, xg), allow_unused=True)
    c = torch.zeros_like(p) if c is None else c
    le = torch.zeros_like(x) if le is None else le
    return le, d, _coord_major(q, P), _coord_major(c, P)


def _wgrad(g, h, mask):
    """``-(g^T h) * mask`` and ``-colsum g``: GPU on the fp32 MFMA weight-gradient kernel."""
    if g.is_cuda:
        g, h = g.contiguous(), h.contiguous()
        dW = torch.empty(g.shape[1], h.shape[1], dtype=g.dtype, device=g.device)
        db = torch.empty(g.shape[1], dtype=g.dtype, device=g.device)
        native().gemm_fp(g, False, h, False, None, dW, False, db)
        return dW.mul_(mask).neg_(), db.neg_()
    return -(g.T @ h) * mask, -g.sum(0)


class _ImplicitSweepFn(torch.autograd.Function):
    """A degree sweep with its implicit gradient. Inputs: the family ``spec``, the input degrees,
    the :class:`SweepPlan`, then ``v``, ``ctx_bias`` (or None) and the weights and biases."""

    @staticmethod
    def forward(ctx, spec, order, plan, v, ctx_bias, *wb):
        n = len(wb) // 2
        weights, biases = [t.detach() for t in wb[:n]], [t.detach() for t in wb[n:]]
        cb = None if ctx_bias is None else ctx_bias.detach()
        x, l = _run_sweep(spec, v.detach(), weights, biases, order, cb, plan)
        ctx.save_for_backward(x, cb, *weights, *biases)
        ctx.spec, ctx.order, ctx.plan = spec, order, plan
        ctx.dtypes = (v.dtype, None if ctx_bias is None else ctx_bias.dtype)
        return x, l

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, xbar, lbar):
        x, cb, *wb = ctx.saved_tensors
        n = len(wb) // 2
        weights, biases = wb[:n], wb[n:]
        spec, plan = ctx.spec, ctx.plan
        P = _spec_planes(spec)
        masks = plan.masks(P, x.device, x.dtype)
        xbar, lbar = xbar.to(x.dtype), lbar.to(x.dtype)
        p, hidden = _masked_pass(x, weights, biases, masks, cb)
        le, d, q, c = _element_derivatives(spec, x, p, lbar)
        w, pbar, a = sweep_adjoint(xbar - le, d, q, c, hidden, weights, ctx.order, plan=plan)
        pbar_pm = pbar.transpose(1, 2).reshape(x.shape[0], -1)    # plane-major, as the MADE's rows
        gW, gb = [], []
        for l in range(n):
            g = a[l] if l < n - 1 else pbar_pm
            h = x if l == 0 else hidden[l - 1]
            dW, db = _wgrad(g, h, masks[l])
            gW.append(dW.to(weights[l].dtype))
            gb.append(db.to(biases[l].dtype))
        gv = w.to(ctx.dtypes[0]) if ctx.needs_input_grad[3] else None
        gc = (-a[0]).to(ctx.dtypes[1]) if cb is not None and ctx.needs_input_grad[4] else None
        return (None, None, None, gv, gc, *gW, *gb)


def _sweep_grad(spec, v, weights, biases, order, ctx_bias, plan):
    if v.dim() != 2 or len(weights) < 2 or len(weights) != len(biases):
        raise ValueError("sweep_grad: v [B, D] and at least one hidden plus the output layer")
    L, H = len(weights) - 1, weights[0].shape[0]
    plan = plan or plan_for(v.shape[1], H, L, order)
    if v.is_cuda and not adjoint_kernel_supported(v.shape[1], H, L, _spec_planes(spec)):
        raise RuntimeError(f"sweep_grad: (D, H, L, P) = ({v.shape[1]}, {H}, {L}, "
                           f"{_spec_planes(spec)}) is outside the adjoint kernel's LDS budget")
    return _ImplicitSweepFn.apply(spec, order, plan, v, ctx_bias, *weights, *biases)


def made_sweep_grad(v, weights, biases, order, kind, *, ctx_bias=None, bound=5.0, gate_bias=1.0,
                    scale=1.0, plan=None):
    """:func:`made_sweep` with the implicit gradient for ``v``, ``ctx_bias``, the weights and the
    biases (once differentiable). The weights are used under the MADE's masks, and their
    gradients are masked."""
    if kind not in KINDS:
        raise ValueError(f"made_sweep_grad: kind must be one of {sorted(KINDS)}, got {kind!r}")
    spec = ("made", kind, float(bound), float(gate_bias), float(scale))
    return _sweep_grad(spec, v, weights, biases, order, ctx_bias, plan)


def dsf_sweep_grad(y, weights, biases, order, units, *, ctx_bias=None, plan=None):
    """:func:`dsf_sweep` with the implicit gradient (see :func:`made_sweep_grad`)."""
    return _sweep_grad(("dsf", _check_units(units)), y, weights, biases, order, ctx_bias, plan)


def rqs_sweep_grad(y, weights, biases, order, bins, bound, *, ctx_bias=None, plan=None):
    """:func:`rqs_sweep` with the implicit gradient (see :func:`made_sweep_grad`)."""
    K, bound = _check_bins(bins, bound)
    return _sweep_grad(("rqs", K, bound), y, weights, biases, order, ctx_bias, plan)


def needs_graph(flow, v, context) -> bool:
    """Grad mode is on and the input, the context or a parameter of ``flow`` requires grad."""
    return torch.is_grad_enabled() and (
        v.requires_grad or (context is not None and context.requires_grad)
        or any(p.requires_grad for p in flow.parameters()))


def grad_supported(made, v, context, out_mult: int = 2) -> bool:
    """A MADE and input the implicit-gradient path handles: ReLU, 1 .. 4 hidden layers, a bias on
    every layer, a context exactly when the MADE projects one; on the CPU any floating dtype, on
    the GPU what :func:`supported` asks plus a shape inside the adjoint kernel's LDS budget."""
    if v.is_cuda:
        return supported(made, v, context, out_mult) and adjoint_kernel_supported(
            made.dim, made.layers[0].weight.shape[0], len(made.layers) - 1, out_mult)
    L = len(made.layers) - 1
    if not (isinstance(made.act, torch.nn.ReLU) and 1 <= L <= MAX_HIDDEN
            and made.out_mult == out_mult):
        return False
    if v.dim() != 2 or not v.is_floating_point() or v.shape[1] != made.dim or v.shape[0] < 1:
        return False
    if any(l.bias is None for l in made.layers):
        return False
    if (made.ctx is not None) != (context is not None):
        return False
    return context is None or (context.dim() == 2 and context.shape[0] == v.shape[0])


def _flow_grad(spec, made, v, context):
    ctx_bias = None
    if made.ctx is not None and context is not None:
        ctx_bias = made.ctx(context)          # under autograd: it receives -a_1
    return _sweep_grad(spec, v, [l.weight for l in made.layers], [l.bias for l in made.layers],
                       made.order, ctx_bias, _plan_of(made))


def made_sweep_flow_grad(flow, v, context=None):
    """:func:`made_sweep_flow` with the implicit gradient."""
    from ..flows.made import IAF, MAF

    if isinstance(flow, MAF):
        spec = ("made", "maf_sample", float(flow.bound), 1.0, 1.0)
    elif isinstance(flow, IAF):
        spec = ("made", "iaf_gated" if flow.mode == "gated" else "iaf_affine", 5.0,
                float(flow.gate_bias), float(flow.scale))
    else:
        raise TypeError("made_sweep_flow_grad: expected a MAF or IAF layer, got "
                        f"{type(flow).__name__}")
    return _flow_grad(spec, flow.made, v, context)


def dsf_sweep_flow_grad(flow, y, context=None):
    """:func:`dsf_sweep_flow` with the implicit gradient."""
    return _flow_grad(("dsf", int(flow.units)), flow.made, y, context)


def rqs_sweep_flow_grad(layer, y, context=None):
    """:func:`rqs_sweep_flow` with the implicit gradient."""
    return _flow_grad(("rqs", int(layer.bins), float(layer.bound)), layer.made, y, context)
