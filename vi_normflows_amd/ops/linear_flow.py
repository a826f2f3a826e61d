"""Solves against an LU-parameterised (or Cholesky-type) linear map, per batch row.

The map is ``y = x W^T + b`` with ``W = (L U)[perm, :]``, that is ``y = (x (L U)^T)[:, perm] + b``.
The factors come packed in one matrix ``A [D, D]``:

* ``mode="lu"``: the strict lower triangle of ``A`` is ``L`` (unit diagonal implied, never read),
  the upper triangle with the diagonal is ``U``;
* ``mode="lower"``: the lower triangle of ``A`` with its diagonal is the one factor (a
  Cholesky-type scale); the strict upper triangle is never read and may hold anything.

:func:`lu_solve` returns

* ``transpose=False``: ``x = W^-1 (y - b)``: stage ``s[:, perm[i]] = y[:, i] - b[i]``, solve
  ``L z = s`` then ``U x = z``;
* ``transpose=True``: ``W^-T y``: solve ``U^T q = y`` then ``L^T g = q`` and return
  ``g[:, perm]`` (no bias) - the cotangent of ``y`` for a cotangent of ``x``.

fp32 GPU tensors with ``D`` inside the kernel's limits run ``csrc/kernels/lu_solve.hip``: one
launch, a tile of rows per block with its vectors in LDS across both solves, permutation and bias
folded into the staging; a row's result is bitwise independent of the batch around it. Everything
else (CPU tensors, other dtypes, larger ``D``) runs :func:`lu_solve_reference`, the composite of
``torch.linalg.solve_triangular`` calls that is also the test oracle. ``impl="auto"`` (what the
modules pass) takes the kernel only where it measured at least as fast as the composite
(:func:`kernel_preferred`, docs/PERF_NOTES.md "LU solve").

The gradient is one ``autograd.Function``: one more launch with ``transpose=True`` gives ``gy``;
then with ``g_s`` = ``gy`` scattered back through ``perm``, ``gM = -(g_s^T x)`` and
``gb = -colsum(gy)`` (GPU: the fp32 weight-gradient product ``gemm_fp``), and ``gM`` maps to the
packed layout as ``tril(gM U^T, -1) + triu(L^T gM)`` (``mode="lu"``, two products through
``ops.linear.linear``) or ``tril(gM)`` (``mode="lower"``). It is differentiable once.
"""
from __future__ import annotations

import torch

from ._ext import native

MODES = {"lu": 0, "lower": 1}

_solve_launches = 0


def solve_launches(reset: bool = False) -> int:
    """Number of ``lu_solve`` kernel launches so far (evidence that the HIP path ran)."""
    global _solve_launches
    n = _solve_launches
    if reset:
        _solve_launches = 0
    return n


def kernel_supported(D: int) -> bool:
    """``lu_solve_supported`` of the native library."""
    return bool(native().lu_solve_supported(int(D)))


def kernel_rows(D: int) -> int:
    """Rows per block the launcher picks for ``D``; 0 when unsupported."""
    return int(native().lu_solve_rows(int(D)))


# Dispatch of impl="auto", from the measurement in docs/PERF_NOTES.md ("LU solve"): the kernel
# is taken for D <= AUTO_MAX_D and the composite above.
AUTO_MAX_D = 256


def kernel_preferred(B: int, D: int) -> bool:
    """Where the kernel measured at least as fast as the composite on the MI355X."""
    return D <= AUTO_MAX_D


def _factors(A, mode):
    if mode == "lu":
        eye = torch.eye(A.shape[0], dtype=A.dtype, device=A.device)
        return torch.tril(A, -1) + eye, torch.triu(A)
    return torch.tril(A), None


def _check(y, A, perm, bias, mode, transpose):
    if mode not in MODES:
        raise ValueError(f"lu_solve: mode must be one of {sorted(MODES)}, got {mode!r}")
    if y.dim() != 2 or A.dim() != 2 or A.shape[0] != A.shape[1] or A.shape[0] != y.shape[1]:
        raise ValueError(f"lu_solve: y [B, D] and A [D, D], got {tuple(y.shape)} and "
                         f"{tuple(A.shape)}")
    D = y.shape[1]
    if perm is not None and (perm.dim() != 1 or perm.numel() != D or perm.is_floating_point()):
        raise ValueError(f"lu_solve: perm must be an integer tensor of {D} elements")
    if bias is not None and (bias.dim() != 1 or bias.numel() != D):
        raise ValueError(f"lu_solve: bias must have {D} elements")
    if bias is not None and transpose:
        raise ValueError("lu_solve: transpose=True takes no bias")


# Rows per vendor triangular solve on the GPU: at (B, D) = (65536, 784) the fp32 solve fails to
# allocate its workspace on the MI355X while 32768 rows run, so larger batches go in row chunks.
COMPOSITE_MAX_ROWS = 32768


def lu_solve_reference(y, A, perm=None, bias=None, *, mode="lu", transpose=False):
    """The composite, in the dtype of ``y`` (``A`` and ``bias`` are cast to it): two
    ``torch.linalg.solve_triangular`` calls (one for ``mode="lower"``) plus the gather / scatter
    through ``perm`` and the bias. Differentiable by torch's own autograd. The CPU path and the
    oracle. GPU batches above ``COMPOSITE_MAX_ROWS`` rows are solved in row chunks."""
    _check(y, A, perm, bias, mode, transpose)
    if y.is_cuda and y.shape[0] > COMPOSITE_MAX_ROWS:
        return torch.cat([lu_solve_reference(c, A, perm, bias, mode=mode, transpose=transpose)
                          for c in y.split(COMPOSITE_MAX_ROWS)])
    A = A.to(y.dtype)
    F1, F2 = _factors(A, mode)
    idx = None if perm is None else perm.to(device=y.device, dtype=torch.long)
    st = torch.linalg.solve_triangular
    if not transpose:
        s = y if bias is None else y - bias.to(y.dtype)
        if idx is not None:
            s = s[:, torch.argsort(idx)]          # s[:, perm[i]] = (y - b)[:, i]
        if mode == "lu":
            z = st(F1, s.mT, upper=False, unitriangular=True)
            return st(F2, z, upper=True).mT
        return st(F1, s.mT, upper=False).mT
    if mode == "lu":
        q = st(F2.mT, y.mT, upper=False)
        g = st(F1.mT, q, upper=True, unitriangular=True).mT
    else:
        g = st(F1.mT, y.mT, upper=True).mT
    return g if idx is None else g[:, idx]


def _rows(t):   # unit inner stride
    return t if t.shape[1] == 1 or t.stride(1) == 1 else t.contiguous()


def _perm32(perm, device):
    if perm is None:
        return None
    return perm.to(device=device, dtype=torch.int32).contiguous()


def lu_solve_kernel(y, A, perm=None, bias=None, *, mode="lu", transpose=False, At=None,
                    out=None, check_perm=True):
    """One launch of the HIP kernel; no-grad, fp32 GPU tensors only, raising outside its limits.
    ``At``: ``A^T`` when the caller keeps one (``transpose=False`` reads only that orientation and
    makes it here otherwise; ``transpose=True`` reads ``A`` itself). ``out``: an fp32 [B, D] view
    with unit inner stride to write into (any row stride). ``check_perm=False`` skips the range
    check of ``perm`` for a caller that has validated it."""
    global _solve_launches
    _check(y, A, perm, bias, mode, transpose)
    if not y.is_cuda:
        raise RuntimeError("lu_solve_kernel: GPU tensors only (lu_solve_reference is the CPU path)")
    if any(t is not None and t.dtype != torch.float32 for t in (y, A, bias, At, out)):
        raise RuntimeError("lu_solve: the HIP kernel takes fp32 tensors only")
    ops = native()
    B, D = y.shape
    if not ops.lu_solve_supported(D):
        raise RuntimeError(f"lu_solve: D = {D} is outside the kernel's limits")
    y, A = _rows(y.detach()), A.detach()
    if transpose:
        A, At = _rows(A), None
    else:
        At = A.t().contiguous() if At is None else _rows(At.detach())
        A = None
    x = torch.empty(B, D, device=y.device, dtype=torch.float32) if out is None else out
    ops.lu_solve(y, A, At, _perm32(perm, y.device),
                 None if bias is None else bias.detach().contiguous(), MODES[mode],
                 bool(transpose), bool(check_perm), x)
    if B > 0:
        _solve_launches += 1
    return x


def _takes_kernel(y, A, bias, impl) -> bool:
    if impl == "composite" or not y.is_cuda:
        return False
    ok = (all(t is None or (t.is_cuda and t.dtype == torch.float32) for t in (y, A, bias))
          and kernel_supported(y.shape[1]))
    if impl == "kernel" and not ok:
        raise RuntimeError("lu_solve: impl='kernel' needs fp32 GPU tensors and a supported D")
    if impl == "auto":
        return ok and kernel_preferred(y.shape[0], y.shape[1])
    return ok


def _solve(y, A, perm, bias, mode, transpose, use_kernel, check_perm):
    if use_kernel:
        return lu_solve_kernel(y, A, perm, bias, mode=mode, transpose=transpose,
                               check_perm=check_perm)
    return lu_solve_reference(y, A, perm, bias, mode=mode, transpose=transpose)


def _wgrad(g, h):
    """``g^T h`` and ``colsum g``: on the GPU the exact MFMA weight-gradient kernel."""
    if g.is_cuda and g.dtype in (torch.float32, torch.float64):
        g, h = g.contiguous(), h.contiguous()
        dW = torch.empty(g.shape[1], h.shape[1], dtype=g.dtype, device=g.device)
        db = torch.empty(g.shape[1], dtype=g.dtype, device=g.device)
        native().gemm_fp(g, False, h, False, None, dW, False, db)
        return dW, db
    return g.T @ h, g.sum(0)


class _LuSolveFn(torch.autograd.Function):
    """:func:`lu_solve` with its gradient for ``y``, ``A`` and ``bias``."""

    @staticmethod
    def forward(ctx, y, A, bias, perm, mode, transpose, use_kernel, check_perm):
        dt = y.dtype
        with torch.no_grad():
            x = _solve(y.detach(), A.detach().to(dt), perm,
                       None if bias is None else bias.detach().to(dt), mode, transpose,
                       use_kernel, check_perm)
        ctx.save_for_backward(x, A.detach(), perm)
        ctx.cfg = (mode, transpose, use_kernel, A.dtype, None if bias is None else bias.dtype)
        return x

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gx):
        from .linear import linear

        x, A, perm = ctx.saved_tensors
        mode, transpose, use_kernel, adt, bdt = ctx.cfg
        dt = x.dtype
        A = A.to(dt)
        gx = gx.to(dt)
        # the cotangent of the input: the same solve, the other way round
        gy = _solve(gx, A, perm, None, mode, not transpose, use_kernel, False)
        gA = gb = None
        if ctx.needs_input_grad[1] or (bdt is not None and ctx.needs_input_grad[2]):
            idx = None if perm is None else perm.to(device=x.device, dtype=torch.long)
            inv = None if idx is None else torch.argsort(idx)
            if not transpose:     # x = M^-1 s: gM = -(g_s^T x), g_s = gy scattered through perm
                gs = gy if inv is None else gy[:, inv]
                gM, db = _wgrad(gs, x)
                if bdt is not None and ctx.needs_input_grad[2]:
                    gb = (-(db if idx is None else db[idx])).to(bdt)
            else:                 # h = M^-T y, x = h[:, perm]: gM = -(h^T gy)
                h = x if inv is None else x[:, inv]
                gM, _ = _wgrad(h, gy)
            gM = -gM
            if ctx.needs_input_grad[1]:
                if mode == "lu":
                    L, U = _factors(A, mode)
                    prec = "fp32" if dt == torch.float32 else None
                    gL = linear(gM, U, None, precision=prec)                 # gM U^T
                    gU = linear(gM.T.contiguous(), L.T.contiguous(), None,   # (gM^T L)^T = L^T gM
                                precision=prec).T
                    gA = torch.tril(gL, -1) + torch.triu(gU)
                else:
                    gA = torch.tril(gM)
                gA = gA.to(adt)
        return (gy if ctx.needs_input_grad[0] else None), gA, gb, None, None, None, None, None


def lu_solve(y, A, perm=None, bias=None, *, mode="lu", transpose=False, impl=None,
             check_perm=True):
    """``W^-1 (y - b)`` (``transpose=False``) or ``W^-T y`` (``transpose=True``) for
    ``W = (L U)[perm, :]`` packed in ``A`` (module docstring); differentiable once in ``y``, ``A``
    and ``bias``.

    ``impl``: None = the HIP kernel for fp32 GPU tensors with a supported ``D`` and the composite
    for everything else; ``"auto"`` = additionally the composite where it measured faster
    (:func:`kernel_preferred`); ``"kernel"`` raises where the kernel does not apply;
    ``"composite"`` never launches it. ``check_perm=False`` skips the kernel path's range check of
    ``perm`` (a host read) for a caller that has validated it."""
    if impl not in (None, "auto", "kernel", "composite"):
        raise ValueError(f"lu_solve: unknown impl {impl!r}")
    _check(y, A, perm, bias, mode, transpose)
    use_kernel = _takes_kernel(y, A, bias, impl)
    needs_grad = torch.is_grad_enabled() and any(
        t is not None and t.requires_grad for t in (y, A, bias))
    if not needs_grad:
        dt = y.dtype
        return _solve(y.detach(), A.detach().to(dt), perm,
                      None if bias is None else bias.detach().to(dt), mode, transpose,
                      use_kernel, check_perm)
    return _LuSolveFn.apply(y, A, bias, perm, mode, bool(transpose), use_kernel, check_perm)
