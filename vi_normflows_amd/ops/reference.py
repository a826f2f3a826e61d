"""Pure-PyTorch composites of every native op.

These are (a) the CPU plumbing path (north-star config 1 runs on CPU) and
(b) the fp32 oracles that the HIP kernels are tested against. Signatures
mirror the ``torch.ops.vinf`` schemas: outputs are passed in and mutated.
"""
from __future__ import annotations

import math

import torch

LOG2PI = math.log(2.0 * math.pi)


# ----------------------------------------------------------------- coupling
def coupling_fwd(st, x, y, ybf, ssav, ldj, scale, inverse, ldj_init):
    Dh = x.shape[1]
    sh = st[:, :Dh].float()
    t = st[:, Dh:2 * Dh].float()
    s = scale * torch.tanh(sh)
    if inverse:
        yv = (x - t) * torch.exp(-s)
        d = -s.sum(1)
    else:
        yv = x * torch.exp(s) + t
        d = s.sum(1)
    y.copy_(yv)
    if ybf is not None:
        ybf[:, :Dh].copy_(yv.to(ybf.dtype))
        if ybf.shape[1] > Dh:
            ybf[:, Dh:].zero_()
    if ssav is not None:
        ssav.copy_(s)
    if ldj_init:
        ldj.copy_(d)
    else:
        ldj.add_(d)


def coupling_bwd(gy, s, x, c, c_row, dst, gx, scale, gx_accumulate):
    Dh = x.shape[1]
    cc = c_row.view(-1, 1) if c_row is not None else c
    es = torch.exp(s)
    ds = gy * x * es + cc
    dsh = ds * (scale - s * s / scale)
    dst[:, :Dh].copy_(dsh.to(dst.dtype))
    dst[:, Dh:2 * Dh].copy_(gy.to(dst.dtype))
    if dst.shape[1] > 2 * Dh:
        dst[:, 2 * Dh:].zero_()
    if gx_accumulate:
        gx.add_(gy * es)
    else:
        gx.copy_(gy * es)


# ----------------------------------------------------------------- ELBO targets
def target_logp(kind, z, params=None, p0=1.0, p1=1.0, p2=0.0, cst=0.0):
    """log p(z) for a full [B, D] state (differentiable composite)."""
    if kind == 0:
        D = z.shape[1]
        m, iv = params[:D], params[D:]
        return -0.5 * ((z - m) ** 2 * iv).sum(1) + cst
    s1, s2, bend = p0, p1, p2
    if kind == 2:   # split pairing (z_i, z_{D/2+i})
        Dh = z.shape[1] // 2
        x, yv = z[:, :Dh], z[:, Dh:2 * Dh]
    else:           # interleaved pairing (z_2i, z_2i+1)
        x, yv = z[:, 0::2], z[:, 1::2]
    r = yv - bend * (x * x - s1 * s1)
    return -0.5 * ((x * x) / (s1 * s1) + (r * r) / (s2 * s2)).sum(1) + cst


def target_logp_grad(kind, A, Bh, gA, gB, grad_accumulate, params, p0, p1, p2, cst, beta,
                     beta_host, row_weight, logq0, ldj, logp_out, frow_out):
    Dh = A.shape[1]
    z = torch.cat([A, Bh], 1).detach().requires_grad_(True)
    with torch.enable_grad():
        lp = target_logp(kind, z, params, p0, p1, p2, cst)
        (g,) = torch.autograd.grad(lp.sum(), z)
    b = beta.reshape(()) if beta is not None else torch.tensor(beta_host, dtype=A.dtype,
                                                                device=A.device)
    coef = -b * row_weight
    if gA is not None:
        ga, gb = coef * g[:, :Dh], coef * g[:, Dh:]
        if grad_accumulate:
            gA.add_(ga)
            gB.add_(gb)
        else:
            gA.copy_(ga)
            gB.copy_(gb)
    lp = lp.detach()
    if logp_out is not None:
        logp_out.copy_(lp)
    if frow_out is not None:
        q = logq0 if logq0 is not None else torch.zeros_like(lp)
        l = ldj if ldj is not None else torch.zeros_like(lp)
        frow_out.copy_(q - l - b * lp)


def bernoulli_logits(logits, x, dlogits, coef, coef_host, logpx):
    l = logits.float()
    if logpx is not None:
        logpx.copy_((x * l - torch.nn.functional.softplus(l)).sum(1))
    if dlogits is not None:
        c = coef.reshape(()) if coef is not None else coef_host
        dlogits.copy_((c * (x - torch.sigmoid(l))).to(dlogits.dtype))


# ----------------------------------------------------------------- sampling
def reparam_sample(mu, logvar, seed, offset, offset_host, stream_id, z, eps, zbf, nbf, logq0,
                   generator=None):
    B, D = z.shape
    off = int(offset.item()) if offset is not None else int(offset_host)
    if generator is None:
        generator = torch.Generator(device="cpu")
        generator.manual_seed((int(seed) * 1_000_003 + off * 7919 + int(stream_id) * 104_729)
                              & 0x7FFF_FFFF_FFFF_FFFF)
    e = torch.randn(B, D, generator=generator, dtype=torch.float32).to(z.device)
    lv = logvar if logvar is not None else torch.zeros(D, device=z.device)
    m = mu if mu is not None else torch.zeros(D, device=z.device)
    zv = m + torch.exp(0.5 * lv) * e
    z.copy_(zv)
    if eps is not None:
        eps.copy_(e)
    if zbf is not None:
        zbf[:, :nbf].copy_(zv[:, :nbf].to(zbf.dtype))
        if zbf.shape[1] > nbf:
            zbf[:, nbf:].zero_()
    if logq0 is not None:
        logq0.copy_(-0.5 * D * LOG2PI - 0.5 * lv.sum() - 0.5 * (e * e).sum(1))


def reparam_grad(g_lo, g_hi, eps, logvar, partial, gmu, glv):
    g = torch.cat([g_lo, g_hi], 1)
    gmu.copy_(g.sum(0))
    glv.copy_(0.5 * torch.exp(0.5 * logvar) * (g * eps).sum(0) - 0.5)


# ----------------------------------------------------------------- optimizer
def flat_optimizer(kind, p, g, m, v, pbf, lr, b1, b2, eps, wd, step, step_host, gscale,
                   gscale_host, skip, warmup=0.0):
    if skip is not None and float(skip.reshape(())) != 0.0:
        return
    t = float(step.reshape(())) if step is not None else float(step_host)
    if warmup > 0 and t < warmup:
        lr = lr * max(t, 1.0) / warmup
    gs = float(gscale.reshape(())) if gscale is not None else float(gscale_host)
    gg = g * gs
    if kind == 0:
        m.mul_(b1).add_((1 - b1) * gg)
        v.mul_(b2).add_((1 - b2) * gg * gg)
        mh = m / (1 - b1 ** t)
        vh = v / (1 - b2 ** t)
        p.sub_(lr * (mh / (vh.sqrt() + eps) + wd * p))
    elif kind == 1:
        v.mul_(b2).add_((1 - b2) * gg * gg)
        p.sub_(lr * (gg / (v.sqrt() + eps) + wd * p))
    elif kind == 2:
        m.mul_(b1).add_(-(1 - b1) * gg)
        p.add_(lr * m - lr * wd * p)
    else:
        v.mul_(b2).add_((1 - b2) * gg * gg)
        m.mul_(b1).add_(-lr * gg / (v + eps).sqrt())
        p.add_(m - lr * wd * p)
    if pbf is not None:
        pbf.copy_(p.to(pbf.dtype))


def sumsq_guard(x, partial, out_sumsq, skip, scale, max_norm, base_scale):
    total = (x.double() ** 2).sum().float() * base_scale * base_scale
    if out_sumsq is not None:
        out_sumsq.fill_(total)
    bad = not math.isfinite(float(total))
    if skip is not None:
        skip.fill_(1.0 if bad else 0.0)
    if scale is not None:
        sc = base_scale
        if max_norm > 0 and not bad:
            nrm = math.sqrt(float(total))
            if nrm > max_norm:
                sc *= max_norm / (nrm + 1e-6)
        scale.fill_(sc)


# ---------------------------------------------------------------- MAF transform (maf.hip oracle)
def maf_fwd(x, o, bound, u, ubf, ldj, ldj_init):
    """u = (x - mu) exp(-alpha), alpha = bound tanh(s_raw / bound); ldj (+)= -sum(alpha)."""
    D = x.shape[1]
    mu, sr = o[:, :D].float(), o[:, D:2 * D].float()
    al = bound * torch.tanh(sr / bound)
    uv = (x - mu) * torch.exp(-al)
    u.copy_(uv)
    if ubf is not None:
        ubf.copy_(uv.to(ubf.dtype))
    if ldj_init:
        ldj.copy_(-al.sum(1))
    else:
        ldj.sub_(al.sum(1))


def maf_bwd(gu, u, o, bound, c_ldj, dout, gx):
    D = gu.shape[1]
    t = torch.tanh(o[:, D:2 * D].float() / bound)
    ea = torch.exp(-bound * t)
    gx.copy_(gu * ea)
    dout[:, :D].copy_((-gu * ea).to(dout.dtype))
    dout[:, D:2 * D].copy_(((c_ldj - gu * u) * (1 - t * t)).to(dout.dtype))


# ------------------------------------------- rational-quadratic spline (spline.hip oracle)
RQS_MIN = 1e-3                                   # min_w = min_h = min_d
RQS_C0 = math.log(math.expm1(1.0 - RQS_MIN))     # softplus(RQS_C0) + RQS_MIN == 1


def rqs_knots(params, K: int, bound: float):
    """Knots of the monotone rational-quadratic spline (Durkan et al. 2019) from the plane-major
    conditioner output ``params`` [B, (3K-1) Dh]: planes 0..K-1 unnormalised widths, K..2K-1
    heights, 2K..3K-2 interior derivatives. Returns ``xk, w, yk, h, d`` with knots / derivatives
    [B, K+1, Dh] and bin sizes [B, K, Dh]; the end knots are exactly -+bound, the end
    derivatives exactly 1 (linear tails), and all-zero params give the identity spline."""
    B = params.shape[0]
    if not 2 <= K <= 32 or K * RQS_MIN >= 1.0:
        raise ValueError(f"rqs: need 2 <= K <= 32, got {K}")
    if not bound > 0:
        raise ValueError(f"rqs: need bound > 0, got {bound}")
    if params.shape[1] % (3 * K - 1):
        raise ValueError(f"rqs: params width {params.shape[1]} is no multiple of 3K-1")
    p = params.reshape(B, 3 * K - 1, -1)
    lo = p.new_full((B, 1, p.shape[2]), -bound)
    one = torch.ones_like(lo)

    def bins(u):
        sz = 2.0 * bound * (RQS_MIN + (1.0 - K * RQS_MIN) * torch.softmax(u, 1))
        kn = torch.cat([lo, lo + torch.cumsum(sz, 1)[:, :-1], -lo], 1)
        return kn, sz

    xk, w = bins(p[:, :K])
    yk, h = bins(p[:, K:2 * K])
    d = torch.cat([one, RQS_MIN + torch.nn.functional.softplus(p[:, 2 * K:] + RQS_C0), one], 1)
    return xk, w, yk, h, d


def rqs_transform(params, x, K: int, bound: float, inverse: bool = False):
    """Differentiable element-wise RQ-spline transform of ``x`` [B, Dh] in the dtype of ``x``;
    returns ``(y, ldj)`` with ``ldj`` [B] the summed log-derivative of the direction taken.
    Outside (-bound, bound) it is the identity with log-derivative 0."""
    params = params.to(x.dtype)
    xk, w, yk, h, d = rqs_knots(params, K, bound)
    inside = (x > -bound) & (x < bound)
    v = x.clamp(-bound, bound)
    kn = yk if inverse else xk
    k = (v.unsqueeze(1) >= kn[:, 1:K]).sum(1, keepdim=True)     # interior knots <= v

    def at(t, i):
        return t.gather(1, i).squeeze(1)

    bx, bw, by, bh = at(xk, k), at(w, k), at(yk, k), at(h, k)
    d0, d1 = at(d, k), at(d, k + 1)
    s = bh / bw
    e = d1 + d0 - 2.0 * s
    if inverse:
        dl = v - by
        a = bh * (s - d0) + dl * e
        b = bh * d0 - dl * e
        c = -s * dl
        th = 2.0 * c / (-b - torch.sqrt((b * b - 4.0 * a * c).clamp_min(0.0)))
        out = th * bw + bx
    else:
        th = (v - bx) / bw
    t1 = th * (1.0 - th)
    den = s + e * t1
    if not inverse:
        out = by + bh * (s * th * th + d0 * t1) / den
    lg = (2.0 * torch.log(s) + torch.log(d1 * th * th + 2.0 * s * t1 + d0 * (1.0 - th) ** 2)
          - 2.0 * torch.log(den))
    if inverse:
        lg = -lg
    out = torch.where(inside, out, x)
    return out, torch.where(inside, lg, torch.zeros_like(lg)).sum(1)


# ------------------------------------------------------ deep sigmoidal flow (dsf.hip oracle)
DSF_C0 = math.log(math.e - 1.0)     # softplus(DSF_C0) == 1
DSF_BISECT = 64                     # halvings of the inverse's bracket


def dsf_units(params, H: int):
    """Units of the deep sigmoidal flow (Huang et al. 2018) from the plane-major conditioner
    output ``params`` [B, 3H D]: planes 0..H-1 raw slopes, H..2H-1 shifts, 2H..3H-1 mixture
    logits. Returns ``a, b, logw`` [B, H, D] with a = softplus(ua + c0) > 0 and
    logw = log softmax(uw); all-zero params give a = 1, b = 0, w = 1/H: the identity."""
    if not 1 <= H <= 32:
        raise ValueError(f"dsf: need 1 <= H <= 32, got {H}")
    if params.dim() != 2 or params.shape[1] % (3 * H):
        raise ValueError(f"dsf: params width {tuple(params.shape)} is no multiple of 3H")
    p = params.reshape(params.shape[0], 3 * H, -1)
    a = torch.nn.functional.softplus(p[:, :H] + DSF_C0)
    return a, p[:, H:2 * H], torch.log_softmax(p[:, 2 * H:], 1)


def _dsf_lse(t):
    """logsumexp over the units (dim 1) of [B, H, D]. The shift carries no gradient; written out
    because torch.logsumexp is slow over a short strided dimension on the CPU."""
    m = torch.nan_to_num(t.detach().amax(1, keepdim=True), nan=0.0, posinf=0.0, neginf=0.0)
    return torch.log(torch.exp(t - m).sum(1)) + m.squeeze(1)


def _dsf_eval(a, b, logw, x):
    """y = logit(sum_h w_h sigmoid(a_h x + b_h)) and log dy/dx, element-wise [B, D], in log
    space: nothing overflows and no mixture term is lost for large |x| or spread logits."""
    pj = a * x.unsqueeze(1) + b
    lsp = torch.nn.functional.logsigmoid(pj)
    lsn = torch.nn.functional.logsigmoid(-pj)
    logs = _dsf_lse(logw + lsp)
    log1ms = _dsf_lse(logw + lsn)       # sum w = 1
    L = _dsf_lse(logw + torch.log(a) + lsp + lsn) - logs - log1ms
    return logs - log1ms, L


def dsf_transform(params, x, H: int, inverse: bool = False):
    """Differentiable element-wise deep-sigmoidal-flow transform of ``x`` [B, D] in the dtype of
    ``x``; returns ``(y, ldj)`` with ``ldj`` [B] the summed log-derivative of the direction taken.

    The inverse has no closed form. y lies in [min_h p_h, max_h p_h], so the root lies in
    [min_h (y - b_h) / a_h, max_h (y - b_h) / a_h]; that bracket is bisected without a graph and
    one Newton step with a detached slope, x = x* - (f(x*, p) - y) / f'(x*), re-attaches it, so
    autograd gives the implicit-function gradients for ``params`` and ``y``; ldj = -L(x, p)."""
    a, b, logw = dsf_units(params.to(x.dtype), H)
    if not inverse:
        y, L = _dsf_eval(a, b, logw, x)
        return y, L.sum(1)
    with torch.no_grad():
        r = (x.unsqueeze(1) - b) / a
        lo, hi = r.amin(1), r.amax(1)
        for _ in range(DSF_BISECT):
            mid = 0.5 * lo + 0.5 * hi
            below = _dsf_eval(a, b, logw, mid)[0] < x
            lo = torch.where(below, mid, lo)
            hi = torch.where(below, hi, mid)
        xs = 0.5 * lo + 0.5 * hi
    f, L = _dsf_eval(a, b, logw, xs)
    out = xs - (f - x) / torch.exp(L).detach()
    return out, -_dsf_eval(a, b, logw, out)[1].sum(1)


# ------------------------------------------------- Sylvester flow stack (sylvester.hip oracle)
SYL_EPS = 1e-7        # log(|psi| + eps): the guard of the planar stack
SYL_VV_MIN = 1e-20    # v.v is clamped from below: v = 0 is the identity reflection


def tri_index(D: int, device=None):
    """Rows and columns of the strict upper part of a D x D matrix in packed order: by column,
    entry (i, j) with i < j at index j (j - 1) / 2 + i."""
    cols = torch.repeat_interleave(torch.arange(D, device=device), torch.arange(D, device=device))
    rows = torch.arange(D * (D - 1) // 2, device=device) - cols * (cols - 1) // 2
    return rows, cols


def tri_pack(R):
    """[..., D, D] -> [..., D (D - 1) / 2]: the strict upper part, packed by column."""
    rows, cols = tri_index(R.shape[-1], R.device)
    return R[..., rows, cols]


def tri_unpack(Rp, D: int):
    """[..., D (D - 1) / 2] -> [..., D, D] strictly upper triangular (differentiable)."""
    if Rp.shape[-1] != D * (D - 1) // 2:
        raise ValueError(f"tri_unpack: {Rp.shape[-1]} packed entries, D = {D} needs "
                         f"{D * (D - 1) // 2}")
    rows, cols = tri_index(D, Rp.device)
    out = Rp.new_zeros(*Rp.shape[:-1], D, D)
    out[..., rows, cols] = Rp
    return out


def householder(x, v):
    """H_v x = x - 2 v (v.x) / max(v.v, 1e-20) over the last dim; v [D] or [N, D]."""
    n = (v * v).sum(-1, keepdim=True).clamp_min(SYL_VV_MIN)
    return x - 2.0 * v * ((v * x).sum(-1, keepdim=True) / n)


def sylvester_basis_apply(x, Vk, flip: bool, transpose: bool):
    """Q x (``transpose=False``) or Q^T x for Q = P^flip H_1 ... H_H; x [N, D], Vk [H, D] or
    [N, H, D], P the coordinate reversal."""
    H = Vk.shape[-2]
    if transpose:
        if flip:
            x = x.flip(-1)
        for h in range(H):
            x = householder(x, Vk[..., h, :])
        return x
    for h in reversed(range(H)):
        x = householder(x, Vk[..., h, :])
    return x.flip(-1) if flip else x


def sylvester_stack_reference(z, R1, R2, d1, d2, b, V, flips):
    """Composite K-layer Sylvester flow stack (van den Berg et al. 2018) with M = D, in the dtype
    of ``z`` and differentiable in every tensor argument. Per layer k:

        t  = Q^T z,  Q = P^flip_k H_1 ... H_H     (Householder reflections of V[k], reversal P)
        h  = tanh(d2 * t + R2 t + b)
        z' = z + Q (d1 * h + R1 h)
        ldj += sum_i log(|1 + (1 - h_i^2) d1_i d2_i| + 1e-7)

    ``R1`` / ``R2`` are strictly upper triangular, packed by column ([.., D (D - 1) / 2],
    :func:`tri_pack`); ``d1`` / ``d2`` are the already squashed diagonals. Each parameter is
    shared ([K, ...]) or per-sample ([N, K, ...]); ``V`` is [.., K, H, D] (H may be 0);
    ``flips`` holds K truth values. Returns ``(z_K, ldj[N])``.
    """
    N, D = z.shape
    K = d1.shape[-2]
    if len(flips) != K:
        raise ValueError(f"sylvester: {len(flips)} flips for K = {K} layers")

    def layer(t, k, shared_dim):
        return t[k] if t.dim() == shared_dim else t[:, k]

    def mv(A, x):   # A [D, D] or [N, D, D], x [N, D]
        return x @ A.t() if A.dim() == 2 else torch.einsum("nij,nj->ni", A, x)

    ld = torch.zeros(N, dtype=z.dtype, device=z.device)
    for k in range(K):
        A1 = tri_unpack(layer(R1, k, 2), D)
        A2 = tri_unpack(layer(R2, k, 2), D)
        e1, e2, bk = layer(d1, k, 2), layer(d2, k, 2), layer(b, k, 2)
        Vk = layer(V, k, 3)
        flip = bool(flips[k])
        t = sylvester_basis_apply(z, Vk, flip, transpose=True)
        h = torch.tanh(e2 * t + mv(A2, t) + bk)
        y = e1 * h + mv(A1, h)
        z = z + sylvester_basis_apply(y, Vk, flip, transpose=False)
        ld = ld + torch.log(torch.abs(1.0 + (1.0 - h * h) * e1 * e2) + SYL_EPS).sum(-1)
    return z, ld


# -------------------------------------------------------------------- stein
STEIN_KINDS = {"rbf": 0, "imq": 1}


def _stein_h(h, x):
    if isinstance(h, torch.Tensor):
        return h.detach().reshape(()).to(device=x.device, dtype=x.dtype)
    return torch.tensor(float(h), device=x.device, dtype=x.dtype)


def stein_kernel_terms_reference(r2, h, kernel: str = "rbf"):
    """``(f, f', f'')`` of ``r2 = |x_i - x_j|^2`` for the two Stein kernel functions:
    ``"rbf"`` f = exp(-r2 / h), ``"imq"`` f = (h + r2)^(-1/2)."""
    if kernel == "rbf":
        f = torch.exp(-r2 / h)
        return f, -f / h, f / (h * h)
    if kernel == "imq":
        t = h + r2
        return t ** -0.5, -0.5 * t ** -1.5, 0.75 * t ** -2.5
    raise ValueError(f"stein: kernel must be rbf or imq, got {kernel!r}")


def svgd_direction_reference(x, score, h, kernel: str = "rbf", chunk: int = 1024,
                             return_abs: bool = False):
    """SVGD direction ``phi_i = (1/N) sum_j [f_ij s_j - 2 f'_ij (x_i - x_j)]`` in the dtype of
    ``x``, ``chunk`` rows i at a time (memory O(chunk N D)). ``return_abs=True`` also returns
    ``A_i = (1/N) sum_j (|f_ij s_j| + |2 f'_ij (x_i - x_j)|)``, elementwise: the scale an
    implementation's rounding error is measured against."""
    N, D = x.shape
    x, score = x.detach(), score.detach().to(x.dtype)
    hh = _stein_h(h, x)
    phi = torch.empty_like(x)
    A = torch.empty_like(x) if return_abs else None
    for i0 in range(0, N, chunk):
        i1 = min(i0 + chunk, N)
        d = x[i0:i1, None, :] - x[None, :, :]
        f, fp, _ = stein_kernel_terms_reference((d * d).sum(-1), hh, kernel)
        phi[i0:i1] = (f @ score - 2.0 * (fp[..., None] * d).sum(1)) / N
        if return_abs:
            A[i0:i1] = (f.abs() @ score.abs() + 2.0 * (fp.abs()[..., None] * d.abs()).sum(1)) / N
    return (phi, A) if return_abs else phi


def ksd_rows_reference(x, score, h, kernel: str = "imq", chunk: int = 1024,
                       return_abs: bool = False):
    """Row sums and diagonal of the Stein kernel matrix ``u_ij = f s_i.s_j + 2 f' (s_j - s_i).
    (x_i - x_j) - 2 D f' - 4 f'' r2``: ``(rows, diag)`` with ``rows[i] = sum_j u_ij`` and
    ``diag[i] = u_ii``, ``chunk`` rows at a time. ``return_abs=True`` appends ``B_i = sum_j (|f
    s_i.s_j| + |2 f' (s_j - s_i).(x_i - x_j)| + |2 D f'| + |4 f'' r2|)``."""
    N, D = x.shape
    x, score = x.detach(), score.detach().to(x.dtype)
    hh = _stein_h(h, x)
    rows = torch.empty(N, dtype=x.dtype, device=x.device)
    diag = torch.empty_like(rows)
    B = torch.empty_like(rows) if return_abs else None
    for i0 in range(0, N, chunk):
        i1 = min(i0 + chunk, N)
        d = x[i0:i1, None, :] - x[None, :, :]
        r2 = (d * d).sum(-1)
        f, fp, fpp = stein_kernel_terms_reference(r2, hh, kernel)
        t1 = f * (score[i0:i1] @ score.T)
        t2 = 2.0 * fp * ((score[None, :, :] - score[i0:i1, None, :]) * d).sum(-1)
        t3 = 2.0 * D * fp
        t4 = 4.0 * fpp * r2
        u = t1 + t2 - t3 - t4
        rows[i0:i1] = u.sum(1)
        diag[i0:i1] = u[torch.arange(i1 - i0, device=x.device),
                        torch.arange(i0, i1, device=x.device)]
        if return_abs:
            B[i0:i1] = (t1.abs() + t2.abs() + t3.abs() + t4.abs()).sum(1)
    return (rows, diag, B) if return_abs else (rows, diag)


# ---------------------------------------------------------------------- glm
GLM_FAMILIES = {"bernoulli": 0, "poisson": 1, "gaussian": 2}
GLM_CHUNK_ELEMS = 1 << 24   # elements of one [chunk, N] block of the composite


def glm_prior_prec(prior_prec, theta):
    """The prior precision as ``None`` (flat prior) or a ``[D]`` tensor like ``theta``."""
    if prior_prec is None:
        return None
    if isinstance(prior_prec, torch.Tensor):
        p = prior_prec.detach().to(device=theta.device, dtype=theta.dtype).reshape(-1)
        if p.numel() == 1:
            p = p.expand(theta.shape[1])
        if p.shape[0] != theta.shape[1]:
            raise ValueError(f"glm: prior_prec has {p.shape[0]} entries, theta has D = "
                             f"{theta.shape[1]}")
        return p
    return torch.full((theta.shape[1],), float(prior_prec), device=theta.device, dtype=theta.dtype)


def glm_terms_reference(y, eta, family: str = "bernoulli", noise_var: float = 1.0):
    """``(ll, r)`` of one GLM family at linear predictor ``eta``, without the terms of ``ll``
    that are constant in ``eta``: bernoulli ``y eta - softplus(eta)``, ``y - sigmoid(eta)``;
    poisson ``y eta - exp(eta)``, ``y - exp(eta)``; gaussian ``-(y - eta)^2 / (2 noise_var)``,
    ``(y - eta) / noise_var``."""
    if family == "bernoulli":
        ll = y * eta - eta.clamp_min(0) - torch.log1p(torch.exp(-eta.abs()))
        return ll, y - torch.sigmoid(eta)
    if family == "poisson":
        ex = torch.exp(eta)
        return y * eta - ex, y - ex
    if family == "gaussian":
        d = y - eta
        return -0.5 * d * d / noise_var, d / noise_var
    raise ValueError(f"glm: family must be one of {sorted(GLM_FAMILIES)}, got {family!r}")


def glm_likelihood_const(y, family: str = "bernoulli", noise_var: float = 1.0) -> float:
    """The part of ``sum_n log p(y_n | eta_n)`` that does not depend on ``eta``, as a float
    (fp64): poisson ``-sum lgamma(y + 1)``, gaussian ``-0.5 N log(2 pi noise_var)``, bernoulli 0."""
    if family == "poisson":
        return -float(torch.lgamma(y.detach().double() + 1.0).sum())
    if family == "gaussian":
        return -0.5 * y.numel() * math.log(2 * math.pi * noise_var)
    if family == "bernoulli":
        return 0.0
    raise ValueError(f"glm: family must be one of {sorted(GLM_FAMILIES)}, got {family!r}")


def glm_logp_grad_reference(theta, X, y, family: str = "bernoulli", prior_prec=1.0,
                            noise_var: float = 1.0, scale: float = 1.0, chunk: int | None = None,
                            return_abs: bool = False):
    """``(logp [B], grad [B, D])`` of ``B`` parameter rows of a GLM posterior in the dtype of
    ``theta``, ``chunk`` rows at a time (memory O(chunk N)):

        logp_i = scale sum_n ll(y_n, theta_i . x_n) + log prior(theta_i)
        grad_i = scale sum_n r(y_n, theta_i . x_n) x_n - prec theta_i

    with ``ll`` and ``r`` of :func:`glm_terms_reference` and the prior ``N(0, diag(1 / prec))``,
    ``log prior = -0.5 sum prec_c theta_c^2 + 0.5 sum log prec_c - D/2 log 2 pi`` over the
    coordinates with ``prec_c > 0`` (``prec_c = 0``: flat in that coordinate; ``prior_prec=None``:
    no prior at all). ``return_abs=True`` appends ``A_i = scale sum_n |ll_in| + |log prior_i|``
    and ``G_ic = scale sum_n |r_in x_nc| + |prec_c theta_ic|``: the scales an implementation's
    rounding error is measured against."""
    theta = theta.detach()
    X, y = X.detach().to(theta.dtype), y.detach().to(theta.dtype).reshape(-1)
    B, D = theta.shape
    N = X.shape[0]
    if X.shape[1] != D or y.shape[0] != N:
        raise ValueError(f"glm: theta {tuple(theta.shape)}, X {tuple(X.shape)} and y "
                         f"{tuple(y.shape)} do not fit together ([B, D], [N, D], [N])")
    if not scale > 0 or not noise_var > 0:
        raise ValueError(f"glm: scale and noise_var must be positive, got {scale} and {noise_var}")
    prec = glm_prior_prec(prior_prec, theta)
    chunk = chunk or max(1, GLM_CHUNK_ELEMS // max(N, 1))
    logp = torch.empty(B, dtype=theta.dtype, device=theta.device)
    grad = torch.empty_like(theta, memory_format=torch.contiguous_format)
    A = torch.empty_like(logp) if return_abs else None
    G = torch.empty_like(grad) if return_abs else None
    if prec is not None:
        on = prec > 0
        cst = 0.5 * torch.log(prec[on]).sum() - 0.5 * int(on.sum()) * math.log(2 * math.pi)
    Xa = X.abs() if return_abs else None
    for i0 in range(0, B, chunk):
        th = theta[i0:i0 + chunk]
        ll, r = glm_terms_reference(y[None, :], th @ X.T, family, noise_var)
        lp, g = scale * ll.sum(1), scale * (r @ X)
        if prec is not None:
            prior = -0.5 * (prec * th * th).sum(1) + cst
            lp, g = lp + prior, g - prec * th
        logp[i0:i0 + chunk], grad[i0:i0 + chunk] = lp, g
        if return_abs:
            A[i0:i0 + chunk] = scale * ll.abs().sum(1)
            G[i0:i0 + chunk] = scale * (r.abs() @ Xa)
            if prec is not None:
                A[i0:i0 + chunk] += prior.abs()
                G[i0:i0 + chunk] += (prec * th).abs()
    return (logp, grad, A, G) if return_abs else (logp, grad)


def glm_weights_reference(eta, family: str = "bernoulli", noise_var: float = 1.0):
    """``w = -d r / d eta`` of one GLM family, the weight of a data row in the negative Hessian:
    bernoulli ``sigmoid(eta) (1 - sigmoid(eta))`` (as ``e / (1 + e)^2`` with ``e = exp(-|eta|)``,
    which only underflows), poisson ``exp(eta)``, gaussian ``1 / noise_var``."""
    if family == "bernoulli":
        e = torch.exp(-eta.abs())
        return e / ((1 + e) * (1 + e))
    if family == "poisson":
        return torch.exp(eta)
    if family == "gaussian":
        return torch.full_like(eta, 1.0 / noise_var)
    raise ValueError(f"glm: family must be one of {sorted(GLM_FAMILIES)}, got {family!r}")


def glm_hessian_reference(theta, X, y, family: str = "bernoulli", prior_prec=1.0,
                          noise_var: float = 1.0, scale: float = 1.0, return_abs: bool = False,
                          chunk: int | None = None):
    """``(logp [B], grad [B, D], H [B, D, D])`` of ``B`` parameter rows of a GLM posterior in the
    dtype of ``theta``: ``logp`` and ``grad`` of :func:`glm_logp_grad_reference` and the negative
    Hessian of ``logp``

        H_b = scale sum_n w(theta_b . x_n) x_n x_n^T + diag(prec)

    with ``w`` of :func:`glm_weights_reference`, ``chunk`` rows at a time so that the ``[chunk,
    N, D]`` block of weighted data stays within ``GLM_CHUNK_ELEMS``. ``return_abs=True`` appends
    ``A``, ``G`` (of :func:`glm_logp_grad_reference`) and ``W_bjk = scale sum_n |w x_nj x_nk| +
    prec_j delta_jk``."""
    out = glm_logp_grad_reference(theta, X, y, family, prior_prec, noise_var, scale,
                                  return_abs=return_abs)
    theta = theta.detach()
    X = X.detach().to(theta.dtype)
    B, D = theta.shape
    N = X.shape[0]
    prec = glm_prior_prec(prior_prec, theta)
    chunk = chunk or max(1, GLM_CHUNK_ELEMS // max(N * D, 1))
    H = torch.empty(B, D, D, dtype=theta.dtype, device=theta.device)
    W = torch.empty_like(H) if return_abs else None
    Xa = X.abs() if return_abs else None
    for i0 in range(0, B, chunk):
        w = glm_weights_reference(theta[i0:i0 + chunk] @ X.T, family, noise_var)
        H[i0:i0 + chunk] = scale * ((w[:, :, None] * X).mT @ X)
        if return_abs:
            W[i0:i0 + chunk] = scale * ((w.abs()[:, :, None] * Xa).mT @ Xa)
    if prec is not None:
        H.diagonal(dim1=1, dim2=2).add_(prec)
        if return_abs:
            W.diagonal(dim1=1, dim2=2).add_(prec.abs())
    return (out[0], out[1], H, out[2], out[3], W) if return_abs else (out[0], out[1], H)
