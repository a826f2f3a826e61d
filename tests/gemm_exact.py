"""Exact-operand oracle for the MFMA GEMM family.

Operands are small integers times a power of two (bf16: integers in [-7, 7], e4m3: [-8, 8];
fp32 addends on the product's grid). Every product and every partial sum is then an integer
below 2^24 in units of the grid, i.e. exactly representable in fp32: the accumulator is exact
for any K order, split-K, MFMA shape or tile schedule, and a kernel's output must equal the
mathematically exact value after ONE correctly rounded store. The tests built on this compare
bit patterns: no tolerance, no normalisation, no dependence on how another kernel rounds.

The reference is an fp64 torch product on the CPU (exact: every partial sum is far below
2^53), the epilogue in exact arithmetic, then one conversion (`.float()` /
`.float().to(torch.bfloat16)` / `.to(torch.float8_e4m3fn)`).
"""
from __future__ import annotations

import torch

BF16_INT = 7            # bf16 operand integers in [-7, 7]
E4M3_INT = 8            # e4m3 operand integers in [-8, 8]
EXACT = 1 << 24         # integers below this are exact in fp32
ZERO_SHARE = 0.25       # fixed share of zero entries (non-trivial ReLU masks / bitmasks)
CANARY = 0x5A           # byte pattern around output views
E4M3_NAN = 0x7F         # float8_e4m3fn NaN code


class Exact:
    """An operand: `i` int64 integers (CPU), `shift` (value = i * 2**-shift), `t` the tensor in
    its storage dtype (CPU), `d` the value in fp64."""

    def __init__(self, i: torch.Tensor, shift: int, dtype: torch.dtype):
        self.i = i
        self.shift = shift
        self.d = i.double() * 2.0 ** -shift
        self.t = self.d.float().to(dtype)
        # the storage dtype holds the value exactly
        assert torch.equal(self.t.double(), self.d), "operand not representable in its dtype"

    def to(self, device):
        return self.t.to(device)


def _ints(shape, bound: int, seed: int, zero_share: float = ZERO_SHARE) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    i = torch.randint(-bound, bound + 1, tuple(shape), generator=g, dtype=torch.int64)
    if zero_share > 0:
        i = i * (torch.rand(tuple(shape), generator=g) >= zero_share)
    return i


def gen_bf16(shape, seed: int, shift: int = 0, zero_share: float = ZERO_SHARE) -> Exact:
    return Exact(_ints(shape, BF16_INT, seed, zero_share), shift, torch.bfloat16)


def gen_e4m3(shape, seed: int, shift: int = 0, zero_share: float = ZERO_SHARE) -> Exact:
    return Exact(_ints(shape, E4M3_INT, seed, zero_share), shift, torch.float8_e4m3fn)


def gen_grid(shape, seed: int, shift: int, bound: int, dtype=torch.float32,
             zero_share: float = ZERO_SHARE) -> Exact:
    """An addend (accumulate base, G, bias) on the grid 2**-shift with |integer| <= bound."""
    return Exact(_ints(shape, bound, seed, zero_share), shift, dtype)


def assert_exact_bound(a: Exact, b_t: Exact, *addends: Exact) -> int:
    """max over outputs of sum_k |a_mk| |b_kn| (+ |addend|), in units of the product grid
    2**-(a.shift + b.shift), must stay below 2^24: the condition under which fp32 accumulation
    is exact in any order. a: [M, K], b_t: [K, N]; addends broadcast against [M, N] and lie
    on the product grid or a coarser one. Returns that maximum."""
    s = a.shift + b_t.shift
    # fp64 holds these integer sums exactly (< 2^53)
    mag = a.i.abs().double() @ b_t.i.abs().double()
    for e in addends:
        assert e.shift <= s, "addend finer than the product grid"
        mag = mag + e.i.abs().double() * 2.0 ** (s - e.shift)
    worst = int(mag.max().item()) if mag.numel() else 0
    assert worst < EXACT, f"sum |a||b| = {worst} >= 2^24: fp32 accumulation is not exact"
    return worst


def product(a: Exact, b_t: Exact) -> torch.Tensor:
    """Exact a @ b_t in fp64 (CPU)."""
    return a.d @ b_t.d


def to_f32(x64: torch.Tensor) -> torch.Tensor:
    y = x64.float()
    assert torch.equal(y.double(), x64), "reference not exact in fp32"
    return y


def to_bf16(x64: torch.Tensor) -> torch.Tensor:
    """The one correctly rounded (nearest-even) bf16 store of an exact fp32 value."""
    return to_f32(x64).to(torch.bfloat16)


def to_e4m3(x64: torch.Tensor) -> torch.Tensor:
    """e4m3 copy: saturate at +-448, then torch's round-to-nearest-even conversion."""
    return x64.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn)


def pack_bits(pos: torch.Tensor) -> torch.Tensor:
    """[M, N] bool -> [M, N/8] uint8, bit e of byte j <-> column 8 j + e."""
    M, N = pos.shape
    w = 2 ** torch.arange(8, dtype=torch.int32, device=pos.device)
    return (pos.view(M, N // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)


# ------------------------------------------------------------------------------- views
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _ld_unit(dtype: torch.dtype) -> int:
    """Elements per 16 bytes: leading dimensions and offsets in these units keep every row
    16-B aligned (chk_mat: bf16 ld % 8; chk_q: e4m3 ld % 16; fp32 ld % 4 for staged_ok)."""
    return 16 // torch.empty((), dtype=dtype).element_size()


def _fill_nan(t: torch.Tensor) -> None:
    if t.dtype == torch.float8_e4m3fn or t.dtype == torch.uint8:
        t.view(torch.uint8).fill_(E4M3_NAN if t.dtype != torch.uint8 else 0xFF)
    else:
        t.fill_(float("nan"))


def place_operand(t: torch.Tensor, device, row_off: int = 3, col_off: int = 1, pad: int = 1):
    """`t` as a view inside a larger buffer: non-zero row offset, column offset of `col_off`
    16-B units, leading dimension `pad` units wider than needed; everything around it is NaN
    (e4m3: the NaN code), so a kernel that reads outside the operand poisons its output."""
    R, C = t.shape
    u = _ld_unit(t.dtype)
    c0 = col_off * u
    ld = (c0 + C + u - 1) // u * u + pad * u
    buf = torch.empty(R + row_off + 2, ld, dtype=t.dtype, device=device)
    _fill_nan(buf)
    view = buf[row_off:row_off + R, c0:c0 + C]
    view.copy_(t.to(device))
    return view


def place_output(shape, dtype: torch.dtype, device, init: torch.Tensor | None = None,
                 row_off: int = 2, col_off: int = 1, pad: int = 1, fill: int | None = None):
    """An output view inside a larger buffer whose surroundings hold the CANARY byte pattern.
    The view is pre-filled with NaN (uint8: `fill`, default 0xFF) unless `init` (the base of an
    accumulating op) is given. Returns (buffer, view)."""
    R, C = shape
    u = _ld_unit(dtype)
    c0 = col_off * u
    ld = (c0 + C + u - 1) // u * u + pad * u
    buf = torch.empty(R + row_off + 2, ld, dtype=dtype, device=device)
    buf.view(torch.uint8).fill_(CANARY)
    view = buf[row_off:row_off + R, c0:c0 + C]
    if init is not None:
        view.copy_(init.to(device))
    elif fill is not None:
        view.view(torch.uint8).fill_(fill) if dtype != torch.uint8 else view.fill_(fill)
    else:
        _fill_nan(view)
    return buf, view


def place_vector(n: int, dtype: torch.dtype, device, init: torch.Tensor | None = None):
    """A contiguous, 16-B aligned [n] output inside a canary buffer. Returns (buffer, view)."""
    u = _ld_unit(dtype)
    buf = torch.empty(n + 2 * u, dtype=dtype, device=device)
    buf.view(torch.uint8).fill_(CANARY)
    view = buf[u:u + n]
    if init is not None:
        view.copy_(init.to(device))
    else:
        _fill_nan(view)
    return buf, view


def assert_canary(buffer: torch.Tensor, view: torch.Tensor, what: str = "") -> None:
    """Every byte of `buffer` outside `view` still holds the CANARY pattern."""
    es = buffer.element_size()
    raw = buffer.detach().cpu().contiguous().view(torch.uint8).reshape(-1).clone()
    off = (view.data_ptr() - buffer.data_ptr())
    assert off >= 0 and off % es == 0
    if view.dim() == 1:
        inside = off + torch.arange(view.shape[0] * es)
    else:
        rows = torch.arange(view.shape[0]) * view.stride(0) * es
        inside = (off + rows[:, None] + torch.arange(view.shape[1] * es)[None, :]).reshape(-1)
    raw[inside] = CANARY
    bad = (raw != CANARY).nonzero().reshape(-1)
    if bad.numel():
        ldb = (buffer.stride(0) if buffer.dim() == 2 else buffer.numel()) * es
        where = [(int(b) // ldb, int(b) % ldb // es) for b in bad[:8]]
        raise AssertionError(f"{what}: {bad.numel()} byte(s) outside the output view changed; "
                             f"first (buffer row, buffer column): {where}")


def assert_exact(out: torch.Tensor, ref: torch.Tensor, what: str = "") -> None:
    """Bit patterns of `out` and `ref` (same dtype and shape) are equal. On failure: how many
    elements differ, the first few (row, column, got, want), and the 256x256 tile, 128x128 tile
    and 16-column group each falls in."""
    out = out.detach().cpu()
    ref = ref.detach().cpu()
    assert out.dtype == ref.dtype, (what, out.dtype, ref.dtype)
    assert out.shape == ref.shape, (what, tuple(out.shape), tuple(ref.shape))
    iv = _INT_VIEW[out.element_size()]
    o = out.contiguous().view(iv)
    r = ref.contiguous().view(iv)
    if torch.equal(o, r):
        return
    if o.dim() == 1:
        o, r, out, ref = o[None], r[None], out[None], ref[None]
    bad = (o != r).nonzero()
    lines = []
    as_num = (lambda t, i, j: int(t[i, j])) if out.dtype == torch.uint8 else \
        (lambda t, i, j: float(t[i, j].float()))
    for i, j in bad[:6].tolist():
        lines.append(f"  ({i}, {j}): got {as_num(out, i, j)!r} [{int(o[i, j]) & 0xffffffff:#x}] "
                     f"want {as_num(ref, i, j)!r} [{int(r[i, j]) & 0xffffffff:#x}]  "
                     f"tile256 ({i // 256}, {j // 256}) tile128 ({i // 128}, {j // 128}) "
                     f"colgroup16 {j // 16}")
    t256 = sorted({(i // 256, j // 256) for i, j in bad.tolist()})[:8]
    nan = int(torch.isnan(out.float()).sum()) if out.dtype != torch.uint8 else 0
    raise AssertionError(f"{what}: {bad.shape[0]} of {o.numel()} elements differ bitwise "
                         f"({nan} NaN in the output); 256x256 tiles hit: {t256}\n" + "\n".join(lines))
