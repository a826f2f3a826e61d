"""Every MFMA GEMM product, bitwise, at the smallest shapes that reach each dispatch state.

Operands are small integers times a power of two (tests/gemm_exact.py), so the fp32 accumulator
is exact in any K order and every output must equal the exact value after one correctly rounded
store. Each case demands: outputs bitwise equal to the fp64-derived reference, the canary bytes
around every strided output untouched, no NaN from the poisoned surroundings of the strided
operands, and the same bits again on a second launch into a fresh NaN-filled output.

The fused coupling / MAF epilogues (section "fused epilogues") start from values that are known
bit for bit; their stored s_hat / s_raw, zero pads and bf16 / e4m3 copies are checked bitwise,
and their transform outputs per element against the fp64 formulas under the one measured bound
of this module (CPL_MULT, docs/PERF_NOTES.md "Exact-operand GEMM oracle").
"""
import functools
import itertools

import pytest
import torch

import gemm_exact as gx
from vi_normflows_amd.flows.made import made_degrees, made_masks
from vi_normflows_amd.ops.masked import MaskPlan, tile_ranges

pytestmark = pytest.mark.gpu

BF, F32, U8, F8 = torch.bfloat16, torch.float32, torch.uint8, torch.float8_e4m3fn
SWITCHES = ("gemm_set_mode", "gemm_persist", "gemm_grid_reserve", "gemm_pair",
            "gemm_wgrad_xcd_pack", "gemm_cpl4w")


@pytest.fixture
def ops(gpu):
    """torch.ops.vinf with every process-global GEMM switch saved by its query form and
    restored afterwards, so no later test sees a setting of this module."""
    o = torch.ops.vinf
    saved = [(n, getattr(o, n)(-1)) for n in SWITCHES]
    try:
        yield o
    finally:
        for n, v in saved:
            getattr(o, n)(v)
        assert [getattr(o, n)(-1) for n, _ in saved] == [v for _, v in saved]


def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


# name -> (gemm_set_mode, gemm_persist, grid): grid "8" = a reserve of every CU (the launcher
# keeps 8 blocks), "16" = CUs - 16 reserved, "all" = nothing reserved
STATES = {"t128": (1, None, None), "t256": (2, 0, "all"), "fix8": (2, 1, "8"), "fix16": (2, 1, "16"),
          "fix": (2, 1, "all"), "dyn8": (2, 2, "8"), "dyn16": (2, 2, "16"), "dyn": (2, 2, "all")}
PERSISTENT = ("fix8", "fix16", "fix", "dyn8", "dyn16", "dyn")


def set_state(o, name):
    mode, persist, grid = STATES[name]
    o.gemm_set_mode(mode)
    if persist is not None:
        o.gemm_persist(persist)
        o.gemm_grid_reserve({"8": _cus(), "16": _cus() - 16, "all": 0}[grid])


def transposed(e: gx.Exact) -> gx.Exact:
    return gx.Exact(e.i.t().contiguous(), e.shift, e.t.dtype)


def twice(run):
    """The four demands hold on a first launch and again on a second one into fresh outputs."""
    for rep in range(2):
        run(rep)


# ------------------------------------------------------------------ forward products (NT)
@functools.lru_cache(maxsize=None)
def nt_data(M, N, K):
    x = gx.gen_bf16((M, K), seed=1000 + M + 3 * K, shift=1)
    w = gx.gen_bf16((N, K), seed=2000 + N + 5 * K, shift=2)
    b = gx.gen_grid((N,), seed=3000 + N, shift=1, bound=255, dtype=BF)
    gx.assert_exact_bound(x, transposed(w), b)
    return x, w, b, gx.product(x, transposed(w))


def check_nt(o, dev, M, N, K, bias, relu, mask, tag=""):
    x, w, b, p = nt_data(M, N, K)
    r = p + b.d if bias else p
    r = r.clamp_min(0) if relu else r
    ref = gx.to_bf16(r)
    xv, wv = gx.place_operand(x.t, dev), gx.place_operand(w.t, dev)
    bd = b.to(dev) if bias else None
    what = f"gemm_nt {tag} M{M} N{N} K{K} bias{bias} relu{relu}"

    def run(rep):
        yb, y = gx.place_output((M, N), BF, dev)
        mb = m = None
        if mask:
            mb, m = gx.place_output((M, N // 8), U8, dev, fill=0x00 if rep else 0xFF)
        o.gemm_nt(xv, wv, bd, y, relu, m)
        gx.assert_exact(y, ref, f"{what} y rep{rep}")
        gx.assert_canary(yb, y, what)
        if mask:
            gx.assert_exact(m, gx.pack_bits(ref > 0), f"{what} bitmask rep{rep}")
            gx.assert_canary(mb, m, what + " bitmask")
    twice(run)


NT_VARIANTS = [(1, 1, 1), (1, 1, 0), (0, 0, 0), (1, 0, 0), (0, 1, 1)]   # bias, relu, bitmask

T128 = list(itertools.product([1, 127, 129, 300], [8, 136, 264], [32, 64, 96, 320]))
T256 = list(itertools.product([1, 255, 257, 520], [8, 136, 264, 520], [64, 96, 160, 320, 416]))


@pytest.mark.parametrize("M,N,K", T128)
def test_nt_t128(ops, gpu, M, N, K):
    set_state(ops, "t128")
    for bias, relu, mask in NT_VARIANTS:
        check_nt(ops, gpu, M, N, K, bias, relu, mask, "t128")
    x, w, _, p = nt_data(M, N, K)
    xv, wv = gx.place_operand(x.t, gpu), gx.place_operand(w.t, gpu)

    def run(rep):
        yb, y = gx.place_output((M, N), F32, gpu)
        ops.gemm_nt_f32out(xv, wv, y)
        gx.assert_exact(y, gx.to_f32(p), f"gemm_nt_f32out M{M} N{N} K{K} rep{rep}")
        gx.assert_canary(yb, y, "gemm_nt_f32out")
    twice(run)


@pytest.mark.parametrize("M,N,K", T256)
def test_nt_t256(ops, gpu, M, N, K):
    set_state(ops, "t256")
    for bias, relu, mask in NT_VARIANTS:
        check_nt(ops, gpu, M, N, K, bias, relu, mask, "t256")


# Persistent grids made small with gemm_grid_reserve. With 8 blocks: 1 x 520 is 3 tiles (fewer
# tiles than blocks, not a multiple of 8: xcd_remap's remainder), 1324 x 520 is 18 tiles
# (uneven lists), 2048 x 264 is 16 (equal lists, column rotation off: (16 >> 3) % 2 == 0 but
# (8 >> 3) % 2 != 0). With 16 blocks: 4096 x 264 is 32 tiles and meets all four rotation
# conditions. K = 96 / 416 end in a 32-deep tail; K = 128 is two K-tiles, the shortest tile the
# tile-boundary burst can meet.
PERSIST_SHAPES = [(1, 520, 96), (300, 520, 128), (1324, 520, 416), (1324, 520, 128),
                  (2048, 264, 96), (4096, 264, 128), (4096, 264, 96)]


@pytest.mark.parametrize("state", PERSISTENT)
@pytest.mark.parametrize("M,N,K", PERSIST_SHAPES)
def test_nt_persistent(ops, gpu, state, M, N, K):
    set_state(ops, state)
    check_nt(ops, gpu, M, N, K, 1, 1, 1, state)
    check_nt(ops, gpu, M, N, K, 0, 0, 0, state)


# -------------------------------------------------------------- input gradients (NN / Wt)
@functools.lru_cache(maxsize=None)
def nn_data(M, N, K):
    dy = gx.gen_bf16((M, K), seed=4000 + M + 3 * K, shift=2)
    w = gx.gen_bf16((K, N), seed=5000 + N + 5 * K, shift=1)
    h = gx.gen_bf16((M, N), seed=6000 + M + N, shift=0, zero_share=0.3)
    base = gx.gen_grid((M, N), seed=7000 + M + N, shift=3, bound=4000, dtype=F32)
    gx.assert_exact_bound(dy, w, base)
    return dy, w, h, base, gx.product(dy, w)


def check_nn(o, dev, M, N, K, tag, with_wt):
    dy, w, h, base, p = nn_data(M, N, K)
    dyv, wv, hv = (gx.place_operand(t.t, dev) for t in (dy, w, h))
    wtv = gx.place_operand(transposed(w).t, dev)
    keep = h.d > 0
    bits = gx.place_operand(gx.pack_bits(keep), dev)
    zero = torch.zeros((), dtype=torch.float64)
    ref_plain, ref_mask = gx.to_bf16(p), gx.to_bf16(torch.where(keep, p, zero))
    what = f"gemm_nn {tag} M{M} N{N} K{K}"

    def run(rep):
        for name, ref, kw in (("plain", ref_plain, {}), ("h", ref_mask, {"h": hv}),
                              ("hbits", ref_mask, {"hbits": bits})):
            for wt in ((None, wtv) if with_wt else (None,)):
                ob, out = gx.place_output((M, N), BF, dev)
                o.gemm_nn(dyv, wv, kw.get("h"), out, False, kw.get("hbits"), wt)
                w_ = f"{what} {name}{' Wt' if wt is not None else ''} rep{rep}"
                gx.assert_exact(out, ref, w_)
                gx.assert_canary(ob, out, w_)
        ob, out = gx.place_output((M, N), F32, dev)
        o.gemm_nn(dyv, wv, None, out, False)
        gx.assert_exact(out, gx.to_f32(p), f"{what} f32 rep{rep}")
        gx.assert_canary(ob, out, what)
        ob, out = gx.place_output((M, N), F32, dev, init=base.t)
        o.gemm_nn(dyv, wv, None, out, True)
        gx.assert_exact(out, gx.to_f32(p + base.d), f"{what} f32 accumulate rep{rep}")
        gx.assert_canary(ob, out, what)
    twice(run)


@pytest.mark.parametrize("M,N,K", T128)
def test_nn_t128(ops, gpu, M, N, K):
    set_state(ops, "t128")
    check_nn(ops, gpu, M, N, K, "t128", with_wt=False)


@pytest.mark.parametrize("M,N,K", T256)
def test_nn_t256(ops, gpu, M, N, K):
    set_state(ops, "t256")
    check_nn(ops, gpu, M, N, K, "t256", with_wt=True)


@pytest.mark.parametrize("state", PERSISTENT)
@pytest.mark.parametrize("M,N,K", PERSIST_SHAPES)
def test_nn_persistent(ops, gpu, state, M, N, K):
    set_state(ops, state)
    check_nn(ops, gpu, M, N, K, state, with_wt=True)


# ----------------------------------------------------------------------- weight gradients
@functools.lru_cache(maxsize=None)
def tn_data(K, M, N, seed=0):
    dy = gx.gen_bf16((K, M), seed=8000 + K + M + seed, shift=1)
    x = gx.gen_bf16((K, N), seed=9000 + K + N + seed, shift=2)
    gx.assert_exact_bound(transposed(dy), x)
    return dy, x, gx.product(transposed(dy), x), dy.d.sum(0)


# K = 2080: 65 / 33 K-tiles, the split-K slabs and the reduce launch (mode 0: up to 16 splits,
# mode 3: 8); K = 416 and 96 end in a 32-deep tail
TN_SHAPES = [(32, 8, 8), (64, 264, 136), (96, 136, 264), (320, 520, 264), (416, 304, 520),
             (2080, 520, 264)]


@pytest.mark.parametrize("mode", [0, 3], ids=["auto", "t256"])
@pytest.mark.parametrize("K,M,N", TN_SHAPES)
def test_tn(ops, gpu, mode, K, M, N):
    ops.gemm_set_mode(mode)
    dy, x, p, colsum = tn_data(K, M, N)
    dyv, xv = gx.place_operand(dy.t, gpu), gx.place_operand(x.t, gpu)

    def run(rep):
        for with_db in (True, False):
            wb, dW = gx.place_output((M, N), F32, gpu)
            bb, db = gx.place_vector(M, F32, gpu) if with_db else (None, None)
            ops.gemm_tn(dyv, xv, dW, db)
            what = f"gemm_tn mode{mode} K{K} M{M} N{N} db{with_db} rep{rep}"
            gx.assert_exact(dW, gx.to_f32(p), what)
            gx.assert_canary(wb, dW, what)
            if with_db:
                gx.assert_exact(db, gx.to_f32(colsum), what + " db")
                gx.assert_canary(bb, db, what + " db")
    twice(run)


GROUP = [(264, 136), (136, 264), (520, 40)]


def _cmask(M, N, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(M, N, generator=g) < 0.6).to(U8)


def _skip128(M, N):
    """Skip flags per 128x128 tile: every second tile off the first tile column."""
    tm, tn = (M + 127) // 128, (N + 127) // 128
    return torch.tensor([[int((i + j) % 2 == 1) for j in range(tn)] for i in range(tm)], dtype=U8)


def _skip_ref(p, skip, has_db):
    """Skipped 128x128 tiles read exactly zero, except the first tile column when the bias
    gradient is computed from it."""
    r = p.clone()
    for i in range(skip.shape[0]):
        for j in range(skip.shape[1]):
            if skip[i, j] and not (has_db and j == 0):
                r[128 * i:128 * i + 128, 128 * j:128 * j + 128] = 0
    return r


@pytest.mark.parametrize("mode", [0, 3], ids=["auto", "t256"])
@pytest.mark.parametrize("B", [96, 416, 2080])
@pytest.mark.parametrize("masked", [False, True], ids=["dense", "skip_cmask"])
def test_tn_group(ops, gpu, mode, B, masked):
    ops.gemm_set_mode(mode)
    data = [tn_data(B, M, N, seed=p) for p, (M, N) in enumerate(GROUP)]
    dys = [gx.place_operand(d[0].t, gpu) for d in data]
    xs = [gx.place_operand(d[1].t, gpu) for d in data]
    has_db = [True, False, True]
    skips = [_skip128(*GROUP[0]), None, None] if masked else []
    cms = [None, _cmask(*GROUP[1], seed=5), None] if masked else []

    def run(rep):
        outs = [gx.place_output(s, F32, gpu, col_off=0, pad=0) for s in GROUP]   # dense dW (cmask)
        dbs = [gx.place_vector(s[0], F32, gpu) if has_db[p] else (None, None)
               for p, s in enumerate(GROUP)]
        ops.gemm_tn_group(dys, xs, [v for _, v in outs], [v for _, v in dbs],
                          [None if s is None else s.reshape(-1).to(gpu) for s in skips],
                          [None if c is None else c.to(gpu) for c in cms])
        for p, (M, N) in enumerate(GROUP):
            ref = data[p][2]
            if masked and skips[p] is not None:
                ref = _skip_ref(ref, skips[p], has_db[p])
            if masked and cms[p] is not None:
                ref = torch.where(cms[p] != 0, ref, torch.zeros((), dtype=torch.float64))
            what = f"gemm_tn_group mode{mode} B{B} masked{masked} problem {p} rep{rep}"
            gx.assert_exact(outs[p][1], gx.to_f32(ref), what)
            gx.assert_canary(*outs[p], what)
            if has_db[p]:
                gx.assert_exact(dbs[p][1], gx.to_f32(data[p][3]), what + " db")
                gx.assert_canary(*dbs[p], what + " db")
    twice(run)


MULTI = [(264, 520), (520, 264), (136, 40), (520, 520)]      # 6 + 6 + 1 + 9 = 22 tiles
ACTIVE1 = [0, 2, 3, 5]                                       # of problem 1's 3 x 2 tiles
# partitions of the 6 + 4 + 1 + 9 = 20 tiles left with problem 1's active-tile list
PARTITIONS = {"one": [(0, 20)], "per_problem": [(0, 6), (6, 10), (10, 11), (11, 20)],
              "inside": [(0, 1), (1, 8), (8, 15), (15, 20)]}


def _tiles_ref(p, tiles, M, N):
    """Only the listed 256x256 tiles are computed; the others keep their NaN pre-fill."""
    tn = (N + 255) // 256
    r = torch.full_like(p, float("nan"))
    for t in tiles:
        i, j = t // tn, t % tn
        r[256 * i:256 * i + 256, 256 * j:256 * j + 256] = p[256 * i:256 * i + 256, 256 * j:256 * j + 256]
    return r


@pytest.mark.parametrize("pack", [0, 1], ids=["nopack", "xcdpack"])
@pytest.mark.parametrize("B", [96, 128, 416])
@pytest.mark.parametrize("part", list(PARTITIONS))
def test_tn_multi_partitions(ops, gpu, pack, B, part):
    """WgradPlan / gemm_tn_multi over partitions of the global tile range, one problem with an
    active-tile list and a cmask (its other tiles are never written)."""
    from vi_normflows_amd.ops.gemm import WgradPlan

    ops.gemm_wgrad_xcd_pack(pack)
    data = [tn_data(B, M, N, seed=10 + p) for p, (M, N) in enumerate(MULTI)]
    dys = [gx.place_operand(d[0].t, gpu) for d in data]
    xs = [gx.place_operand(d[1].t, gpu) for d in data]
    act, total, ranges = ACTIVE1, 20, PARTITIONS[part]
    cm = _cmask(*MULTI[1], seed=6)

    def run(rep):
        outs = [gx.place_output(s, F32, gpu, col_off=0 if p == 1 else 1, pad=0 if p == 1 else 1)
                for p, s in enumerate(MULTI)]
        dbs = [gx.place_vector(s[0], F32, gpu) if p % 2 == 0 else (None, None)
               for p, s in enumerate(MULTI)]
        items = [(dys[p], xs[p], outs[p][1], dbs[p][1]) for p in range(4)]
        items[1] = items[1] + (torch.tensor(act, dtype=torch.int16, device=gpu), cm.to(gpu))
        plan = WgradPlan(items)
        assert plan.total == total
        for a, b in ranges:
            plan.run(a, b - a)
        for p, (M, N) in enumerate(MULTI):
            ref = data[p][2]
            if p == 1:
                ref = torch.where(cm != 0, ref, torch.zeros((), dtype=torch.float64))
                ref = _tiles_ref(ref, act, M, N)
            what = f"gemm_tn_multi pack{pack} B{B} {part} problem {p} rep{rep}"
            gx.assert_exact(outs[p][1], ref.float(), what)
            gx.assert_canary(*outs[p], what)
            if dbs[p][1] is not None:
                gx.assert_exact(dbs[p][1], gx.to_f32(data[p][3]), what + " db")
                gx.assert_canary(*dbs[p], what + " db")
    twice(run)


@pytest.mark.parametrize("layout", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("B", [96, 128, 416])
def test_tn_multi_layouts(ops, gpu, layout, B):
    """Every operand layout of the many-problem launch: 1 takes x as [N][K], 2 dy as [M][K],
    3 forces the 4-wave kernel (falling back at B = 96 and 416: no whole K-tile pairs), 4 the
    8-wave one."""
    data = [tn_data(B, M, N, seed=10 + p) for p, (M, N) in enumerate(MULTI)]
    dys = [gx.place_operand(transposed(d[0]).t if layout == 2 else d[0].t, gpu) for d in data]
    xs = [gx.place_operand(transposed(d[1]).t if layout == 1 else d[1].t, gpu) for d in data]

    def run(rep):
        outs = [gx.place_output(s, F32, gpu) for s in MULTI]
        dbs = [gx.place_vector(s[0], F32, gpu) if p % 2 == 0 else (None, None)
               for p, s in enumerate(MULTI)]
        for t0, n in ((0, 7), (7, 15)):
            ops.gemm_tn_multi_layout(dys, xs, [v for _, v in outs], [v for _, v in dbs], t0, n,
                                     layout)
        for p in range(4):
            what = f"gemm_tn_multi_layout {layout} B{B} problem {p} rep{rep}"
            gx.assert_exact(outs[p][1], gx.to_f32(data[p][2]), what)
            gx.assert_canary(*outs[p], what)
            if dbs[p][1] is not None:
                gx.assert_exact(dbs[p][1], gx.to_f32(data[p][3]), what + " db")
                gx.assert_canary(*dbs[p], what + " db")
    twice(run)


# --------------------------------------------------------------------------- MADE-masked
def _order(name, D):
    if name == "natural":
        return None
    if name == "reversed":
        return torch.arange(D, 0, -1)
    return torch.randperm(D, generator=torch.Generator().manual_seed(17)) + 1


@functools.lru_cache(maxsize=None)
def made_case(order, D=256, H=512):
    m1, m2 = made_masks(*made_degrees(D, H, 1, _order(order, D)), 2)     # [H, D], [2D, H]
    return m1, m2


def synthetic_mask(N=512, K=512):
    """Block staircase with an all-zero first 128-row tile (an empty K range) and a hole in the
    last tile's columns (two K ranges for the transposed, 256-wide tiles)."""
    m = torch.zeros(N, K)
    m[128:256, :64] = 1
    m[128:192, 256:320] = 1
    m[256:384, 64:256] = 1
    m[384:, :128] = 1
    m[384:, 384:] = 1
    return m


def _masked_weights(mask, seed, shift):
    w = gx.gen_bf16(tuple(mask.shape), seed=seed, shift=shift, zero_share=0.1)
    return gx.Exact(w.i * mask.long(), shift, BF)          # pre-multiplied, as in ops/masked.py


MASKS = ["natural-hidden", "natural-out", "reversed-hidden", "reversed-out", "random-hidden",
         "random-out", "synthetic"]


def _mask_of(name):
    if name == "synthetic":
        return synthetic_mask()
    order, which = name.split("-")
    return made_case(order)[0 if which == "hidden" else 1]


@pytest.mark.parametrize("state", ["t128", "t256-pair0", "t256-pair2"])
@pytest.mark.parametrize("mask_name", MASKS)
def test_masked_products(ops, gpu, state, mask_name):
    """masked_gemm_nt / masked_gemm_nn under MaskPlan K ranges equal the dense products of the
    pre-masked weights, bitwise, on the 128 and 256 kernels, with column tiles paired or not."""
    mask = _mask_of(mask_name)
    Nw, Kw = mask.shape
    plan = MaskPlan(mask.to(gpu))
    if mask_name == "synthetic":
        assert plan.fwd[0].tolist() == [0, 0] and plan.bwd256.shape[1] == 4
    if mask_name in ("natural-out", "reversed-out"):
        assert plan.bwd256.shape[1] == 4                   # two K ranges per tile chosen
    ops.gemm_set_mode(1 if state == "t128" else 2)
    ops.gemm_pair(2 if state.endswith("pair2") else 0)
    B = 300
    w = _masked_weights(mask, seed=21, shift=2)
    x = gx.gen_bf16((B, Kw), seed=22, shift=1)
    b = gx.gen_grid((Nw,), seed=23, shift=1, bound=255, dtype=BF)
    dy = gx.gen_bf16((B, Nw), seed=24, shift=1)
    h = gx.gen_bf16((B, Kw), seed=25, zero_share=0.3)
    base = gx.gen_grid((B, Kw), seed=26, shift=3, bound=4000, dtype=F32)
    gx.assert_exact_bound(x, transposed(w), b)
    gx.assert_exact_bound(dy, w, base)
    fwd = gx.product(x, transposed(w)) + b.d
    bwd = gx.product(dy, w)
    keep = h.d > 0
    zero = torch.zeros((), dtype=torch.float64)
    xv, wv, dyv, hv = (gx.place_operand(t.t, gpu) for t in (x, w, dy, h))
    wtv = gx.place_operand(transposed(w).t, gpu)
    bd = b.to(gpu)
    what = f"masked {mask_name} {state}"

    def run(rep):
        for relu in (0, 1):
            yb, y = gx.place_output((B, Nw), BF, gpu)
            ops.masked_gemm_nt(xv, wv, bd, y, relu, plan.fwd, plan.fwd256)
            gx.assert_exact(y, gx.to_bf16(fwd.clamp_min(0) if relu else fwd), f"{what} nt relu{relu} rep{rep}")
            gx.assert_canary(yb, y, what)
        for wt in (None, wtv):
            ob, out = gx.place_output((B, Kw), BF, gpu)
            ops.masked_gemm_nn(dyv, wv, hv, out, plan.bwd, False, plan.bwd256, wt)
            gx.assert_exact(out, gx.to_bf16(torch.where(keep, bwd, zero)), f"{what} nn h wt{wt is not None} rep{rep}")
            gx.assert_canary(ob, out, what)
            ob, out = gx.place_output((B, Kw), F32, gpu, init=base.t)
            ops.masked_gemm_nn(dyv, wv, None, out, plan.bwd, True, plan.bwd256, wt)
            gx.assert_exact(out, gx.to_f32(bwd + base.d), f"{what} nn accumulate wt{wt is not None} rep{rep}")
            gx.assert_canary(ob, out, what)
        ob, out = gx.place_output((B, Kw), F32, gpu)
        ops.masked_gemm_nn(dyv, wv, None, out, plan.bwd, False, plan.bwd256)
        gx.assert_exact(out, gx.to_f32(bwd), f"{what} nn f32 rep{rep}")
        gx.assert_canary(ob, out, what)
    twice(run)


@pytest.mark.parametrize("mask_name", MASKS)
@pytest.mark.parametrize("B", [96, 416])
def test_masked_wgrad(ops, gpu, mask_name, B):
    """masked_gemm_tn with MaskPlan skip flags: computed tiles exact, skipped tiles exactly zero,
    the first tile column exact when db is asked for (it feeds the bias gradient)."""
    mask = _mask_of(mask_name)
    M, N = mask.shape
    plan = MaskPlan(mask.to(gpu))
    skip = plan.wskip.cpu().reshape((M + 127) // 128, (N + 127) // 128)
    assert mask_name.startswith("random") or int(skip.sum()) > 0
    dy, x, p, colsum = tn_data(B, M, N, seed=30)
    dyv, xv = gx.place_operand(dy.t, gpu), gx.place_operand(x.t, gpu)

    def run(rep):
        for with_db in (True, False):
            wb, dW = gx.place_output((M, N), F32, gpu)
            bb, db = gx.place_vector(M, F32, gpu) if with_db else (None, None)
            ops.masked_gemm_tn(dyv, xv, dW, db, plan.wskip)
            what = f"masked_gemm_tn {mask_name} B{B} db{with_db} rep{rep}"
            gx.assert_exact(dW, gx.to_f32(_skip_ref(p, skip, with_db)), what)
            gx.assert_canary(wb, dW, what)
            if with_db:
                gx.assert_exact(db, gx.to_f32(colsum), what + " db")
                gx.assert_canary(bb, db, what + " db")
    twice(run)


@pytest.mark.parametrize("mask_name", MASKS)
def test_masked_wgrad_active_tiles(ops, gpu, mask_name):
    """The many-problem launch on MaskPlan's active 256x256 tile list with the dense mask as
    cmask: listed tiles hold the masked product, the others are never written, db is exact."""
    from vi_normflows_amd.ops.gemm import WgradPlan

    mask = _mask_of(mask_name)
    M, N = mask.shape
    plan = MaskPlan(mask.to(gpu))
    act = plan.wtiles256.cpu().tolist()
    dy, x, p, colsum = tn_data(128, M, N, seed=31)
    dyv, xv = gx.place_operand(dy.t, gpu), gx.place_operand(x.t, gpu)
    cm = mask.to(U8)
    ref = _tiles_ref(torch.where(cm != 0, p, torch.zeros((), dtype=torch.float64)), act, M, N)

    def run(rep):
        wb, dW = gx.place_output((M, N), F32, gpu, col_off=0, pad=0)
        bb, db = gx.place_vector(M, F32, gpu)
        wp = WgradPlan([(dyv, xv, dW, db, plan.wtiles256, cm.to(gpu))])
        assert wp.total == len(act)
        wp.run(0, wp.total)
        what = f"gemm_tn_multi MADE tiles {mask_name} rep{rep}"
        gx.assert_exact(dW, ref.float(), what)
        gx.assert_canary(wb, dW, what)
        gx.assert_exact(db, gx.to_f32(colsum), what + " db")
        gx.assert_canary(bb, db, what + " db")
    twice(run)


# ------------------------------------------------------------------- fp32 / fp64 gemm_fp
@pytest.mark.parametrize("dtype", [F32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("M,N,K", [(1, 8, 32), (37, 65, 96), (130, 67, 33), (9, 5, 4096)])
def test_gemm_fp(ops, gpu, dtype, M, N, K):
    """Exact fp32 / fp64 products in all four operand layouts with bias, accumulate and dbias;
    (9, 5, 4096) is a one-tile long-K product, split over K (nf_gemm_fp_splits > 1)."""
    a = gx.gen_grid((M, K), seed=41, shift=2, bound=7, dtype=dtype)
    b = gx.gen_grid((N, K), seed=42, shift=1, bound=7, dtype=dtype)
    bias = gx.gen_grid((N,), seed=43, shift=3, bound=2000, dtype=dtype)
    base = gx.gen_grid((M, N), seed=44, shift=3, bound=2000, dtype=dtype)
    gx.assert_exact_bound(a, transposed(b), bias, base)
    p = gx.product(a, transposed(b))
    rowsum = a.d.sum(1)

    def run(rep):
        for akm, bkm in itertools.product((True, False), (True, False)):
            av = gx.place_operand(a.t if akm else a.t.t().contiguous(), gpu)
            bv = gx.place_operand(b.t if bkm else b.t.t().contiguous(), gpu)
            for with_bias, acc, with_db in ((1, 0, 1), (0, 1, 0), (1, 1, 1), (0, 0, 0)):
                cb, C = gx.place_output((M, N), dtype, gpu, init=base.t if acc else None)
                db_, db = gx.place_vector(M, dtype, gpu) if with_db else (None, None)
                ops.gemm_fp(av, akm, bv, bkm, bias.to(gpu) if with_bias else None, C, bool(acc), db)
                ref = p + (bias.d if with_bias else 0) + (base.d if acc else 0)
                what = f"gemm_fp {dtype} {M}x{N}x{K} akm{akm} bkm{bkm} bias{with_bias} acc{acc} rep{rep}"
                gx.assert_exact(C, ref.to(dtype), what)
                gx.assert_canary(cb, C, what)
                if with_db:
                    gx.assert_exact(db, rowsum.to(dtype), what + " dbias")
                    gx.assert_canary(db_, db, what + " dbias")
    twice(run)


# ------------------------------------------------------------------------------ e4m3 (fp8)
def _pow2(n, seed, lo=-3, hi=1):
    g = torch.Generator().manual_seed(seed)
    return 2.0 ** torch.randint(lo, hi + 1, (n,), generator=g).double()


def _amax_state(dev, k):
    """Delayed-scale state with amax_prev = 448 * 2**k: s = 2**k and 1 / s are exact."""
    prev = torch.tensor([448.0 * 2.0 ** k], device=dev)
    scale = torch.full((1,), float("nan"), device=dev)
    cur = torch.zeros(64, device=dev)
    return prev, scale, cur


@functools.lru_cache(maxsize=None)
def f8_data(M, N, K):
    x = gx.gen_e4m3((M, K), seed=50 + M + K)
    w = gx.gen_e4m3((N, K), seed=51 + N + K)
    b = gx.gen_grid((N,), seed=52 + N, shift=1, bound=255, dtype=BF)
    gx.assert_exact_bound(x, transposed(w))
    return x, w, b, gx.product(x, transposed(w))


# (a one-row e4m3 copy has its width as leading dimension, which chk_q wants % 16: N = 16 at M = 1)
F8_SHAPES = [(1, 16, 128), (127, 136, 128), (300, 264, 384), (257, 520, 256)]


@pytest.mark.parametrize("mode", [1, 2], ids=["fp8hip", "t256"])
@pytest.mark.parametrize("M,N,K", F8_SHAPES)
def test_fp8_nt(ops, gpu, mode, M, N, K):
    """gemm_fp8_nt on the 128 kernel (fp8.hip) and the 256 kernel: per-row and per-tensor sx,
    bias, relu, the e4m3 copy under a delayed scale (amax_cur and q_scale exact)."""
    ops.gemm_set_mode(mode)
    ops.gemm_persist(0)
    x, w, b, p = f8_data(M, N, K)
    xv, wv = gx.place_operand(x.t, gpu), gx.place_operand(w.t, gpu)
    sw = _pow2(N, seed=53)
    what = f"gemm_fp8_nt mode{mode} M{M} N{N} K{K}"

    def run(rep):
        for per_row, bias, relu, with_q in ((1, 1, 1, 1), (0, 0, 0, 0), (1, 0, 1, 0), (0, 1, 0, 1)):
            sx = _pow2(M, seed=54) if per_row else _pow2(1, seed=55)
            r = p * sx[:, None] * sw[None, :] + (b.d if bias else 0)
            r = r.clamp_min(0) if relu else r
            ref = gx.to_bf16(r)
            yb, y = gx.place_output((M, N), BF, gpu)
            qb = q = None
            st = (None, None, None)
            if with_q:
                qb, q = gx.place_output((M, N), F8, gpu)
                st = _amax_state(gpu, k=-2)
            ops.gemm_fp8_nt(xv, sx.float().to(gpu), wv, sw.float().to(gpu),
                            b.to(gpu) if bias else None, y, relu, None, q, *st)
            w_ = f"{what} row{per_row} bias{bias} relu{relu} rep{rep}"
            gx.assert_exact(y, ref, w_)
            gx.assert_canary(yb, y, w_)
            if with_q:
                gx.assert_exact(q, gx.to_e4m3(ref.double() * 4.0), w_ + " e4m3 copy")
                gx.assert_canary(qb, q, w_ + " e4m3 copy")
                assert st[1].item() == 0.25, (w_, st[1].item())
                assert st[2].max().item() == ref.float().abs().max().item(), w_
    twice(run)


@pytest.mark.parametrize("mode", [1, 2], ids=["fp8hip", "t256"])
@pytest.mark.parametrize("mask_name", ["natural-hidden", "reversed-hidden", "random-hidden", "synthetic"])
def test_fp8_nt_kranges(ops, gpu, mode, mask_name):
    """MADE K ranges on e4m3 operands (krange on fp8.hip, krange256 on the 256 kernel, paired
    and unpaired) equal the dense product of the pre-masked weights."""
    mask = _mask_of(mask_name)
    N, K = mask.shape
    M = 300
    plan = MaskPlan(mask.to(gpu))
    x = gx.gen_e4m3((M, K), seed=60)
    w = gx.gen_e4m3((N, K), seed=61, zero_share=0.1)
    w = gx.Exact(w.i * mask.long(), 0, F8)
    gx.assert_exact_bound(x, transposed(w))
    sx, sw = _pow2(1, seed=62), _pow2(N, seed=63)
    ref = gx.to_bf16(gx.product(x, transposed(w)) * sx * sw[None, :])
    xv, wv = gx.place_operand(x.t, gpu), gx.place_operand(w.t, gpu)
    ops.gemm_set_mode(mode)
    for pair in ((0, 2) if mode == 2 else (0,)):
        ops.gemm_pair(pair)

        def run(rep):
            yb, y = gx.place_output((M, N), BF, gpu)
            ops.gemm_fp8_nt(xv, sx.float().to(gpu), wv, sw.float().to(gpu), None, y, 0, plan.fwd,
                            None, None, None, None, plan.fwd256)
            what = f"gemm_fp8_nt kranges {mask_name} mode{mode} pair{pair} rep{rep}"
            gx.assert_exact(y, ref, what)
            gx.assert_canary(yb, y, what)
        twice(run)


@pytest.mark.parametrize("M,N,K", F8_SHAPES)
def test_fp8_nt_lean_forms(ops, gpu, M, N, K):
    """The y-less forms (256 kernel): ReLU bitmask and / or e4m3 copy without the bf16 output."""
    x, w, b, p = f8_data(M, N, K)
    xv, wv = gx.place_operand(x.t, gpu), gx.place_operand(w.t, gpu)
    sx, sw = _pow2(M, seed=54), _pow2(N, seed=53)
    ref = gx.to_bf16((p * sx[:, None] * sw[None, :] + b.d).clamp_min(0))
    dense = torch.tensor([[0, K]] * ((N + 255) // 256), dtype=torch.int32, device=gpu)

    def run(rep):
        for with_y, with_q, with_m in ((0, 1, 1), (0, 0, 1), (0, 1, 0), (1, 1, 1)):
            yb, y = gx.place_output((M, N), BF, gpu) if with_y else (None, None)
            qb, q = gx.place_output((M, N), F8, gpu) if with_q else (None, None)
            mb, m = (gx.place_output((M, N // 8), U8, gpu, fill=0x00 if rep else 0xFF)
                     if with_m else (None, None))
            st = _amax_state(gpu, k=1) if with_q else (None, None, None)
            ops.gemm_fp8_nt(xv, sx.float().to(gpu), wv, sw.float().to(gpu), b.to(gpu), y, 1, None,
                            q, *st, dense, m)
            what = f"gemm_fp8_nt lean M{M} N{N} K{K} y{with_y} q{with_q} m{with_m} rep{rep}"
            if with_y:
                gx.assert_exact(y, ref, what)
                gx.assert_canary(yb, y, what)
            if with_q:
                gx.assert_exact(q, gx.to_e4m3(ref.double() * 0.5), what + " e4m3 copy")
                gx.assert_canary(qb, q, what + " e4m3 copy")
                assert st[1].item() == 2.0 and st[2].max().item() == ref.float().abs().max().item(), what
            if with_m:
                gx.assert_exact(m, gx.pack_bits(ref > 0), what + " bitmask")
                gx.assert_canary(mb, m, what + " bitmask")
    twice(run)


@pytest.mark.parametrize("pair", [0, 2])
@pytest.mark.parametrize("M,N,K,segs", [(1, 16, 128, 1), (257, 136, 256, 1), (300, 512, 512, 2),
                                        (520, 264, 384, 1)])
def test_fp8_dgrad(ops, gpu, pair, M, N, K, segs):
    """fp8_dgrad: h as bf16 and as bitmask, one and two K ranges, dx / dxq / both."""
    ops.gemm_pair(pair)
    dy = gx.gen_e4m3((M, K), seed=70 + M)
    wt = gx.gen_e4m3((N, K), seed=71 + N, zero_share=0.1)
    nt = (N + 255) // 256
    if segs == 2:      # K ranges [0, 128) and [384, 512) for tile 0, [128, 384) + none for tile 1
        kr = torch.tensor([[0, 128, 384, 512], [128, 384, 0, 0]], dtype=torch.int32)
        live = torch.zeros(N, K, dtype=torch.long)
        live[:256, :128] = 1
        live[:256, 384:] = 1
        live[256:, 128:384] = 1
        wt = gx.Exact(wt.i * live, 0, F8)
    else:
        kr = torch.tensor([[0, K]] * nt, dtype=torch.int32)
    h = gx.gen_bf16((M, N), seed=72, zero_share=0.3)
    gx.assert_exact_bound(dy, transposed(wt))
    sa, sb = _pow2(1, seed=73), _pow2(N, seed=74)
    keep = h.d > 0
    r = torch.where(keep, gx.product(dy, transposed(wt)) * sa * sb[None, :], torch.zeros((), dtype=torch.float64))
    ref = gx.to_bf16(r)
    dyv, wtv, hv = (gx.place_operand(t.t, gpu) for t in (dy, wt, h))
    bits = gx.place_operand(gx.pack_bits(keep), gpu)
    sbd = sb.float().to(gpu)
    assert sbd.data_ptr() % 16 == 0

    def run(rep):
        for hop, with_dx, with_q in itertools.product((hv, bits), (1, 0), (1, 0)):
            if not (with_dx or with_q):
                continue
            xb, dx = gx.place_output((M, N), BF, gpu) if with_dx else (None, None)
            qb, q = gx.place_output((M, N), F8, gpu) if with_q else (None, None)
            st = _amax_state(gpu, k=-1) if with_q else (None, None, None)
            ops.fp8_dgrad(dyv, sa.float().to(gpu), wtv, sbd, hop, dx, kr.to(gpu), q, *st)
            what = f"fp8_dgrad pair{pair} M{M} N{N} K{K} segs{segs} bits{hop is bits} dx{with_dx} q{with_q} rep{rep}"
            if with_dx:
                gx.assert_exact(dx, ref, what)
                gx.assert_canary(xb, dx, what)
            if with_q:
                gx.assert_exact(q, gx.to_e4m3(ref.double() * 2.0), what + " e4m3 copy")
                gx.assert_canary(qb, q, what + " e4m3 copy")
                assert st[1].item() == 0.5 and st[2].max().item() == ref.float().abs().max().item(), what
    twice(run)


@pytest.mark.parametrize("B", [128, 384])
def test_fp8_wgrad_and_colsum(ops, gpu, B):
    """gemm_tn_multi_f8 (e4m3 weight gradients, scales from a pool by index) and fp8_colsum."""
    shapes = [(272, 528), (528, 144), (16, 16)]
    dys = [gx.gen_e4m3((B, M), seed=80 + p) for p, (M, _) in enumerate(shapes)]
    xs = [gx.gen_e4m3((B, N), seed=85 + p) for p, (_, N) in enumerate(shapes)]
    pool = _pow2(6, seed=88)
    sa_idx, sb_idx = [0, 2, 4], [1, 3, 5]
    total = sum(((M + 255) // 256) * ((N + 255) // 256) for M, N in shapes)
    for d, x in zip(dys, xs):
        gx.assert_exact_bound(transposed(d), x)
    dyv = [gx.place_operand(d.t, gpu) for d in dys]
    xv = [gx.place_operand(x.t, gpu) for x in xs]
    poold = pool.float().to(gpu)

    def run(rep):
        outs = [gx.place_output(s, F32, gpu) for s in shapes]
        for t0, n in ((0, 5), (5, total - 5)):
            ops.gemm_tn_multi_f8(dyv, xv, [v for _, v in outs], [None] * 3, t0, n, [], [], poold,
                                 sa_idx, sb_idx)
        sums = [gx.place_vector(M, F32, gpu) for M, _ in shapes]
        part = torch.empty(8 * sum(M for M, _ in shapes), device=gpu)
        ops.fp8_colsum(dyv, [v for _, v in sums], poold, sa_idx, part)
        for p in range(3):
            ref = gx.product(transposed(dys[p]), xs[p]) * pool[sa_idx[p]] * pool[sb_idx[p]]
            what = f"gemm_tn_multi_f8 B{B} problem {p} rep{rep}"
            gx.assert_exact(outs[p][1], gx.to_f32(ref), what)
            gx.assert_canary(*outs[p], what)
            gx.assert_exact(sums[p][1], gx.to_f32(dys[p].d.sum(0) * pool[sa_idx[p]]), what + " colsum")
            gx.assert_canary(*sums[p], what + " colsum")
    twice(run)


# --------------------------------------------------------------------- binding preconditions
def test_bindings_reject_what_the_launchers_abort_on(ops, gpu):
    """Argument combinations that used to pass the bindings' checks and reach a launcher's
    abort(): they must raise instead."""
    M, D, H = 8, 128, 160
    kr = torch.tensor([[0, 160]], dtype=torch.int32, device=gpu)
    z = lambda *s, dt=F32: torch.zeros(*s, dtype=dt, device=gpu)            # noqa: E731
    with pytest.raises(RuntimeError, match="multiple of 32"):               # bf16 K = 40
        ops.maf_gemm_fwd(z(M, 40, dt=BF), None, z(2 * D, 40, dt=BF), None, None, kr, z(M, D, dt=BF),
                         z(M, D), z(M, D), None, z(1, M), True, 3.0)
    with pytest.raises(RuntimeError, match="multiple of 32"):               # e4m3 K = 160
        ops.maf_gemm_fwd(z(M, H, dt=F8), z(1), z(2 * D, H, dt=F8), z(2 * D), None, kr,
                         z(M, D, dt=BF), z(M, D), z(M, D), None, z(1, M), True, 3.0)
    with pytest.raises(RuntimeError, match="K % 128"):                      # e4m3 K = 160
        ops.maf_gemm_bwd(z(M, H, dt=F8), z(D, H, dt=F8), kr, z(M, D), z(M, D, dt=BF), z(M, D),
                         z(M, 2 * D, dt=BF), z(M, D), 3.0, 0.0, z(1), z(D))
    big = z(M, 72)
    with pytest.raises(RuntimeError, match="aligned"):                      # G off a 16-B boundary
        ops.gemm_nn_cpl(z(M, 32, dt=BF), z(32, 64, dt=BF), big[:, 1:65], z(M, 64, dt=BF), z(M, 32),
                        z(M, 64, dt=BF), z(M, 32), 1.0, 0.0)
    with pytest.raises(RuntimeError, match="multiples of 4"):               # x rows of 34 floats
        ops.gemm_nn_cpl(z(M, 32, dt=BF), z(32, 64, dt=BF), z(M, 64), z(M, 64, dt=BF),
                        z(M, 34)[:, :32], z(M, 64, dt=BF), z(M, 32), 1.0, 0.0)


# ------------------------------------------------------------------------- fused epilogues
# The coupling / MAF epilogues start from bf16(acc + bias) and G + acc, which the exact operands
# fix bit for bit. Their transform outputs use fast_tanhf, __expf and v_rcp by design
# (nf_common.h fast_tanhf, gemm256.hip epi_coupling_fwd, gemm_tile.h epi_tile_staged) and are
# compared per element with the fp64 evaluation of the documented formulas at those exact
# inputs: |out - ref| <= CPL_MULT * unit, unit = eps32 ((1 + scale) |ref| + 8 max|inputs|), the
# second term a floor where the reference cancels (inputs = the magnitudes the element is formed
# from). CPL_MULT is twice the worst err / unit measured on the MI355X over every case of this
# section, rounded up to a power of two (docs/PERF_NOTES.md, "Exact-operand GEMM oracle").
# The relative part must stay below 2^-12 (asserted): a one-ulp bf16 slip in mu, t or s_raw
# (2^-8 of a term that is at least a quarter of the output on most elements) cannot hide.
EPS32 = 2.0 ** -23
# worst measured err / unit 0.516 (maf_gemm_fwd u, bf16 operands, M 520, D 256, K 416, natural
# order, bound 3): twice that, rounded up to a power of two. Relative part at bound 3: 2^-20.
CPL_MULT = 2.0


def _ratio_report(kind, ratio, what):
    print(f"CPL_RATIO {kind} {ratio:.4f} {what}")


def check_transform(out, ref, scale, inputs_max, kind, what, half_ulp_bf16=False):
    """Per element |out - ref| <= CPL_MULT * unit (+ half a bf16 ulp of the reference for bf16
    transform outputs). Prints the worst err / unit before asserting."""
    assert CPL_MULT * EPS32 * (1 + scale) < 2.0 ** -12
    out = out.detach().cpu().double()
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    unit = EPS32 * ((1 + scale) * ref.abs() + 8 * inputs_max)
    err = (out - ref).abs()
    if half_ulp_bf16:    # ulp from the reference's exponent: 2^(e - 7), half of it 2^(e - 8)
        e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
        err = (err - 2.0 ** (e - 8)).clamp_min(0)
    ratio = torch.where(unit > 0, err / unit.clamp_min(1e-300),
                        torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    _ratio_report(kind, worst, what)
    bad = ratio > CPL_MULT
    if bad.any():
        idx = bad.nonzero()[:6].tolist()
        rows = [f"  {tuple(i)}: got {out[tuple(i)].item()!r} want {ref[tuple(i)].item()!r} "
                f"ratio {ratio[tuple(i)].item():.2f}" for i in idx]
        raise AssertionError(f"{what} [{kind}]: {int(bad.sum())} of {bad.numel()} elements beyond "
                             f"CPL_MULT = {CPL_MULT} units (worst {worst:.2f})\n" + "\n".join(rows))


def _shift_for(K):
    """Product grid 2**-S with 14 sqrt(K) 2**-S ~ 1: conditioner outputs of order one."""
    return 8 if K > 256 else 7


def _tile_sums(v, width):
    """[M, F] -> [ceil(F / width), M] sums over feature tiles."""
    return torch.stack([v[:, j:j + width].sum(1) for j in range(0, v.shape[1], width)])


CPL_SHAPES = list(itertools.product([1, 37, 257, 520, 272], [8, 136, 392], [96, 128, 416]))


@pytest.mark.parametrize("M,Dh,K", CPL_SHAPES)
def test_coupling_forward_epilogue(ops, gpu, M, Dh, K):
    """gemm_nt_cpl, forward and inverse, on the 8-wave kernel (one tile per block, persistent)
    and the 4-wave one (gemm_cpl4w(1); taken when M % 16 == 0 and K % 128 == 0: M = 272)."""
    S = _shift_for(K)
    rows = 2 * Dh + 8
    h = gx.gen_bf16((M, K), seed=100 + M + K, shift=3)
    w = gx.gen_bf16((rows, K), seed=101 + Dh + K, shift=S - 3)
    b = gx.gen_grid((rows,), seed=102 + Dh, shift=S, bound=min(255, 2 ** S), dtype=BF)
    gx.assert_exact_bound(h, transposed(w), b)
    o = gx.product(h, transposed(w)) + b.d
    sh, t = gx.to_bf16(o[:, :Dh]), gx.to_bf16(o[:, Dh:2 * Dh])
    x = gx.gen_grid((M, Dh), seed=103 + M, shift=4, bound=48, dtype=F32, zero_share=0.05)
    l0 = gx.gen_grid(((Dh + 127) // 128 + 1, M), seed=104, shift=4, bound=64, dtype=F32)
    hv, wv, xv = (gx.place_operand(e.t, gpu) for e in (h, w, x))
    bd = b.to(gpu)
    ybw = (Dh + 7) // 8 * 8 + 8
    ntn = (Dh + 127) // 128

    def run(rep):
        # (inverse, ldj_init, cpl4w, persist, reserve, scale, st given)
        for inv, init, c4, persist, scale, has_st in ((0, 1, 0, 1, 1.0, 1), (0, 0, 1, 0, 2.0, 1),
                                                      (1, 1, 1, 1, 2.0, 0), (1, 0, 0, 0, 1.0, 1),
                                                      (0, 1, 0, 8, 1.0, 1)):
            ops.gemm_cpl4w(c4)
            ops.gemm_persist(1 if persist else 0)
            ops.gemm_grid_reserve(_cus() if persist == 8 else 0)
            fat = bool(c4) and M % 16 == 0 and K % 128 == 0
            sv = scale * torch.tanh(sh.double())
            if inv:
                yr = (x.d - t.double()) * torch.exp(-sv)
                terms = torch.maximum(x.d.abs(), t.double().abs()) * torch.exp(-sv)
                lr = -_tile_sums(sv, 136 if fat else 128)
            else:
                yr = x.d * torch.exp(sv) + t.double()
                terms = torch.maximum((x.d * torch.exp(sv)).abs(), t.double().abs())
                lr = _tile_sums(sv, 136 if fat else 128)
            labs = _tile_sums(sv.abs(), 136 if fat else 128)
            stb, st = gx.place_output((M, Dh), BF, gpu) if has_st else (None, None)
            yb_, y = gx.place_output((M, Dh), F32, gpu)
            ybb, ybf = gx.place_output((M, ybw), BF, gpu)
            lb, ldjp = gx.place_output((ntn + 1, M), F32, gpu, init=None if init else l0.t)
            ops.gemm_nt_cpl(hv, wv, bd, st, xv, y, ybf, ldjp, bool(init), scale, bool(inv))
            what = (f"gemm_nt_cpl M{M} Dh{Dh} K{K} inverse{inv} init{init} cpl4w{c4} "
                    f"persist{persist} scale{scale} rep{rep}")
            if has_st:
                gx.assert_exact(st, sh, what + " s_hat")
                gx.assert_canary(stb, st, what + " s_hat")
            check_transform(y, yr, scale, terms, "cpl_fwd_y", what)
            gx.assert_canary(yb_, y, what + " y")
            ref_yb = torch.zeros(M, ybw, dtype=BF)
            ref_yb[:, :Dh] = y.detach().cpu().to(BF)           # self-consistent copy, zero pad
            gx.assert_exact(ybf, ref_yb, what + " yb")
            gx.assert_canary(ybb, ybf, what + " yb")
            used = lr.shape[0]
            got = ldjp.detach().cpu()
            lold = torch.zeros_like(lr) if init else l0.d[:used]
            check_transform(got[:used], lr + lold, scale, labs + lold.abs(), "cpl_fwd_ldj", what)
            # rows no feature tile owns: untouched (NaN pre-fill / old value), or zeroed by the
            # 4-wave kernel's first step
            rest = got[used:]
            keep = torch.full_like(rest, float("nan")) if init else l0.t[used:]
            if fat and init:
                keep[:ntn - used] = 0
            gx.assert_exact(rest, keep, what + " unowned ldjp rows")
            gx.assert_canary(lb, ldjp, what + " ldjp")
    twice(run)


@pytest.mark.parametrize("M,Dh,K", CPL_SHAPES)
def test_coupling_backward_epilogue(ops, gpu, M, Dh, K):
    """gemm_nn_cpl: W and Wt forms, fp32 / bf16 x, and the bf16 G chain."""
    S = _shift_for(K)
    N = Dh + 24
    pad = 2 * Dh + 16
    dy = gx.gen_bf16((M, K), seed=110 + M + K, shift=3)
    w = gx.gen_bf16((K, N), seed=111 + Dh + K, shift=S - 3)
    G = gx.gen_grid((M, N), seed=112 + M, shift=S, bound=4 * 2 ** S, dtype=F32)
    Gb = gx.gen_grid((M, N), seed=113 + M, shift=S - 2, bound=255, dtype=BF)
    gx.assert_exact_bound(dy, w, G)
    gx.assert_exact_bound(dy, w, Gb)
    acc = gx.product(dy, w)
    s_hat = gx.gen_grid((M, Dh), seed=114 + Dh, shift=6, bound=100, dtype=BF, zero_share=0.05)
    x = gx.gen_grid((M, Dh), seed=115 + M, shift=4, bound=48, dtype=F32, zero_share=0.05)
    xb = gx.gen_grid((M, Dh), seed=116 + M, shift=6, bound=192, dtype=BF, zero_share=0.05)
    dyv, wv, sv_, xv, xbv, Gv, Gbv = (gx.place_operand(e.t, gpu) for e in (dy, w, s_hat, x, xb, G, Gb))
    wtv = gx.place_operand(transposed(w).t, gpu)
    c = -1.0 / 64

    def run(rep):
        for form, scale in (("W", 1.0), ("Wt", 2.0), ("Wt-xb", 1.0), ("Wt-xb-gb", 2.0)):
            xe, Ge = (xb if "xb" in form else x), (Gb if "gb" in form else G)
            gy = (Ge.d + acc)[:, :Dh]
            sv = scale * torch.tanh(s_hat.d)
            es = torch.exp(sv)
            fac = scale - sv * sv / scale
            dS = (gy * xe.d * es + c) * fac
            gxr = gy * es
            db_, dst = gx.place_output((M, pad), BF, gpu)
            gdt = BF if "gb" in form else F32
            gb_, gxo = gx.place_output((M, Dh), gdt, gpu)
            ops.gemm_nn_cpl(dyv, wv, Gbv if "gb" in form else Gv, sv_, xbv if "xb" in form else xv,
                            dst, gxo, scale, c, None if form == "W" else wtv)
            what = f"gemm_nn_cpl M{M} Dh{Dh} K{K} {form} scale{scale} rep{rep}"
            d = dst.detach().cpu()
            gx.assert_exact(d[:, Dh:2 * Dh], gx.to_bf16(gy), what + " dT = bf16(G + acc)")
            gx.assert_exact(d[:, 2 * Dh:], torch.zeros(M, pad - 2 * Dh, dtype=BF), what + " dst pad")
            check_transform(d[:, :Dh], dS, scale,
                            torch.maximum((gy * xe.d * es).abs(), torch.full_like(gy, abs(c))) * scale,
                            "cpl_bwd_dS", what, half_ulp_bf16=True)
            check_transform(gxo, gxr, scale, gxr.abs(), "cpl_bwd_gx", what, half_ulp_bf16=gdt == BF)
            gx.assert_canary(db_, dst, what + " dst")
            gx.assert_canary(gb_, gxo, what + " gx")
    twice(run)


def _maf_masks(D, H, order):
    """(P2pair K ranges [D/128, 2] of the fused forward, m2 [2D, H], m1 [H, D]), as the MAF
    engine builds them."""
    m1, m2 = made_masks(*made_degrees(D, H, 1, _order(order, D)), 2)
    pair = torch.cat([torch.cat([m2[D + t:D + t + 128], m2[t:t + 128]]) for t in range(0, D, 128)])
    return tile_ranges(pair, 256).contiguous(), m2, m1


MAF_SHAPES = ([(M, D, K, "bf16") for M, D, K in itertools.product([1, 37, 257, 520], [128, 256], [96, 128, 416])]
              + [(M, D, K, "e4m3") for M, D, K in itertools.product([1, 37, 257, 520], [128, 256], [128, 384])])


@pytest.mark.parametrize("M,D,K,kind", MAF_SHAPES)
def test_maf_forward_epilogue(ops, gpu, M, D, K, kind):
    """maf_gemm_fwd on bf16 and e4m3 operands: dense and MADE K ranges (natural, reversed),
    fp32 and bf16 x, the u-less bf16-state form, the e4m3 copy of u under a delayed scale."""
    f8 = kind == "e4m3"
    S = _shift_for(K)
    x = gx.gen_grid((M, D), seed=123 + M, shift=4, bound=48, dtype=F32, zero_share=0.05)
    xb = gx.gen_grid((M, D), seed=124 + M, shift=6, bound=192, dtype=BF, zero_share=0.05)
    b = gx.gen_grid((2 * D,), seed=122 + D, shift=S, bound=min(255, 2 ** S), dtype=BF)
    l0 = gx.gen_grid((D // 128, M), seed=125, shift=4, bound=64, dtype=F32)
    xv, xbv, bd = gx.place_operand(x.t, gpu), gx.place_operand(xb.t, gpu), b.to(gpu)
    if f8:
        h = gx.gen_e4m3((M, K), seed=120 + M + K)
        hs = torch.tensor([2.0 ** -3], dtype=torch.float64)
        ws = 2.0 ** -(S - 3 + torch.arange(2 * D) % 2).double()
    else:
        h = gx.gen_bf16((M, K), seed=120 + M + K, shift=3)
    hv = gx.place_operand(h.t, gpu)

    def run(rep):
        for order, bound, init, state in (("dense", 2.0, 1, "f32"), ("natural", 3.0, 0, "f32-q"),
                                          ("reversed", 3.0, 1, "xb"), ("natural", 2.0, 1, "xb-noU")):
            if order == "dense":
                kr, mask = torch.tensor([[0, K]] * (D // 128), dtype=torch.int32), torch.ones(2 * D, K)
            else:
                kr, mask, _ = _maf_masks(D, K, order)
            if f8:
                w = gx.gen_e4m3((2 * D, K), seed=121 + D + K, zero_share=0.1)
                w = gx.Exact(w.i * mask.long(), 0, F8)
                gx.assert_exact_bound(h, transposed(w))
                o = gx.product(h, transposed(w)) * hs * ws[None, :] + b.d
            else:
                w = gx.gen_bf16((2 * D, K), seed=121 + D + K, shift=S - 3, zero_share=0.1)
                w = gx.Exact(w.i * mask.long(), S - 3, BF)
                gx.assert_exact_bound(h, transposed(w), b)
                o = gx.product(h, transposed(w)) + b.d
            wv = gx.place_operand(w.t, gpu)
            mu, sr = gx.to_bf16(o[:, :D]), gx.to_bf16(o[:, D:])
            xe = xb if state.startswith("xb") else x
            al = bound * torch.tanh(sr.double() / bound)
            ur = (xe.d - mu.double()) * torch.exp(-al)
            terms = torch.maximum(xe.d.abs(), mu.double().abs()) * torch.exp(-al)
            lold = torch.zeros(D // 128, M, dtype=torch.float64) if init else l0.d
            lr = -_tile_sums(al, 128) + lold
            with_q = f8 and state == "f32-q"
            sb_, s_out = gx.place_output((M, D), BF, gpu)
            ub_, u = (None, None) if state == "xb-noU" else gx.place_output((M, D), F32, gpu)
            fb_, ubf = gx.place_output((M, D), BF, gpu)
            lb_, ldjp = gx.place_output((D // 128, M), F32, gpu, init=None if init else l0.t)
            qb_, uq = gx.place_output((M, D), F8, gpu) if with_q else (None, None)
            st = _amax_state(gpu, k=-3) if with_q else (None, None, None)
            ops.maf_gemm_fwd(hv, hs.float().to(gpu) if f8 else None, wv,
                             ws.float().to(gpu) if f8 else None, bd, kr.to(gpu), s_out,
                             xbv if state.startswith("xb") else xv, u, ubf, ldjp, bool(init), bound,
                             uq, *st)
            what = f"maf_gemm_fwd {kind} M{M} D{D} K{K} {order} bound{bound} init{init} {state} rep{rep}"
            gx.assert_exact(s_out, sr, what + " s_raw")
            gx.assert_canary(sb_, s_out, what + " s_raw")
            if u is not None:
                check_transform(u, ur, bound, terms, "maf_fwd_u", what)
                gx.assert_exact(ubf, u.detach().cpu().to(BF), what + " ubf = bf16(u)")
                gx.assert_canary(ub_, u, what + " u")
            else:
                check_transform(ubf, ur, bound, terms, "maf_fwd_ubf", what, half_ulp_bf16=True)
            gx.assert_canary(fb_, ubf, what + " ubf")
            check_transform(ldjp, lr, bound, _tile_sums(al.abs(), 128) + lold.abs(), "maf_fwd_ldj", what)
            gx.assert_canary(lb_, ldjp, what + " ldjp")
            if with_q:
                uk = u.detach().cpu()
                gx.assert_exact(uq, gx.to_e4m3(uk.double() * 8.0), what + " uq = e4m3(u / s)")
                gx.assert_canary(qb_, uq, what + " uq")
                assert st[1].item() == 0.125 and st[2].max().item() == uk.abs().max().item(), what
    twice(run)


@pytest.mark.parametrize("M,D,K,kind", MAF_SHAPES)
def test_maf_backward_epilogue(ops, gpu, M, D, K, kind):
    """maf_gemm_bwd on bf16 and e4m3 operands under MaskPlan's 256-tile K ranges of real MADE
    hidden masks; fp32 and bf16 u; dst, its e4m3 copy, and the dst-less e4m3 form."""
    f8 = kind == "e4m3"
    S = _shift_for(K)
    G = gx.gen_grid((M, D), seed=132 + M, shift=S, bound=4 * 2 ** S, dtype=F32)
    s_raw = gx.gen_grid((M, D), seed=133 + D, shift=5, bound=100, dtype=BF, zero_share=0.05)
    u = gx.gen_grid((M, D), seed=134 + M, shift=4, bound=48, dtype=F32, zero_share=0.05)
    ub = gx.gen_grid((M, D), seed=135 + M, shift=6, bound=192, dtype=BF, zero_share=0.05)
    Gv, sv_, uv, ubv = (gx.place_operand(e.t, gpu) for e in (G, s_raw, u, ub))
    c = 1.0 / 128
    if f8:
        dy = gx.gen_e4m3((M, K), seed=130 + M + K)
        sa = torch.tensor([2.0 ** -3], dtype=torch.float64)
        sb = 2.0 ** -(S - 3 + torch.arange(D) % 2).double()
    else:
        dy = gx.gen_bf16((M, K), seed=130 + M + K, shift=3)
    dyv = gx.place_operand(dy.t, gpu)

    def run(rep):
        for order, bound, state in (("dense", 2.0, "f32"), ("natural", 3.0, "ub"),
                                    ("reversed", 3.0, "f32-q"), ("window", 2.0, "f32-qonly")):
            if state.endswith("qonly") and not f8:
                state = "f32"
            if order == "dense":
                mask = torch.ones(K, D)
            elif order == "window":      # D <= 256 is one tile whose MADE range is all of K:
                mask = torch.ones(K, D)  # a K range that starts inside K, from a hand-made mask
                mask[:64] = 0
            else:
                mask = made_masks(*made_degrees(D, K, 1, _order(order, D)), 2)[0]     # [H = K, D]
            kr = MaskPlan(mask).bwd256 if order != "dense" else \
                torch.tensor([[0, K]] * ((D + 255) // 256), dtype=torch.int32)
            if f8:
                wt = gx.gen_e4m3((D, K), seed=131 + D + K, zero_share=0.1)
                wt = gx.Exact(wt.i * mask.t().long(), 0, F8)
                gx.assert_exact_bound(dy, transposed(wt))
                gy = G.d + gx.product(dy, transposed(wt)) * sa * sb[None, :]
                gx.to_f32(gy)
            else:
                wt = gx.gen_bf16((D, K), seed=131 + D + K, shift=S - 3, zero_share=0.1)
                wt = gx.Exact(wt.i * mask.t().long(), S - 3, BF)
                gx.assert_exact_bound(dy, transposed(wt), G)
                gy = G.d + gx.product(dy, transposed(wt))
            wtv = gx.place_operand(wt.t, gpu)
            ue = ub if state == "ub" else u
            t = torch.tanh(s_raw.d / bound)
            gxr = gy * torch.exp(-bound * t)
            ds = (c - gy * ue.d) * (1 - t * t)
            ref = torch.cat([-gxr, ds], 1)
            terms = torch.cat([gxr.abs(), torch.maximum((gy * ue.d).abs(), torch.full_like(gy, c))], 1)
            with_q = f8 and "q" in state
            with_dst = not state.endswith("qonly")
            db_, dst = gx.place_output((M, 2 * D), BF, gpu) if with_dst else (None, None)
            gb_, gxo = gx.place_output((M, D), F32, gpu)
            qb_, dq = gx.place_output((M, 2 * D), F8, gpu) if with_q else (None, None)
            st = _amax_state(gpu, k=-2) if with_q else (None, None, None)
            ops.maf_gemm_bwd(dyv, wtv, kr.to(gpu), Gv, sv_, ubv if state == "ub" else uv, dst, gxo,
                             bound, c, sa.float().to(gpu) if f8 else None,
                             sb.float().to(gpu) if f8 else None, dq, *st)
            what = f"maf_gemm_bwd {kind} M{M} D{D} K{K} {order} bound{bound} {state} rep{rep}"
            check_transform(gxo, gxr, bound, gxr.abs(), "maf_bwd_gx", what)
            gx.assert_canary(gb_, gxo, what + " gx")
            if with_dst:
                check_transform(dst, ref, bound, terms, "maf_bwd_dst", what, half_ulp_bf16=True)
                gx.assert_canary(db_, dst, what + " dst")
            if with_q:
                # the copy is quantised from the fp32 values, which are not stored: it must lie
                # between the e4m3 codes of the reference moved by the fp32 bound either way
                # (the conversion is monotone), under the exact scale 2^-2
                bnd = CPL_MULT * EPS32 * ((1 + bound) * ref.abs() + 8 * terms)
                lo = gx.to_e4m3((ref - bnd) * 4.0).float()
                hi = gx.to_e4m3((ref + bnd) * 4.0).float()
                q = dq.detach().cpu().float()
                bad = (q < lo) | (q > hi)
                assert not bad.any(), (what, int(bad.sum()), bad.nonzero()[:4].tolist())
                gx.assert_canary(qb_, dq, what + " dstq")
                amax = st[2].max().item()
                assert st[1].item() == 0.25, what
                assert abs(amax - ref.abs().max().item()) <= bnd.max().item(), (what, amax)
    twice(run)
