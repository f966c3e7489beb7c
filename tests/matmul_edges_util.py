"""Inputs, expected values and the wave census of the values-matmul kernels' edge tests (numpy only).

The idea: out[b] = Qx(x[b]) @ Qy(y[b]).  If every output element is the sum of ONE non-zero product and exact zeros, `out` shows one
operand's quantised values bit for bit -- products of two values with <= 8 significant bits are exact in fp32, and so is adding zeros.

  construction A (x side)   x [B, M, K] = the edge set in [1,16] blocks along K; y [B, K, N] a column selector: column n holds one
                            non-zero, the constant d, at row sel[n] -- every [1,16] block of y along N is d and zeros and quantises to
                            q = Q(d).  out[m, n] = Qx(x)[m, sel[n]] q.  N < K: ceil(K / N) selectors.  block_log does not quantise y:
                            its non-zeros are seeded values with full 24-bit fractions in [0.5, 2) (Qx is a signed power of two, so the
                            product is still exact -- which also holds FMT_RAW's three-plane split to exactness).
  construction B (y side)   y [B, K, N] = the edge set in blocks along N, x = d I (M = K rows): out[m, :] = Q(d) Qy(y)[m, :].  block_fp
                            and block_minifloat only: block_log's x has no zeros.

Block sets (block_set): kv_edges_util's "bfp" / "bm" / "bm64", and "bl" / "bl64" -- the x of edge_blockmax_bl / edge_dense_bl and of
edge_blockmaxx64_bl / edge_densex64_bl in tests/golden/quantizers.npz.

Orders of the 1822 blocks (order):
  "sorted"    row_edges_util.short_order(): neighbouring blocks alike, so whole waves sit in the kernels' `near` redo;
  "strided"   blocks dealt with stride 131 (coprime to 1822, as row_edges_util.long deals them) -- but a wave of either product kernel is
              16 rows x the four blocks of a 64-step, 64 blocks, and more than half of the set's block maxima lie near a power of two:
              dealt over the whole set no wave would stay on the fused path.  So the blocks that are `calm` for the format (no lane of
              theirs raises `near`, by the census below) are dealt first, among themselves, and the others behind them: the leading
              row groups are whole calm waves.  Every block is still there exactly once.

Expected values: the oracle's quantiser per operand, with the kernels' one documented rule (head comment of csrc/mi355q_matmul.hip):
elements 0 < |x| <= 1e-8, which block_fp / block_minifloat pass through unquantised, enter the product rounded to bf16.  The product is
formed in float64, where one non-zero term per output makes it exact, and must be representable in fp32."""
import functools
import re
from pathlib import Path

import numpy as np

from tests import kv_edges_util as KV
from tests import row_edges_util as R
from tests.conftest import GOLDEN

F32 = np.float32
N_EDGE = R.N_EDGE
STRIDE = R.STRIDE
D = F32(0.75)
INC = Path(__file__).resolve().parents[1] / "llm-mixed-q_amd" / "csrc" / "log2_tables.inc"


# ---------------------------------------------------------------------------------------------------
# formats: ("bfp", width, exponent_width, exponent_bias) / ("bm", width, exponent_width, exponent_bias_width) / ("bl", width, ebw)
# ---------------------------------------------------------------------------------------------------
def bfp(width, ew=8, bias=127):
    return ("bfp", width, ew, bias)


def bm(width, ew, ebw):
    return ("bm", width, ew, ebw)


def bl(width, ebw):
    return ("bl", width, ebw)


def fmt_id(fmt):
    return fmt[0] + "_" + "_".join(str(v) for v in fmt[1:])


def oracle_cfg(fmt):
    """the registry config oracle.np_oracle.matmul_quantized takes for this format, both operands alike"""
    kind, p = fmt[0], fmt[1:]
    if kind == "bfp":
        one = dict(width=p[0], exponent_width=p[1], exponent_bias=p[2], block_size=[1, 16])
        name = "block_fp"
    elif kind == "bm":
        one = dict(width=p[0], exponent_width=p[1], exponent_bias_width=p[2], block_size=[1, 16])
        name = "block_minifloat"
    else:
        one = dict(width=p[0], exponent_bias_width=p[1], block_size=[1, 16])
        name = "block_log"
    cfg = dict(name=name, bypass=False)
    for prefix in ("data_in", "weight"):
        cfg.update({f"{prefix}_{k}": v for k, v in one.items()})
    return cfg


def quantise(t, fmt):
    """the oracle's quantiser on t [B, rows, cols], [1,16] blocks along cols (block_log: the all-zero blocks' fill is tensor-wide)"""
    from oracle import np_oracle as O
    kind, p = fmt[0], fmt[1:]
    t = np.ascontiguousarray(t, F32)
    if kind == "bfp":
        return O.block_fp_quantize(t, p[0], p[1], p[2], block_size=[1, 16], skip_first_dim=True)
    if kind == "bm":
        return O.block_minifloat_quantize(t, *p, block_size=[1, 16], skip_first_dim=True)
    return O.block_log_quantize(t, *p, block_size=[1, 16], skip_first_dim=True)


def operand(t, fmt):
    """what the product kernels multiply with for an operand they quantise: the oracle's values, elements 0 < |x| <= 1e-8 (which
    block_fp / block_minifloat pass through; block_log has no pass-through) rounded to bf16 -- csrc/mi355q_matmul.hip:18-19"""
    from oracle import compare
    q = quantise(t, fmt)
    return q if fmt[0] == "bl" else np.where(KV.tiny(t), compare.bf16_rne(np.ascontiguousarray(t, F32)), q)


# ---------------------------------------------------------------------------------------------------
# blocks, orders, layouts
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block_set(name):
    """[1822, 16] fp32, read-only: blockmax blocks first, dense blocks behind them"""
    if name in ("bfp", "bm", "bm64"):
        return KV.block_set(name)
    tags = {"bl": ("edge_blockmax_bl", "edge_dense_bl"), "bl64": ("edge_blockmaxx64_bl", "edge_densex64_bl")}[name]
    z = np.load(GOLDEN / "quantizers.npz")
    b = np.concatenate([z[f"{t}/x"] for t in tags]).astype(F32)
    assert b.shape == (N_EDGE, 16)
    b.setflags(write=False)
    return b


GOLDEN_TAGS = {("bfp", bfp(6)): ("edge_blockmax_bfp_w6", "edge_dense_bfp_w6"), ("bm", bm(8, 4, 8)): ("edge_blockmax_bm", "edge_dense_bm"),
               ("bm64", bm(8, 4, 8)): ("edge_blockmaxx64_bm", "edge_densex64_bm"), ("bl", bl(8, 8)): ("edge_blockmax_bl", "edge_dense_bl"),
               ("bl64", bl(8, 8)): ("edge_blockmaxx64_bl", "edge_densex64_bl")}


def _deal(idx):
    """the indices dealt with stride 131 among themselves (131 is prime: a permutation unless it divides the count)"""
    n = len(idx)
    if n == 0:
        return idx
    step = STRIDE if np.gcd(STRIDE, n) == 1 else STRIDE + 2
    assert np.gcd(step, n) == 1
    return idx[(np.arange(n) * step) % n]


@functools.lru_cache(maxsize=None)
def order(name, fmt, kind):
    """permutation of block_set(name): position -> block index"""
    if kind == "sorted":
        return R.short_order()
    assert kind == "strided"
    calm = calm_blocks(block_set(name), fmt)
    return np.concatenate([_deal(np.flatnonzero(calm)), _deal(np.flatnonzero(~calm))])


def rows_of(K, B=1):
    rows = -(-N_EDGE // (K // 16))
    return -(-rows // B)


def x_layout(blocks, K, B=1):
    """[B, M, K]: the blocks in order along K, then M, then B; the remainder padded with whole all-zero blocks"""
    assert K % 16 == 0
    n, per = len(blocks), K // 16
    M = -(-(-(-n // per)) // B)
    pad = np.zeros((B * M * per, 16), F32)
    pad[:n] = blocks
    return pad.reshape(B, M, K)


def y_layout(blocks, K, N, B=1):
    """[B, K, N]: the blocks in order along N, then K, then B; whole all-zero blocks behind them"""
    assert N % 16 == 0 and B * K * (N // 16) >= len(blocks)
    pad = np.zeros((B * K * (N // 16), 16), F32)
    pad[:len(blocks)] = blocks
    return pad.reshape(B, K, N)


def layout_blocks(t):
    return np.ascontiguousarray(t).reshape(-1, 16)


@functools.lru_cache(maxsize=None)
def x_case(name, fmt, kind, K, B):
    x = x_layout(block_set(name)[order(name, fmt, kind)], K, B)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def clamp_case(B):
    """row_edges_util.clamp_layout() ([114, 320], for exponent_width 4 / bias 7), its rows cut into B"""
    x = R.clamp_layout()
    M = -(-x.shape[0] // B)
    pad = np.zeros((B * M, x.shape[1]), F32)
    pad[:x.shape[0]] = x
    pad = pad.reshape(B, M, x.shape[1])
    pad.setflags(write=False)
    return pad


@functools.lru_cache(maxsize=None)
def y_case(name, fmt, kind, K, N):
    y = y_layout(block_set(name)[order(name, fmt, kind)], K, N)
    y.setflags(write=False)
    return y


# ---------------------------------------------------------------------------------------------------
# selectors
# ---------------------------------------------------------------------------------------------------
def selectors(K, N, d=D, B=1, raw=False):
    """[(y [B, K, N], sel [N])]: column n of selector j holds one non-zero at row sel[n] = j N + n (none where that is >= K), so that
    the selectors together read every K position once.  raw (block_log, y not quantised): the non-zeros are seeded values in
    [0.5, 2) with full 24-bit fractions, the lowest bit set; else all of them are d."""
    out = []
    r = np.random.default_rng(K * 1000 + N)
    for j in range(-(-K // N)):
        sel = j * N + np.arange(N)
        ok = sel < K
        y = np.zeros((B, K, N), F32)
        if raw:
            bits = (r.integers(0, 1 << 22, size=(B, N), dtype=np.int64) << 1 | 1).astype(np.uint32)
            val = ((np.uint32(126) + r.integers(0, 2, size=(B, N)).astype(np.uint32)) << np.uint32(23) | bits).view(F32)
        else:
            val = np.full((B, N), d, F32)
        y[:, sel[ok], np.arange(N)[ok]] = val[:, ok]
        out.append((y, np.where(ok, sel, -1)))
    return out


def row_selector(K, d=D, B=1):
    """x [B, K, K] = d I"""
    return np.broadcast_to(np.eye(K, dtype=F32) * d, (B, K, K)).copy()


def single_q(t, fmt):
    """the one non-zero value a selector operand quantises to"""
    q = quantise(t, fmt)
    vals = np.unique(q[q != 0])
    assert len(vals) == 1 and np.array_equal(q != 0, t != 0), f"{fmt}: the selector quantises to {vals}"
    return F32(vals[0])


def _product(xq, yq):
    terms = np.matmul((xq != 0).astype(np.int64), (yq != 0).astype(np.int64))
    assert terms.max() <= 1, "an output element is the sum of more than one non-zero product"
    with np.errstate(over="ignore", under="ignore"):
        e = np.matmul(xq.astype(np.float64), yq.astype(np.float64))
        e32 = e.astype(F32)
    assert np.isfinite(e32).all() and np.array_equal(e32.astype(np.float64), e), "the expected product is not representable in fp32"
    return e32


def expected_x(x, fmt, y):
    """construction A, fp32 [B, M, N]: operand(x) times the selector's q (block_log: times y itself)"""
    if fmt[0] == "bl":
        return _product(operand(x, fmt), y)
    q = single_q(y, fmt)
    return _product(operand(x, fmt), np.where(y != 0, q, F32(0)))


def expected_y(y, fmt, x):
    """construction B, fp32 [B, M, N]: the selector's q times operand(y)"""
    assert fmt[0] != "bl"
    q = single_q(x, fmt)
    return _product(np.where(x != 0, q, F32(0)), operand(y, fmt))


def differing(got, want):
    return KV.differing(got, want)


def same(got, want, what):
    """integer equality of the fp32 words, a zero's sign aside (the oracle does not pin it: kv_edges_util.differing)"""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    bad = differing(got, want)
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {want.size} values differ, first at {tuple(int(j) for j in i)}: got {float(got[i])!r} "
                             f"({int(got.view(np.uint32)[i]):#010x}), want {float(want[i])!r} ({int(want.view(np.uint32)[i]):#010x})")


# ---------------------------------------------------------------------------------------------------
# the `near` census: csrc/mi355q_matmul.hip's quantise_lane (kernel 3) and quantise_xblk (kernel 2) restated
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bands():
    txt = INC.read_text()
    return {n: int(re.search(rf"#define MI355Q_LOG2_{n} (0x[0-9a-f]+)u", txt).group(1), 16)
            for n in ("CEIL_THR_MAX", "FLOOR_THR_MIN", "RND_LO_MIN", "RND_HI_MAX")}


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32).astype(np.int64)


def _block_params(blocks, fmt):
    """(the oracle's block parameter [n] -- block_fp: exponent, else the shared bias --, the block maximum with the fill [n])"""
    from oracle import np_oracle as O
    kind, p = fmt[0], fmt[1:]
    if kind == "bfp":
        code = O.bfp_encode(blocks, p[0], p[1], p[2], [1, 16], True)
        par = code.exp
    elif kind == "bm":
        par = O.bm_encode(blocks, *p, [1, 16], True).bias
    else:
        par = O.bl_encode(blocks, *p, [1, 16], True).bias
    bmax = np.abs(blocks).max(axis=1)
    if kind == "bl":
        bmax = O.filled_block_max(blocks)                  # (zfill: the statistics pass's tensor-wide fill)
    else:
        bmax = np.where(bmax > 0, bmax, F32(1.0))          # (zfill = 1: block_fp / block_minifloat zeros stay zeros)
    return par.astype(np.int64), bmax.astype(F32)


def near_block(blocks, fmt):
    """[n] bool, kernel 3 only: quantise_lane's `near` of the lane that holds the block -- a subnormal maximum, or a fraction inside
    the band where its own in-lane exponent could differ from the table's (block_fp / block_log: 1 .. CEIL_THR_MAX above a power of
    two; block_minifloat: >= FLOOR_THR_MIN, just below one)"""
    _, bmax = _block_params(blocks, fmt)
    bb = _bits(bmax)
    m = bb & 0x7FFFFF
    sub = bb < 0x00800000
    if fmt[0] == "bm":
        return sub | (m >= bands()["FLOOR_THR_MIN"])
    return sub | ((m >= 1) & (m <= bands()["CEIL_THR_MAX"]))


def near_elem(blocks, fmt):
    """[n, 16] bool, kernels 2 and 3: bm_elem_fused's / bl_elem_fused's `near` (block_fp's quant_elem_fused has none)"""
    kind = fmt[0]
    if kind == "bfp":
        return np.zeros(blocks.shape, bool)
    par, _ = _block_params(blocks, fmt)
    if kind == "bm":
        vb = _bits(np.abs(blocks) + F32(1e-9))
        return (vb & 0x7FFFFF) >= bands()["FLOOR_THR_MIN"]
    eps = np.ldexp(F32(0.1), -par).astype(F32)[:, None]
    vb = _bits(np.abs(blocks) + eps)
    m = vb & 0x7FFFFF
    return ((m >= bands()["RND_LO_MIN"]) & (m <= bands()["RND_HI_MAX"])) | (vb < 0x00800000)


def calm_blocks(blocks, fmt):
    """[n] bool: no lane that holds the block, or an element of it, raises `near` in either kernel"""
    return ~(near_block(blocks, fmt) | near_elem(blocks, fmt).any(axis=1))


def ties_and_clamps(blocks, fmt):
    """([n] ties, [n] clamps) per block, the decisions a wrong rounding or a wrong exponent moves:
    block_fp         ties: elements whose mantissa before rounding is j + 1/2 (row_edges_util.tie_mask); clamps: the block maximum
                     rounds up to 2^mb and is clamped (kv_edges_util.bfp_masks);
    block_minifloat  ties: kv_edges_util.bm_masks'; clamps: non-zero elements whose own exponent floor(log2(|x| + 1e-9)) lies
                     outside the block's [e_min, e_max] and is clamped;
    block_log        ties: elements whose |x| + eps has its fraction inside [RND_LO_MIN, RND_HI_MAX], where the table decides the
                     rounding of log2 -- by definition `near`, so only redo waves hold them; clamps: elements whose rounded log2 lies
                     outside [e_min, e_max]."""
    from oracle import np_oracle as O
    kind, p = fmt[0], fmt[1:]
    n = len(blocks)
    if kind == "bfp":
        m = KV.bfp_masks(np.ascontiguousarray(blocks).reshape(n, 16), p[0]) if (p[1], p[2]) == (8, 127) else None
        if m is None:
            m = dict(ties=np.zeros((n, 1, 16), bool), clamps=np.zeros((n, 1), bool))
        return m["ties"].reshape(n, 16).sum(axis=1), m["clamps"].reshape(n).astype(np.int64)
    if kind == "bm":
        m = KV.bm_masks(np.ascontiguousarray(blocks).reshape(n, 16), p)
        code = O.bm_encode(blocks, *p, [1, 16], True)
        with np.errstate(divide="ignore"):
            raw = np.floor(O.log2_f32(np.abs(blocks) + F32(1e-9)))
        clamped = (raw != code.exp.reshape(n, 16)) & (blocks != 0) & ~KV.tiny(blocks)
        return m["ties"].reshape(n, 16).sum(axis=1), clamped.sum(axis=1)
    code = O.bl_encode(blocks, *p, [1, 16], True)
    eps = np.ldexp(F32(0.1), -code.bias.astype(np.int64)).astype(F32)[:, None]
    v = np.abs(blocks) + eps
    mfrac = _bits(v) & 0x7FFFFF
    ties = (mfrac >= bands()["RND_LO_MIN"]) & (mfrac <= bands()["RND_HI_MAX"]) & (v > 0)
    with np.errstate(divide="ignore"):
        raw = np.rint(O.log2_f32(v))
    clamped = (raw != code.exp.reshape(n, 16)) & (blocks != 0)
    return ties.sum(axis=1), clamped.sum(axis=1)


def wave_census(x, fmt):
    """x [B, M, K]: what the 64-lane waves of the product kernels hold.  A wave of kernel 2 (quantise_xblk: four elements a lane) and
    of kernel 3 (quantise_lane: one block a lane) covers the SAME 64 blocks: 16 rows (a 16-row group of one batch entry; the last
    group of an entry may be short: its lanes repeat the last row) x the four blocks of a 64-step (blocks behind K are zeroed: the
    fill).  Kernel 2 redoes a wave's elements when an element of it is `near` (never for block_fp); kernel 3 as well, and it also
    falls back to the table for the block parameter when a block maximum of the wave is `near`.
    Returns dict kernel -> dict(redo=(waves, ties, clamps), fused=(waves, ties, clamps))."""
    B, M, K = x.shape
    blocks = layout_blocks(x)
    nb = near_block(blocks, fmt).reshape(B, M, K // 16)
    ne = near_elem(blocks, fmt).any(axis=1).reshape(B, M, K // 16)
    t, c = ties_and_clamps(blocks, fmt)
    t, c = t.reshape(B, M, K // 16), c.reshape(B, M, K // 16)
    out = {2: dict(redo=[0, 0, 0], fused=[0, 0, 0]), 3: dict(redo=[0, 0, 0], fused=[0, 0, 0])}
    for b in range(B):
        for m0 in range(0, M, 16):
            for s in range(0, K // 16, 4):
                w = (b, slice(m0, m0 + 16), slice(s, s + 4))
                for kernel, redo in ((2, ne[w].any()), (3, ne[w].any() or nb[w].any())):
                    acc = out[kernel]["redo" if redo else "fused"]
                    acc[0] += 1
                    acc[1] += int(t[w].sum())
                    acc[2] += int(c[w].sum())
    return {k: {r: tuple(v) for r, v in d.items()} for k, d in out.items()}


# ---------------------------------------------------------------------------------------------------
# what the GPU file runs (tests/test_gpu_matmul_edges.py, tests/matmul_edges_child.py), checked on the CPU by
# tests/test_matmul_edges_host.py
# ---------------------------------------------------------------------------------------------------
SHAPES_A = ((64, 64), (128, 128), (192, 192), (208, 208), (256, 64), (256, 128))      # (K, N): one per launch branch
SHAPES_B = ((64, 464), (208, 144))                                                    # (K, N) of y; x = d I [K, K]
ORDERS = ("sorted", "strided")
BATCHES = (1, 2)
CLAMP_FMT = bfp(6, 4, 7)
CLAMP_N = 64
# (block set, format)
SETS_A = ([("bfp", bfp(w)) for w in (2, 4, 6, 8, 9)]
          + [("bm", bm(8, 4, 8)), ("bm64", bm(8, 4, 8)), ("bm", bm(6, 3, 4)), ("bm", bm(4, 2, 3)), ("bm", bm(7, 3, 5))]
          + [("bl", bl(8, 8)), ("bl64", bl(8, 8)), ("bl", bl(4, 3)), ("bl", bl(6, 2))])
SETS_B = [s for s in SETS_A if s[1][0] != "bl"]


def set_id(s):
    return f"{s[0]}-{fmt_id(s[1])}"


def cases_a(name, fmt, kind, B):
    """[(key, x, y, K, N, sel)] of construction A for one block set, format, order and batch cut"""
    out = []
    for K, N in SHAPES_A:
        x = x_case(name, fmt, kind, K, B)
        for j, (y, sel) in enumerate(selectors(K, N, B=B, raw=fmt[0] == "bl")):
            out.append((f"A/{set_id((name, fmt))}/{kind}/B{B}/K{K}N{N}/s{j}", x, y, K, N, sel))
    return out


def cases_clamp(B):
    x = clamp_case(B)
    K = x.shape[2]
    return [(f"A/clamp-{fmt_id(CLAMP_FMT)}/B{B}/K{K}N{CLAMP_N}/s{j}", x, y, K, CLAMP_N, sel)
            for j, (y, sel) in enumerate(selectors(K, CLAMP_N, B=B))]


def cases_b(name, fmt, kind):
    return [(f"B/{set_id((name, fmt))}/{kind}/K{K}N{N}", row_selector(K), y_case(name, fmt, kind, K, N), K, N) for K, N in SHAPES_B]


def bl_extra_cases():
    """block_log's all-zero blocks, where the statistics pass's fill shows in the output.  On the whole set the smallest non-zero block
    maximum is 3.7e-14: the fill's 2^-bias lies below fp32 and a zero block reads 0 whatever the fill.  So, under (8, 8), these take
    the rows of the x64 set's sorted order whose blocks all have exponents >= 4: the fill is then 2^-(127 - e) >= 2^-123, a normal
    number that 1 in its place (2^-127) is not.  "planted": two all-zero blocks inside otherwise non-zero rows; "padded": three rows
    of zero blocks behind them; "allzero": every block of x zero (fill 1, bl_zero_fill's 0xFFFFFFFF path) under (4, 3), where
    2^-bias = 2^-7 is representable."""
    fmt = bl(8, 8)
    full = x_case("bl64", fmt, "sorted", 64, 1)
    blocks = layout_blocks(full)
    e = np.where(np.abs(blocks).max(axis=1) > 0, R._block_exponents(blocks), -999).reshape(full.shape[1], 4)
    x = full[:, (e >= 4).all(axis=1)].copy()
    assert x.shape[1] >= 40
    planted = x.copy()
    planted[0, 3, 16:32] = 0
    planted[0, 21, 48:64] = 0
    padded = np.concatenate([x, np.zeros((1, 3, 64), F32)], axis=1)
    y, sel = selectors(64, 64, raw=True)[0]
    return [("A/bl-extra/planted", planted, y, 64, 64, sel, fmt), ("A/bl-extra/padded", padded, y, 64, 64, sel, fmt),
            ("A/bl-extra/allzero", np.zeros((1, 37, 64), F32), y, 64, 64, sel, bl(4, 3))]


def run_case(ops, torch, fmt, x, y):
    """one product on the library, through the public ops, as numpy"""
    xt, yt = torch.from_numpy(np.array(x, F32)).to("cuda:0"), torch.from_numpy(np.array(y, F32)).to("cuda:0")
    kind, p = fmt[0], fmt[1:]
    if kind == "bfp":
        out = ops.bfp_matmul(xt, yt, p[0], p[1], p[2], p[0], p[1], p[2])
    elif kind == "bm":
        out = ops.values_matmul(xt, yt, "block_minifloat", p, p)
    else:
        out = ops.values_matmul(xt, yt, "block_log", p)
    return out.cpu().numpy()


def all_cases(short_only=False, kinds=("bfp", "bm", "bl")):
    """every (key, fmt, x, y) the GPU file and its children run; short_only: contractions of at most three 64-steps (where the RW
    latch matters)"""
    out = []
    for name, fmt in SETS_A:
        if fmt[0] not in kinds:
            continue
        for kind in ORDERS:
            for B in BATCHES:
                out += [(key, fmt, x, y) for key, x, y, K, N, sel in cases_a(name, fmt, kind, B) if not short_only or K <= 192]
    if not short_only and "bfp" in kinds:
        for B in BATCHES:
            out += [(key, CLAMP_FMT, x, y) for key, x, y, K, N, sel in cases_clamp(B)]
    for name, fmt in SETS_B:
        if fmt[0] not in kinds:
            continue
        for kind in ORDERS:
            out += [(key, fmt, x, y) for key, x, y, K, N in cases_b(name, fmt, kind) if not short_only or K <= 192]
    if "bl" in kinds:
        out += [(key, fmt, x, y) for key, x, y, K, N, sel, fmt in bl_extra_cases()]
    return out


def expected_of(key, fmt, x, y):
    return expected_y(y, fmt, x) if key.startswith("B/") else expected_x(x, fmt, y)


@functools.lru_cache(maxsize=None)
def fixed_point_case(name, fmt):
    """(x [1, M, 64], blocks kept): the oracle's quantised values of the sorted K = 64 layout, with every block that is not a fixed
    point of the quantiser (block_fp: a quantised maximum of exactly 2^k takes the next exponent down and clamps) and every block
    with a passed-through element zeroed -- an operand whose blocks are already representable"""
    x = x_case(name, fmt, "sorted", 64, 1)
    q = quantise(x, fmt)
    qb, xb = layout_blocks(q).copy(), layout_blocks(x)
    again = layout_blocks(quantise(qb.reshape(q.shape), fmt))
    keep = (again.view(np.uint32) == qb.view(np.uint32)).all(axis=1) & ~KV.tiny(xb).any(axis=1) & (np.abs(qb).max(axis=1) > 0)
    qb[~keep] = 0
    out = qb.reshape(q.shape)
    assert np.array_equal(layout_blocks(quantise(out, fmt)).view(np.uint32) & 0x7FFFFFFF, qb.view(np.uint32) & 0x7FFFFFFF)
    out.setflags(write=False)
    return out, int(keep.sum())
