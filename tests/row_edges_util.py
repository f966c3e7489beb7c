"""Inputs, expected values and an operand decoder for the row quantiser's edge tests (numpy only; torch and the library are
touched by the decoder alone, when a GPU test hands it an operand).

Inputs: the reference's boundary set -- the `x` arrays of edge_blockmax_bfp_w6 (1714 blocks, each edge value as the largest
of its own block) and edge_dense_bfp_w6 (108 blocks of edge values side by side) in tests/golden/quantizers.npz -- laid out as
rows of a [rows, K] activation, in two ways:

  short(K)        K <= 1024: the blocks as they are, ordered by the oracle's block exponent (then by original index) and cut
                  into rows of K / 16 blocks; the last row is padded with all-zero blocks.  Magnitudes are the reference's,
                  so the 1e-8 / 1e-9 neighbourhood and the half-way mantissas at block maximum 1 are what the reference saw.
  long(K, rows)   any K: row r cycles through the blocks from block 131 r on (131 is coprime to 1822), each non-zero block
                  scaled by the exact power of two that puts its oracle exponent on the row's target t_r (cycle -20, -3, 0,
                  1, 9, 30).  Block g = r K/16 + j of the tensor is an exception block when g % exc_every == exc_every - 1
                  (d = 5..9 exponents below t_r, d cycling; one further down where no scale lands on t_r - d, see long())
                  and all zeros when g % 97 == 96.  A power of two keeps the
                  fraction bits: "a few ulps from 2^k" and the ties stay; the +1e-9 of the rule does not scale, so expected
                  values are always computed on the assembled tensor.

Expected values: oracle.np_oracle.bfp_encode, which tests/test_oracle_golden.py pins bit for bit to the reference on exactly
these tags.  One rule is the library's own: an all-zero block is filled with 1 (MI355Q_ZERO_BLOCK_FAST, the only rule the
row quantiser has) where the reference fills it with the tensor's smallest non-zero block maximum; such a block's
mantissas are 0 and its exponent is not compared."""
import functools

import numpy as np

from tests.conftest import GOLDEN

TARGETS = (-20, -3, 0, 1, 9, 30)
STRIDE = 131
N_EDGE = 1714 + 108


def edge_blocks():
    """[1822, 16] fp32: blockmax blocks first, dense blocks behind them"""
    z = np.load(GOLDEN / "quantizers.npz")
    b = np.concatenate([z["edge_blockmax_bfp_w6/x"], z["edge_dense_bfp_w6/x"]]).astype(np.float32)
    assert b.shape == (N_EDGE, 16)
    return b


def _block_exponents(blocks):
    """the oracle's exponent of every block of [n, 16] (exponent_width 8, bias 127: no clamp in reach), all-zero blocks -> 0"""
    from oracle import np_oracle as O
    code = O.bfp_encode(blocks, 6, 8, 127, [1, 16], True)
    return np.where(np.abs(blocks).max(axis=1) > 0, code.exp, 0).astype(np.int64)


def short_order():
    """permutation of the edge blocks used by short(): by oracle exponent, then by original index"""
    return np.argsort(_block_exponents(edge_blocks()), kind="stable")


def short(K):
    assert K % 16 == 0 and K <= 1024
    b = edge_blocks()[short_order()]
    nkb = K // 16
    rows = -(-N_EDGE // nkb)
    x = np.zeros((rows * nkb, 16), np.float32)
    x[:N_EDGE] = b
    return x.reshape(rows, K)


def long(K, rows, exc_every=64, zero_every=97, exc_depth=(5, 6, 7, 8, 9)):
    """exc_every = 0: no exception blocks (every block of a row on the row's target); exc_depth: the cycle of d"""
    assert K % 16 == 0
    b = edge_blocks()
    e = _block_exponents(b)
    nz = np.abs(b).max(axis=1) > 0
    nkb = K // 16
    r = np.arange(rows)[:, None]
    j = np.arange(nkb)[None, :]
    src = (r * STRIDE + j) % N_EDGE
    g = r * nkb + j
    tgt = np.asarray(TARGETS)[r % len(TARGETS)] + 0 * j
    if exc_every:
        is_exc = g % exc_every == exc_every - 1
        tgt = np.where(is_exc, tgt - np.asarray(exc_depth)[(g // exc_every) % len(exc_depth)], tgt)
    shift = np.where(nz[src], tgt - e[src], 0)
    # The exponent is ceil of an fp32 log2, which rounds onto the integer k for maxima a few ulps above 2^k -- how many depends
    # on |k| (six for |k| >= 17, none for |k| <= 4): a scaled block can land one off and is moved by that one.  Where the
    # count changes between k - 1 and k (|k| = 4, 8, 16) a block can have no scale that lands on k; it stays one below.
    # None of the row targets is such a k, so only exception blocks are affected: d or d + 1 below the row's target.
    is_exc = np.zeros((rows, nkb), bool) if not exc_every else is_exc
    for step in range(3):
        x = np.ldexp(b[src].astype(np.float64), shift[..., None]).astype(np.float32)   # (exact: no value leaves fp32's normals)
        off = np.where(nz[src], tgt - _block_exponents(x.reshape(-1, 16)).reshape(rows, nkb), 0)
        if step == 0:
            shift = shift + off
        elif step == 1:
            shift = shift + np.minimum(off, 0)
    assert set(np.unique(off)) <= {0, 1} and (exc_every == 0 or not off[~is_exc].any()) and (exc_every != 0 or not off.any())
    assert np.array_equal(np.ldexp(x.astype(np.float64), -shift[..., None]), b[src].astype(np.float64))
    x[g % zero_every == zero_every - 1] = 0
    return np.ascontiguousarray(x.reshape(rows, K))


def oracle_codes(x, width, ew=8, bias=127):
    """(mant [rows, K/16, 16] int64, exp [rows, K/16] int64, nonzero [rows, K/16] bool) of x [rows, K]; all-zero blocks:
    mantissas 0 (the library's fill, see the module docstring), exponent left as the oracle gives it and masked by `nonzero`"""
    from oracle import np_oracle as O
    rows, K = x.shape
    code = O.bfp_encode(x, width, ew, bias, [1, 16], True)
    mant = code.mant.reshape(rows, K // 16, 16).astype(np.int64)
    exp = code.exp.reshape(rows, K // 16).astype(np.int64)
    nonzero = np.abs(x.reshape(rows, K // 16, 16)).max(axis=2) > 0
    mant[~nonzero] = 0
    return mant, exp, nonzero


def expected_values(x, width, ew=8, bias=127):
    """float64 [rows, K]: mant * 2^(exp - (width - 1)) per element"""
    mant, exp, _ = oracle_codes(x, width, ew, bias)
    return np.ldexp(mant.astype(np.float64), (exp - (width - 1))[..., None]).reshape(x.shape)


# ---------------------------------------------------------------------------------------------------
# the operand as the library stores it
# ---------------------------------------------------------------------------------------------------
def _row_exceptions(al, rows, nkb):
    from mi355q import ops
    over, ent = ops.row_list_entries(al.sparse, rows, al.list_cap)
    mant = np.zeros((rows, nkb, 16), np.int64)
    exp = np.zeros((rows, nkb), np.int64)
    mask = np.zeros((rows, nkb), bool)
    for e in ent:
        assert not mask[e[0], e[1]], "a block is listed once"
        assert e[0] // 256 == e[0] // 256
        mask[e[0], e[1]] = True
        exp[e[0], e[1]] = e[2]
        mant[e[0], e[1]] = e[4:8].astype(np.int32).view(np.int8)
    return over, mant, exp, mask


def _untile(tiled, rows, K):
    """tiled aligned mantissas (1-KiB pieces of 16 rows x 64 B laid out [block 0..3][row 0..15][16 B]) -> [rows, K] int8"""
    t = tiled.cpu().numpy().view(np.int8)
    kp = K // 64
    rp = (t.size // (kp * 1024)) * 16
    return np.ascontiguousarray(t[: (rp // 16) * kp * 1024].reshape(rp // 16, kp, 4, 16, 16).transpose(0, 3, 1, 2, 4)
                                ).reshape(rp, K)[:rows]


def operand_codes(op, rows, K):
    """(mant [rows, K/16, 16] int64, stored exponent codes [rows, K/16] int64) of an AlignedOperand, exception list aside"""
    mant = _untile(op.tiled, rows, K).reshape(rows, K // 16, 16).astype(np.int64)
    code = op.exp.cpu().numpy().reshape(rows, K // 16).astype(np.int64)
    return mant, code


def decode_operand(op, rows, K):
    """float64 [rows, K]: what the operand denotes -- untiled int8 mantissa x 2^(stored code - bias - (width - 1)), plus the
    exception entries of its row list"""
    mant, code = operand_codes(op, rows, K)
    off = op.exp_bias + op.mbits
    v = np.ldexp(mant.astype(np.float64), (code - off)[..., None])
    if op.sparse is not None:
        _, em, ee, emask = _row_exceptions(op, rows, K // 16)
        assert np.all(mant[emask] == 0), "an exception block is zeroed in the operand"
        v = v + np.ldexp(em.astype(np.float64), (ee - off)[..., None]) * emask[..., None]
    return v.reshape(rows, K)


# ---------------------------------------------------------------------------------------------------
# the row rule of csrc/mi355q_align_row.h, restated (host test: how many exception blocks a layout produces)
# ---------------------------------------------------------------------------------------------------
def row_rule(mant, exp, nonzero, bias=127):
    """per row: (E or None when the row has no non-zero block, exception mask [K/16]) for oracle codes of one row.
    E is the smallest exponent if every block can be shifted left onto it inside int8 (head-room = 7 - bit length of the
    block's largest |mantissa|); otherwise the start of the window [E, E + head-room(block)] that holds the most blocks,
    the smallest such start; blocks outside it are exceptions."""
    amax = np.abs(mant).max(axis=1)
    has = nonzero & (amax > 0)
    if not has.any():
        return None, np.zeros(len(exp), bool)
    code = exp + bias
    head = np.array([7 - int(a).bit_length() for a in amax])
    c, h = code[has], head[has]
    if c.min() >= (c - h).max():
        return int(c.min()) - bias, np.zeros(len(exp), bool)
    cnt = np.zeros(256, np.int64)
    for ci, hi in zip(c, h):
        cnt[max(ci - hi, 0): ci + 1] += 1
    best = int(np.argmax(cnt))                   # (first maximum: the smallest start)
    inside = (code >= best) & (code - best <= head)
    return best - bias, has & ~inside


def exceptions_per_bucket(x, width, ew=8, bias=127):
    """exception blocks per 256-row bucket of x's row-aligned operand, were every bucket large enough"""
    mant, exp, nonzero = oracle_codes(x, width, ew, bias)
    rows = x.shape[0]
    out = np.zeros(-(-rows // 256), np.int64)
    for r in range(rows):
        out[r // 256] += int(row_rule(mant[r], exp[r], nonzero[r], bias)[1].sum())
    return out


def edge_counts(x, width, ew=8, bias=127):
    """what a layout holds, counted from the oracle's codes: ties (elements whose pre-rounding mantissa (|x| + 1e-9) 2^(mb - e),
    in fp32 as the oracle forms it, is k + 1/2), clamps (blocks whose maximum rounds up to 2^mb and is clamped), near
    (non-zero blocks whose maximum lies within 8 ulps of a power of two, either side), the signs present, elements with
    x + 1e-9 == 0 and with 0 < |x| <= 1e-8"""
    F32 = np.float32
    mb = width - 1
    rows, K = x.shape
    mant, exp, nonzero = oracle_codes(x, width, ew, bias)
    xb = x.reshape(rows, K // 16, 16)
    value = np.abs(xb) + F32(1e-9)
    p2e = np.ldexp(np.float64(1.0), exp).astype(F32)[..., None]
    with np.errstate(over="ignore"):
        pre = (value / p2e) * F32(2 ** mb)
    assert pre.dtype == np.float32
    frac = pre.astype(np.float64) - np.floor(pre.astype(np.float64))
    ties = (frac == 0.5) & nonzero[..., None] & (pre < 2 ** mb)
    bmax = np.abs(xb).max(axis=2)
    with np.errstate(over="ignore"):
        bpre = ((bmax + F32(1e-9)) / p2e[..., 0]) * F32(2 ** mb)
    clamps = nonzero & (np.rint(bpre) >= 2 ** mb) & (bpre < 2 ** mb + 1)
    bits = bmax.view(np.uint32).astype(np.int64)
    frac_bits = bits & 0x7FFFFF
    near = nonzero & ((frac_bits <= 8) | (frac_bits >= 0x800000 - 8))
    return dict(ties=int(ties.sum()), clamps=int(clamps.sum()), near=int(near.sum()),
                pos=int((mant > 0).sum()), neg=int((mant < 0).sum()),
                cancel=int(((x + F32(1e-9)) == 0).sum()), tiny=int(((np.abs(x) > 0) & (np.abs(x) <= F32(1e-8))).sum()))


# ---------------------------------------------------------------------------------------------------
# the layouts the GPU tests run (tests/test_gpu_row_quantiser_edges.py), checked on the CPU by tests/test_row_edges_host.py
# ---------------------------------------------------------------------------------------------------
ELEMENT_WIDTHS = (2, 4, 5, 6, 8)
ELEMENT_SHORT_K = (64, 320, 1024)
ELEMENT_LONG_K = (1088, 2048, 2112, 4096, 5120, 8192, 11008, 12352, 16384)   # one K per build: planned_build(), tests/test_quant_rows_plan.py
ELEMENT_LONG_ROWS = 19
GRID_WALK_ROWS = 429                                       # rows of short(64) the grid-walk case takes (not a multiple of 128)

ALIGNED_WIDTHS = (4, 6)
# K -> rows.  One exception block per max(64, 2 K/16 + 1) blocks: about every other row has one, the rest none; the rows are
# as many as it takes for 200 ties over the two widths (tests/test_row_edges_host.py counts them)
ALIGNED_ROWS = {64: 456, 1024: 29, 2048: 24, 4096: 19, 8192: 12, 11008: 12, 16384: 12}
OVERFLOW_K, OVERFLOW_WIDTH = 1024, 8                       # short(1024) at W8: no head-room, every exponent step is an exception

MX_WIDTHS = (4, 5)
MX_ROWS = {256: 456, 4096: 38}                             # no exception blocks: every 32-group's two blocks share an exponent


def rows_env_words(env):
    """the 3 words of RowsEnv (csrc/mi355q_quant_plan.h) for a set of environment strings: what read_rows_env() makes of them"""
    return [max(int(env.get("MI355Q_QROWS_GRID", 0)), 0), int("MI355Q_QROWS_VARIANT" in env and int(env["MI355Q_QROWS_VARIANT"]) == 0),
            int(env.get("MI355Q_QROWS_SHORT", 1))]


@functools.lru_cache(maxsize=None)
def _rows_plan_hook():
    import ctypes as C
    from mi355q import _lib
    fn = C.CDLL(str(_lib.library_path())).mi355q_debug_quant_rows_plan
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    return fn


def rows_plan(kind, rows, cols, pre_op=0, segmented=0, env=None):
    """[maxit, full, seg, mx, pre, st16, wps, grid, rc] of a row quantiser launch, from mi355q_debug_quant_rows_plan (no GPU, no launch).
    kind: 0 int8 rows, 1 MX rows, 2 class-aware rows; env: environment strings, None: the process environment"""
    import ctypes as C
    out = (C.c_int32 * 12)(*([-99] * 12))
    words = None if env is None else (C.c_int32 * 3)(*rows_env_words(env))
    assert _rows_plan_hook()((C.c_int64 * 5)(kind, rows, cols, pre_op, segmented), words, out) == 0
    assert list(out[9:]) == [0, 0, 0]
    return [out[i] & 0xFFFFFFFF if i == 7 else out[i] for i in range(9)]


def planned_build(K, pre_op=0, segmented=0, kind=0, env=None):
    """(kind, MAXIT, FULL, SEG, MX, PRE, ST16, WPS): the compiled build a call of the GPU edge tests runs"""
    plan = rows_plan(kind, ELEMENT_LONG_ROWS, K, pre_op, segmented, env or {})
    assert plan[8] == 0
    return (kind, *plan[:7])


def _frozen(x):
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def element_layout(K):
    return _frozen(short(K) if K <= 1024 else long(K, ELEMENT_LONG_ROWS))


@functools.lru_cache(maxsize=None)
def aligned_layout(K):
    return _frozen(long(K, ALIGNED_ROWS[K], exc_every=max(64, 2 * (K // 16) + 1)))


@functools.lru_cache(maxsize=None)
def mx_layout(K):
    return _frozen(long(K, MX_ROWS[K], exc_every=0))


DEEP_K = (1024, 4096, 11008)
DEEP_WIDTHS = (4, 6, 8)


@functools.lru_cache(maxsize=None)
def deep_layout(K):
    """long(K, 19) with the exception blocks 24..28 exponents below the row's target instead of 5..9: blocks below 2^-23
    next to blocks at ordinary magnitudes.  A wave that holds such a block takes the kernel's exact per-element rule
    (mant_f) for all its blocks, the ties at exponents -3 .. 30 among them -- in the other layouts the only rows with so
    small a block are those around 2^-20, where the +1e-9 leaves no tie."""
    return _frozen(long(K, ELEMENT_LONG_ROWS, exc_depth=(24, 25, 26, 27, 28)))


def exact_rule_waves(x, width):
    """[rows, K/16] bool: blocks whose wave (blocks 64 i + 16 w .. 64 i + 16 w + 15, all i, of one row) holds a block with
    mantissa scale 2^(mb - e) >= 2^28 -- the condition under which bfp_quant_align_rows_kernel leaves its fused fast path"""
    rows, K = x.shape
    nkb = K // 16
    _, exp, nz = oracle_codes(x, width)
    big = nz & ((width - 1) - exp >= 28)
    wave = (np.arange(nkb) % 64) // 16
    out = np.zeros((rows, nkb), bool)
    for w in range(4):
        out[:, wave == w] = big[:, wave == w].any(axis=1)[:, None]
    return out


def tie_mask(x, width, rounded_down=False):
    """[rows, K/16, 16] bool: elements of non-zero blocks whose mantissa before rounding is k + 1/2 (edge_counts);
    rounded_down: only those with k even, which round-half-even takes to k and round-half-away to k + 1"""
    mb = width - 1
    rows, K = x.shape
    _, exp, nz = oracle_codes(x, width)
    value = np.abs(x.reshape(rows, K // 16, 16)) + np.float32(1e-9)
    p2e = np.ldexp(np.float64(1.0), exp).astype(np.float32)[..., None]
    with np.errstate(over="ignore"):
        pre = ((value / p2e) * np.float32(2 ** mb)).astype(np.float64)
    ties = (pre - np.floor(pre) == 0.5) & nz[..., None] & (pre < 2 ** mb)
    return ties & (np.floor(pre) % 2 == 0) if rounded_down else ties


def clamp_layout():
    """short(320) with every third row scaled by 2^12 and every third by 2^-12, for exponent_width 4 / bias 7 (exponents
    clamped to [-7, 8]): blocks at both clamps and in between"""
    x = short(320).copy()
    x[1::3] = np.ldexp(x[1::3], 12)
    x[2::3] = np.ldexp(x[2::3], -12)
    return x


def all_layouts():
    """(name, x, widths, kind) of every base tensor the GPU file quantises; kind: "element" (no alignment), "aligned",
    "overflow", "mx"."""
    out = [(f"element K={K}", element_layout(K), ELEMENT_WIDTHS, "element") for K in ELEMENT_SHORT_K + ELEMENT_LONG_K]
    out.append((f"grid walk K=64 rows={GRID_WALK_ROWS}", element_layout(64)[:GRID_WALK_ROWS], ELEMENT_WIDTHS, "element"))
    out += [(f"aligned K={K}", aligned_layout(K), ALIGNED_WIDTHS, "aligned") for K in ALIGNED_ROWS]
    out.append((f"overflow K={OVERFLOW_K}", element_layout(OVERFLOW_K), (OVERFLOW_WIDTH,), "overflow"))
    out += [(f"mx K={K}", mx_layout(K), MX_WIDTHS, "mx") for K in MX_ROWS]
    out += [(f"deep K={K}", deep_layout(K), DEEP_WIDTHS, "deep") for K in DEEP_K]
    return out
