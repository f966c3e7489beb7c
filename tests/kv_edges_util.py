"""Inputs, expected values and the comparison rule of the KV caches' edge tests (numpy only).

Inputs: the reference's boundary set of tests/row_edges_util.py -- the 1714 + 108 blocks of 16 of edge_blockmax_* / edge_dense_* in
tests/golden/quantizers.npz -- laid out so that every block is one quantiser block of a cache:

  k_layout(blocks, D, tiles)   K [B, 16 tiles, D]: a K block is the 16 keys of one tile at one d.  Block g lies at (b, d, t), g counted
                               in row-major [B, D, tiles] order: `pad.reshape(B, D, 16 tiles)` is k^T.  The remainder of the last row is
                               padded with all-zero blocks, whole blocks only: a zero never shares a block with an edge value.
                               `shift`: block g lies in tile (t + shift) % tiles instead (see FILLS)
  v_layout(blocks, D, L)       V [B, L, D]: a V block is 16 consecutive d of one key, the blocks in order along D, then L, then B
  kv_layout(blocks, D, L)      both, with equal B and L: one cache holds the set in either orientation

Block sets (block_set): "bfp" / "bm" -- the x of the _bfp_w6 tags, which is also the x of edge_blockmax_bm / edge_dense_bm -- and
"bm64", the x of edge_blockmaxx64_bm / edge_densex64_bm, the same set scaled into shared biases > 0.

Expected values: the oracle's quantiser (np_oracle.block_fp_quantize for an int format = the width, exponent_width 8, bias 127;
np_oracle.block_minifloat_quantize for a (width, exponent_width, exponent_bias_width) format) on k^T[:, :, :L] and on v[:, :L],
rounded to bf16 -- what tests/test_gpu_kv8_cache.py and tests/test_gpu_kvbm_cache.py compare their seeded inputs with.  The oracle is
pinned to the reference's recorded outputs on these very blocks, in these layouts, by tests/test_kv_edges_host.py."""
import functools

import numpy as np

from tests import row_edges_util as R
from tests.conftest import GOLDEN

F32 = np.float32
N_EDGE = R.N_EDGE
ATOL = F32(1e-8)

# The append schedules, 64 keys each.  The block maximum of 1712 of the 1714 edge_blockmax blocks is element 5: key 5 of a K tile.
# The pieces stop before and after key 5 of tiles 0 and 1 (5, 1 and 5, 1: the open tile is quantised WITHOUT its maximum, then again
# with it -- DESIGN 7b's open-block rule moves the shared exponent), make one key alone, cross a tile (10: the staging pass), cross two
# tiles in one append (26) and end with a whole closed tile (16).  Only tiles 0 and 1 are ever open at 5 keys, so the piecewise runs
# take the K layout twice, with shift 0 and shift 2: every block is once in a tile that is.
FILLS = ((64,), (5, 1, 10, 5, 1, 26, 16))
SHIFTS = (0, 2)
L = 64
assert all(sum(f) == L for f in FILLS)


def lengths_of(fill):
    return tuple(int(n) for n in np.cumsum(fill))


@functools.lru_cache(maxsize=None)
def block_set(name="bfp"):
    """[1822, 16] fp32, read-only: blockmax blocks first, dense blocks behind them"""
    if name in ("bfp", "bm"):
        b = R.edge_blocks()
        if name == "bm":
            z = np.load(GOLDEN / "quantizers.npz")
            assert np.array_equal(b, np.concatenate([z["edge_blockmax_bm/x"], z["edge_dense_bm/x"]]))
    else:
        assert name == "bm64"
        z = np.load(GOLDEN / "quantizers.npz")
        b = np.concatenate([z["edge_blockmaxx64_bm/x"], z["edge_densex64_bm/x"]]).astype(F32)
    assert b.shape == (N_EDGE, 16)
    b.setflags(write=False)
    return b


def rows_for(n_blocks, D, L=L):
    return -(-n_blocks // (D * L // 16))


def k_layout(blocks, D, tiles, shift=0):
    n = len(blocks)
    B = -(-n // (D * tiles))
    pad = np.zeros((B * D * tiles, 16), F32)
    pad[:n] = blocks
    kt = np.roll(pad.reshape(B, D, tiles, 16), shift, axis=2).reshape(B, D, 16 * tiles)          # k^T
    return np.ascontiguousarray(np.swapaxes(kt, 1, 2))


def k_blocks(k, shift=0):
    """k_layout undone: [B D tiles, 16], the padding blocks included"""
    B, L, D = k.shape
    kt = np.swapaxes(k, 1, 2).reshape(B, D, L // 16, 16)
    return np.ascontiguousarray(np.roll(kt, -shift, axis=2)).reshape(-1, 16)


def v_layout(blocks, D, L):
    n = len(blocks)
    per = D * L // 16
    B = -(-n // per)
    pad = np.zeros((B * per, 16), F32)
    pad[:n] = blocks
    return pad.reshape(B, L, D)


def v_blocks(v):
    return np.ascontiguousarray(v).reshape(-1, 16)


def kv_layout(blocks, D, L=L, shift=0):
    k, v = k_layout(blocks, D, L // 16, shift), v_layout(blocks, D, L)
    assert k.shape == v.shape
    return k, v


@functools.lru_cache(maxsize=None)
def layout(name, D, shift=0):
    """(k, v) [B, 64, D] of block_set(name), read-only and shared by the tests"""
    k, v = kv_layout(block_set(name), D, L, shift)
    k.setflags(write=False)
    v.setflags(write=False)
    return k, v


# ---------------------------------------------------------------------------------------------------
# expected values
# ---------------------------------------------------------------------------------------------------
def _quantise(x, fmt):
    """the oracle's quantiser on x [B, rows, cols], blocks of 16 along cols"""
    from oracle import np_oracle as O
    if isinstance(fmt, int):
        return O.block_fp_quantize(x, fmt, 8, 127, block_size=[1, 16])
    return O.block_minifloat_quantize(x, *fmt, block_size=[1, 16], skip_first_dim=True)


def quantised_kv(k, v, fmt):
    """fp32, not yet rounded to bf16: the quantiser on k^T (blocks of 16 keys at one d; the last one padded with zeros, as the open
    tile is) and on v"""
    kq = _quantise(np.ascontiguousarray(np.swapaxes(k, 1, 2)), fmt)
    return np.ascontiguousarray(np.swapaxes(kq, 1, 2)), _quantise(v, fmt)


def expected_bf16(k, v, fmt):
    """what KVCache / PagedKVCache / MinifloatKVCache hold of k, v [B, L, D] (the first L keys): the quantised values are exact in
    bf16, the values 0 < |x| <= 1e-8 the quantisers pass through are rounded to it"""
    from oracle import compare
    kq, vq = quantised_kv(k, v, fmt)
    return compare.bf16_rne(kq), compare.bf16_rne(vq)


def tiny(x):
    return (np.abs(x) > 0) & (np.abs(x) <= ATOL)


def expected_mantissa(k, v, fmt):
    """what PackedKVCache / NibbleKVCache / PagedPackedKVCache hold: expected_bf16 with 0 where 0 < |x| <= 1e-8 -- the one documented
    deviation of a storage of mantissas and block exponents (csrc/mi355q_kvp.h), part of the expectation and not an exclusion"""
    kq, vq = expected_bf16(k, v, fmt)
    return np.where(tiny(k), F32(0), kq), np.where(tiny(v), F32(0), vq)


# ---------------------------------------------------------------------------------------------------
# the comparison rule
# ---------------------------------------------------------------------------------------------------
def differing(got, want):
    """indices [n, ndim] where `got` is not `want`, compared as uint32 WORDS.  Where the expected value is a zero the sign bit is
    masked: the oracle does not pin the sign of a zero output -- the reference gives -0 for a negative input that rounds to mantissa 0
    where the oracle gives +0 (503 elements of the set at width 6), as for the all-zero blocks of
    test_zero_block_fill_speculation_hits_and_misses -- and no cache promises one.  Every non-zero word is compared exactly, and a zero
    is only ever equal to a zero."""
    g, w = np.ascontiguousarray(got, F32).view(np.uint32), np.ascontiguousarray(want, F32).view(np.uint32)
    assert g.shape == w.shape, (g.shape, w.shape)
    keep = np.where((w & np.uint32(0x7FFFFFFF)) == 0, np.uint32(0x7FFFFFFF), np.uint32(0xFFFFFFFF))
    return np.argwhere((g & keep) != (w & keep))


def same(got, want, x, what, must=None, skip=None):
    """assert differing() finds nothing, else report the first index, its input, got and want.  `skip`: elements left out of this
    comparison; `must` (edge_mask): elements that may never be -- they are the reason for the test."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    if must is not None:
        assert must.shape == want.shape and must.any(), f"{what}: no edge element to compare"
        assert skip is None or not (must & skip).any(), f"{what}: {int((must & skip).sum())} edge elements are left out of the comparison"
    if skip is not None:
        got, want = np.where(skip, F32(0), got), np.where(skip, F32(0), want)
    bad = differing(got, want)
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} values differ, first at {tuple(int(j) for j in i)}: input {float(x[i])!r} "
                             f"({int(np.asarray(x[i], F32).view(np.uint32)):#010x}), got {float(got[i])!r} ({int(got.view(np.uint32)[i]):#010x}), "
                             f"want {float(want[i])!r} ({int(want.view(np.uint32)[i]):#010x})"
                             + (f"; {int(must[tuple(bad.T)].sum())} of them edge elements" if must is not None else ""))


# ---------------------------------------------------------------------------------------------------
# what a layout holds: the decisions, as masks
# ---------------------------------------------------------------------------------------------------
def _near_pow2(a, ulps=8):
    """|a| within `ulps` ulps of a power of two, either side (R.edge_counts' `near`)"""
    f = np.abs(a).astype(F32).view(np.uint32).astype(np.int64) & 0x7FFFFF
    return (np.abs(a) > 0) & ((f <= ulps) | (f >= 0x800000 - ulps))


def bfp_masks(x2, width):
    """x2 [rows, 16 n]: dict of bool arrays -- ties [rows, n, 16] (R.tie_mask), clamps and near [rows, n] (blocks, by R.edge_counts'
    definitions: the maximum rounds up to 2^mb and is clamped; the maximum lies within 8 ulps of a power of two), tiny [rows, n, 16]"""
    mb = width - 1
    rows, K = x2.shape
    _, exp, nz = R.oracle_codes(x2, width)
    xb = x2.reshape(rows, K // 16, 16)
    p2e = np.ldexp(np.float64(1.0), exp).astype(F32)
    bmax = np.abs(xb).max(axis=2)
    with np.errstate(over="ignore"):
        bpre = ((bmax + F32(1e-9)) / p2e) * F32(2 ** mb)
    return dict(ties=R.tie_mask(x2, width), clamps=nz & (np.rint(bpre) >= 2 ** mb) & (bpre < 2 ** mb + 1), near=nz & _near_pow2(bmax),
                tiny=tiny(xb))


def bm_masks(x2, fmt):
    """the same for block_minifloat: ties (the fraction before rounding, as bm_encode forms it, is j + 1/2 below the clamp), near (the
    block maximum within 8 ulps of a power of two: the shared bias's floor band) and near_elem (|x| + 1e-9 within 8 ulps: the element
    exponent's), tiny"""
    from oracle import np_oracle as O
    width, ew, bw = fmt
    mb = width - ew - 1
    rows, K = x2.shape
    code = O.bm_encode(x2, width, ew, bw, [1, 16], True)
    xb = x2.reshape(rows, K // 16, 16)
    nz = np.abs(xb).max(axis=2) > 0
    value = np.abs(code.blocks).reshape(xb.shape)
    e = code.exp.reshape(xb.shape)
    shift = F32(2 ** mb)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        mant = value / O.pow2_f32(e)
        pre = np.where(code.normal.reshape(xb.shape), mant * shift - shift, mant * shift / F32(2.0)).astype(np.float64)
    ties = (pre - np.floor(pre) == 0.5) & (pre > 0) & (pre < 2 ** mb - 1) & nz[..., None] & ~tiny(xb) & (xb != 0)
    return dict(ties=ties, near=nz & _near_pow2(np.abs(xb).max(axis=2)), near_elem=_near_pow2(np.abs(xb) + F32(1e-9)) & (xb != 0) & ~tiny(xb),
                tiny=tiny(xb))


def _elementwise(m):
    """ties | tiny | every element of a clamp / near block"""
    out = m["ties"] | m["tiny"] | m["near"][..., None]
    for name in ("clamps",):
        if name in m:
            out = out | m[name][..., None]
    if "near_elem" in m:
        out = out | m["near_elem"]
    return out


def masks(x2, fmt):
    return bfp_masks(x2, fmt) if isinstance(fmt, int) else bm_masks(x2, fmt)


def edge_mask(k, v, fmt):
    """(K mask, V mask) [B, L, D] bool over the first L keys: the elements no comparison may leave out -- the ties, the elements
    0 < |x| <= 1e-8 and every element of a block whose maximum is clamped or lies near a power of two, with the oracle's exponents at
    this length (an open K tile is its keys so far and zeros)"""
    B, L, D = k.shape
    Lp = -(-L // 16) * 16
    kt = np.zeros((B, D, Lp), F32)
    kt[:, :, :L] = np.swapaxes(k, 1, 2)
    mk = _elementwise(masks(kt.reshape(B * D, Lp), fmt)).reshape(B, D, Lp)
    mv = _elementwise(masks(np.ascontiguousarray(v).reshape(B * L, D), fmt)).reshape(B, L, D)
    return np.ascontiguousarray(np.swapaxes(mk, 1, 2)[:, :L]), mv


def counts_at(k, v, fmt):
    """ties and near-power-of-two block maxima among the blocks complete or open at this length (k, v [B, L, D]), K and V apart"""
    B, L, D = k.shape
    Lp = -(-L // 16) * 16
    kt = np.zeros((B, D, Lp), F32)
    kt[:, :, :L] = np.swapaxes(k, 1, 2)
    out = {}
    for name, x2 in (("K", kt.reshape(B * D, Lp)), ("V", np.ascontiguousarray(v).reshape(B * L, D))):
        m = masks(x2, fmt)
        out[name] = dict(ties=int(m["ties"].sum()), near=int(m["near"].sum()))
    return out


def k_exponents(k, width=6):
    """the oracle's shared exponent of every K block of k [B, L, D] (L a multiple of 16 after zero padding), [B, D, tiles], and
    whether the block holds a non-zero value"""
    B, L, D = k.shape
    Lp = -(-L // 16) * 16
    kt = np.zeros((B, D, Lp), F32)
    kt[:, :, :L] = np.swapaxes(k, 1, 2)
    _, exp, nz = R.oracle_codes(kt.reshape(B * D, Lp), width)
    return exp.reshape(B, D, Lp // 16), nz.reshape(B, D, Lp // 16)


# ---------------------------------------------------------------------------------------------------
# what the GPU file runs (tests/test_gpu_kv_edges.py), checked on the CPU by tests/test_kv_edges_host.py
# ---------------------------------------------------------------------------------------------------
SHAPES = (32, 128)                                         # D: B = 15 and B = 4 at L = 64
D_CHUNKS = 96                                              # three chunks of 32: B = 5
BFP_WIDTHS = (2, 4, 6, 8, 9)
GOLDEN_WIDTHS = (4, 6, 8)                                  # widths with recorded reference outputs on the edge set
BM_FORMATS = ((8, 4, 8), (6, 3, 8), (8, 3, 2))             # recorded outputs: (8, 4, 8) only
BM_SETS = ("bm", "bm64")
RAGGED_SHORT = 27                                          # the ragged run's shorter row: ends inside tile 1
