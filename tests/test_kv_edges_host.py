"""CPU: the inputs and expected values of tests/test_gpu_kv_edges.py do what those tests rely on, shown with the oracle and the
reference's recorded outputs alone (tests/kv_edges_util.py).

* both layouts hold each of the 1822 edge blocks exactly once, the rest being whole all-zero blocks;
* the oracle on the full-length K and V layouts gives the golden `y` of edge_blockmax_bfp_w{4,6,8} / edge_dense_bfp_w{4,6,8} and of
  edge_blockmax_bm / edge_dense_bm / edge_blockmaxx64_bm / edge_densex64_bm block for block, under the comparison rule the GPU file
  uses (a zero's sign is not pinned) -- the tags tests/test_oracle_golden.py pins the oracle to.  Widths 2 and 9 and the minifloat
  formats (6, 3, 8) and (8, 3, 2) have no recorded outputs on the edge set: for those the oracle alone is the expectation;
* the layouts hold the tie counts of the reference set per width (20 / 43 / 158 / 280 / 0 at widths 2 / 4 / 6 / 8 / 9), both signs
  and the 2960 elements 0 < |x| <= 1e-8, and every quantised value is exact in bf16;
* at every intermediate length of the append schedules, every width and every minifloat format the GPU file runs, the blocks complete
  or open at that length hold block maxima near a power of two in K and in V, and ties wherever the format has any (block_fp width 9
  has none at all: 2^8 (|x| + 1e-9) / 2^e is never k + 1/2 on this set);
* the open tile really moves exponents: the K blocks whose shared exponent at 5 keys of their tile differs from the one at 6 keys, or
  that are still all zero at 5, number 1714 over the two tile shifts the piecewise runs take (857 each: tiles 0 and 1 of 4)."""
import numpy as np
import pytest

from tests import kv_edges_util as U
from tests import row_edges_util as R

TIES = {2: 20, 4: 43, 6: 158, 8: 280, 9: 0}
PIECEWISE = U.lengths_of(U.FILLS[1])
SETS = [("bfp", w) for w in U.BFP_WIDTHS] + [(s, f) for s in U.BM_SETS for f in U.BM_FORMATS]


def test_the_schedules():
    assert U.FILLS == ((64,), (5, 1, 10, 5, 1, 26, 16)) and PIECEWISE == (5, 6, 16, 21, 22, 48, 64)
    assert U.RAGGED_SHORT % 16 != 0 and 16 < U.RAGGED_SHORT < U.L


@pytest.mark.parametrize("name", ["bfp", "bm64"])
@pytest.mark.parametrize("D,B", [(32, 15), (96, 5), (128, 4)])
def test_layouts_hold_every_block_once(name, D, B):
    blocks = U.block_set(name)
    for shift in U.SHIFTS:
        k, v = U.layout(name, D, shift)
        assert k.shape == v.shape == (B, 64, D) and k.dtype == v.dtype == np.float32
        for got in (U.k_blocks(k, shift), U.v_blocks(v)):
            assert np.array_equal(got[:U.N_EDGE].view(np.uint32), blocks.view(np.uint32)), "a block is not where the layout says"
            assert not got[U.N_EDGE:].any(), "the padding is not whole all-zero blocks"
        # the K layout as the issue words it: block g is keys 16 t .. 16 t + 15 at dimension d of row b, (b, d, t) row-major
        for g in (0, 5, 131, U.N_EDGE - 1):
            b, d, t = np.unravel_index(g, (B, D, 4))
            t = (t + shift) % 4
            assert np.array_equal(k[b, 16 * t:16 * t + 16, d], blocks[g])
            b, key, dt = np.unravel_index(g, (B, 64, D // 16))
            assert np.array_equal(v[b, key, 16 * dt:16 * dt + 16], blocks[g])
    assert np.array_equal(np.swapaxes(U.layout(name, D)[0], 1, 2).reshape(-1, 16)[:U.N_EDGE], blocks)      # pad.reshape(B, D, L) is k^T


def test_bm_set_is_the_bfp_set():
    assert U.block_set("bm") is U.block_set("bfp") or np.array_equal(U.block_set("bm"), U.block_set("bfp"))
    assert not np.array_equal(U.block_set("bm64"), U.block_set("bfp"))


def _golden_y(data, tags):
    return np.concatenate([data[f"{t}/y"] for t in tags]).astype(np.float32)


@pytest.mark.parametrize("D", U.SHAPES)
@pytest.mark.parametrize("width", U.GOLDEN_WIDTHS)
def test_oracle_on_the_layouts_is_the_reference_block_fp(D, width, golden_quantizers):
    _, data = golden_quantizers
    want = _golden_y(data, (f"edge_blockmax_bfp_w{width}", f"edge_dense_bfp_w{width}"))
    x = U.block_set("bfp")
    for shift in U.SHIFTS:
        k, v = U.layout("bfp", D, shift)
        kq, vq = U.quantised_kv(k, v, width)
        for what, got in (("K", U.k_blocks(kq, shift)), ("V", U.v_blocks(vq))):
            U.same(got[:U.N_EDGE], want, x, f"{what} layout, width {width}, shift {shift}: oracle vs the reference's y")
            assert not got[U.N_EDGE:].any()
    # the rule's mask is needed, and only for zeros: the reference's -0 where the oracle gives +0
    differ = U.v_blocks(vq)[:U.N_EDGE].view(np.uint32) != want.view(np.uint32)
    assert (want[differ] == 0).all() and (U.v_blocks(vq)[:U.N_EDGE][differ] == 0).all() and (x[differ] < 0).all()
    if width == 6:
        assert int(differ.sum()) == 503


@pytest.mark.parametrize("D", U.SHAPES)
@pytest.mark.parametrize("name,tags", [("bm", ("edge_blockmax_bm", "edge_dense_bm")), ("bm64", ("edge_blockmaxx64_bm", "edge_densex64_bm"))])
def test_oracle_on_the_layouts_is_the_reference_block_minifloat(D, name, tags, golden_quantizers):
    _, data = golden_quantizers
    want = _golden_y(data, tags)
    x = U.block_set(name)
    assert np.array_equal(x, np.concatenate([data[f"{t}/x"] for t in tags]))
    for shift in U.SHIFTS:
        k, v = U.layout(name, D, shift)
        kq, vq = U.quantised_kv(k, v, (8, 4, 8))
        for what, got in (("K", U.k_blocks(kq, shift)), ("V", U.v_blocks(vq))):
            U.same(got[:U.N_EDGE], want, x, f"{what} layout of {name}, shift {shift}: oracle vs the reference's y")
            assert not got[U.N_EDGE:].any()


@pytest.mark.parametrize("name,fmt", SETS, ids=[f"{s}-{f}" for s, f in SETS])
def test_quantised_values_are_exact_in_bf16(name, fmt):
    from oracle import compare
    k, v = U.layout(name, 32)
    for x, q in zip((k, v), U.quantised_kv(k, v, fmt)):
        big = np.abs(x) > U.ATOL
        assert np.array_equal(compare.bf16_rne(q)[big].view(np.uint32), q[big].view(np.uint32))
        assert np.array_equal(q[~big].view(np.uint32) & 0x7FFFFFFF, x[~big].view(np.uint32) & 0x7FFFFFFF), "the pass-through values"
    # expected_mantissa is expected_bf16 but for exactly the tiny elements, which are +0
    for x, a, b in zip((k, v), U.expected_bf16(k, v, fmt), U.expected_mantissa(k, v, fmt)):
        t = U.tiny(x)
        assert np.array_equal(a[~t].view(np.uint32), b[~t].view(np.uint32)) and (b[t].view(np.uint32) == 0).all() and (a[t] != 0).all()


@pytest.mark.parametrize("D", U.SHAPES + (U.D_CHUNKS,))
def test_full_length_layouts_hold_the_reference_counts(D):
    k, v = U.layout("bfp", D)
    B = k.shape[0]
    for x2 in (np.swapaxes(k, 1, 2).reshape(B * D, 64), v.reshape(B * 64, D)):
        for width in U.BFP_WIDTHS:
            c, m = R.edge_counts(x2, width), U.bfp_masks(x2, width)
            assert c["ties"] == TIES[width] == int(m["ties"].sum()), (width, c)
            assert c["clamps"] == int(m["clamps"].sum()) == {2: 853, 4: 669, 6: 616, 8: 588, 9: 572}[width], (width, c)
            assert c["near"] == int(m["near"].sum()) == 1007, (width, c)
            assert c["tiny"] == int(m["tiny"].sum()) == 2960, (width, c)
            assert c["pos"] > 0 and c["neg"] > 0, (width, c)
            if TIES[width]:
                assert R.tie_mask(x2, width, rounded_down=True).any(), "no tie that round-half-away would move"
    for x in (k, v):
        assert (x > 0).any() and (x < 0).any() and int(U.tiny(x).sum()) == 2960


@pytest.mark.parametrize("name,fmt", SETS, ids=[f"{s}-{f}" for s, f in SETS])
def test_every_length_of_the_schedules_holds_edges(name, fmt):
    """counted, not recorded: ties and near-power-of-two block maxima among the blocks complete or open at each length, K and V apart.
    Near maxima: in K and in V at every length.  Ties: in K or V (either tile shift) at every length, for every format that has a tie
    at all; at 5 keys the set "bm" under (8, 4, 8), four ties in all, has none yet and takes its first at 6."""
    full = U.counts_at(*U.layout(name, 32), fmt)
    has_ties = full["K"]["ties"] > 0
    assert has_ties == (fmt != 9), full
    seen = {}
    for n in PIECEWISE:
        per_shift = [U.counts_at(*(x[:, :n] for x in U.layout(name, D, s)), fmt) for s in U.SHIFTS for D in U.SHAPES]
        seen[n] = per_shift
        for c in per_shift:
            assert c["K"]["near"] > 0 and c["V"]["near"] > 0, (name, fmt, n, c)
        ties = sum(c[o]["ties"] for c in per_shift for o in "KV")
        if has_ties and not (n == 5 and (name, fmt) == ("bm", (8, 4, 8))):
            assert ties > 0, (name, fmt, n, per_shift)
        # the mask no comparison may leave out is not empty in either operand
        mk, mv = U.edge_mask(*(x[:, :n] for x in U.layout(name, 32)), fmt)
        assert mk.any() and mv.any()
    assert [c["K"]["near"] for c in seen[64]] == [1007] * len(seen[64])


def test_the_open_tile_moves_exponents():
    """DESIGN 7b's open-block rule: a K tile holding 5 keys is quantised without its block's maximum (element 5) and again, with
    another shared exponent, when key 5 arrives.  Tiles 0 (lengths 5 -> 6) and 1 (21 -> 22) are open at 5 keys; over the two tile
    shifts every block is in one of them once."""
    per_shift = []
    for shift in U.SHIFTS:
        k, _ = U.layout("bfp", 32, shift)
        moved = 0
        for before, after, tile in ((5, 6, 0), (21, 22, 1)):
            (ea, na), (eb, nb) = U.k_exponents(k[:, :before]), U.k_exponents(k[:, :after])
            moved += int((((ea[:, :, tile] != eb[:, :, tile]) | ~na[:, :, tile]) & nb[:, :, tile]).sum())
        per_shift.append(moved)
    assert sum(per_shift) >= 1700 and min(per_shift) >= 850, per_shift


def test_comparison_rule():
    want = np.array([0.0, -0.0, 1.5, -2.0, 0.0], np.float32)
    assert len(U.differing(np.array([-0.0, 0.0, 1.5, -2.0, 0.0], np.float32), want)) == 0              # a zero's sign is not pinned
    assert U.differing(np.array([0.0, 0.0, 1.5, 2.0, 1e-45], np.float32), want).ravel().tolist() == [3, 4]    # a value's is; 0 is only 0
    assert len(U.differing(np.array([np.nan], np.float32), np.array([0.0], np.float32))) == 1
    x = np.arange(5, dtype=np.float32)
    with pytest.raises(AssertionError, match=r"2 values differ, first at \(3,\): input 3.0"):
        U.same(np.array([0.0, 0.0, 1.5, 2.0, 1e-45], np.float32), want, x, "rule")
    must = np.array([False, False, True, False, False])
    with pytest.raises(AssertionError, match="left out"):
        U.same(want, want, x, "rule", must=must, skip=must)
    U.same(want, want, x, "rule", must=must, skip=~must)
