"""CPU: the inputs of tests/test_gpu_row_quantiser_edges.py do what those tests rely on, shown with the oracle alone.

* short(64) is the reference's edge set: the oracle on it reproduces the golden mantissas and exponents of
  edge_blockmax_bfp_w{4,6,8} / edge_dense_bfp_w{4,6,8} block for block.
* every layout the GPU file quantises holds the decisions it is there for (tests/row_edges_util.py: edge_counts).  A tie is
  an (element, width) pair -- the mantissa before rounding depends on the width -- so ties are counted over the widths the
  GPU file runs the layout at; the fixture's half-way values were made for 1, 3, 5 and 7 mantissa bits, and those below
  ~2^-5 leave the tie when the fp32 sum |x| + 1e-9 rounds up, which is why W5 and small widths contribute few.
* the row rule of csrc/mi355q_align_row.h, restated in numpy, gives the exception blocks per 256-row bucket: within the
  default bucket (120) for the aligned layouts, beyond it for the overflow layout.
The counts are in the assertion messages; when this was written (ties per width in the order the layout is run at):

  layout (rows)            ties                        clamps >=  near   exception blocks per 256-row bucket
  element K=64/320/1024    20/43/32/158/280            588        1007
  element K=1088 (19)      12/18/8/87/148              522        788
  element K=2048 (19)      25/36/29/141/266            964        1471
  element K=4096 (19)      25/40/36/172/374            1863       2818
  element K=11008 (19)     101/216/149/711/1119        4526       6506
  element K=16384 (19)     166/370/289/1158/2099       6457       9496
  grid walk K=64 (429)     20/42/32/158/280            531        943
  aligned K=64 (456)       44/232    (W4/W6)           651        992    16, 12
  aligned K=1024 (29)      45/175                      659        1034   14
  aligned K=2048 (24)      59/199                      1015       1512   11
  aligned K=4096 (19)      40/172                      1882       2818   9
  aligned K=8192 (12)      119/358                     2093       3023   5
  aligned K=11008 (12)     182/598                     2791       4077   5
  aligned K=16384 (12)     272/869                     4336       6549   5
  overflow K=1024 W8 (29)  280                         588        1007   626
  mx K=256 (456)           177/107   (W4/W5)           2679       3968
  mx K=4096 (38)           198/158                     3436       4994
  deep K=1024 (19)         18/83/101 (W4/W6/W8)        486        744    on exact-rule waves: 5/7/30, rounded down 2/4/15
  deep K=4096 (19)         40/172/374                  1845       2818   17/9/59, 8/5/29
  deep K=11008 (19)        203/711/1118                4481       6506   15/50/162, 8/25/80
"""
import numpy as np
import pytest

from tests import row_edges_util as U

LAYOUTS = U.all_layouts()


@pytest.mark.parametrize("width", [4, 6, 8])
def test_short_64_is_the_reference_edge_set(width, golden_quantizers):
    from oracle import np_oracle as O
    _, data = golden_quantizers
    x = U.short(64)
    assert x.shape == (456, 64) and not x.reshape(-1, 16)[U.N_EDGE:].any()
    code = O.bfp_encode(x, width, 8, 127, [1, 16], True)
    order = U.short_order()
    mant = np.empty((U.N_EDGE, 16), np.int64)
    exp = np.empty(U.N_EDGE, np.int64)
    mant[order], exp[order] = code.mant[:U.N_EDGE], code.exp[:U.N_EDGE]            # undo the ordering
    gm = np.concatenate([data[f"edge_blockmax_bfp_w{width}/mant"], data[f"edge_dense_bfp_w{width}/mant"]])
    ge = np.concatenate([data[f"edge_blockmax_bfp_w{width}/exp"], data[f"edge_dense_bfp_w{width}/exp"]])
    assert np.array_equal(mant, gm) and np.array_equal(exp, ge)
    # and the tensor is the fixture's, block for block
    assert np.array_equal(x.reshape(-1, 16)[:U.N_EDGE][np.argsort(order)], U.edge_blocks())
    assert np.all(np.diff(U._block_exponents(x.reshape(-1, 16)[:U.N_EDGE])) >= 0)


def test_long_layout_visits_every_block_and_lands_on_its_targets():
    assert np.gcd(U.STRIDE, U.N_EDGE) == 1
    K, rows = 4096, U.ELEMENT_LONG_ROWS
    x = U.long(K, rows)
    nkb = K // 16
    _, exp, nz = U.oracle_codes(x, 6)
    g = np.arange(rows * nkb).reshape(rows, nkb)
    is_exc, is_zero = g % 64 == 63, g % 97 == 96
    tgt = np.asarray(U.TARGETS)[np.arange(rows) % 6][:, None] + 0 * g
    plain = nz & ~is_exc
    assert np.array_equal(exp[plain], tgt[plain]), "power-of-two scaling puts every block on its row's target"
    d = (tgt - exp)[is_exc & nz]
    assert {5, 6, 7, 8, 9} <= set(d) <= {5, 6, 7, 8, 9, 10}     # (10: a block no scale puts on its exponent, row_edges_util.long)
    assert not nz[is_zero].any() and is_zero.sum() > 40
    # scaled blocks keep their fraction bits
    b = U.edge_blocks()
    src = (np.arange(rows)[:, None] * U.STRIDE + np.arange(nkb)[None]) % U.N_EDGE
    keep = ~is_zero
    got = x.reshape(rows, nkb, 16)[keep].view(np.uint32) & 0x807FFFFF
    assert np.array_equal(got[b[src][keep] != 0], (b[src][keep].view(np.uint32) & 0x807FFFFF)[b[src][keep] != 0])
    # 1822 consecutive blocks from any start are the whole set
    assert len(set(((np.arange(U.N_EDGE) * U.STRIDE) % U.N_EDGE).tolist())) == U.N_EDGE


@pytest.mark.parametrize("name,x,widths,kind", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_layout_holds_the_decisions_it_is_there_for(name, x, widths, kind):
    counts = {w: U.edge_counts(x, w) for w in widths}
    msg = f"{name}: " + "; ".join(f"W{w} {c}" for w, c in counts.items())
    assert sum(c["ties"] for c in counts.values()) >= 200, msg
    for c in counts.values():
        assert c["clamps"] >= 20, msg
        assert c["near"] >= 50, msg
        assert c["pos"] > 0 and c["neg"] > 0, msg
        if kind in ("element", "overflow") and x.shape[1] <= 1024:      # the short layouts: magnitudes as the reference saw them
            assert c["cancel"] >= 1 and c["tiny"] >= 1, msg


@pytest.mark.parametrize("name,x,widths,kind", [l for l in LAYOUTS if l[3] in ("aligned", "overflow")],
                         ids=[l[0] for l in LAYOUTS if l[3] in ("aligned", "overflow")])
def test_exception_blocks_per_bucket(name, x, widths, kind):
    for w in widths:
        per = U.exceptions_per_bucket(x, w)
        msg = f"{name} W{w}: exception blocks per 256-row bucket {per.tolist()}"
        if kind == "aligned":
            assert per.max() <= 120 and per.sum() >= 1, msg
            mant, exp, nz = U.oracle_codes(x, w)
            free = [r for r in range(x.shape[0]) if nz[r].any() and not U.row_rule(mant[r], exp[r], nz[r])[1].any()]
            assert free, msg + ": no row without an exception"
        else:
            assert per.max() > 120, msg


@pytest.mark.parametrize("K", U.DEEP_K)
def test_deep_layout_puts_ties_on_the_exact_rule_path(K):
    """ties that round-half-even and round-half-away treat differently (k + 1/2 with k even) in waves that take the
    kernel's per-element rule: at least one per width (one suffices to tell the two roundings apart; the counts are in
    the message).  The element layouts have none there, which is why this layout exists."""
    x = U.deep_layout(K)
    found = {}
    for w in U.DEEP_WIDTHS:
        on_path = U.exact_rule_waves(x, w)[..., None]
        found[w] = (int((U.tie_mask(x, w) & on_path).sum()), int((U.tie_mask(x, w, rounded_down=True) & on_path).sum()))
    msg = f"deep K={K}: (ties, of them rounded down to even) on exact-rule waves per width {found}"
    assert all(even >= 1 for _, even in found.values()), msg
    for Ke in (64, 1024, 4096):
        xe = U.element_layout(Ke)
        assert not any((U.tie_mask(xe, w) & U.exact_rule_waves(xe, w)[..., None]).any() for w in U.ELEMENT_WIDTHS)


@pytest.mark.parametrize("K", sorted(U.MX_ROWS))
def test_mx_layout_fits_every_group(K):
    """two blocks of a 32-group at most 3 (W4) / 2 (W5) exponents apart: here every non-zero block of a row has the row's one"""
    x = U.mx_layout(K)
    for w in U.MX_WIDTHS:
        mant, exp, nz = U.oracle_codes(x, w)
        tgt = np.asarray(U.TARGETS)[np.arange(x.shape[0]) % 6][:, None] + 0 * exp
        assert np.array_equal(exp[nz], tgt[nz])
        assert np.abs(mant).max() <= 2 ** (w - 1) - 1 and 127 + exp[nz].min() - (w - 1) + 3 >= 0


def test_row_rule_restated_on_hand_made_rows():
    """the restatement against rows whose answer is plain from the header comment of csrc/mi355q_align_row.h"""
    def rule(codes, amaxes):
        mant = np.zeros((len(codes), 16), np.int64)
        mant[:, 0] = amaxes
        nz = np.asarray(amaxes) > 0
        return U.row_rule(mant, np.asarray(codes, np.int64), nz)
    E, exc = rule([3, 5, 4], [16, 31, 20])              # head-room 2 each: all shift onto 3
    assert E == 3 and not exc.any()
    E, exc = rule([3, 6, 6, 6], [16, 31, 20, 17])       # 3 is out of reach of the 6s: window start 4 keeps the three 6s
    assert E == 4 and exc.tolist() == [True, False, False, False]
    E, exc = rule([0, 9, 0, 9], [31, 31, 31, 31])       # two windows tie: the smaller start
    assert E == -2 and exc.tolist() == [False, True, False, True]
    E, exc = rule([2, 5], [1, 31])                      # every window holds one block: the smallest start, 2 - head-room 6
    assert E == -4 and exc.tolist() == [False, True]
    E, exc = rule([7, 7], [0, 0])
    assert E is None and not exc.any()
