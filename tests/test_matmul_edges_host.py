"""CPU: the inputs and expected values of tests/test_gpu_matmul_edges.py do what those tests rely on, shown with the oracle and the
reference's recorded outputs alone (tests/matmul_edges_util.py).

* every layout (x along K, y along N; sorted and strided order; rows whole and cut in two) holds each of the 1822 edge blocks exactly
  once as one quantiser block, the rest being whole all-zero blocks;
* on these layouts the oracle gives the reference's recorded y of the golden tags (edge_blockmax / edge_dense of bfp_w6, bm, bmx64, bl,
  blx64) block for block, and on edge_zeros_bl / edge_allzero_bl (+ x64) the reference's tensor-wide fill of all-zero blocks;
* for every case the GPU file and its children run (613 products): the selector quantises to ONE non-zero q, every output is one
  non-zero product at most, the float64 product is representable in fp32, is no bf16 / fp32 subnormal and does not overflow; with q
  and the `<= 1e-8 -> bf16` rule the expectation is O.matmul_quantized itself wherever no tiny element is read;
* every layout holds ties, clamps, near maxima, both signs and the 2960 tiny elements (row_edges_util.edge_counts);
* the wave census (kernel 2: quantise_xblk, kernel 3: quantise_lane; a wave of either = 16 rows x the four blocks of a 64-step), summed
  over the construction-A layouts of both orders at B = 1, K = 64 .. 256: (waves, ties, clamps) on the redo path / on the fused path
      block_fp w6          kernel 2: no redo exists (quant_elem_fused has no `near`), 314 fused waves hold 1580 ties, 6160 clamps
                           kernel 3: redo 206 waves, 769 ties, 3840 clamps; fused 108 waves, 811 ties, 2320 clamps
      block_fp w9          no tie in the whole set (as on the KV caches); clamps on both paths
      block_minifloat 848  kernel 2: redo 174 waves, 20 ties; fused 140 waves, 20 ties; kernel 3: redo 205 / 20, fused 109 / 20
      block_log (4,3)      kernel 2: redo 100 waves, fused 214; kernel 3: redo 219, fused 95; clamps on both paths.  A block_log "tie" is an
                           element whose log2 the table decides, which IS `near`: only redo waves can hold one (1830 of them); fused
                           waves hold elements on both sides of the band instead.  (8, 8) clamps nothing on this set.
  The sorted order puts the ties into redo waves, the strided order -- calm blocks dealt first -- into fused ones; the conditions are
  asserted per format and kernel below, the counts above are what they were when this was written."""
import numpy as np
import pytest

from tests import kv_edges_util as KV
from tests import matmul_edges_util as U
from tests import row_edges_util as R


@pytest.mark.parametrize("name", ["bfp", "bm64", "bl", "bl64"])
@pytest.mark.parametrize("kind", U.ORDERS)
def test_layouts_hold_every_block_once(name, kind):
    fmt = {"bfp": U.bfp(6), "bm64": U.bm(8, 4, 8), "bl": U.bl(8, 8), "bl64": U.bl(4, 3)}[name]
    blocks = U.block_set(name)
    perm = U.order(name, fmt, kind)
    assert sorted(perm.tolist()) == list(range(U.N_EDGE))
    for K, rows in ((64, 456), (128, 228), (192, 152), (208, 141), (256, 114)):
        for B in U.BATCHES:
            x = U.x_case(name, fmt, kind, K, B)
            M = -(-rows // B)
            assert x.shape == (B, M, K) and x.dtype == np.float32 and M % 128 != 0
            got = U.layout_blocks(x)
            assert np.array_equal(got[:U.N_EDGE].view(np.uint32), blocks[perm].view(np.uint32)) and not got[U.N_EDGE:].any()
            for g in (0, 7, 500, U.N_EDGE - 1):
                b, m, kb = np.unravel_index(g, (B, M, K // 16))
                assert np.array_equal(x[b, m, 16 * kb:16 * kb + 16], blocks[perm[g]])
    for K, N in U.SHAPES_B:
        y = U.y_case(name, fmt, kind, K, N)
        got = U.layout_blocks(y)
        assert y.shape == (1, K, N) and np.array_equal(got[:U.N_EDGE].view(np.uint32), blocks[perm].view(np.uint32)) and not got[U.N_EDGE:].any()
        k, nb = np.unravel_index(1000, (K, N // 16))
        assert np.array_equal(y[0, k, 16 * nb:16 * nb + 16], blocks[perm[1000]])


def test_block_log_sets():
    assert np.array_equal(U.block_set("bl"), U.block_set("bfp")) and np.array_equal(U.block_set("bl64"), U.block_set("bfp") * np.float32(64))


@pytest.mark.parametrize("key", list(U.GOLDEN_TAGS), ids=lambda k: U.set_id(k))
@pytest.mark.parametrize("kind", U.ORDERS)
def test_oracle_on_the_layouts_is_the_reference(key, kind, golden_quantizers):
    _, data = golden_quantizers
    name, fmt = key
    want = np.concatenate([data[f"{t}/y"] for t in U.GOLDEN_TAGS[key]]).astype(np.float32)
    perm = U.order(name, fmt, kind)
    for K, N in ((64, 64), (208, 208)):
        got = U.layout_blocks(U.quantise(U.x_case(name, fmt, kind, K, 2), fmt))
        assert len(KV.differing(got[:U.N_EDGE], want[perm])) == 0, (key, kind, K)
    if fmt[0] != "bl":
        got = U.layout_blocks(U.quantise(U.y_case(name, fmt, kind, 208, 144), fmt))
        assert len(KV.differing(got[:U.N_EDGE], want[perm])) == 0 and not got[U.N_EDGE:].any()


@pytest.mark.parametrize("tag", ["edge_zeros_bl", "edge_zerosx64_bl", "edge_allzero_bl", "edge_allzerox64_bl"])
def test_oracle_gives_the_reference_fill_of_all_zero_blocks(tag, golden_quantizers):
    meta, data = golden_quantizers
    p = meta[tag]["params"]
    x = data[f"{tag}/x"]
    got = U.quantise(x[None], U.bl(p["width"], p["exponent_bias_width"]))[0]
    assert np.array_equal(got.view(np.uint32), data[f"{tag}/y"].view(np.uint32))
    assert (np.abs(x).reshape(-1, 16).max(axis=1) == 0).any()


def test_every_case_is_an_exact_read_back():
    from oracle import np_oracle as O
    cases = U.all_cases()
    assert len(cases) == 613 and len({c[0] for c in cases}) == 613
    checked = 0
    for n, (key, fmt, x, y) in enumerate(cases):
        e = U.expected_of(key, fmt, x, y)            # (asserts: one q, one term per output, representable in fp32)
        nz = np.abs(e[e != 0])
        assert e.shape == (x.shape[0], x.shape[1], y.shape[2]) and np.isfinite(e).all()
        assert nz.size and nz.min() >= 2.0 ** -126, key
        for t in (U.operand(x, fmt), y if fmt[0] == "bl" else U.operand(y, fmt)):
            a = np.abs(t[t != 0])
            assert a.size == 0 or a.min() >= 2.0 ** -126, f"{key}: an operand value is subnormal in bf16"
        if n % 9 == 0:                                   # the expectation is the oracle's product wherever no tiny element is read
            ref = O.matmul_quantized(x, y, U.oracle_cfg(fmt))
            tiny = np.matmul(KV.tiny(x).astype(np.int64), (y != 0).astype(np.int64)) + np.matmul((x != 0).astype(np.int64), KV.tiny(y).astype(np.int64))
            keep = (tiny == 0) | (fmt[0] == "bl")
            assert len(KV.differing(np.where(keep, e, 0), np.where(keep, ref, 0))) == 0, key
            assert fmt[0] == "bl" or key.startswith("A/clamp") or (~keep).any() or "B/" in key
            checked += 1
    assert checked >= 60
    # d = 0.75 and what it quantises to
    y = U.selectors(64, 64)[0][0]
    # (block_fp width 2: the one mantissa step; block_minifloat (6, 3, 4) and (4, 2, 3): 0.75 is a subnormal of bias 0 whose mantissa
    #  1.5 rounds to even, 2 -- one value each, which is all the read-back needs)
    other = {U.bfp(2): 0.5, U.bm(6, 3, 4): 1.0, U.bm(4, 2, 3): 1.0}
    assert all(U.single_q(y, f) == other.get(f, 0.75) for _, f in U.SETS_B) and U.single_q(y, U.CLAMP_FMT) == 0.75
    one = np.where(y != 0, np.float32(1), np.float32(0))
    assert U.single_q(one, U.bfp(6)) != 1, "1.0 is no fixed point of block_fp: the identity would not do"


def test_selectors_read_every_position_once():
    for K, N in U.SHAPES_A + ((320, 64),):
        for raw in (False, True):
            sels = U.selectors(K, N, B=2, raw=raw)
            assert len(sels) == -(-K // N)
            seen = np.concatenate([s[s >= 0] for _, s in sels])
            assert sorted(seen.tolist()) == list(range(K))
            for y, s in sels:
                assert y.shape == (2, K, N) and ((y != 0).sum(axis=1) == (s >= 0)[None]).all()
                ok = s >= 0
                v = y[:, s[ok], np.arange(N)[ok]]
                if raw:
                    assert (np.abs(v) >= 0.5).all() and (np.abs(v) < 2).all() and (v.view(np.uint32) & 1).all() and len(np.unique(v)) == v.size
                else:
                    assert (v == U.D).all()


@pytest.mark.parametrize("kind", U.ORDERS)
def test_layouts_hold_the_reference_counts(kind):
    for K in (64, 128, 192, 208, 256):
        x = U.x_case("bfp", U.bfp(6), kind, K, 1)[0]
        for width, ties in ((2, 20), (4, 43), (6, 158), (8, 280)):
            c = R.edge_counts(x, width)
            assert c["ties"] == ties and c["clamps"] > 0 and c["near"] == 1007 and c["tiny"] == 2960 and c["pos"] > 0 and c["neg"] > 0, (K, width, c)
    c = R.edge_counts(U.clamp_case(1)[0], 6, 4, 7)
    assert c["clamps"] > 0 and c["tiny"] > 0 and c["pos"] > 0 and c["neg"] > 0, c


def _census(name, fmt):
    tot = {k: {r: np.zeros(3, np.int64) for r in ("redo", "fused")} for k in (2, 3)}
    for kind in U.ORDERS:
        for K in (64, 128, 192, 208, 256):
            c = U.wave_census(U.x_case(name, fmt, kind, K, 1), fmt)
            for k in (2, 3):
                for r in ("redo", "fused"):
                    tot[k][r] += np.array(c[k][r])
    return tot


@pytest.mark.parametrize("s", U.SETS_A, ids=U.set_id)
def test_wave_census(s):
    """redo waves hold a tie and a clamp, and so do waves that stay on the fused path, per format and kernel mapping -- wherever
    the format has a tie / a clamp on this set at all, and a redo at all (see the module docstring)"""
    name, fmt = s
    tot = _census(name, fmt)
    print(U.set_id(s), {k: {r: tuple(int(v) for v in a) for r, a in d.items()} for k, d in tot.items()})
    t, c = U.ties_and_clamps(U.block_set(name), fmt)
    has_ties, has_clamps = t.sum() > 0, c.sum() > 0
    assert has_ties == (fmt != U.bfp(9)) and has_clamps == (fmt not in (U.bl(8, 8),))
    for kernel in (2, 3):
        redo, fused = tot[kernel]["redo"], tot[kernel]["fused"]
        assert redo[0] + fused[0] == 314
        if kernel == 2 and fmt[0] == "bfp":
            assert redo[0] == 0                           # quantise_xblk has no redo for block_fp
        else:
            assert redo[0] > 0 and (not has_ties or redo[1] > 0) and (not has_clamps or redo[2] > 0), (kernel, tot)
        assert fused[0] > 0 and (not has_clamps or fused[2] > 0), (kernel, tot)
        if fmt[0] == "bl":
            assert fused[1] == 0                          # a block_log tie is `near` by definition
        else:
            assert not has_ties or fused[1] > 0, (kernel, tot)
    if fmt[0] == "bl":
        # fused waves hold elements on both sides of the band: both roundings of log2 are decided without the table
        b = U.block_set(name)[U.calm_blocks(U.block_set(name), fmt)]
        from oracle import np_oracle as O
        code = O.bl_encode(b, *fmt[1:], [1, 16], True)
        m = U._bits(np.abs(b) + np.ldexp(np.float32(0.1), -code.bias.astype(np.int64)).astype(np.float32)[:, None]) & 0x7FFFFF
        assert (m < U.bands()["RND_LO_MIN"]).any() and (m > U.bands()["RND_HI_MAX"]).any()


def test_census_restates_the_bands():
    assert U.bands() == dict(CEIL_THR_MAX=0x2D, FLOOR_THR_MIN=0x7FFFA8, RND_LO_MIN=0x3504B5, RND_HI_MAX=0x350531)
    f = lambda bits: np.array([[bits] + [0] * 15], np.uint32).view(np.float32)
    assert U.near_block(f(0x3F800001), U.bfp(6))[0] and U.near_block(f(0x3F80002D), U.bfp(6))[0]
    assert not U.near_block(f(0x3F800000), U.bfp(6))[0] and not U.near_block(f(0x3F80002E), U.bfp(6))[0]
    assert U.near_block(f(0x3F7FFFA8), U.bm(8, 4, 8))[0] and not U.near_block(f(0x3F7FFFA7), U.bm(8, 4, 8))[0]
    assert U.near_block(f(0x00400000), U.bl(8, 8))[0]
    assert not U.near_elem(f(0x3F7FFFFF), U.bfp(6)).any() and U.near_elem(f(0x3F7FFFFF), U.bm(8, 4, 8))[0, 0]


def test_fixed_points():
    kept = {U.set_id(s): U.fixed_point_case(*s)[1] for s in U.SETS_A if s[1][0] != "bl"}
    assert kept["bfp-bfp_2_8_127"] == 0 and all(v >= 33 for k, v in kept.items() if k != "bfp-bfp_2_8_127"), kept


def test_block_log_extras_show_the_fill():
    (k0, x0, y0, _, _, _, f0), (k1, x1, *_), (k2, x2, _, _, _, _, f2) = U.bl_extra_cases()
    q = U.quantise(x0, f0)
    fill = np.unique(q[0, 3, 16:32])
    assert len(fill) == 1 and 2.0 ** -125 <= fill[0] < 2.0 ** -100 and fill[0] != np.float32(2.0 ** -127)
    assert (np.abs(x1).reshape(-1, 16).max(axis=1) == 0).sum() == 12 and not x2.any()
    assert (U.quantise(x2, f2) == np.float32(2.0 ** -7)).all()
