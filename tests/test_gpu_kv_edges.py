"""The append quantiser of every KV-cache storage on the reference's edge set: the 1822 boundary blocks of tests/golden/quantizers.npz
(mantissa ties, block maxima a few ulps either side of a power of two, clamped maxima, the 1e-8 / 1e-9 neighbourhood) laid out so that
each is one K block (16 keys of a tile at one d) and one V block (16 d of one key) of a cache (tests/kv_edges_util.py).  After every
piece of an append schedule dequantised() is compared AS BITS with the oracle's quantiser on the first L keys (a zero's sign aside:
kv_edges_util.differing says why); after the last piece the raw storage must be that of a cache filled by one append.  The schedules
stop before and after key 5 of a tile, where 1712 of the blocks have their maximum: the open tile is quantised without it, then with
it.  tests/test_kv_edges_host.py shows on the CPU that these inputs hold the decisions and that the oracle is the reference on them.

Expected values: expected_bf16 for the bf16 storages (KVCache, PagedKVCache, MinifloatKVCache), expected_mantissa -- 0 where
0 < |x| <= 1e-8, the documented deviation -- for the mantissa storages (PackedKVCache, PagedPackedKVCache, NibbleKVCache).  Widths 2
and 9 and the minifloat formats (6, 3, 8) and (8, 3, 2) have no recorded reference outputs on the set; there the oracle alone speaks."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))

from tests import kv_edges_util as U  # noqa: E402
from tests import paged_util as PU  # noqa: E402
from tests import row_edges_util as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = U.L
PAGE = 32
FILL_IDS = ["one_append", "pieces"]


def _par(fmt):
    if isinstance(fmt, int):
        return (fmt, 8, 127, fmt, 8, 127)
    return (8, 4, 8) + tuple(fmt)                          # the cached operands are the weight sides


def _i32(values):
    import torch
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _storage(cache):
    return tuple(getattr(cache, name) for name in cache.STORAGE)


_EXPECT = {}


def _expected(expect, name, D, shift, fmt, n):
    """(K, V expected, K, V edge mask) of the first n keys of layout(name, D, shift): computed once, shared by the tests, read-only"""
    key = (expect.__name__, name, D, shift, fmt, n)
    if key not in _EXPECT:
        k, v = U.layout(name, D, shift)
        out = expect(k[:, :n], v[:, :n], fmt) + U.edge_mask(k[:, :n], v[:, :n], fmt)
        for a in out:
            a.setflags(write=False)
        _EXPECT[key] = out
    return _EXPECT[key]


def _check(cache, k, v, n, want, what, read=None):
    """dequantised() of the first n keys against (K, V expected, K, V edge mask): everything is compared, the edge elements included"""
    kd, vd = (t.cpu().numpy() for t in (read() if read else cache.dequantised()))
    assert kd.shape == vd.shape == (k.shape[0], n, k.shape[2])
    U.same(kd, want[0], k[:, :n], f"{what}: K at length {n}", must=want[2])
    U.same(vd, want[1], v[:, :n], f"{what}: V at length {n}", must=want[3])
    return kd, vd


def _fill_contiguous(cls, name, D, fmt, fill, expect, shift=0, also=None):
    """a cache of class `cls` filled by `fill` and checked after every piece -> (cache, (kd, vd) at the end).  `also`: called with
    (n, kd, vd) after every piece"""
    k, v = U.layout(name, D, shift)
    B = k.shape[0]
    cache = cls(B, L, D, _par(fmt), _par(fmt), DEV)
    kt, vt = _dev(k), _dev(v)
    at = 0
    for n in fill:
        cache.append(kt[:, at:at + n], vt[:, at:at + n])
        at += n
        assert cache.length == at
        got = _check(cache, k, v, at, _expected(expect, name, D, shift, fmt, at), f"{cls.__name__} {name} D={D} fmt={fmt} shift={shift}")
        if also:
            also(at, *got)
    assert at == L
    return cache, got


def _run_contiguous(cls, name, D, fmt, fill, expect):
    """the schedule (the piecewise one under both tile shifts), then: the raw storage is that of a one-append cache"""
    import torch
    for shift in (U.SHIFTS if len(fill) > 1 else (0,)):
        cache, got = _fill_contiguous(cls, name, D, fmt, fill, expect, shift)
        if len(fill) > 1:
            k, v = U.layout(name, D, shift)
            once = cls(k.shape[0], L, D, _par(fmt), _par(fmt), DEV)
            once.append(_dev(k), _dev(v))
            for a, b, what in zip(_storage(cache), _storage(once), "KV"):
                assert torch.equal(a, b), f"{cls.__name__} D={D} fmt={fmt} shift={shift}: {what} storage after {fill} is not one append's"
    return cache, got


# ---------------------------------------------------------------------------------------------------
# KVCache
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", U.FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("D", U.SHAPES)
@pytest.mark.parametrize("width", U.BFP_WIDTHS)
def test_kvcache(width, D, fill):
    from mi355q import ops
    _run_contiguous(ops.KVCache, "bfp", D, width, fill, U.expected_bf16)


def test_kvcache_three_chunks():
    from mi355q import ops
    _run_contiguous(ops.KVCache, "bfp", U.D_CHUNKS, 6, U.FILLS[1], U.expected_bf16)


# ---------------------------------------------------------------------------------------------------
# the ragged run: three extra rows in front of the edge rows
# ---------------------------------------------------------------------------------------------------
def _ragged(cls, name, fmt, expect, D=32):
    """Rows 0 .. 2 are copies of edge rows 0 .. 2 and reach L, U.RAGGED_SHORT (inside tile 1) and 0 keys; the edge rows behind them
    all reach L.  Every piece is one ragged append (lengths=, counts=), the input rows behind a row's count full of NaN.  Expected per
    row: the oracle on THAT ROW ALONE at its own length, zeros behind it."""
    import torch
    k0, v0 = U.layout(name, D)
    k, v = np.concatenate([k0[:3], k0]), np.concatenate([v0[:3], v0])
    B = k.shape[0]
    goal = [L, U.RAGGED_SHORT, 0] + [L] * (B - 3)
    cache = cls(B, L, D, _par(fmt), _par(fmt), DEV)
    have = [0] * B
    for n in U.FILLS[1]:
        counts = [min(n, g - h) for g, h in zip(goal, have)]
        kin, vin = np.full((B, n, D), np.nan, np.float32), np.full((B, n, D), np.nan, np.float32)
        for b, c in enumerate(counts):
            kin[b, :c], vin[b, :c] = k[b, have[b]:have[b] + c], v[b, have[b]:have[b] + c]
        cache.append(_dev(kin), _dev(vin), lengths=_i32(have), counts=_i32(counts), max_length=max(have))
        have = [h + c for h, c in zip(have, counts)]
        top = max(have)
        kd, vd = (t.cpu().numpy() for t in cache.dequantised(lengths=_i32(have), max_length=top))
        assert kd.shape == (B, top, D)
        for b, n_b in enumerate(have):
            what = f"{cls.__name__} ragged, row {b} at {n_b} of {have[:4]}"
            assert not kd[b, n_b:].any() and not vd[b, n_b:].any(), f"{what}: values behind its length"
            if n_b == 0:
                continue
            kb, vb = k[b:b + 1, :n_b], v[b:b + 1, :n_b]
            (kq, vq), (mk, mv) = expect(kb, vb, fmt), U.edge_mask(kb, vb, fmt)
            U.same(kd[b:b + 1, :n_b], kq, kb, what + ": K", must=mk if mk.any() else None)
            U.same(vd[b:b + 1, :n_b], vq, vb, what + ": V", must=mv if mv.any() else None)
    assert have == goal
    # the rows that are copies hold their originals' bits as far as they go
    kd, vd = cache.dequantised(lengths=_i32(have), max_length=L)
    assert torch.equal(kd[0], kd[3]) and torch.equal(vd[0], vd[3])
    assert torch.equal(vd[1, :U.RAGGED_SHORT], vd[4, :U.RAGGED_SHORT]) and torch.equal(kd[1, :16], kd[4, :16])
    torch.cuda.synchronize()


def test_kvcache_ragged():
    from mi355q import ops
    _ragged(ops.KVCache, "bfp", 6, U.expected_bf16)


def test_packed_ragged():
    from mi355q import ops
    _ragged(ops.PackedKVCache, "bfp", 6, U.expected_mantissa)


def test_minifloat_ragged():
    from mi355q import ops
    _ragged(ops.MinifloatKVCache, "bm64", (8, 4, 8), U.expected_bf16)


# ---------------------------------------------------------------------------------------------------
# the mantissa storages
# ---------------------------------------------------------------------------------------------------
def _against_kvcache(D, width, shift):
    """-> a callback for _fill_contiguous: at every length the cache holds, as bits, what a KVCache fed the same pieces holds, on every
    element outside 0 < |x| <= 1e-8 (the ties and the clamp / near blocks' other elements are all inside the comparison); at those it
    holds 0 where KVCache holds the value passed through"""
    from mi355q import ops
    k, v = U.layout("bfp", D, shift)
    plain, done = ops.KVCache(k.shape[0], L, D, _par(width), _par(width), DEV), [0]

    def also(at, kd, vd):
        plain.append(_dev(k[:, done[0]:at]), _dev(v[:, done[0]:at]))
        done[0] = at
        masks = U.edge_mask(k[:, :at], v[:, :at], width)
        for x, got, ref, m, what in zip((k[:, :at], v[:, :at]), (kd, vd), (t.cpu().numpy() for t in plain.dequantised()), masks, "KV"):
            t = U.tiny(x)
            U.same(got, ref, x, f"width {width} D={D} shift={shift}: {what} at length {at} against KVCache", skip=t, must=m & ~t)
            assert (got[t] == 0).all() and (ref[t] != 0).all(), "the deviation: 0 < |x| <= 1e-8 is 0 here and passed through by KVCache"
    return also


def _run_mantissa(cls, D, width, fill, also_nibble=False):
    import torch
    for shift in (U.SHIFTS if len(fill) > 1 else (0,)):
        cache, (kd, vd) = _fill_contiguous(cls, "bfp", D, width, fill, U.expected_mantissa, shift, _against_kvcache(D, width, shift))
        k, v = U.layout("bfp", D, shift)
        if len(fill) > 1:
            once = cls(k.shape[0], L, D, _par(width), _par(width), DEV)
            once.append(_dev(k), _dev(v))
            for a, b, what in zip(_storage(cache), _storage(once), "KV"):
                assert torch.equal(a, b), f"{cls.__name__} D={D} width={width} shift={shift}: {what} storage after {fill} is not one append's"
        if also_nibble:
            _mantissas_fit(k, v, kd, vd, width)


def _mantissas_fit(k, v, kd, vd, width):
    """from dequantised(), not from bytes: every value is an integer mantissa |m| <= 2^mb - 1 under the oracle's block exponent, and
    the clamped block maxima -- (|x| + 1e-9) 2^(mb - e) rounds to 2^mb -- sit at exactly 2^mb - 1, sign kept"""
    B, _, D = k.shape
    mb = width - 1
    ek, _ = U.k_exponents(k, width)                                                # [B, D, tiles]
    mk = np.ldexp(np.swapaxes(kd, 1, 2).reshape(B, D, L // 16, 16).astype(np.float64), (mb - ek)[..., None])
    _, ev, _ = R.oracle_codes(v.reshape(B * L, D), width)
    mv = np.ldexp(vd.reshape(B * L, D // 16, 16).astype(np.float64), (mb - ev)[..., None])
    xk = np.swapaxes(k, 1, 2).reshape(B, D, L // 16, 16)
    xv = v.reshape(B * L, D // 16, 16)
    for what, m, x in (("K", mk, xk), ("V", mv, xv)):
        assert np.array_equal(m, np.rint(m)) and np.abs(m).max() == 2 ** mb - 1, f"{what}: mantissas outside -{2 ** mb - 1} .. {2 ** mb - 1}: {np.abs(m).max()}"
        clamps = U.bfp_masks(x.reshape(-1, x.shape[-2] * 16), width)["clamps"].reshape(x.shape[:-1])
        assert clamps.sum() >= 500
        at = np.abs(x).argmax(axis=-1)[..., None]
        top, xin = np.take_along_axis(m, at, -1)[..., 0], np.take_along_axis(x, at, -1)[..., 0]
        clamps = clamps & (np.abs(xin) > U.ATOL)            # (a maximum 0 < |x| <= 1e-8 is stored as 0: the tiny-value rule, four blocks)
        assert np.array_equal(top[clamps], np.sign(xin[clamps]) * (2 ** mb - 1)), f"{what}: a clamped maximum is not +-{2 ** mb - 1}"


@pytest.mark.parametrize("fill", U.FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("D", U.SHAPES)
@pytest.mark.parametrize("width", [4, 6, 8])
def test_packed(width, D, fill):
    from mi355q import ops
    _run_mantissa(ops.PackedKVCache, D, width, fill)


def test_packed_three_chunks():
    from mi355q import ops
    _run_mantissa(ops.PackedKVCache, U.D_CHUNKS, 8, U.FILLS[1])


@pytest.mark.parametrize("fill", U.FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("D", U.SHAPES)
@pytest.mark.parametrize("width", [2, 4])
def test_nibble(width, D, fill):
    from mi355q import ops
    _run_mantissa(ops.NibbleKVCache, D, width, fill, also_nibble=True)


def test_nibble_three_chunks():
    from mi355q import ops
    _run_mantissa(ops.NibbleKVCache, U.D_CHUNKS, 4, U.FILLS[1], also_nibble=True)


# ---------------------------------------------------------------------------------------------------
# the paged storages: pages of 32 keys, two a row, placed by hand -- interleaved over the rows, descending, row 1 ascending, spare
# pages at either end and a poison page in the middle that no row holds (tests/paged_util.py)
# ---------------------------------------------------------------------------------------------------
def _paged(cls, B, D, width):
    """an empty paged cache of `cls` with tests/paged_util.py's placement plan, its pools full of a sentinel byte"""
    from mi355q import ops
    if cls is ops.PagedKVCache:
        cache, plan = PU.make_paged(B, D, PAGE, L // PAGE, width)
        return cache, plan, lambda: PU.assert_untouched(cache)
    mp = L // PAGE
    num_pages = B * mp + 3
    poison = num_pages // 2
    cache = cls(B, D, _par(width), _par(width), DEV, page_size=PAGE, num_pages=num_pages, max_pages=mp, pad_page=poison)
    for pool in cache.POOLS:
        getattr(cache, pool).fill_(0x7F)                   # (a finite mantissa under a finite exponent)
    ids = [p for p in range(num_pages - 1, -1, -1) if p != poison][1:]
    plan = [[ids[i * B + b] for i in range(mp)] for b in range(B)]
    plan[1].reverse()

    def untouched():
        import torch
        used = {p for row in cache.held for p in row}
        idle = [p for p in range(num_pages) if p not in used]
        assert poison in idle
        for pool in cache.POOLS:
            pages = getattr(cache, pool).view(torch.uint8).view(num_pages, -1)
            assert bool((pages[idle] == 0x7F).all()), f"{pool}: the poison page or a page no row holds was written"
    return cache, plan, untouched


def _fill_paged(cls, D, width, fill, expect, shift=0):
    k, v = U.layout("bfp", D, shift)
    B = k.shape[0]
    cache, plan, untouched = _paged(cls, B, D, width)
    assert any(row != sorted(row) for row in plan) and plan[1] == sorted(plan[1]), "the page table is an identity"
    kt, vt = _dev(k), _dev(v)
    at = 0
    for n in fill:
        PU.grow(cache, plan, [at + n] * B)
        cache.append(kt[:, at:at + n].contiguous(), vt[:, at:at + n].contiguous(), lengths=_i32([at] * B), max_length=at)
        at += n
        lens = _i32([at] * B)
        _check(cache, k, v, at, _expected(expect, "bfp", D, shift, width, at), f"{cls.__name__} D={D} width={width} shift={shift}",
               read=lambda: cache.dequantised(lens, at))
        untouched()
    return cache


def _run_paged(cls, contiguous, D, width, fill, expect):
    """the schedule through the page table; then the rows' contents are, as bits, those of a one-append cache of the same class and of
    the contiguous storage of the same kind fed the same pieces"""
    import torch
    for shift in (U.SHIFTS if len(fill) > 1 else (0,)):
        cache = _fill_paged(cls, D, width, fill, expect, shift)
        k, v = U.layout("bfp", D, shift)
        B = k.shape[0]
        lens = _i32([L] * B)
        got = cache.dequantised(lens, L)
        if len(fill) > 1:
            once = _fill_paged(cls, D, width, (L,), expect, shift)
            assert once.table.equal(cache.table)
            for a, b, what in zip(_storage(cache), _storage(once), "KV"):
                pa, pb = (t.view(torch.uint8).view(cache.num_pages, -1) for t in (a, b))
                used = sorted({p for row in cache.held for p in row})
                assert torch.equal(pa[used], pb[used]), f"{cls.__name__} D={D} width={width} shift={shift}: {what} pages after {fill} are not one append's"
        flat = contiguous(B, L, D, _par(width), _par(width), DEV)
        at = 0
        for n in fill:
            flat.append(_dev(k[:, at:at + n]), _dev(v[:, at:at + n]))
            at += n
        for a, b, what in zip(got, flat.dequantised(), "KV"):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: not the bits of {contiguous.__name__}"


@pytest.mark.parametrize("fill", U.FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("D", U.SHAPES)
@pytest.mark.parametrize("width", [6, 9])
def test_paged(width, D, fill):
    from mi355q import ops
    _run_paged(ops.PagedKVCache, ops.KVCache, D, width, fill, U.expected_bf16)


@pytest.mark.parametrize("fill", U.FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("D", U.SHAPES)
@pytest.mark.parametrize("width", [6, 8])
def test_paged_packed(width, D, fill):
    from mi355q import ops
    _run_paged(ops.PagedPackedKVCache, ops.PackedKVCache, D, width, fill, U.expected_mantissa)


# ---------------------------------------------------------------------------------------------------
# MinifloatKVCache: (8, 4, 8) has recorded reference outputs on both sets, the other formats the oracle alone
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", U.FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("D", U.SHAPES)
@pytest.mark.parametrize("name", U.BM_SETS)
@pytest.mark.parametrize("fmt", U.BM_FORMATS, ids=lambda f: "w%d_e%d_b%d" % f)
def test_minifloat(fmt, name, D, fill):
    from mi355q import ops
    _run_contiguous(ops.MinifloatKVCache, name, D, fmt, fill, U.expected_bf16)


def test_minifloat_three_chunks():
    from mi355q import ops
    _run_contiguous(ops.MinifloatKVCache, "bm64", U.D_CHUNKS, (8, 4, 8), U.FILLS[1], U.expected_bf16)
