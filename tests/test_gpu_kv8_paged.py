"""ops.PagedPackedKVCache (int8 mantissas in paged pools, csrc/mi355q_kvp.hip with PG = true) on the GPU.  The arithmetic is that of
ops.PackedKVCache -- only a piece's place goes through the page table -- so EVERY comparison with the other caches here is bit equality;
the decode cases are first held to the fp64-softmax oracle with the helper and the bounds of tests/test_gpu_kv8_decode.py.
Four cache rows reach (37, 64, 5, 0) keys by appends of 1, 15, 17 and 33 input rows; their pages are placed by hand, interleaved and out
of order; the pools start out full of 0x7F bytes (a finite mantissa under a finite exponent), the table entries behind a row's pages
name a poison page no row holds.  No input has 0 < |x| <= 1e-8, the packed storage's one stated deviation (asserted), which makes
equality with the bf16 caches a fair demand.  No test here uses a table entry to reach outside a pool: the wrong entries of
test_a_wrong_table_entry_is_clamped are clamped by the kernels, as the bf16 paged kernels clamp theirs."""
import ctypes
import math
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_gpu_kv8_decode import PATTERNS, _hold, _reference  # noqa: E402
from window_util import DEV, bits, i32, inputs, par  # noqa: E402

pytestmark = pytest.mark.gpu
LENGTHS, WIDTH, B = (37, 64, 5, 0), 6, 4
STEPS = ((1, (1, 1, 1, 0)), (15, (15, 15, 4, 0)), (17, (17, 17, 0, 0)), (33, (4, 31, 0, 0)))      # (input rows, each row's count)
SHAPES = [(32, 32), (32, 64), (128, 32), (128, 64)]      # (D, P)
PAD = np.float32(3e38)                                   # input rows behind a row's count: never read
_MEMO = {}


def _no_tiny(*arrays):
    for x in arrays:
        a = np.abs(np.asarray(x))
        assert not ((a > 0) & (a <= 1e-8)).any(), "an input of magnitude 0 < |x| <= 1e-8: the packed storage stores 0 there"


def _max_pages(P):
    return 128 // P                                       # 128 keys a row: room for the fork's 37 + 21 and a page to spare at P = 32


def _paged(cls, D, P):
    """an empty paged cache of `cls`, its pools full of 0x7F bytes, and the pages its rows will take: interleaved over the rows,
    descending, row 1 ascending (tests/paged_util.py's placement)"""
    import torch
    mp = _max_pages(P)
    num_pages = B * mp + 4
    poison = num_pages // 2
    c = cls(B, D, par(WIDTH), par(WIDTH), DEV, page_size=P, num_pages=num_pages, max_pages=mp, pad_page=poison)
    for name in c.POOLS:
        getattr(c, name).fill_(0x7F)
    ids = [p for p in range(num_pages - 1, -1, -1) if p != poison][1:]
    plan = [[ids[i * B + b] for i in range(mp)] for b in range(B)]
    plan[1].reverse()
    assert poison not in c.free and bool((c.table == poison).all())
    return c, plan


def _grow(c, plan, lengths_after):
    for b, n in enumerate(lengths_after):
        have, want = len(c.held[b]), c.pages_for(n)
        if want > have:
            c.assign(b, plan[b][have:want], upload=False)
    c._upload()


def _pages(c, name):
    import torch
    return getattr(c, name).view(torch.uint8).view(c.num_pages, -1)


def _idle_untouched(c):
    import torch
    used = {p for row in c.held for p in row}
    idle = [p for p in range(c.num_pages) if p not in used]
    assert c.pad_page in idle
    for name in c.POOLS:
        assert bool((_pages(c, name)[idle] == 0x7F).all()), f"{name}: the poison page or a page no row holds was written"
    assert torch.equal(c.block_table.cpu(), c.table)


def _fill(D, P, seed):
    """-> (k, v [4, 64, D] numpy, the paged packed cache, a PackedKVCache, a PagedKVCache): all three fed the same rows by the four appends"""
    import torch
    from mi355q import ops
    _, k, v = inputs(B, 1, max(LENGTHS), D, seed=seed)
    _no_tiny(k, v)
    new, plan = _paged(ops.PagedPackedKVCache, D, P)
    paged, plan16 = _paged(ops.PagedKVCache, D, P)
    packed = ops.PackedKVCache(B, _max_pages(P) * P, D, par(WIDTH), par(WIDTH), DEV)
    before = [0] * B
    for n, counts in STEPS:
        kin, vin = np.full((B, n, D), PAD, np.float32), np.full((B, n, D), PAD, np.float32)
        for b, c in enumerate(counts):
            kin[b, :c], vin[b, :c] = k[b, before[b]:before[b] + c], v[b, before[b]:before[b] + c]
        after = [l + c for l, c in zip(before, counts)]
        _grow(new, plan, after)
        _grow(paged, plan16, after)
        for c in (new, packed, paged):
            c.append(torch.from_numpy(kin).to(DEV), torch.from_numpy(vin).to(DEV), lengths=i32(before), counts=i32(counts), max_length=max(before))
        before = after
    assert tuple(before) == LENGTHS
    return k, v, new, packed, paged


def _filled(D, P):
    """_fill, kept per shape for the tests that only read; row 3 then SHARES row 1's first page (share_prefix) in both paged caches,
    and holds the same P keys in the contiguous one: lengths (37, 64, 5, 0) leave it empty, (37, 64, 5, P) read the shared page"""
    import torch
    if (D, P) not in _MEMO:
        k, v, new, packed, paged = _fill(D, P, seed=D + P)
        for c in (new, paged):
            c.share_prefix(1, 3, 1)
        assert new.held[3] == [new.held[1][0]] and new.refs[new.held[1][0]] == 2
        kin, vin = (torch.from_numpy(np.repeat(x[1:2, :P], B, 0)).to(DEV) for x in (k, v))
        packed.append(kin, vin, lengths=i32([0] * B), counts=i32([0, 0, 0, P]), max_length=0)
        k, v = k.copy(), v.copy()
        k[3, :P], v[3, :P] = k[1, :P], v[1, :P]
        _MEMO[(D, P)] = (k, v, new, packed, paged)
    return _MEMO[(D, P)]


@pytest.mark.parametrize("D,P", SHAPES)
def test_append_gives_the_other_caches_bits_and_leaves_idle_pages_alone(D, P):
    import torch
    k, v, new, packed, paged = _fill(D, P, seed=3 * D + P)
    assert new.k8.numel() == new.v8.numel() == new.num_pages * P * D * 17 // 16
    assert (new.k8.numel() + new.v8.numel()) * 32 == (paged.kq.numel() + paged.vq.numel()) * 17
    lengths = i32(LENGTHS)
    got = new.dequantised(lengths, max(LENGTHS))
    for other in (packed, paged):
        want = other.dequantised(lengths, max(LENGTHS))
        for g, w, what in zip(got, want, "KV"):
            assert torch.equal(bits(g), bits(w)), f"{what}: not the bits of {type(other).__name__}"
    for b, L in enumerate(LENGTHS):
        assert float(got[0][b, :L].abs().max() if L else 1.0) > 0 and not bool(got[0][b, L:].any()) and not bool(got[1][b, L:].any())
    _idle_untouched(new)
    assert [len(r) for r in new.held] == [new.pages_for(n) for n in LENGTHS]


@pytest.mark.parametrize("D,P", SHAPES)
@pytest.mark.parametrize("M", [1, 7, 16])
def test_decode_against_the_oracle_then_the_other_caches(D, P, M):
    """M queries a row, causal and not, every `splits`: the oracle first, then the bits of PackedKVCache and of PagedKVCache, then the same
    bits again.  Lengths (37, 64, 5, 0): row 2 has fewer keys than 7 or 16 queries and row 3 none -- exact zeros, and no page looked up."""
    import torch
    from mi355q import ops
    k, v, new, packed, paged = _filled(D, P)
    q = inputs(B, M, 1, D, seed=D + P + M)[0]
    _no_tiny(q)
    lengths, sd, qt = i32(LENGTHS), math.sqrt(D), torch.from_numpy(q).to(DEV)
    for kw in (dict(causal=True, scale_div=sd), dict(causal=False, scale_div=sd, q_scale=0.37)):
        refs = _reference(q * np.float32(kw.get("q_scale", 1.0)), k, v, LENGTHS, WIDTH, sd, causal=kw["causal"])
        assert refs[3] is None and refs[0] is not None and (refs[2] is None) == (M > 5)
        for splits in (None, 1, 3):
            call = dict(lengths=lengths, max_length=max(LENGTHS), splits=splits, **kw)
            out = ops.bfp_attention_decode(qt, new, **call)
            _hold(out, refs, f"{kw} splits={splits}")
            for other in (packed, paged):
                assert torch.equal(bits(out), bits(ops.bfp_attention_decode(qt, other, **call))), \
                    f"{kw} splits={splits}: not the bits of {type(other).__name__}"
            assert torch.equal(bits(out), bits(ops.bfp_attention_decode(qt, new, **call))), "two runs, two results"
    _idle_untouched(new)


@pytest.mark.parametrize("D,P", [(32, 64), (128, 32)])
def test_token_major(D, P):
    """q as a [1, H, M, D] head view with a token-major output, row 3 reading the page it shares with row 1"""
    import torch
    from mi355q import ops
    k, v, new, packed, paged = _filled(D, P)
    M, lens = 7, (37, 64, 5, P)
    q = inputs(B, M, 1, D, seed=7 + D)[0]
    _no_tiny(q)
    refs = _reference(q, k, v, lens, WIDTH, 8.0)
    assert refs[2] is None and refs[3] is not None
    qt = torch.from_numpy(q).to(DEV)[None]
    for splits in (None, 1, 3):
        call = dict(scale_div=8.0, token_major=True, lengths=i32(lens), max_length=64, splits=splits)
        out = ops.bfp_attention_decode(qt, new, **call)
        assert out.shape == (1, B, M, D) and out.permute(0, 2, 1, 3).is_contiguous()
        _hold(out[0], refs, "token_major")
        for other in (packed, paged):
            want = ops.bfp_attention_decode(qt, other, **call)
            assert want.stride() == out.stride() and torch.equal(bits(out), bits(want))


@pytest.mark.parametrize("D,P", SHAPES)
@pytest.mark.parametrize("G,M", [(4, 1), (6, 4)])
def test_grouped(D, P, G, M):
    """G query heads a cache row, lengths (37, 64, 5, P): row 3 reads the page it shares with row 1"""
    import torch
    from mi355q import ops
    k, v, new, packed, paged = _filled(D, P)
    lens = (37, 64, 5, P)
    q = inputs(B * G, M, 1, D, seed=D + P + G)[0]
    _no_tiny(q)
    sd = math.sqrt(D)
    refs = _reference(q, k, v, lens, WIDTH, sd, group=G)
    assert all(r is not None for r in refs)
    qt = torch.from_numpy(q).to(DEV)
    for splits in (None, 1, 3):
        call = dict(scale_div=sd, lengths=i32(lens), max_length=64, splits=splits, group=G)
        out = ops.bfp_attention_decode(qt, new, **call)
        _hold(out, refs, f"G={G} splits={splits}")
        for other in (packed, paged):
            assert torch.equal(bits(out), bits(ops.bfp_attention_decode(qt, other, **call))), f"G={G}: not the bits of {type(other).__name__}"
        assert torch.equal(bits(out), bits(ops.bfp_attention_decode(qt, new, **call)))


@pytest.mark.parametrize("D,P", [(32, 32), (128, 64)])
def test_a_wrong_table_entry_is_clamped(D, P):
    """row 0's first table entry on the DEVICE becomes -5, then num_pages + 7: the kernels clamp the page id into the pool, so the call
    returns, every output is finite, and the other rows' bits do not move.  (The host mirror is not changed, and is copied back.)"""
    import torch
    from mi355q import ops
    k, v, new, _, _ = _filled(D, P)
    q = torch.from_numpy(inputs(B, 7, 1, D, seed=5)[0]).to(DEV)
    call = dict(scale_div=8.0, lengths=i32((37, 64, 5, P)), max_length=64)
    good = ops.bfp_attention_decode(q, new, **call)
    try:
        for bad in (-5, new.num_pages + 7):
            new.block_table[0, 0] = bad
            out = ops.bfp_attention_decode(q, new, **call)
            kd, vd = new.dequantised(i32((37, 64, 5, P)), 64)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(kd).all()) and bool(torch.isfinite(vd).all())
            assert torch.equal(bits(out[1:]), bits(good[1:])), f"entry {bad}: another row's output moved"
    finally:
        new._upload()
    assert torch.equal(bits(ops.bfp_attention_decode(q, new, **call)), bits(good))


@pytest.fixture(scope="module")
def poison():
    import torch
    so = ROOT / "tools" / "lds_poison" / "liblds_poison.so"
    if not so.exists():
        pytest.fail("tools/lds_poison/liblds_poison.so is not built (__graft_entry__.build())")
    lib = ctypes.CDLL(str(so))

    def fill(pattern):
        rc = lib.lds_poison(ctypes.c_uint(pattern), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
    return fill


@pytest.mark.parametrize("rows,M,L,D,P,splits,G", [
    (2, 16, 250, 128, 64, 5, 1),      # partial outputs through the workspace, the widest LDS reduction, four pages a row
    (3, 3, 70, 32, 32, 2, 2),         # one chunk; grouped, two splits, three pages a row
])
def test_stale_lds(poison, rows, M, L, D, P, splits, G):
    """tests/test_gpu_kv8_decode.py::test_stale_lds for the paged kernels: every compute unit's LDS is filled with a pattern in front of
    each append and decode, and the output must be the same bits under every pattern"""
    import torch
    from mi355q import ops
    torch.manual_seed(L + D)
    q, k, v = torch.randn(rows * G, M, D, device=DEV), torch.randn(rows, L, D, device=DEV), torch.randn(rows, L, D, device=DEV)
    outs = []
    for p in PATTERNS:
        cache = ops.PagedPackedKVCache(rows, D, par(6), par(6), DEV, page_size=P, num_pages=rows * 4, max_pages=256 // P)
        cache.ensure([L] * rows)
        poison(p)
        cache.append(k[:, :L - M], v[:, :L - M], lengths=i32([0] * rows), max_length=0)
        poison(p)
        cache.append(k[:, L - M:], v[:, L - M:], lengths=i32([L - M] * rows), max_length=L - M)
        poison(p)
        outs.append(ops.bfp_attention_decode(q, cache, causal=True, scale_div=math.sqrt(D), splits=splits, group=G, lengths=i32([L] * rows),
                                             max_length=L).clone())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    for p, o in zip(PATTERNS[1:], outs[1:]):
        assert torch.equal(o.view(torch.uint8), outs[0].view(torch.uint8)), f"output depends on stale LDS (pattern {p:#010x})"


@pytest.mark.parametrize("D,P", SHAPES)
def test_fork_and_reorder(D, P):
    """fork row 0 at 37 keys into the empty row 3, then 1 + 20 keys into the fork alone: the source is unchanged, the fork is a one-row
    PackedKVCache of its lineage in content and in decode, and the launch wrote the fork's private page only.  Then a swap and a
    duplicating reorder: every row is what its source was.  After release every page is free."""
    import torch
    from mi355q import ops
    k, v, new, _, _ = _fill(D, P, seed=11 + D + P)
    ext = inputs(1, 1, 21, D, seed=13)
    _no_tiny(ext[1], ext[2])
    lens = list(LENGTHS)
    was = new.dequantised(i32(lens), 64)
    snap = {name: _pages(new, name).clone() for name in new.POOLS}
    free_before = list(new.free)
    new.fork(0, 3, 37)
    drawn = new.held[3][-1]
    assert drawn in free_before and new.held[3][:-1] == new.held[0][:37 // P] and new.held[0][-1] != drawn
    others = [p for p in range(new.num_pages) if p != drawn]
    for name in new.POOLS:
        pages = _pages(new, name)
        assert torch.equal(pages[others], snap[name][others]), f"{name}: the fork wrote a page no job names"
        assert torch.equal(pages[drawn], snap[name][new.held[0][-1]]), f"{name}: the private page is not the source's partial page"
    lens[3] = 37
    for n, at in ((1, 0), (20, 1)):
        after = lens[:3] + [lens[3] + n]
        new.ensure(after)
        kin, vin = (torch.from_numpy(np.repeat(x[:, at:at + n], B, 0)).to(DEV) for x in ext[1:])
        new.append(kin, vin, lengths=i32(lens), counts=i32([0, 0, 0, n]), max_length=max(lens))
        lens = after
    assert lens == [37, 64, 5, 58]
    now = new.dequantised(i32(lens), 64)
    for a, b_ in zip(now, was):
        assert torch.equal(bits(a[:3]), bits(b_[:3])), "an append into the fork changed another row"
    line_k, line_v = np.concatenate([k[0:1, :37], ext[1]], 1), np.concatenate([v[0:1, :37], ext[2]], 1)
    alone = ops.PackedKVCache(1, 64, D, par(WIDTH), par(WIDTH), DEV)
    for lo, hi in ((0, 37), (37, 38), (38, 58)):                     # the fork's own schedule: 37 keys, then 1, then 20
        alone.append(torch.from_numpy(line_k[:, lo:hi].copy()).to(DEV), torch.from_numpy(line_v[:, lo:hi].copy()).to(DEV))
    want = alone.dequantised()
    for a, w in zip(now, want):
        assert torch.equal(bits(a[3, :58]), bits(w[0])), "the fork does not hold its lineage"
    for M in (1, 7):
        q = inputs(B, M, 1, D, seed=17 + M)[0]
        _no_tiny(q)
        refs = _reference(q[3:4], line_k, line_v, (58,), WIDTH, 8.0)
        for splits in (None, 1):
            out = ops.bfp_attention_decode(torch.from_numpy(q).to(DEV), new, scale_div=8.0, lengths=i32(lens), max_length=64, splits=splits)
            _hold(out[3:4], refs, f"fork M={M}")
            one = ops.bfp_attention_decode(torch.from_numpy(q[3:4]).to(DEV), alone, scale_div=8.0, splits=splits)
            assert ops.decode_splits(B, 64, D, splits) == ops.decode_splits(1, 58, D, splits) == 1       # (two key pairs: one split either way)
            assert torch.equal(bits(out[3:4]), bits(one)), f"fork M={M}: not its lineage's decode"
    # a swap, then a duplication
    for src in ((1, 0, 2, 3), (0, 0, 2, 1)):
        before = new.dequantised(i32(lens), 64)
        stage = new.stage.clone().view(B, -1)
        new.reorder(src, lens)
        lens = [lens[s] for s in src]
        after = new.dequantised(i32(lens), 64)
        for a, b_ in zip(after, before):
            assert torch.equal(bits(a), bits(b_[list(src)])), f"reorder {src}: a row is not what its source was"
        assert torch.equal(new.stage.view(B, -1), stage[list(src)]), f"reorder {src}: the open tiles did not travel"
        assert sum(new.refs) == sum(len(r) for r in new.held)
    new.release(range(B))
    assert sorted(new.free) == [p for p in range(new.num_pages) if p != new.pad_page] and not any(new.refs), "a page leaked"
