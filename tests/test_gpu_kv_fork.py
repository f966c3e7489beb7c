"""Copy-on-write on the paged block_fp KV cache: ops.PagedKVCache.fork / .reorder on the GPU.  Rows of 37, 64, 5 and 0 keys -- a partial
page with an open 16-key tile, a page-aligned row, a row that is one open tile, an empty row -- at head_dim 32 and 128 (one and four
32-wide chunks a K piece) and pages of 32 and 64 keys.  Everything is compared as BITS: with what the source row held, and with a
one-row contiguous ops.KVCache that was given the lineage's keys in the same append calls.  Tables are out of order and the pools are
full of a sentinel (tests/paged_util.py)."""
import math
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from paged_util import DEV, bits, fill_both, i32, par  # noqa: E402

pytestmark = pytest.mark.gpu
B, LENGTHS, MAX_PAGES = 4, (37, 64, 5, 0), 3
CASES = [(D, P) for D in (32, 128) for P in (32, 64)]


def _kv(L, D, seed, rows=B):
    import torch
    g = torch.Generator(device=DEV).manual_seed(seed)
    k = torch.randn(rows, L, D, device=DEV, generator=g) * torch.exp(0.5 * torch.randn(rows, 1, D, device=DEV, generator=g))
    return k, torch.randn(rows, L, D, device=DEV, generator=g), g


def _filled(D, P, seed=0):
    k, v, g = _kv(64, D, 1000 * seed + D + P)
    paged, _ = fill_both(k, v, list(LENGTHS), D, P, MAX_PAGES)
    return paged, k, v, g


def _content(cache, lengths, L=None):
    """(K bits, V bits) [B, L, D] and the stage rows [B, 16 * D * 4] bytes"""
    kd, vd = cache.dequantised(i32(lengths), max_length=L or max(max(lengths), 1))
    return bits(kd).clone(), bits(vd).clone(), cache.stage.view(cache.B, -1).clone()


def _reordered_is_the_source(D, P, src_rows):
    import torch
    paged, _, _, _ = _filled(D, P)
    old = _content(paged, LENGTHS, 64)
    pools = paged.kq.clone(), paged.vq.clone()
    held = {p for row in paged.held for p in row}
    stage_before = paged.stage.data_ptr()
    paged.reorder(src_rows, LENGTHS)
    new_len = [LENGTHS[s] for s in src_rows]
    assert paged.stage.data_ptr() != stage_before and paged.stage_alt.data_ptr() == stage_before, "the stage buffers did not swap"
    assert [len(r) for r in paged.held] == [paged.pages_for(n) for n in new_len] and torch.equal(paged.block_table.cpu(), paged.table)
    new = _content(paged, new_len, 64)
    for b, s in enumerate(src_rows):
        for what, a, o in zip(("K", "V"), new, old):
            assert torch.equal(a[b], o[s]), f"{what} of row {b} is not what row {s} held"
        if LENGTHS[s]:
            assert torch.equal(new[2][b], old[2][s]), f"the stage rows of row {b} are not those of row {s}"
    # whole pages: the drawn pages hold their source's bytes, every other page of either pool is untouched -- sentinel or not
    drawn = sorted({p for row in paged.held for p in row} - held)
    assert len(drawn) == sum(1 for b, s in enumerate(src_rows) if LENGTHS[s] % P and not (b == s))
    keep = torch.ones(paged.num_pages, dtype=torch.bool, device=DEV)
    keep[drawn] = False
    for pool, before in zip((paged.kq, paged.vq), pools):
        assert torch.equal(pool.view(paged.num_pages, -1)[keep], before.view(paged.num_pages, -1)[keep]), "a page no job names was written"
    return new


@pytest.mark.parametrize("D,P", CASES)
def test_reorder_gives_every_row_its_sources_bits(D, P):
    """reorder((2, 0, 0, 3)): a duplication (rows 1 and 2 <- 0), a row of one open tile moving (0 <- 2), an empty row staying; twice,
    for equal bits"""
    import torch
    first = _reordered_is_the_source(D, P, (2, 0, 0, 3))
    again = _reordered_is_the_source(D, P, (2, 0, 0, 3))
    assert all(torch.equal(a, b) for a, b in zip(first, again)), "two runs differ"


@pytest.mark.parametrize("D,P", CASES)
def test_a_swap_is_not_done_in_place(D, P):
    """reorder((1, 0, 3, 2)): rows 0 and 1 trade places -- stage rows permuted in place would give one of them its own back"""
    _reordered_is_the_source(D, P, (1, 0, 3, 2))


def _lineage(k, v, row, n0, steps, D, P):
    """a one-row contiguous cache given k[row, :n0] and then `steps` (lists of [n, D] tensors) in the same append calls"""
    from mi355q import ops
    ref = ops.KVCache(1, MAX_PAGES * P, D, par(), par(), DEV)
    ref.append(k[row:row + 1, :n0].contiguous(), v[row:row + 1, :n0].contiguous(), lengths=i32([0]), max_length=0)
    at = n0
    for kn, vn in steps:
        ref.append(kn[None].contiguous(), vn[None].contiguous(), lengths=i32([at]), max_length=at)
        at += kn.shape[0]
    return ref, at


def _attend(q, cache, lengths, group=1, extend_counts=None):
    """decode (q [rows, M <= 16, D]) or extend with explicit splits and the paged cache's bound, so that a one-row cache partitions alike"""
    from mi355q import ops
    kw = dict(causal=True, scale_div=math.sqrt(q.shape[-1]), lengths=i32(lengths), max_length=64, group=group)
    if extend_counts is not None:
        return ops.bfp_attention_extend(q, cache, counts=i32(extend_counts), **kw)
    return ops.bfp_attention_decode(q, cache, splits=2, **kw)


def _fork_is_a_copy(D, P, G):
    import torch
    paged, k, v, g = _filled(D, P)
    qs = {M: torch.randn(B * G, M, D, device=DEV, generator=g) for M in (1, 7, 20)}
    row0 = _content(paged, LENGTHS, 64)
    out0 = {M: _attend(qs[M], paged, LENGTHS, G)[:G].clone() for M in (1, 7)}
    paged.fork(0, 3, 37)
    if P == 32:       # one full page by reference, the partial one private
        assert paged.held[3][0] == paged.held[0][0] and paged.held[3][1] != paged.held[0][1] and paged.refs[paged.held[0][0]] == 2
    else:             # the only page is the partial one
        assert len(paged.held[3]) == 1 and paged.held[3][0] != paged.held[0][0]
    assert all(paged.refs[p] == 1 for p in (paged.held[0][-1], paged.held[3][-1]))
    steps = [tuple(torch.randn(n, D, device=DEV, generator=g) for _ in range(2)) for n in (1, 20)]
    lengths = list(LENGTHS[:3]) + [37]
    for kn, vn in steps:
        n = kn.shape[0]
        after = lengths[:3] + [lengths[3] + n]
        paged.ensure(after)
        paged.append(kn[None].expand(B, n, D).contiguous(), vn[None].expand(B, n, D).contiguous(), lengths=i32(lengths),
                     counts=i32([0, 0, 0, n]), max_length=64)
        lengths = after
    assert lengths[3] == 58
    # row 0 (and every other row) is what it was: content, stage rows, decode output
    now = _content(paged, lengths, 64)
    for what, a, o in zip(("K", "V", "stage"), now, row0):
        assert torch.equal(a[:3], o[:3]), f"{what} of the rows that took no key changed"
    for M in (1, 7):
        assert torch.equal(bits(_attend(qs[M], paged, lengths, G)[:G]), bits(out0[M])), f"row 0's decode output changed (M = {M})"
    # row 3 is the one-row cache of its lineage: row 0's 37 keys, then 1, then 20
    ref, n_ref = _lineage(k, v, 0, 37, steps, D, P)
    assert n_ref == 58
    want = _content(ref, [58], 64)
    for what, a, o in zip(("K", "V", "stage"), now, want):
        assert torch.equal(a[3], o[0]), f"{what} of the fork differs from its lineage's own cache"
    for M in (1, 7):
        got, alone = _attend(qs[M], paged, lengths, G)[3 * G:], _attend(qs[M][3 * G:], ref, [58], G)
        assert torch.equal(bits(got), bits(alone)) and bool(got.any()), f"decode of the fork, M = {M}"
    got = _attend(qs[20], paged, lengths, G, extend_counts=[0, 0, 0, 20])[3 * G:]
    assert torch.equal(bits(got), bits(_attend(qs[20][3 * G:], ref, [58], G, extend_counts=[20]))) and bool(got.any()), "extend of the fork"
    return now


@pytest.mark.parametrize("D,P", CASES)
def test_fork_copies_the_partial_page_and_the_open_tile(D, P):
    """fork(0, 3) at 37 keys, then 1 and 20 keys into row 3 alone (they fill the open tile and open the next): a shared partial page
    would change row 0, a stage that was not copied would re-quantise the open tile from the wrong rows.  Twice, for equal bits."""
    import torch
    first, again = _fork_is_a_copy(D, P, 1), _fork_is_a_copy(D, P, 1)
    assert all(torch.equal(a, b) for a, b in zip(first, again)), "two runs differ"


def test_fork_under_grouped_queries():
    """the same with two query heads a cache row (group = 2): decode and extend of the forked row against its lineage's own cache"""
    _fork_is_a_copy(64, 32, 2)


@pytest.mark.parametrize("D,P", CASES)
def test_rows_diverge_after_a_duplicating_reorder(D, P):
    """reorder((0, 0, 1, 1)), then 12 steps of one DIFFERENT key a row: rows 0 and 1 continue row 0's 37 keys, over the tile edge at 48;
    rows 2 and 3 continue row 1's 64 keys, over the page edge at 64 into a page of their own each.  After every step each row decodes,
    bit for bit, as the one-row cache of its lineage."""
    import torch
    from mi355q import ops
    paged, k, v, g = _filled(D, P)
    src = (0, 0, 1, 1)
    paged.reorder(src, LENGTHS)
    lengths = [LENGTHS[s] for s in src]
    q = torch.randn(B, 1, D, device=DEV, generator=g)
    refs = [_lineage(k, v, s, LENGTHS[s], [], D, P)[0] for s in src]
    for step in range(12):
        kn, vn = (torch.randn(B, 1, D, device=DEV, generator=g) for _ in range(2))
        after = [n + 1 for n in lengths]
        paged.ensure(after)
        paged.append(kn, vn, lengths=i32(lengths), max_length=max(lengths))
        for b, ref in enumerate(refs):
            ref.append(kn[b:b + 1], vn[b:b + 1], lengths=i32([lengths[b]]), max_length=lengths[b])
        lengths = after
        kw = dict(causal=True, scale_div=math.sqrt(D), splits=2, max_length=MAX_PAGES * P)
        got = ops.bfp_attention_decode(q, paged, lengths=i32(lengths), **kw)
        for b, ref in enumerate(refs):
            alone = ops.bfp_attention_decode(q[b:b + 1], ref, lengths=i32([lengths[b]]), **kw)
            assert torch.equal(bits(got[b:b + 1]), bits(alone)), f"step {step}, row {b} (lineage of row {src[b]})"
    assert lengths == [49, 49, 76, 76]
    used = [p for row in paged.held for p in row]
    assert sorted(set(used)) == sorted(p for p in range(paged.num_pages) if paged.refs[p]) and not set(used) & set(paged.free)
    paged.release(range(B))
    assert len(paged.free) == len(set(paged.free)) == paged.num_pages - 1 and not any(paged.refs)      # (all but the poison page)
