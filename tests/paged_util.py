"""Shared by the paged-cache GPU tests (tests/test_gpu_paged_*.py): a PagedKVCache whose pools are filled with a finite bf16 sentinel,
whose table entries behind a row's pages all name one valid "poison" page, and whose rows get their pages by explicit placement --
interleaved with the other rows' pages, descending for most rows and ascending for row 1 -- never in the order a fresh allocator
would give.  No test uses an out-of-range page id: a test must not be able to fault the card."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "llm-mixed-q_amd", ROOT):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

DEV = "cuda:0"
SENTINEL = 0x4E4E            # bf16 1.6 * 2^29: finite, and nothing an append of unit-scale inputs writes


def par(width=6):
    return (width, 8, 127, width, 8, 127)


def i32(values, device=DEV):
    import torch
    return torch.tensor(list(values), dtype=torch.int32, device=device)


def bits(t):
    import torch
    return t.contiguous().view(torch.uint8)


def pool_pages(cache, pool):
    """a pool as int16 [num_pages, halfwords of a page]"""
    import torch
    return pool.view(torch.int16).view(cache.num_pages, -1)


def make_paged(B, D, P, max_pages, width=6, spare=2):
    """-> (cache, plan): pools full of SENTINEL; the poison page in the middle of the pool; plan[b] = the pages row b will take, in
    logical order (grow() hands them out)"""
    from mi355q import ops
    num_pages = B * max_pages + 1 + spare
    poison = num_pages // 2
    cache = ops.PagedKVCache(B, D, par(width), par(width), DEV, page_size=P, num_pages=num_pages, max_pages=max_pages, pad_page=poison)
    for pool in (cache.kq, cache.vq):
        pool_pages(cache, pool).fill_(SENTINEL)
    ids = [p for p in range(num_pages - 1, -1, -1) if p != poison][spare // 2:]      # descending; some spare pages at either end
    plan = [[ids[i * B + b] for i in range(max_pages)] for b in range(B)]             # interleaved over the rows
    if B > 1:
        plan[1].reverse()                                                             # one row ascending
    assert poison not in cache.free and all(p in cache.free for row in plan for p in row)
    assert bool((cache.table == poison).all())
    return cache, plan


def grow(cache, plan, lengths_after):
    """every row gets, from ITS planned pages, what lengths_after needs (PagedKVCache.assign)"""
    for b, n in enumerate(lengths_after):
        have, want = len(cache.held[b]), cache.pages_for(n)
        if want > have:
            cache.assign(b, plan[b][have:want], upload=False)
    cache._upload()


def assert_untouched(cache):
    """the poison page and every page in no row's table still hold the sentinel, and the device table is the host mirror"""
    import torch
    used = {p for row in cache.held for p in row}
    idle = [p for p in range(cache.num_pages) if p not in used]
    assert cache.pad_page in idle
    for pool in (cache.kq, cache.vq):
        assert bool((pool_pages(cache, pool)[idle] == SENTINEL).all()), "a page in no row's table (or the poison page) was written"
    assert torch.equal(cache.block_table.cpu(), cache.table)
    behind = [cache.table[b, len(row):] for b, row in enumerate(cache.held)]
    assert all(bool((t == cache.pad_page).all()) for t in behind)


def fill_both(k, v, lengths, D, P, max_pages, width=6):
    """-> (paged, contiguous): row b holds k[b, :lengths[b]], v[b, :lengths[b]] in both, by one ragged append from empty rows"""
    import torch
    from mi355q import ops
    B = k.shape[0]
    paged, plan = make_paged(B, D, P, max_pages, width)
    grow(paged, plan, lengths)
    contig = ops.KVCache(B, max_pages * P, D, par(width), par(width), DEV)
    zero, cnt = i32([0] * B), i32(lengths)
    n = max(max(lengths), 1)
    for c in (paged, contig):
        c.append(k[:, :n].contiguous(), v[:, :n].contiguous(), lengths=zero, counts=cnt, max_length=0)
    return paged, contig
