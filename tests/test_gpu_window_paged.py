"""Sliding window on the paged cache: the paged windowed decode and extend give the contiguous windowed call's bits through out-of-order
tables; after PagedKVCache.trim the trimmed entries name a poison page of NaN bit patterns and nothing changes; and a pool far smaller
than the sequence serves append -> decode -> trim for as long as one likes, where the same loop without trim runs out of pages."""
import math
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from paged_util import DEV, bits, fill_both, i32, par, pool_pages  # noqa: E402

pytestmark = pytest.mark.gpu
NAN16 = 0x7FC1                # a bf16 NaN (as int16); two of them are an fp32 NaN


@pytest.mark.parametrize("P", [32, 64])
def test_paged_is_contiguous_before_and_after_trim(P):
    """rows of 200, 131 and 40 keys, W = 24, 20 queries (extend) / 4 and 1 (decode), G = 1 and 2.  Then trim: the pages wholly below the
    window go back, their entries name the poison page -- now full of NaN patterns -- and every call still gives the same bits: no
    windowed kernel looks up a page without a visible key"""
    import torch
    from mi355q import ops
    lengths, W, D, M = [200, 131, 40], 24, 64, 20
    B, n = len(lengths), max(lengths)
    torch.manual_seed(P)
    k, v = torch.randn(B, n, D, device=DEV), torch.randn(B, n, D, device=DEV)
    paged, contig = fill_both(k, v, lengths, D, P, -(-n // P))
    L = i32(lengths)
    outs = []
    for G in (1, 2):
        q = torch.randn(B * G, M, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(G))
        kw = dict(scale_div=8.0, lengths=L, max_length=n, window=W, group=G)
        for M_, fn, extra in ((4, ops.bfp_attention_decode, dict(splits=2)), (1, ops.bfp_attention_decode, {}), (M, ops.bfp_attention_extend, {})):
            qq = q[:, :M_].contiguous()
            ref = fn(qq, contig, **kw, **extra)
            got = fn(qq, paged, **kw, **extra)
            assert torch.equal(bits(got), bits(ref)), (G, M_, fn.__name__)
            outs.append((fn, qq, dict(kw, **extra), ref))
    # trim speaks of queries at positions >= lengths[b]; the calls above are run AGAIN below, and their first query (the extend call's)
    # lies M positions back: its window is that of a later query with W + M keys
    poison = paged.pad_page
    held = [list(r) for r in paged.held]
    paged.trim(lengths, W + M)
    gone = [max(lengths[b] - (W + M) + 1, 0) // P for b in range(B)]
    assert gone[0] >= 1 and gone[2] == 0
    for b in range(B):
        assert paged.held[b] == [None] * gone[b] + held[b][gone[b]:]
        assert bool((paged.table[b, :gone[b]] == poison).all()) and bool((paged.table[b, len(held[b]):] == poison).all())
    assert torch.equal(paged.block_table.cpu(), paged.table)
    for pool in (paged.kq, paged.vq):
        pool_pages(paged, pool)[poison].fill_(NAN16)
    snap = [pool_pages(paged, pool)[poison].clone() for pool in (paged.kq, paged.vq)]
    for fn, qq, kw, ref in outs:
        got = fn(qq, paged, **kw)
        assert bool(torch.isfinite(got).all())
        assert torch.equal(bits(got), bits(ref)), ("after trim", fn.__name__, kw.get("group"))
    for pool, s in zip((paged.kq, paged.vq), snap):
        assert torch.equal(pool_pages(paged, pool)[poison], s), "the poison page was written"


@pytest.mark.parametrize("P", [32, 64])
def test_pool_smaller_than_the_sequence(P):
    """ceil((W + 16) / P) + 1 pages a row; append -> decode -> trim over 6 P steps matches the contiguous cache step by step, bit for bit;
    without trim `ensure` runs out of pages"""
    import torch
    from mi355q import ops
    B, D, W = 2, 64, 24
    steps = 6 * P
    pages = -(-(W + 16) // P) + 1
    torch.manual_seed(P)
    k, v, q = (torch.randn(B, steps, D, device=DEV) for _ in range(3))
    contig = ops.KVCache(B, steps, D, par(), par(), DEV)
    for trim in (True, False):
        paged = ops.PagedKVCache(B, D, par(), par(), DEV, page_size=P, num_pages=B * pages, max_pages=steps // P)
        try:
            for t in range(steps):
                paged.ensure([t + 1] * B)
                before, after = i32([t] * B), i32([t + 1] * B)
                paged.append(k[:, t:t + 1], v[:, t:t + 1], lengths=before, max_length=t)
                got = ops.bfp_attention_decode(q[:, t:t + 1], paged, scale_div=8.0, lengths=after, max_length=t + 1, window=W)
                if trim:
                    contig.append(k[:, t:t + 1], v[:, t:t + 1], lengths=before, max_length=t)
                    ref = ops.bfp_attention_decode(q[:, t:t + 1], contig, scale_div=8.0, lengths=after, max_length=t + 1, window=W)
                    assert torch.equal(bits(got), bits(ref)), f"step {t}"
                    paged.trim([t + 1] * B, W)
            assert trim, "the pool cannot hold the untrimmed sequence"
            assert all(sum(p is not None for p in row) <= pages for row in paged.held)
        except RuntimeError as e:
            assert not trim and "more pages" in str(e), e
