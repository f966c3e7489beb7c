"""The paged block_fp KV cache on the GPU (ops.PagedKVCache.append / dequantised): three successive ragged appends on a paged cache
and on a contiguous ops.KVCache with the same inputs.  The property: PAGING CHANGES WHERE A PIECE LIES, NOT ITS BITS -- the quantised
K and V read back through the table, and the staged rows, are those of the contiguous cache as integers; pages in no table keep
their sentinel, and a row that takes no key keeps every byte."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from paged_util import DEV, assert_untouched, bits, grow, i32, make_paged, par, pool_pages  # noqa: E402

pytestmark = pytest.mark.gpu


def _appends(P):
    """counts of the three appends (B = 3) and the edge each is there for"""
    return ([10, P - 5, 20],        # into empty rows
            [0, 12, 50],            # a count of 0; P - 5 -> P + 7 crosses a page edge; 20 -> 70 crosses two pages at P = 32 (32, 64)
            [12, P - 7, 0])         # 10 -> 22 crosses the 16-key tile edge inside a page; P + 7 -> 2 P ends exactly on a page edge


@pytest.mark.parametrize("width", [6, 4])
@pytest.mark.parametrize("D", [32, 64, 96, 128])
@pytest.mark.parametrize("P", [32, 64, 128])
def test_paged_appends_give_the_contiguous_caches_integers(P, D, width):
    import torch
    from mi355q import ops
    B, max_pages = 3, 3
    r = np.random.default_rng(P + D + width)
    paged, plan = make_paged(B, D, P, max_pages, width)
    contig = ops.KVCache(B, max_pages * P, D, par(width), par(width), DEV)
    lengths = [0] * B
    for counts in _appends(P):
        n = max(counts)
        k = (r.normal(size=(B, n, D)) * np.exp(r.normal(size=(B, 1, D)) * 0.5)).astype(np.float32)
        v = r.normal(size=(B, n, D)).astype(np.float32)
        k[2, 0, 5] = v[0, 1, 3] = 0.0
        for b, c in enumerate(counts):                         # input rows behind a row's count never arrive
            k[b, c:] = np.nan
            v[b, c:] = np.nan
        kt, vt = torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV)
        after = [l + c for l, c in zip(lengths, counts)]
        grow(paged, plan, after)
        kept = [(pool_pages(paged, paged.kq)[paged.held[b]].clone(), pool_pages(paged, paged.vq)[paged.held[b]].clone(),
                 bits(paged.stage).view(B, -1)[b].clone()) for b in range(B)]
        for c in (paged, contig):
            c.append(kt, vt, lengths=i32(lengths), counts=i32(counts), max_length=max(lengths))
        lengths = after
        got = paged.dequantised(lengths=i32(lengths), max_length=max(lengths))
        want = contig.dequantised(lengths=i32(lengths), max_length=max(lengths))
        for name, g, w in zip("KV", got, want):
            assert torch.equal(g.view(torch.int32), w.view(torch.int32)), f"{name} differs from the contiguous cache at lengths {lengths}"
            assert bool(torch.isfinite(g).all())
        assert torch.equal(bits(paged.stage), bits(contig.stage)), f"staged rows differ at lengths {lengths}"
        for b, c in enumerate(counts):
            if c == 0:
                now = (pool_pages(paged, paged.kq)[paged.held[b]], pool_pages(paged, paged.vq)[paged.held[b]], bits(paged.stage).view(B, -1)[b])
                assert all(torch.equal(x, y) for x, y in zip(kept[b], now)), f"row {b} took no key and changed"
        assert_untouched(paged)
    assert lengths == [22, 2 * P, 70]
    # the rows' pages lie where the plan put them: interleaved, row 0 descending, row 1 ascending
    assert paged.held[0] == plan[0][:1] and paged.held[1] == plan[1][:2] and paged.held[2] == plan[2][:paged.pages_for(70)]
    assert plan[0][0] > plan[0][1] and plan[1][0] < plan[1][1] and plan[2][0] > plan[2][1]
    assert all(abs(row[0] - row[1]) >= B for row in plan), "between a row's consecutive pages lie the other rows' pages"
