"""Chunked prefill on the paged block_fp KV cache: ops.bfp_attention_extend on an ops.PagedKVCache gives the bits of the same call on
an ops.KVCache holding the same keys.  Rows (B = 3, after the append): 170 keys with 70 queries (M = 70 behind L = 100), 100 keys with
no query, 70 keys with 33 queries -- the last has need = 5 key tiles for its last query block: an odd count whose last tile, tile 4,
is the FIRST tile of a page at P = 32 and P = 64, so the last step's second tile does not exist (the clamp case, and a last pair
without its second tile); the table entry behind that page is the poison page."""
import math
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from paged_util import DEV, assert_untouched, bits, fill_both, i32  # noqa: E402

pytestmark = pytest.mark.gpu
B, M = 3, 70
AFTER, COUNTS = [170, 100, 70], [70, 0, 33]


def _case(P, D, rows=B, seed=0):
    import torch
    g = torch.Generator(device=DEV).manual_seed(P + D + seed)
    k = torch.randn(B, max(AFTER), D, device=DEV, generator=g) * torch.exp(0.5 * torch.randn(B, 1, D, device=DEV, generator=g))
    v = torch.randn(B, max(AFTER), D, device=DEV, generator=g)
    q = torch.randn(rows, M, D, device=DEV, generator=g)
    paged, contig = fill_both(k, v, AFTER, D, P, -(-max(AFTER) // P))
    need = (AFTER[2] - 1) // 16 + 1
    assert need % 2 == 1 and (need - 1) % (P // 16) == 0       # the clamp case, restated
    return q, paged, contig


def _both(q, paged, contig, **kw):
    import torch
    from mi355q import ops
    got, want = ops.bfp_attention_extend(q, paged, **kw), ops.bfp_attention_extend(q, contig, **kw)
    assert torch.equal(bits(got), bits(want)) and bool(torch.isfinite(got).all()) and bool(got.any())
    assert_untouched(paged)
    return got


@pytest.mark.parametrize("D", [32, 64, 96, 128])
@pytest.mark.parametrize("P", [32, 64])
def test_paged_extend_equals_contiguous_bit_for_bit(P, D):
    q, paged, contig = _case(P, D)
    out = _both(q, paged, contig, causal=True, scale_div=math.sqrt(D), lengths=i32(AFTER), counts=i32(COUNTS), max_length=max(AFTER))
    assert not out[1].any() and not out[2, 33:].any() and bool(out[2, 32].any())
    # every row with all M queries: row 2 (70 keys, 70 queries) walks its odd tile count in every query block
    _both(q, paged, contig, causal=True, scale_div=math.sqrt(D), lengths=i32(AFTER), max_length=max(AFTER))


@pytest.mark.parametrize("P", [32, 64])
def test_grouped_queries(P):
    q, paged, contig = _case(P, 64, rows=B * 4)
    _both(q, paged, contig, causal=True, scale_div=8.0, lengths=i32(AFTER), counts=i32(COUNTS), max_length=max(AFTER), group=4)


@pytest.mark.parametrize("P", [32, 64])
def test_noncausal_with_q_scale_and_scale_div(P):
    """every query sees all of its row's keys: each query block walks all need = 5 (row 2), 7 (row 1) and 11 (row 0) tiles"""
    q, paged, contig = _case(P, 128)
    _both(q, paged, contig, causal=False, q_scale=0.25, scale_div=3.0, lengths=i32(AFTER), counts=i32([70, 5, 33]), max_length=max(AFTER))


@pytest.mark.parametrize("P", [32, 64])
def test_token_major(P):
    import torch
    q, paged, contig = _case(P, 64)
    q4 = q.view(1, B, M, 64)
    out = _both(q4, paged, contig, causal=True, scale_div=8.0, lengths=i32(AFTER), counts=i32(COUNTS), max_length=max(AFTER), token_major=True)
    assert out.shape == (1, B, M, 64) and out.stride() == (M * B * 64, 64, B * 64, 1)
    plain = _both(q4, paged, contig, causal=True, scale_div=8.0, lengths=i32(AFTER), counts=i32(COUNTS), max_length=max(AFTER))
    assert torch.equal(out.contiguous(), plain)
