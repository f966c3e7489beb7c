"""Decode attention on the paged block_fp KV cache: ops.bfp_attention_decode on an ops.PagedKVCache gives the bits of the contiguous
ragged call on an ops.KVCache holding the same keys -- same explicit `splits`, same default -- for every head_dim, M, page size and
row length at, next to and across the page edges; one case per head_dim is also held to the fp64 oracle and the bounds of
tests/test_gpu_decode_ragged.py.  Tables are out of order and padded with a poison page (tests/paged_util.py)."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from paged_util import DEV, assert_untouched, bits, fill_both, grow, i32, make_paged, par  # noqa: E402

pytestmark = pytest.mark.gpu
B = 3


def _kv(L, D, seed, rows=B):
    import torch
    g = torch.Generator(device=DEV).manual_seed(seed)
    k = torch.randn(rows, L, D, device=DEV, generator=g) * torch.exp(0.5 * torch.randn(rows, 1, D, device=DEV, generator=g))
    return k, torch.randn(rows, L, D, device=DEV, generator=g), g


def _length_sets(M, P):
    """every length of {0, M - 1, M, P - 1, P, P + 1, 2 P + 17}, three rows at a time"""
    return ([2 * P + 17, P, M - 1], [P + 1, P - 1, M], [0, 2 * P + 17, P + 1])


def _explicit_splits(P, D, rows=B):
    """a request whose partition of max_length = 2 P + 17 keys has a split boundary on a page edge and, where a page holds more than
    one key pair (P > 32), another inside a page -- checked here, on the CPU, from ops.decode_splits"""
    from mi355q import ops
    L = 2 * P + 17
    ask = {32: 3, 64: 5, 128: 5}[P]
    S = ops.decode_splits(rows, L, D, ask)
    NP = (L + 31) // 32
    pps = -(-NP // S)
    edges = [i * pps * 32 for i in range(1, S)]
    assert S > 1 and any(e % P == 0 for e in edges), (S, edges)
    assert P == 32 or any(e % P for e in edges), (S, edges)
    return ask


@pytest.mark.parametrize("M", [1, 7, 16])
@pytest.mark.parametrize("D", [32, 64, 96, 128])
@pytest.mark.parametrize("P", [32, 64, 128])
def test_paged_decode_equals_the_contiguous_ragged_call_bit_for_bit(P, D, M):
    import torch
    from mi355q import ops
    L = 2 * P + 17
    k, v, g = _kv(L, D, P + D + M)
    q = torch.randn(B, M, D, device=DEV, generator=g)
    ask = _explicit_splits(P, D)
    for lengths in _length_sets(M, P):
        paged, contig = fill_both(k, v, lengths, D, P, 3)
        for splits in (ask, None):
            kw = dict(causal=True, scale_div=math.sqrt(D), splits=splits, lengths=i32(lengths), max_length=L)
            got, want = ops.bfp_attention_decode(q, paged, **kw), ops.bfp_attention_decode(q, contig, **kw)
            assert torch.equal(bits(got), bits(want)), f"lengths {lengths}, splits {splits}"
            assert bool(torch.isfinite(got).all())
            for b, n in enumerate(lengths):
                assert bool(got[b].any()) == (n >= M), f"row {b} of {n} keys"
        assert_untouched(paged)


@pytest.mark.parametrize("D", [32, 128])
def test_noncausal_with_q_scale(D):
    import torch
    from mi355q import ops
    P, M = 64, 7
    L = 2 * P + 17
    k, v, g = _kv(L, D, D)
    q = torch.randn(B, M, D, device=DEV, generator=g)
    for lengths in _length_sets(M, P):
        paged, contig = fill_both(k, v, lengths, D, P, 3)
        for splits in (_explicit_splits(P, D), None):
            kw = dict(causal=False, q_scale=D ** -0.5, splits=splits, lengths=i32(lengths), max_length=L)
            assert torch.equal(bits(ops.bfp_attention_decode(q, paged, **kw)), bits(ops.bfp_attention_decode(q, contig, **kw)))
        assert_untouched(paged)


@pytest.mark.parametrize("M", [1, 7])
@pytest.mark.parametrize("P", [32, 128])
def test_grouped_queries(P, M):
    """group = 4: M = 1 puts the four heads into one launch row (gw = 4), M = 7 two heads a launch row and two launch rows a cache row"""
    import torch
    from mi355q import ops
    D, G = 64, 4
    L = 2 * P + 17
    k, v, g = _kv(L, D, P + M)
    q = torch.randn(B * G, M, D, device=DEV, generator=g)
    rows = B * G // ops.decode_group_width(G, M)
    for lengths in _length_sets(M, P):
        paged, contig = fill_both(k, v, lengths, D, P, 3)
        for splits in (_explicit_splits(P, D, rows), None):
            kw = dict(causal=True, scale_div=8.0, splits=splits, lengths=i32(lengths), max_length=L, group=G)
            got, want = ops.bfp_attention_decode(q, paged, **kw), ops.bfp_attention_decode(q, contig, **kw)
            assert torch.equal(bits(got), bits(want)), f"lengths {lengths}, splits {splits}"
        assert_untouched(paged)


@pytest.mark.parametrize("D", [32, 64, 96, 128])
def test_paged_decode_vs_the_fp64_oracle(D):
    """M = 7, P = 64, rows of 145, 64 and 6 keys: the rows that have their 7 queries' keys against the oracle on THEIR keys, with the
    bounds of tests/test_gpu_decode_ragged.py (1e-3 worst, 3e-5 mean, of max|ref|); the row of 6 keys is an empty slot: zeros"""
    import torch
    from mi355q import ops
    from test_gpu_decode_ragged import _cfg, _check, _inputs, _oracle
    P, M, lengths = 64, 7, [145, 64, 6]
    q, k, v = _inputs(B, M, 145, D, seed=D)
    paged, _ = fill_both(torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV), lengths, D, P, 3)
    out = ops.bfp_attention_decode(torch.from_numpy(q).to(DEV), paged, causal=True, scale_div=math.sqrt(D), splits=_explicit_splits(P, D),
                                   lengths=i32(lengths), max_length=145).cpu().numpy()
    for b, n in enumerate(lengths[:2]):
        print("row", b, "length", n, end=": ")
        _check(out[b], _oracle(q[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n], _cfg(6), _cfg(6), causal=True, scale_div=math.sqrt(D))[0])
    assert not out[2].any()


@pytest.mark.parametrize("P", [32, 64])
def test_two_rows_share_their_first_two_pages(P):
    """rows 0 and 1 hold the same first 2 P keys -- row 1 through share_prefix, the pages stored once -- and different tails; the
    decode gives the bits of two private copies (a contiguous cache that holds the prefix twice)"""
    import torch
    from mi355q import ops
    D, M = 64, 3
    tails = [21, 40]
    k, v, g = _kv(2 * P + 40, D, P, rows=2)
    k[1, :2 * P], v[1, :2 * P] = k[0, :2 * P], v[0, :2 * P]
    q = torch.randn(2, M, D, device=DEV, generator=g)
    lengths = [2 * P + t for t in tails]
    paged, plan = make_paged(2, D, P, 4)
    grow(paged, plan, [lengths[0], 0])
    paged.append(k[:, :lengths[0]], v[:, :lengths[0]], lengths=i32([0, 0]), counts=i32([lengths[0], 0]), max_length=0)
    paged.share_prefix(0, 1, 2)
    assert paged.held[1] == paged.held[0][:2]
    grow(paged, plan, lengths)                                  # row 1's own tail pages
    assert not set(paged.held[1][2:]) & set(paged.held[0])
    paged.append(k[:, 2 * P:2 * P + tails[1]].contiguous(), v[:, 2 * P:2 * P + tails[1]].contiguous(), lengths=i32([lengths[0], 2 * P]),
                 counts=i32([0, tails[1]]), max_length=lengths[0])
    contig = ops.KVCache(2, 4 * P, D, par(), par(), DEV)
    contig.append(k, v, lengths=i32([0, 0]), counts=i32(lengths), max_length=0)
    for splits in (3, None):
        kw = dict(causal=True, scale_div=8.0, splits=splits, lengths=i32(lengths), max_length=max(lengths))
        assert torch.equal(bits(ops.bfp_attention_decode(q, paged, **kw)), bits(ops.bfp_attention_decode(q, contig, **kw)))
    for a, b in zip(paged.dequantised(i32(lengths), max(lengths)), contig.dequantised(i32(lengths), max(lengths))):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert_untouched(paged)


def test_one_captured_step_serves_growing_lengths_across_a_page_edge():
    """tests/test_gpu_decode_ragged.py::test_one_captured_step_serves_growing_lengths on the paged cache: one append + decode step
    (n = 1) captured ONCE with the default number of hardware queues; between replays the host hands out pages (ensure: one copy_
    into the table the graph reads) and advances the length tensors in place.  Rows start at 30, 31, 62, 5 keys (P = 32): the three
    replays take rows 0 and 1 over the page edge at 32 and row 2 over the one at 64.  Every replay: the bytes of the eager
    contiguous step."""
    import torch
    from mi355q import ops
    Bn, D, P, max_pages, start = 4, 64, 32, 3, [30, 31, 62, 5]
    C = max_pages * P
    torch.manual_seed(13)
    k0, v0 = torch.randn(Bn, 62, D, device=DEV), torch.randn(Bn, 62, D, device=DEV)
    steps = [tuple(torch.randn(Bn, 1, D, device=DEV) for _ in range(3)) for _ in range(3)]

    def step(cache, kn, vn, q, before, after):
        cache.append(kn, vn, lengths=before, max_length=C - 1)
        return ops.bfp_attention_decode(q, cache, scale_div=8.0, splits=2, lengths=after, max_length=C)

    eager = ops.KVCache(Bn, C, D, par(), par(), DEV)
    eager.append(k0, v0, lengths=i32([0] * Bn), counts=i32(start), max_length=0)
    want = [step(eager, kn, vn, q, i32([s + i for s in start]), i32([s + i + 1 for s in start])).clone() for i, (kn, vn, q) in enumerate(steps)]
    cache = ops.PagedKVCache(Bn, D, par(), par(), DEV, page_size=P, num_pages=Bn * max_pages, max_pages=max_pages)
    cache.ensure([s + 1 for s in start])                        # the warm-up and the first replay append key start[b]
    cache.append(k0, v0, lengths=i32([0] * Bn), counts=i32(start), max_length=0)
    held = [len(h) for h in cache.held]
    kn, vn, q = (t.clone() for t in steps[0])
    before, after = i32(start), i32([s + 1 for s in start])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # (warm-up on the capture stream: the workspace exists before the capture)
        step(cache, kn, vn, q, before, after)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = step(cache, kn, vn, q, before, after)
    for i, new in enumerate(steps):
        for dst, src in zip((kn, vn, q), new):
            dst.copy_(src)
        cache.ensure([s + i + 1 for s in start])
        before.copy_(i32([s + i for s in start]))
        after.copy_(i32([s + i + 1 for s in start]))
        got.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(got), bits(want[i])), f"replay {i} differs from the eager contiguous step"
    assert [len(h) for h in cache.held] == [h + 1 for h in held[:3]] + held[3:], "rows 0 .. 2 each crossed one page edge"
    final = [s + 3 for s in start]
    for a, b in zip(cache.dequantised(i32(final), max(final)), eager.dequantised(lengths=i32(final), max_length=max(final))):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(bits(cache.stage), bits(eager.stage))
