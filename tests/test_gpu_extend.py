"""Chunked prefill on the GPU: ops.bfp_attention_extend (any number of queries per row behind the block_fp KV cache) against the
oracle's restatement of the reference's steps on the concatenated K / V -- the recipe and the bounds of tests/test_gpu_decode.py,
restated here: worst <= 1e-3 max|ref|, mean <= 3e-5 max|ref|."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))

pytestmark = pytest.mark.gpu
FMIN = np.finfo(np.float32).min
DEV = "cuda:0"


def _cfg(width, **extra):
    return dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=width, data_in_exponent_width=8,
                data_in_exponent_bias=127, data_in_block_size=[1, 16], weight_width=width, weight_exponent_width=8,
                weight_exponent_bias=127, weight_block_size=[1, 16], **extra)


def _par(width):
    return (width, 8, 127, width, 8, 127)


def _oracle(q, k, v, c0, c1, causal=False, scale_div=None):
    from oracle import np_oracle as O
    w = O.matmul_quantized(q, np.swapaxes(k, -1, -2), c0)
    if scale_div:
        w = (w / np.float32(scale_div)).astype(np.float32)
    tq, tk = w.shape[-2:]
    if causal:
        m = np.triu(np.full((tq, tk), FMIN, np.float32), 1 + tk - tq)
        with np.errstate(over="ignore"):
            w = np.maximum(w + m, FMIN)
    e = np.exp((w - w.max(-1, keepdims=True)).astype(np.float64))
    p = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    return O.matmul_quantized(p, v, c1)


def _inputs(B, M, T, hd, seed):
    r = np.random.default_rng(seed)
    q = (r.normal(size=(B, M, hd)) * np.exp(r.normal(size=(B, M, 1)) * 0.5) * 0.7).astype(np.float32)
    k = (r.normal(size=(B, T, hd)) * np.exp(r.normal(size=(B, 1, hd)) * 0.5)).astype(np.float32)
    v = r.normal(size=(B, T, hd)).astype(np.float32)
    return q, k, v


def _check(out, ref):
    scale = np.abs(ref).max()
    print("worst", np.abs(out - ref).max() / scale, "mean", np.abs(out - ref).mean() / scale)
    assert np.abs(out - ref).max() <= 1e-3 * scale, (np.abs(out - ref).max(), scale)
    assert np.abs(out - ref).mean() <= 3e-5 * scale, (np.abs(out - ref).mean(), scale)


def _filled(k, v, wqk, wpv, capacity=None, pieces=None):
    import torch
    from mi355q import ops
    B, L, D = k.shape
    cache = ops.KVCache(B, capacity or (L + 15) // 16 * 16, D, _par(wqk), _par(wpv), DEV)
    kt, vt = torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV)
    at = 0
    for n in pieces or (L,):
        cache.append(kt[:, at:at + n], vt[:, at:at + n])
        at += n
    assert cache.length == L
    return cache


def _quantised_v(v, width):
    from oracle import compare, np_oracle as O
    return compare.bf16_rne(O.block_fp_quantize(v, width, 8, 127, block_size=[1, 16]))


def _bits(t):
    import torch
    return t.contiguous().view(torch.uint8)


CASES = [(2, 17, 17, 64, 6, 6), (2, 17, 40, 64, 6, 6), (3, 33, 100, 128, 6, 6), (2, 64, 64, 32, 4, 6), (2, 65, 333, 96, 5, 5),
         (2, 5, 45, 64, 9, 9), (1, 130, 1040, 64, 6, 6)]


@pytest.mark.parametrize("B,M,L,D,wqk,wpv", CASES)
def test_extend_vs_oracle(B, M, L, D, wqk, wpv):
    """causal with scale_div = sqrt(D), and non-causal with q_scale; the cache filled in pieces (L - M, M), so the open block is
    re-quantised.  (2,17,17): the second query tile holds one query, and query 0 sees ONE key -- its probability 1 is quantised to
    (2^(w-1) - 1) / 2^(w-1), the output row is exactly that times the key's quantised V row.  (2,64,64): exactly one full workgroup.
    (2,65,333): two workgroups, 21 key tiles (an odd count), the last V pair half empty.  (1,130,1040): three query blocks, 65 tiles."""
    import torch
    from mi355q import ops
    from oracle import np_oracle as O
    q, k, v = _inputs(B, M, L, D, seed=L + D + M)
    cache = _filled(k, v, wqk, wpv, capacity=(L + 31) // 16 * 16, pieces=(L - M, M) if L > M else (L,))
    qt = torch.from_numpy(q).to(DEV)
    c0, c1 = _cfg(wqk), _cfg(wpv)
    out = ops.bfp_attention_extend(qt, cache, causal=True, scale_div=math.sqrt(D)).cpu().numpy()
    _check(out, _oracle(q, k, v, c0, c1, causal=True, scale_div=math.sqrt(D)))
    if L == M:
        one = np.zeros((1, 16), np.float32)
        one[0, 0] = 1.0
        p1 = O.block_fp_quantize(one, wpv, 8, 127, block_size=[1, 16])[0, 0]
        assert p1 == np.float32(1.0 - 2.0 ** (1 - wpv))
        assert np.array_equal(out[:, 0], p1 * _quantised_v(v, wpv)[:, 0]), "a query that sees one key must return that key's quantised V row times Q(1)"
    scaling = np.float32(D ** -0.5)
    out = ops.bfp_attention_extend(qt, cache, causal=False, q_scale=float(scaling)).cpu().numpy()
    _check(out, _oracle(q * scaling, k, v, c0, c1, causal=False))


def test_capacity_edge_nothing_behind_the_row_is_used():
    """B = 2, D = 64, capacity 48: three key tiles a row (an odd count), both rows full, M = 20.  kq / vq are the leading kv_k_bytes = 12288
    and kv_v_bytes = 16384 bytes (two 32-key pairs a row, the second half empty) of larger buffers whose tails hold bf16 NaNs: the output keeps its bits.  Row 0 keeps
    them too when row 1 holds other keys.  (Not a proof that nothing is loaded from there -- the design note argues that -- but that
    nothing read there is used.)"""
    import torch
    from mi355q import ops
    B, M, L, D = 2, 20, 48, 64
    q, k, v = _inputs(B, M, L, D, seed=48)
    cache = _filled(k, v, 6, 6, capacity=48, pieces=(L - M, M))
    assert cache.kq.numel() == 12288 and cache.vq.numel() == 16384      # exact, no slack: 2 x 3 tiles x 2 KiB, 2 x 2 pairs x 4 KiB
    qt = torch.from_numpy(q).to(DEV)
    want = ops.bfp_attention_extend(qt, cache, causal=True, scale_div=8.0).clone()
    _check(want.cpu().numpy(), _oracle(q, k, v, _cfg(6), _cfg(6), causal=True, scale_div=8.0))
    for name in ("kq", "vq"):
        own = getattr(cache, name).numel()
        big = torch.empty(own + 8192, dtype=torch.uint8, device=DEV)
        big[own:].view(torch.int16).fill_(0x7FC0)
        big[:own].copy_(getattr(cache, name))
        setattr(cache, name, big[:own])
    for causal in (True, False):
        a = ops.bfp_attention_extend(qt, cache, causal=causal, scale_div=8.0)
        assert bool(torch.isfinite(a).all())
        if causal:
            assert torch.equal(_bits(a), _bits(want))
    _, k2, v2 = _inputs(B, M, L, D, seed=49)
    k2[0], v2[0] = k[0], v[0]
    other = _filled(k2, v2, 6, 6, capacity=48, pieces=(L - M, M))
    got = ops.bfp_attention_extend(qt, other, causal=True, scale_div=8.0)
    assert torch.equal(_bits(got[0]), _bits(want[0])) and not torch.equal(_bits(got[1]), _bits(want[1]))


RAGGED = dict(B=4, D=64, C=144, lengths=[45, 16, 0, 130], counts=[17, 16, 0, 33], M=33)


def _ragged_cache(k, v, lengths, counts, C):
    """every row filled in pieces (L_b - m_b, m_b) by two ragged appends"""
    import torch
    from mi355q import ops
    B, _, D = k.shape
    cache = ops.KVCache(B, C, D, _par(6), _par(6), DEV)
    kt, vt = torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV)
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=DEV)
    first = [l - c for l, c in zip(lengths, counts)]
    n1 = max(first)
    cache.append(kt[:, :n1].contiguous(), vt[:, :n1].contiguous(), lengths=i32([0] * B), counts=i32(first), max_length=0)
    n2 = max(counts)
    k2, v2 = torch.zeros(B, n2, D, device=DEV), torch.zeros(B, n2, D, device=DEV)
    for b in range(B):
        k2[b, :counts[b]] = kt[b, first[b]:lengths[b]]
        v2[b, :counts[b]] = vt[b, first[b]:lengths[b]]
    cache.append(k2, v2, lengths=i32(first), counts=i32(counts), max_length=n1)
    return cache


def test_ragged_rows_are_as_if_alone():
    import torch
    from mi355q import ops
    B, D, C, lengths, counts, M = (RAGGED[x] for x in ("B", "D", "C", "lengths", "counts", "M"))
    q, k, v = _inputs(B, M, max(lengths), D, seed=130)
    cache = _ragged_cache(k, v, lengths, counts, C)
    qt = torch.from_numpy(q).to(DEV)
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=DEV)
    out = ops.bfp_attention_extend(qt, cache, causal=True, scale_div=8.0, lengths=i32(lengths), counts=i32(counts), max_length=130)
    for b, (L, m) in enumerate(zip(lengths, counts)):
        assert not out[b, m:].any(), f"row {b}: outputs behind its {m} queries are not zeros"
        if m == 0:
            continue
        _check(out[b:b + 1, :m].cpu().numpy(), _oracle(q[b:b + 1, :m], k[b:b + 1, :L], v[b:b + 1, :L], _cfg(6), _cfg(6), causal=True, scale_div=8.0))
        alone = _filled(k[b:b + 1, :L], v[b:b + 1, :L], 6, 6, capacity=C, pieces=(L - m, m) if L > m else (L,))
        one = ops.bfp_attention_extend(qt[b:b + 1, :m].contiguous(), alone, causal=True, scale_div=8.0)
        assert torch.equal(_bits(one), _bits(out[b:b + 1, :m])), f"row {b} differs from the row alone"
    # a row that asks more queries than it holds keys: an empty slot
    over = ops.bfp_attention_extend(qt, cache, causal=True, scale_div=8.0, lengths=i32(lengths), counts=i32([17, 17, 0, 33]), max_length=130)
    assert not over[1].any() and not over[2].any()
    assert torch.equal(_bits(over[0]), _bits(out[0])) and torch.equal(_bits(over[3]), _bits(out[3]))
    # counts=None: every row asks M = 33; rows 1 and 2 hold fewer keys
    full = ops.bfp_attention_extend(qt, cache, causal=False, q_scale=0.125, lengths=i32(lengths), max_length=130)
    assert not full[1].any() and not full[2].any() and bool(torch.isfinite(full).all())
    _check(full[3:].cpu().numpy(), _oracle(q[3:] * np.float32(0.125), k[3:], v[3:], _cfg(6), _cfg(6), causal=False))


def test_chunk_boundaries_at_multiples_of_16():
    """L = 64 in one call (M = 64) against two calls (M = 32 at L = 32, M = 32 at L = 64): full blocks of K^T are final, so both are
    the one-shot oracle's rows"""
    import torch
    from mi355q import ops
    B, L, D = 2, 64, 64
    q, k, v = _inputs(B, L, L, D, seed=64)
    ref = _oracle(q, k, v, _cfg(6), _cfg(6), causal=True, scale_div=8.0)
    qt, kt, vt = (torch.from_numpy(t).to(DEV) for t in (q, k, v))
    once = ops.bfp_attention_extend(qt, _filled(k, v, 6, 6), causal=True, scale_div=8.0).cpu().numpy()
    cache = ops.KVCache(B, 64, D, _par(6), _par(6), DEV)
    cache.append(kt[:, :32], vt[:, :32])
    a = ops.bfp_attention_extend(qt[:, :32].contiguous(), cache, causal=True, scale_div=8.0).cpu().numpy()
    cache.append(kt[:, 32:], vt[:, 32:])
    b = ops.bfp_attention_extend(qt[:, 32:].contiguous(), cache, causal=True, scale_div=8.0).cpu().numpy()
    _check(once, ref)
    _check(np.concatenate([a, b], 1), ref)
    assert np.abs(b - once[:, 32:]).max() <= 1e-3 * np.abs(ref).max()


def test_chunk_boundary_inside_a_block():
    """a boundary at 37: each call against the oracle at ITS OWN L (the first call's open block 32 .. 36 is quantised without the
    keys behind it: the one-shot result legitimately differs there)"""
    import torch
    from mi355q import ops
    B, L, D, cut = 2, 64, 64, 37
    q, k, v = _inputs(B, L, L, D, seed=37)
    qt, kt, vt = (torch.from_numpy(t).to(DEV) for t in (q, k, v))
    cache = ops.KVCache(B, 64, D, _par(6), _par(6), DEV)
    cache.append(kt[:, :cut], vt[:, :cut])
    a = ops.bfp_attention_extend(qt[:, :cut].contiguous(), cache, causal=True, scale_div=8.0).cpu().numpy()
    _check(a, _oracle(q[:, :cut], k[:, :cut], v[:, :cut], _cfg(6), _cfg(6), causal=True, scale_div=8.0))
    cache.append(kt[:, cut:], vt[:, cut:])
    b = ops.bfp_attention_extend(qt[:, cut:].contiguous(), cache, causal=True, scale_div=8.0).cpu().numpy()
    _check(b, _oracle(q[:, cut:], k, v, _cfg(6), _cfg(6), causal=True, scale_div=8.0))


def test_agrees_with_the_prefill_kernel():
    import torch
    from mi355q import ops
    B, M, L, D = 2, 48, 256, 64
    q, k, v = _inputs(B, M, L, D, seed=L)
    ref = _oracle(q, k, v, _cfg(6), _cfg(6), causal=True, scale_div=8.0)
    cache = _filled(k, v, 6, 6)
    qt, kt, vt = (torch.from_numpy(t).to(DEV) for t in (q, k, v))
    ext = ops.bfp_attention_extend(qt, cache, causal=True, scale_div=8.0).cpu().numpy()
    pre = ops.bfp_attention(qt, kt, vt, _par(6), _par(6), causal=True, scale_div=8.0).cpu().numpy()
    _check(ext, ref)
    _check(pre, ref)
    assert np.abs(ext - pre).max() <= 1e-3 * np.abs(ref).max()


def test_reproducibility_token_major_and_strided_head_views():
    """two runs give equal bits; [1, n, H, D] projections viewed as [1, H, n, D] are read in place, and the token-major output holds the
    bytes of the contiguous call"""
    import torch
    from mi355q import ops
    H, D, L, M = 4, 64, 45, 20
    torch.manual_seed(3)
    kp, vp = torch.randn(1, L, H, D, device=DEV), torch.randn(1, L, H, D, device=DEV)
    qp = torch.randn(1, M, H, D, device=DEV)
    heads = lambda t: t.transpose(1, 2)
    flat = lambda t: heads(t).contiguous().view(H, t.shape[1], D)
    a = ops.KVCache(H, 48, D, _par(6), _par(6), DEV)
    a.append(heads(kp)[:, :, :25], heads(vp)[:, :, :25])
    a.append(heads(kp)[:, :, 25:], heads(vp)[:, :, 25:])
    o_ref = ops.bfp_attention_extend(flat(qp), a, scale_div=8.0)                                  # [H, M, D]
    again = ops.bfp_attention_extend(flat(qp), a, scale_div=8.0)
    assert torch.equal(_bits(o_ref), _bits(again)) and float(o_ref.abs().max()) > 0
    o_tm = ops.bfp_attention_extend(heads(qp), a, scale_div=8.0, token_major=True)                # [1, H, M, D] view of [1, M, H, D]
    assert o_tm.shape == (1, H, M, D) and o_tm.transpose(1, 2).is_contiguous()
    assert torch.equal(_bits(o_tm[0]), _bits(o_ref))
    o_pl = ops.bfp_attention_extend(heads(qp), a, scale_div=8.0)
    assert o_pl.is_contiguous() and torch.equal(_bits(o_pl[0]), _bits(o_ref))


def test_graph_capture_of_one_ragged_call():
    """one ragged extend call captured on a side stream (one stream, no parallel branches) after a warm-up; replayed after lengths
    and counts are rewritten ON THE DEVICE to a second set under the same max_length: each replay gives the bytes of the eager call"""
    import torch
    from mi355q import ops
    B, M, D, C = 3, 20, 64, 64
    q, k, v = _inputs(B, M, C, D, seed=20)
    cache = _filled(k, v, 6, 6, capacity=C)
    qt = torch.from_numpy(q).to(DEV)
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=DEV)
    sets = (([40, 20, 64], [20, 5, 17]), ([64, 33, 0], [20, 20, 0]))
    want = [ops.bfp_attention_extend(qt, cache, scale_div=8.0, lengths=i32(l), counts=i32(c), max_length=C).clone() for l, c in sets]
    assert not torch.equal(_bits(want[0]), _bits(want[1]))
    lengths, counts = i32(sets[0][0]), i32(sets[0][1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.bfp_attention_extend(qt, cache, scale_div=8.0, lengths=lengths, counts=counts, max_length=C)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = ops.bfp_attention_extend(qt, cache, scale_div=8.0, lengths=lengths, counts=counts, max_length=C)
    for (l, c), w in list(zip(sets, want)) + [(sets[0], want[0])]:
        lengths.copy_(i32(l))
        counts.copy_(i32(c))
        got.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _bits(w))
