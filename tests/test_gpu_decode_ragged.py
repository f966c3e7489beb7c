"""Ragged batches on the GPU: per-row lengths in the block_fp KV cache (ops.KVCache.append(lengths=, counts=)) and in the split-key
decode attention (ops.bfp_attention_decode(lengths=)).  The property under test: EACH ROW OF A RAGGED BATCH IS WHAT IT WOULD BE
ALONE -- its cache bytes those of a one-row cache fed the same keys by the uniform append, its attention output the fp64 oracle's
on its own keys (the construction and the bounds of tests/test_gpu_decode.py, restated here)."""
import functools
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


def _cfg(width):
    return dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=width, data_in_exponent_width=8,
                data_in_exponent_bias=127, data_in_block_size=[1, 16], weight_width=width, weight_exponent_width=8,
                weight_exponent_bias=127, weight_block_size=[1, 16])


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


def _i32(values):
    import torch
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


def _ragged_cache(k, v, lengths, width=6, capacity=None):
    """a cache whose row b holds k[b, :lengths[b]], v[b, :lengths[b]]: ONE ragged append from empty rows (rows behind a row's count
    are padding)"""
    import torch
    from mi355q import ops
    B, T, D = k.shape
    cache = ops.KVCache(B, capacity or (T + 15) // 16 * 16, D, _par(width), _par(width), DEV)
    cache.append(torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV), lengths=_i32([0] * B), counts=_i32(lengths), max_length=0)
    assert cache.length == 0                       # the caller owns the lengths
    return cache


def _bytes(t):
    import torch
    return t.contiguous().view(torch.uint8)


# ---- 1. the cache ---------------------------------------------------------------------------------------------------------
APPENDS = ([0, 0, 15, 16, 20, 10],      # a tile filled but for one key (15), filled exactly (16), more than a tile (20)
           [0, 1, 1, 0, 0, 9],          # one key into an empty row; 15 then 1: ends on the tile edge; 10 then 9: crosses it
           [0, 0, 0, 1, 13, 21])        # a key behind a full tile; 20 + 13 crosses the 32-key pair; 21 > 16 from 19 crosses both
FINAL = [0, 1, 16, 17, 33, 40]


@pytest.mark.parametrize("D", [32, 64, 96, 128])
@pytest.mark.parametrize("width", [4, 6, 9])
def test_cache_rows_are_the_one_row_caches_bit_for_bit(D, width):
    """(D = 32, 96: the ragged append at 8 and 2 tiles per workgroup.)  three ragged appends; after each, row b's quantised K and V (as uint32) and its staged rows are those of a uniform one-row
    cache fed the same keys by the existing append; a row with count 0 keeps its bytes; input rows behind a row's count are NaN
    and never arrive"""
    import torch
    from mi355q import ops
    B, C = 6, 48
    r = np.random.default_rng(D + width)
    cache = ops.KVCache(B, C, D, _par(width), _par(width), DEV)
    alone = [ops.KVCache(1, C, D, _par(width), _par(width), DEV) for _ in range(B)]
    lengths = [0] * B
    for counts in APPENDS:
        n = max(counts)
        k = (r.normal(size=(B, n, D)) * np.exp(r.normal(size=(B, 1, D)) * 0.5)).astype(np.float32)
        v = r.normal(size=(B, n, D)).astype(np.float32)
        k[2, 0, 5] = v[4, 1, 3] = 0.0
        k[5, :, 9] = 0.0                                       # an all-zero block at one d
        for b, c in enumerate(counts):
            k[b, c:] = np.nan
            v[b, c:] = np.nan
        kt, vt = torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV)
        before = [(_bytes(t).view(B, -1).clone()) for t in (cache.kq, cache.vq, cache.stage)]
        cache.append(kt, vt, lengths=_i32(lengths), counts=_i32(counts), max_length=max(lengths))
        assert cache.length == 0
        after = [_bytes(t).view(B, -1) for t in (cache.kq, cache.vq, cache.stage)]
        lengths = [l + c for l, c in zip(lengths, counts)]
        kd, vd = (t.cpu().numpy() for t in cache.dequantised(lengths=_i32(lengths), max_length=max(lengths)))
        assert kd.shape == (B, max(lengths), D)
        for b, c in enumerate(counts):
            if c == 0:
                for x, y in zip(before, after):
                    assert torch.equal(x[b], y[b]), f"row {b} took no key and changed"
            else:
                alone[b].append(kt[b:b + 1, :c], vt[b:b + 1, :c])
            L = lengths[b]
            assert alone[b].length == L
            assert not kd[b, L:].any() and not vd[b, L:].any(), f"row {b}: dequantised() is not zero behind its length {L}"
            if L:
                ka, va = (t.cpu().numpy() for t in alone[b].dequantised())
                assert np.array_equal(kd[b, :L].view(np.uint32), ka[0].view(np.uint32)), f"K of row {b} differs at length {L}"
                assert np.array_equal(vd[b, :L].view(np.uint32), va[0].view(np.uint32)), f"V of row {b} differs at length {L}"
            assert torch.equal(after[2][b], _bytes(alone[b].stage).view(-1)), f"staged rows of row {b} differ at length {L}"
    assert lengths == FINAL
    assert bool(torch.isfinite(cache.kq.view(torch.bfloat16).float()).all()) and bool(torch.isfinite(cache.vq.view(torch.bfloat16).float()).all())


# ---- 2. decode against the oracle, row by row --------------------------------------------------------------------------------
def _lengths(M):
    return [max(L, M) for L in (M, 16, 17, 31, 32, 33, 100, 257)]


@functools.lru_cache(maxsize=None)
def _case(M, D):
    """inputs, the ragged cache and every row's oracle output for (M, D): made once, shared by the split cases, never written"""
    B, T = 8, 257
    q, k, v = _inputs(B, M, T, D, seed=M + D)
    lengths = _lengths(M)
    ref = [_oracle(q[b:b + 1], k[b:b + 1, :L], v[b:b + 1, :L], _cfg(6), _cfg(6), causal=True, scale_div=math.sqrt(D))[0]
           for b, L in enumerate(lengths)]
    for a in ref:
        a.setflags(write=False)
    # the queries are each row's LAST M positions: the keys behind lengths[b] are never appended
    return q, k, v, lengths, ref, _ragged_cache(k, v, lengths, capacity=272)


@pytest.mark.parametrize("splits", [None, 1, 4])
@pytest.mark.parametrize("D", [32, 64, 96, 128])
@pytest.mark.parametrize("M", [1, 7, 16])
def test_ragged_decode_vs_oracle_row_by_row(M, D, splits):
    """B = 8, lengths M (or 16), 16, 17, 31, 32, 33, 100, 257: every row against the oracle on ITS keys.  Four splits over
    max_length = 257 (nine key pairs -> three splits of three pairs): every row but the last has entirely empty splits.
    D = 32 and 96 are the ragged kernels' one- and three-chunk instantiations; M = 7 puts each row's causal horizon L_b - 7 + i
    inside, at and across tile and pair edges (rows of 7, 16, 17, 31, 32, 33, 100, 257 keys) with the query columns 7 .. 15 of
    the MFMA tiles clamped."""
    import torch
    from mi355q import ops
    q, k, v, lengths, ref, cache = _case(M, D)
    out = ops.bfp_attention_decode(torch.from_numpy(q).to(DEV), cache, causal=True, scale_div=math.sqrt(D), splits=splits,
                                   lengths=_i32(lengths), max_length=257).cpu().numpy()
    assert np.isfinite(out).all()
    for b, L in enumerate(lengths):
        print("row", b, "length", L, end=": ")
        _check(out[b], ref[b])


@functools.lru_cache(maxsize=None)
def _case_noncausal(M, D):
    """the same rows, the OPT form: q * D^-0.5 in front of the quantiser, every key of the row visible to every query"""
    q, k, v, lengths, _, cache = _case(M, D)
    scaling = np.float32(D ** -0.5)
    ref = [_oracle(q[b:b + 1] * scaling, k[b:b + 1, :L], v[b:b + 1, :L], _cfg(6), _cfg(6), causal=False)[0] for b, L in enumerate(lengths)]
    for a in ref:
        a.setflags(write=False)
    return q, lengths, ref, cache, float(scaling)


@pytest.mark.parametrize("splits", [None, 4])
@pytest.mark.parametrize("D", [32, 128])
def test_ragged_noncausal_decode_with_q_scale_vs_oracle_row_by_row(D, splits):
    """causal=False, q_scale = D^-0.5, M = 7, the lengths above: every row against the oracle on ITS keys, the bounds above"""
    import torch
    from mi355q import ops
    q, lengths, ref, cache, scaling = _case_noncausal(7, D)
    out = ops.bfp_attention_decode(torch.from_numpy(q).to(DEV), cache, causal=False, q_scale=scaling, splits=splits,
                                   lengths=_i32(lengths), max_length=257).cpu().numpy()
    assert np.isfinite(out).all()
    for b, L in enumerate(lengths):
        print("non-causal row", b, "length", L, end=": ")
        _check(out[b], ref[b])


# ---- 3. inactive rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [None, 2])
def test_rows_shorter_than_the_queries_are_zero(splits):
    import torch
    from mi355q import ops
    M, D, lengths = 8, 64, [0, 5, 40]
    q, k, v = _inputs(3, M, 40, D, seed=3)
    cache = _ragged_cache(k, v, lengths)
    out = ops.bfp_attention_decode(torch.from_numpy(q).to(DEV), cache, causal=True, scale_div=8.0, splits=splits, lengths=_i32(lengths),
                                   max_length=40)
    assert not _bytes(out[:2]).any(), "rows with fewer keys than queries must be exactly zero"
    _check(out[2].cpu().numpy(), _oracle(q[2:], k[2:], v[2:], _cfg(6), _cfg(6), causal=True, scale_div=8.0)[0])


# ---- 4. bit equality with the uniform kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("L", [33, 257])
def test_equal_lengths_give_the_uniform_kernels_bits(L, splits):
    import torch
    from mi355q import ops
    B, M, D = 3, 5, 64
    q, k, v = _inputs(B, M, L, D, seed=L)
    cache = ops.KVCache(B, (L + 15) // 16 * 16, D, _par(6), _par(6), DEV)
    cache.append(torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV))
    qt = torch.from_numpy(q).to(DEV)
    uni = ops.bfp_attention_decode(qt, cache, scale_div=8.0, splits=splits)
    rag = ops.bfp_attention_decode(qt, cache, scale_div=8.0, splits=splits, lengths=_i32([L] * B), max_length=L)
    assert torch.equal(_bytes(rag), _bytes(uni))
    # and the ragged append of the same keys makes the same cache
    same = _ragged_cache(k, v, [L] * B)
    assert torch.equal(same.kq, cache.kq) and torch.equal(same.vq, cache.vq)


@pytest.mark.parametrize("M,D", [pytest.param(1, 64, id="1"), pytest.param(3, 64, id="3"), pytest.param(7, 96, id="7-D96")])
def test_one_split_rows_equal_the_one_row_uniform_decode(M, D):
    """splits = 1: row b's bytes are those of the uniform kernel on a one-row cache of length L_b (with more splits an empty split's +0
    partial output can turn a -0 into +0: those cases are held to the oracle above)"""
    import torch
    from mi355q import ops
    q, k, v = _inputs(8, M, 257, D, seed=M)
    lengths = _lengths(M)
    cache = _ragged_cache(k, v, lengths, capacity=272)
    qt, kt, vt = (torch.from_numpy(t).to(DEV) for t in (q, k, v))
    out = ops.bfp_attention_decode(qt, cache, scale_div=8.0, splits=1, lengths=_i32(lengths), max_length=257)
    for b, L in enumerate(lengths):
        one = ops.KVCache(1, 272, D, _par(6), _par(6), DEV)
        one.append(kt[b:b + 1, :L], vt[b:b + 1, :L])
        want = ops.bfp_attention_decode(qt[b:b + 1], one, scale_div=8.0, splits=1)
        assert torch.equal(_bytes(out[b:b + 1]), _bytes(want)), f"row {b} (length {L}) differs from its uniform decode"


# ---- 5. stale storage -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [None, 2])
def test_stale_storage_behind_a_rows_length_never_reaches_its_result(splits):
    import torch
    from mi355q import ops
    B, M, D, lengths = 2, 3, 64, [3, 17]
    q, k, v = _inputs(B, M, 40, D, seed=9)
    kt, vt, qt = (torch.from_numpy(t).to(DEV) for t in (k, v, q))
    used = ops.KVCache(B, 48, D, _par(6), _par(6), DEV)
    used.append(kt * 3e4, vt * 3e4)                            # 40 keys of large values in every tile, pair and staged row
    outs = []
    for cache in (used, ops.KVCache(B, 48, D, _par(6), _par(6), DEV)):
        cache.append(kt[:, :17], vt[:, :17], lengths=_i32([0, 0]), counts=_i32(lengths), max_length=0)
        outs.append(ops.bfp_attention_decode(qt, cache, scale_div=8.0, splits=splits, lengths=_i32(lengths), max_length=40))
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    assert torch.equal(_bytes(outs[0]), _bytes(outs[1]))


# ---- 6. graph capture -----------------------------------------------------------------------------------------------------
def test_one_captured_step_serves_growing_lengths():
    """one ragged append + decode step (n = 1) captured ONCE; replayed after new k, v, q and ADVANCED length tensors were written in
    place -- under the same max_length bound -- it gives the bytes of the eager calls.  The scalar-L path bakes its length into the
    captured launches and cannot do this."""
    import torch
    from mi355q import ops
    B, D, C, start = 4, 64, 64, [5, 16, 31, 37]                # steps take the rows to 7, 18, 33 (over a tile edge and a pair), 39
    torch.manual_seed(13)
    k0, v0 = torch.randn(B, 37, D, device=DEV), torch.randn(B, 37, D, device=DEV)
    steps = [tuple(torch.randn(B, 1, D, device=DEV) for _ in range(3)) for _ in range(2)]

    def prefill():
        cache = ops.KVCache(B, C, D, _par(6), _par(6), DEV)
        cache.append(k0, v0, lengths=_i32([0] * B), counts=_i32(start), max_length=0)
        return cache

    def step(cache, kn, vn, q, before, after):
        cache.append(kn, vn, lengths=before, max_length=C - 1)
        return ops.bfp_attention_decode(q, cache, scale_div=8.0, splits=2, lengths=after, max_length=C)

    eager, want = prefill(), []
    for i, (kn, vn, q) in enumerate(steps):
        want.append(step(eager, kn, vn, q, _i32([s + i for s in start]), _i32([s + i + 1 for s in start])).clone())
    cache = prefill()
    kn, vn, q = (t.clone() for t in steps[0])
    before, after = _i32(start), _i32([s + 1 for s in start])
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
        before.copy_(_i32([s + i for s in start]))
        after.copy_(_i32([s + i + 1 for s in start]))
        got.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bytes(got), _bytes(want[i])), f"replay {i} differs from the eager step"
    assert torch.equal(cache.kq, eager.kq) and torch.equal(cache.vq, eager.vq) and torch.equal(cache.stage, eager.stage)
