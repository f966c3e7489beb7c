"""Grouped-query decode attention on the GPU (ops.bfp_attention_decode(group=G)): G query heads share a cache row.  Each case is held
two ways: BIT-EQUAL to today's ungrouped call on a second cache of cache.B * G rows that was appended with repeat_interleave'd K / V,
with the same explicit `splits` on both sides (the default split count depends on the row count), and against the fp64 oracle's
restatement of the reference's steps on the repeated K / V with the bounds of tests/test_gpu_decode.py (1e-3 max, 3e-5 mean, times the
scale).  K / V are random and distinct per cache row, q is random and distinct per head: a column-to-head mix-up shows."""
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
PAR = (6, 8, 127, 6, 8, 127)
CFG = dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
           data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127, weight_block_size=[1, 16])


def _oracle(q, k, v, causal=False, scale_div=None):
    """tests/test_gpu_decode.py's restatement"""
    from oracle import np_oracle as O
    w = O.matmul_quantized(q, np.swapaxes(k, -1, -2), CFG)
    if scale_div:
        w = (w / np.float32(scale_div)).astype(np.float32)
    tq, tk = w.shape[-2:]
    if causal:
        m = np.triu(np.full((tq, tk), FMIN, np.float32), 1 + tk - tq)
        with np.errstate(over="ignore"):
            w = np.maximum(w + m, FMIN)
    e = np.exp((w - w.max(-1, keepdims=True)).astype(np.float64))
    p = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    return O.matmul_quantized(p, v, CFG)


def _check(out, ref):
    scale = np.abs(ref).max()
    print("worst", np.abs(out - ref).max() / scale, "mean", np.abs(out - ref).mean() / scale)
    assert np.abs(out - ref).max() <= 1e-3 * scale, (np.abs(out - ref).max(), scale)
    assert np.abs(out - ref).mean() <= 3e-5 * scale, (np.abs(out - ref).mean(), scale)


def _bytes(t):
    import torch
    return t.contiguous().view(torch.uint8)


@functools.lru_cache(maxsize=None)
def _case(R, G, M, L, D, causal=True, q_scale=None):
    """-> (q [R * G, M, D], grouped cache of R rows, repeated cache of R * G rows, oracle output) -- made once a case, never written"""
    import torch
    from mi355q import ops
    r = np.random.default_rng(1000 * R + 100 * G + 10 * M + L + D)
    q = (r.normal(size=(R * G, M, D)) * np.exp(r.normal(size=(R * G, M, 1)) * 0.5) * 0.7).astype(np.float32)
    k = (r.normal(size=(R, L, D)) * np.exp(r.normal(size=(R, 1, D)) * 0.5)).astype(np.float32)
    v = r.normal(size=(R, L, D)).astype(np.float32)
    kt, vt = torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV)
    cap = (L + 15) // 16 * 16
    cache, rep = ops.KVCache(R, cap, D, PAR, PAR, DEV), ops.KVCache(R * G, cap, D, PAR, PAR, DEV)
    cache.append(kt, vt)
    rep.append(kt.repeat_interleave(G, 0), vt.repeat_interleave(G, 0))
    if q_scale:
        ref = _oracle((q * np.float32(q_scale)).astype(np.float32), np.repeat(k, G, 0), np.repeat(v, G, 0), causal)
    else:
        ref = _oracle(q, np.repeat(k, G, 0), np.repeat(v, G, 0), causal, math.sqrt(D))
    return torch.from_numpy(q).to(DEV), cache, rep, ref


# (cache rows, G, M, L, D, splits; None: the grouped call's own default, passed to both sides)
CASES = [(2, 4, 1, 40, 64, None),                            # open block, 4 columns
         (2, 8, 2, 70, 128, 1), (2, 8, 2, 70, 128, 2),        # all 16 columns
         (3, 2, 3, 33, 32, None),                             # c16 / M with M not a power of two, causal horizons per query
         (1, 4, 16, 48, 64, None),                            # gw = 1, rpc = 4
         (2, 8, 4, 65, 32, 1), (2, 8, 4, 65, 32, 5),          # gw = 4, rpc = 2
         (2, 6, 4, 50, 96, None)]                             # gw = 3


@pytest.mark.parametrize("R,G,M,L,D,splits", CASES)
def test_grouped_decode_is_the_ungrouped_call_on_repeated_rows(R, G, M, L, D, splits):
    import torch
    from mi355q import ops
    q, cache, rep, ref = _case(R, G, M, L, D)
    gw = ops.decode_group_width(G, M)
    if splits is None:
        splits = ops.decode_splits(R * G // gw, L, D)
    kw = dict(causal=True, scale_div=math.sqrt(D), splits=splits)
    got = ops.bfp_attention_decode(q, cache, group=G, **kw)
    want = ops.bfp_attention_decode(q, rep, **kw)
    torch.cuda.synchronize()
    assert got.shape == want.shape == (R * G, M, D)
    bad = (_bytes(got) != _bytes(want)).reshape(R * G, -1).any(1).nonzero().flatten().tolist()
    assert not bad, f"query rows {bad} differ from the ungrouped call on a private copy of their cache row (gw = {gw}, splits = {splits})"
    _check(got.cpu().numpy(), ref)


def test_non_causal_with_q_scale():
    import torch
    from mi355q import ops
    R, G, M, L, D = 2, 4, 3, 45, 64
    q, cache, rep, ref = _case(R, G, M, L, D, causal=False, q_scale=0.125)
    got = ops.bfp_attention_decode(q, cache, group=G, causal=False, q_scale=0.125, splits=2)
    want = ops.bfp_attention_decode(q, rep, causal=False, q_scale=0.125, splits=2)
    assert torch.equal(_bytes(got), _bytes(want))
    _check(got.cpu().numpy(), ref)


def test_ragged_rows_keep_one_length_per_cache_row():
    """4 cache rows, G = 4, M = 1, lengths [5, 40, 0, 17] under max_length 40: the empty row's four heads return zeros, every other
    head equals the ungrouped ragged call on the repeated cache (same splits) and -- with one split, where the partition cannot
    differ -- its cache row alone in a uniform cache"""
    import torch
    from mi355q import ops
    R, G, D, lengths = 4, 4, 64, [5, 40, 0, 17]
    torch.manual_seed(40)
    q, k, v = torch.randn(R * G, 1, D, device=DEV), torch.randn(R, 40, D, device=DEV), torch.randn(R, 40, D, device=DEV)
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=DEV)
    cache, rep = ops.KVCache(R, 48, D, PAR, PAR, DEV), ops.KVCache(R * G, 48, D, PAR, PAR, DEV)
    cache.append(k, v, lengths=i32([0] * R), counts=i32(lengths), max_length=0)
    rl = [l for l in lengths for _ in range(G)]
    rep.append(k.repeat_interleave(G, 0), v.repeat_interleave(G, 0), lengths=i32([0] * R * G), counts=i32(rl), max_length=0)
    for splits in (1, 2):
        got = ops.bfp_attention_decode(q, cache, group=G, scale_div=8.0, splits=splits, lengths=i32(lengths), max_length=40)
        want = ops.bfp_attention_decode(q, rep, scale_div=8.0, splits=splits, lengths=i32(rl), max_length=40)
        assert torch.equal(_bytes(got), _bytes(want)), splits
        assert not got[2 * G:3 * G].any() and bool(torch.isfinite(got).all())
        for r, L in enumerate(lengths):
            if L:
                assert float(got[r * G:(r + 1) * G].abs().max()) > 0
    one = ops.bfp_attention_decode(q, cache, group=G, scale_div=8.0, splits=1, lengths=i32(lengths), max_length=40)
    for r, L in enumerate(lengths):
        if L:
            alone = ops.KVCache(1, 48, D, PAR, PAR, DEV)
            alone.append(k[r:r + 1, :L], v[r:r + 1, :L])
            want = ops.bfp_attention_decode(q[r * G:(r + 1) * G], alone, group=G, scale_div=8.0, splits=1)
            assert torch.equal(_bytes(one[r * G:(r + 1) * G]), _bytes(want)), f"cache row {r} differs from the row alone"


def test_token_major_and_strided_head_views():
    """batch 1: q as the [1, Hq, M, D] view of a [1, M, Hq, D] projection output is read in place, and token_major writes
    [1, M, Hq, D] -- the same values as the contiguous call"""
    import torch
    from mi355q import ops
    Hkv, G, M, L, D = 2, 4, 2, 40, 64
    q, cache, _, _ = _case(Hkv, G, M, L, D)
    kw = dict(causal=True, scale_div=8.0, splits=2, group=G)
    want = ops.bfp_attention_decode(q, cache, **kw)
    buf = q.reshape(1, Hkv * G, M, D).transpose(1, 2).contiguous()               # [1, M, Hq, D]
    view = buf.transpose(1, 2)
    assert not view.is_contiguous()
    got = ops.bfp_attention_decode(view, cache, **kw)
    assert got.shape == (1, Hkv * G, M, D) and torch.equal(_bytes(got.reshape(Hkv * G, M, D)), _bytes(want))
    tm = ops.bfp_attention_decode(view, cache, token_major=True, **kw)
    assert tm.shape == (1, Hkv * G, M, D) and tm.transpose(1, 2).is_contiguous()
    assert torch.equal(_bytes(tm.reshape(Hkv * G, M, D)), _bytes(want))


def test_two_runs_give_equal_bits():
    import torch
    from mi355q import ops
    q, cache, _, _ = _case(2, 8, 4, 65, 32)
    a = ops.bfp_attention_decode(q, cache, group=8, scale_div=8.0, splits=5).clone()
    b = ops.bfp_attention_decode(q, cache, group=8, scale_div=8.0, splits=5)
    assert torch.equal(_bytes(a), _bytes(b))


def test_one_captured_step_replayed_at_two_lengths():
    """one ragged append + grouped decode step (n = 1) captured once, replayed at two lengths (the second over a tile edge for row 1):
    the bytes of the eager calls, in the manner of tests/test_gpu_decode_ragged.py"""
    import torch
    from mi355q import ops
    R, G, D, C, start = 2, 4, 64, 48, [5, 31]
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=DEV)
    torch.manual_seed(31)
    k0, v0 = torch.randn(R, 31, D, device=DEV), torch.randn(R, 31, D, device=DEV)
    steps = [(torch.randn(R, 1, D, device=DEV), torch.randn(R, 1, D, device=DEV), torch.randn(R * G, 1, D, device=DEV)) for _ in range(2)]

    def prefill():
        cache = ops.KVCache(R, C, D, PAR, PAR, DEV)
        cache.append(k0, v0, lengths=i32([0] * R), counts=i32(start), max_length=0)
        return cache

    def step(cache, kn, vn, q, before, after):
        cache.append(kn, vn, lengths=before, max_length=C - 1)
        return ops.bfp_attention_decode(q, cache, group=G, scale_div=8.0, splits=2, lengths=after, max_length=C)

    eager, want = prefill(), []
    for i, (kn, vn, q) in enumerate(steps):
        want.append(step(eager, kn, vn, q, i32([s + i for s in start]), i32([s + i + 1 for s in start])).clone())
    cache = prefill()
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
        before.copy_(i32([s + i for s in start]))
        after.copy_(i32([s + i + 1 for s in start]))
        got.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bytes(got), _bytes(want[i])), f"replay {i} differs from the eager step"
    assert torch.equal(cache.kq, eager.kq) and torch.equal(cache.vq, eager.vq)
