"""Incremental decoding on the GPU: the block_fp KV cache (ops.KVCache) against the oracle's quantisers bit for bit, and the
split-key decode attention (ops.bfp_attention_decode) against the oracle's restatement of the reference's steps on the
concatenated K / V -- the recipe and the bounds of tests/test_gpu_attention.py, restated here."""
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


def _quantised_kv(k, v, width):
    from oracle import compare, np_oracle as O
    kq = compare.bf16_rne(O.block_fp_quantize(np.ascontiguousarray(np.swapaxes(k, 1, 2)), width, 8, 127, block_size=[1, 16]))
    vq = compare.bf16_rne(O.block_fp_quantize(v, width, 8, 127, block_size=[1, 16]))
    return np.ascontiguousarray(np.swapaxes(kq, 1, 2)), vq


@pytest.mark.parametrize("D", [32, 64, 96, 128])
@pytest.mark.parametrize("width", [4, 6, 9])
def test_cache_is_the_oracles_quantiser_bit_for_bit(D, width):
    """(D = 32, 96: the append's 8 and 2 tiles per workgroup, the latter with idle threads.)  keys appended in pieces: after every piece the cache holds what block_fp_quantize makes of k^T[:, :, :L] (16-key blocks, the open
    one re-quantised) and of v[:, :L]; one append of everything gives the same bytes"""
    import torch
    from mi355q import ops
    B, pieces = 3, (1, 1, 13, 1, 1, 16, 7)
    _, k, v = _inputs(B, 1, 40, D, seed=D + width)
    k[0, 3, 5] = k[1, 20, :7] = v[2, 9, 3] = 0.0
    k[:, 18] = 0.0                                         # an all-zero key
    k[1, 33:, 9] = 0.0                                     # an all-zero open block at one d
    k[2, 2, 11] = 3e-9                                     # passes through (|x| <= 1e-8), rounded to bf16
    cache = ops.KVCache(B, 48, D, _par(width), _par(width), DEV)
    kt, vt = torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV)
    at = 0
    for n in pieces:
        cache.append(kt[:, at:at + n], vt[:, at:at + n])
        at += n
        assert cache.length == at
        kd, vd = (t.cpu().numpy() for t in cache.dequantised())
        kq, vq = _quantised_kv(k[:, :at], v[:, :at], width)
        assert np.array_equal(kd.view(np.uint32), kq.view(np.uint32)), f"K differs at length {at}"
        assert np.array_equal(vd.view(np.uint32), vq.view(np.uint32)), f"V differs at length {at}"
    assert at == 40
    once = ops.KVCache(B, 48, D, _par(width), _par(width), DEV)
    once.append(kt, vt)
    for a, b in ((cache.kq, once.kq), (cache.vq, once.vq)):
        assert torch.equal(a, b)
    # reset: the same keys again give the same bytes
    kq0 = cache.kq.clone()
    cache.reset()
    assert cache.length == 0
    cache.append(kt[:, :17], vt[:, :17])
    cache.append(kt[:, 17:], vt[:, 17:])
    assert torch.equal(cache.kq, kq0)


CASES = [(2, 1, 1, 64, 6, 6, None), (2, 1, 15, 64, 6, 6, 1), (3, 1, 17, 128, 6, 6, 2), (2, 3, 33, 64, 4, 6, 3),
         (2, 16, 16, 128, 6, 6, 1), (2, 16, 250, 128, 9, 9, 5), (5, 7, 80, 96, 5, 5, 3), (2, 1, 1040, 32, 6, 6, None)]


@pytest.mark.parametrize("B,M,L,D,wqk,wpv,splits", CASES)
def test_decode_vs_oracle(B, M, L, D, wqk, wpv, splits):
    """causal with scale_div = sqrt(D), and non-causal with q_scale.  Where a query sees ONE key its probability is 1, which the
    probabilities' quantiser turns into (2^(w-1) - 1) / 2^(w-1) (block_fp keeps no mantissa for 2^e itself): the output row is then
    exactly that times the key's quantised V row."""
    import torch
    from mi355q import ops
    from oracle import np_oracle as O
    q, k, v = _inputs(B, M, L, D, seed=L + D + M)
    cache = _filled(k, v, wqk, wpv, capacity=(L + 31) // 16 * 16, pieces=(L - M, M) if L > M else (L,))
    qt = torch.from_numpy(q).to(DEV)
    c0, c1 = _cfg(wqk), _cfg(wpv)
    out = ops.bfp_attention_decode(qt, cache, causal=True, scale_div=math.sqrt(D), splits=splits).cpu().numpy()
    _check(out, _oracle(q, k, v, c0, c1, causal=True, scale_div=math.sqrt(D)))
    if L == M or L == 1:
        one = np.zeros((1, 16), np.float32)
        one[0, 0] = 1.0
        p1 = O.block_fp_quantize(one, wpv, 8, 127, block_size=[1, 16])[0, 0]
        assert p1 == np.float32(1.0 - 2.0 ** (1 - wpv))
        _, vq = _quantised_kv(k, v, wpv)
        assert np.array_equal(out[:, 0], p1 * vq[:, 0]), "a query that sees one key must return that key's quantised V row times Q(1)"
    scaling = np.float32(D ** -0.5)
    out = ops.bfp_attention_decode(qt, cache, causal=False, q_scale=float(scaling), splits=splits).cpu().numpy()
    _check(out, _oracle(q * scaling, k, v, c0, c1, causal=False))


def test_split_independence_and_reproducibility():
    import torch
    from mi355q import ops
    B, M, L, D = 3, 9, 331, 64
    q, k, v = _inputs(B, M, L, D, seed=7)
    cache = _filled(k, v, 6, 6)
    qt = torch.from_numpy(q).to(DEV)
    ref = _oracle(q, k, v, _cfg(6), _cfg(6), causal=True, scale_div=8.0)
    for s in (1, 2, 5):
        a = ops.bfp_attention_decode(qt, cache, scale_div=8.0, splits=s)
        b = ops.bfp_attention_decode(qt, cache, scale_div=8.0, splits=s)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"two runs with {s} splits differ"
        _check(a.cpu().numpy(), ref)
    a, b = ops.bfp_attention_decode(qt, cache, scale_div=8.0), ops.bfp_attention_decode(qt, cache, scale_div=8.0)
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("L", [64, 256])
def test_agrees_with_the_prefill_kernel(L):
    import torch
    from mi355q import ops
    B, M, D = 2, 16, 64
    q, k, v = _inputs(B, M, L, D, seed=L)
    ref = _oracle(q, k, v, _cfg(6), _cfg(6), causal=True, scale_div=8.0)
    cache = _filled(k, v, 6, 6)
    qt, kt, vt = (torch.from_numpy(t).to(DEV) for t in (q, k, v))
    dec = ops.bfp_attention_decode(qt, cache, causal=True, scale_div=8.0).cpu().numpy()
    pre = ops.bfp_attention(qt, kt, vt, _par(6), _par(6), causal=True, scale_div=8.0).cpu().numpy()
    _check(dec, ref)
    _check(pre, ref)
    assert np.abs(dec - pre).max() <= 1e-3 * np.abs(ref).max()


def test_token_major_and_strided_head_views():
    """[1, n, H, D] projections viewed as [1, H, n, D], read in place; token-major output: the bytes of the contiguous call"""
    import torch
    from mi355q import ops
    H, D, L, M = 4, 64, 45, 5
    torch.manual_seed(3)
    kp, vp = torch.randn(1, L, H, D, device=DEV), torch.randn(1, L, H, D, device=DEV)
    qp = torch.randn(1, M, H, D, device=DEV)
    heads = lambda t: t.transpose(1, 2)
    flat = lambda t: heads(t).contiguous().view(H, t.shape[1], D)
    a = ops.KVCache(H, 48, D, _par(6), _par(6), DEV)
    a.append(heads(kp)[:, :, :40], heads(vp)[:, :, :40])
    a.append(heads(kp)[:, :, 40:], heads(vp)[:, :, 40:])
    b = ops.KVCache(H, 48, D, _par(6), _par(6), DEV)
    b.append(flat(kp)[:, :40], flat(vp)[:, :40])
    b.append(flat(kp)[:, 40:], flat(vp)[:, 40:])
    assert torch.equal(a.kq, b.kq) and torch.equal(a.vq, b.vq) and torch.equal(a.stage, b.stage)
    o_ref = ops.bfp_attention_decode(flat(qp), b, scale_div=8.0)                                  # [H, M, D]
    o_tm = ops.bfp_attention_decode(heads(qp), a, scale_div=8.0, token_major=True)                # [1, H, M, D] view of [1, M, H, D]
    assert o_tm.shape == (1, H, M, D) and o_tm.transpose(1, 2).is_contiguous()
    assert torch.equal(o_tm[0].contiguous().view(torch.uint8), o_ref.view(torch.uint8))
    o_pl = ops.bfp_attention_decode(heads(qp), a, scale_div=8.0)
    assert o_pl.is_contiguous() and torch.equal(o_pl[0].view(torch.uint8), o_ref.view(torch.uint8))


def test_graph_capture_of_one_step():
    """one append + decode step captured at a FIXED length; its replay gives the bytes of the eager step.  (The length is a host
    value baked into the captured launches: replaying one graph at growing lengths is out of scope.)"""
    import torch
    from mi355q import ops
    B, D, L0 = 4, 64, 37
    torch.manual_seed(11)
    k, v = torch.randn(B, L0 + 1, D, device=DEV), torch.randn(B, L0 + 1, D, device=DEV)
    q = torch.randn(B, 1, D, device=DEV)
    eager = ops.KVCache(B, 64, D, _par(6), _par(6), DEV)
    eager.append(k[:, :L0], v[:, :L0])
    eager.append(k[:, L0:], v[:, L0:])
    want = ops.bfp_attention_decode(q, eager, scale_div=8.0, splits=2).clone()
    cache = ops.KVCache(B, 64, D, _par(6), _par(6), DEV)
    cache.append(k[:, :L0], v[:, :L0])
    kn, vn = k[:, L0:].clone(), v[:, L0:].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # (warm-up on the capture stream: workspaces exist before the capture)
        cache.append(kn, vn)
        ops.bfp_attention_decode(q, cache, scale_div=8.0, splits=2)
        cache.length = L0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cache.append(kn, vn)
        got = ops.bfp_attention_decode(q, cache, scale_div=8.0, splits=2)
    got.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    assert torch.equal(cache.kq, eager.kq) and torch.equal(cache.vq, eager.vq)
