"""Decode attention on the block_minifloat KV cache (ops.MinifloatKVCache + ops.bfp_attention_decode) against the oracle's restatement
of the reference's steps on the concatenated K / V -- the fp64-softmax recipe of tests/test_gpu_decode.py::_oracle, written again here
with block_minifloat configs.

Inputs.  With bias 0 every probability below 1 is a subnormal step of 2^(1 - mantissa bits): ordinary inputs (that file's _inputs) give
an oracle output that is exactly 0 in every row, on which any kernel passes.  The queries here are that file's with the factor 0.7
replaced by 3.0 (peaked rows), seed L + D + M.  Asserted on the oracle's own values, before any GPU comparison: at least 75 % of the
rows that see a key are non-zero in the oracle's output, and a row may be left out only if the oracle ITSELF moves by more than
1e-6 max|ref| when its probabilities are scaled by 1 +- 2^-20 (a probability on a quantiser boundary) -- at most 2 % of all rows.
Tolerance on the rows kept: the block_fp tests' worst <= 1e-3 max|ref|, mean <= 3e-5 max|ref|."""
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
PATTERNS = (0x00000000, 0xFFFFFFFF, 0x7FC00000, 0x3F800000, 0x00000001, 0x80000000)


def _cfg(fmt):
    w, ew = fmt
    return dict(name="block_minifloat", is_ptq=True, bypass=False, data_in_width=w, data_in_exponent_width=ew, data_in_exponent_bias_width=8,
                data_in_block_size=[1, 16], weight_width=w, weight_exponent_width=ew, weight_exponent_bias_width=8, weight_block_size=[1, 16])


def _par(fmt):
    return (fmt[0], fmt[1], 8, fmt[0], fmt[1], 8)


def _oracle(q, k, v, c0, c1, causal=False, scale_div=None, p_scale=None):
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
    if p_scale is not None:
        p = (p * np.float32(p_scale)).astype(np.float32)
    return O.matmul_quantized(p, v, c1)


def _inputs(B, M, T, hd, seed):
    r = np.random.default_rng(seed)
    q = (r.normal(size=(B, M, hd)) * np.exp(r.normal(size=(B, M, 1)) * 0.5) * 3.0).astype(np.float32)
    k = (r.normal(size=(B, T, hd)) * np.exp(r.normal(size=(B, 1, hd)) * 0.5)).astype(np.float32)
    v = r.normal(size=(B, T, hd)).astype(np.float32)
    return q, k, v


def _reference(q, k, v, fmt, causal, scale_div, count=True):
    """-> (ref, keep): the oracle's output and the rows it does not itself move under a 2^-20 scaling of its probabilities; the two
    conditions of the header are asserted here"""
    c0, c1 = _cfg(fmt), _cfg(fmt)
    ref = _oracle(q, k, v, c0, c1, causal=causal, scale_div=scale_div)
    scale = np.abs(ref).max()
    keep = np.ones(ref.shape[:-1], bool)
    for s in (1.0 + 2.0 ** -20, 1.0 - 2.0 ** -20):
        moved = _oracle(q, k, v, c0, c1, causal=causal, scale_div=scale_div, p_scale=s)
        keep &= np.abs(moved - ref).max(-1) <= 1e-6 * scale
    nonzero = np.abs(ref).max(-1) > 0
    print("rows", keep.size, "left out", int((~keep).sum()), "non-zero", int(nonzero.sum()))
    if count:
        assert nonzero.mean() >= 0.75, f"only {nonzero.mean():.0%} of the oracle's rows are non-zero: the inputs are not peaked enough"
        assert (~keep).mean() <= 0.02, f"{int((~keep).sum())} of {keep.size} rows sit on a quantiser boundary of the oracle"
    return ref, keep


def _check(out, ref, keep):
    scale = np.abs(ref).max()
    d = np.abs(out - ref)[keep]
    print("worst", d.max() / scale, "mean", d.mean() / scale)
    assert d.max() <= 1e-3 * scale, (d.max(), scale)
    assert d.mean() <= 3e-5 * scale, (d.mean(), scale)


def _filled(k, v, fmt, capacity=None, pieces=None):
    import torch
    from mi355q import ops
    B, L, D = k.shape
    cache = ops.MinifloatKVCache(B, capacity or (L + 15) // 16 * 16, D, _par(fmt), _par(fmt), DEV)
    kt, vt = torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV)
    at = 0
    for n in pieces or (L,):
        cache.append(kt[:, at:at + n], vt[:, at:at + n])
        at += n
    assert cache.length == L
    return cache


def _quantised_v(v, fmt):
    from oracle import compare, np_oracle as O
    return compare.bf16_rne(O.block_minifloat_quantize(v, fmt[0], fmt[1], 8, block_size=[1, 16], skip_first_dim=True))


CASES = [(2, 1, 1, 64, (8, 4)), (2, 1, 15, 64, (8, 4)), (3, 1, 17, 128, (8, 4)), (2, 3, 33, 64, (6, 3)),
         (2, 16, 16, 128, (8, 4)), (2, 16, 250, 128, (8, 3)), (5, 7, 80, 96, (6, 3)), (2, 1, 1040, 32, (8, 4))]


@pytest.mark.parametrize("B,M,L,D,fmt", CASES)
def test_decode_vs_oracle(B, M, L, D, fmt):
    """causal with scale_div = sqrt(D) under 1 / 2 / default splits, bit-identical on a second call, and non-causal with q_scale.  A
    query that sees ONE key has probability 1, which block_minifloat keeps (1.0 stays 1.0): its output row is that key's quantised V
    row exactly -- every row for L = 1, row 0 for L = M."""
    import torch
    from mi355q import ops
    q, k, v = _inputs(B, M, L, D, seed=L + D + M)
    cache = _filled(k, v, fmt, capacity=(L + 31) // 16 * 16, pieces=(L - M, M) if L > M else (L,))
    qt = torch.from_numpy(q).to(DEV)
    ref, keep = _reference(q, k, v, fmt, True, math.sqrt(D))
    for splits in (1, 2, None):
        a = ops.bfp_attention_decode(qt, cache, causal=True, scale_div=math.sqrt(D), splits=splits)
        b = ops.bfp_attention_decode(qt, cache, causal=True, scale_div=math.sqrt(D), splits=splits)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"two runs with splits={splits} differ"
        out = a.cpu().numpy()
        _check(out, ref, keep)
        if L == M or L == 1:
            vq = _quantised_v(v, fmt)
            # (as values: a -0.0 of the row comes out of the product's accumulator as +0.0)
            assert np.array_equal(out[:, 0], vq[:, 0]), "a query that sees one key must return that key's quantised V row"
    scaling = np.float32(D ** -0.5)
    # (non-causal: the rows of one batch entry see the same keys; the conditions are the causal call's, counted there)
    ref, keep = _reference(q * scaling, k, v, fmt, False, None, count=False)
    out = ops.bfp_attention_decode(qt, cache, causal=False, q_scale=float(scaling)).cpu().numpy()
    _check(out, ref, keep)


def test_ragged_rows():
    """rows of (117, 41, 0) keys in one call: each as if it were alone, the empty row zeros"""
    import torch
    from mi355q import ops
    B, M, D, fmt, lens = 3, 1, 64, (8, 4), (117, 41, 0)
    q, k, v = _inputs(B, M, 117, D, seed=117 + D + M)
    cache = ops.MinifloatKVCache(B, 128, D, _par(fmt), _par(fmt), DEV)
    kt, vt, qt = (torch.from_numpy(t).to(DEV) for t in (k, v, q))
    dev = lambda xs: torch.tensor(xs, dtype=torch.int32, device=DEV)
    cache.append(kt, vt, lengths=dev([0] * B), counts=dev(lens), max_length=0)
    for splits in (1, 3, None):
        out = ops.bfp_attention_decode(qt, cache, scale_div=8.0, lengths=dev(lens), max_length=117, splits=splits).cpu().numpy()
        for b, L in enumerate(lens):
            if L == 0:
                assert not out[b].any()
                continue
            ref, keep = _reference(q[b:b + 1], k[b:b + 1, :L], v[b:b + 1, :L], fmt, True, 8.0, count=False)
            assert keep.all()
            _check(out[b:b + 1], ref, keep)


@pytest.mark.parametrize("G,M", [(2, 3), (4, 1), (4, 5)])
def test_grouped_queries(G, M):
    """G query heads a cache row: each head's bits are those of group=1 on a cache holding the repeated K / V, with the same splits"""
    import torch
    from mi355q import ops
    Bkv, L, D, fmt = 2, 70, 64, (8, 4)
    q, k, v = _inputs(Bkv * G, M, L, D, seed=L + D + M + G)
    k, v = k[::G].copy(), v[::G].copy()
    shared = _filled(k, v, fmt, capacity=80, pieces=(L - M, M))
    private = _filled(np.repeat(k, G, 0), np.repeat(v, G, 0), fmt, capacity=80, pieces=(L - M, M))
    qt = torch.from_numpy(q).to(DEV)
    for splits in (1, 2):
        a = ops.bfp_attention_decode(qt, shared, scale_div=8.0, group=G, splits=splits)
        b = ops.bfp_attention_decode(qt, private, scale_div=8.0, splits=splits)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    ref, keep = _reference(q, np.repeat(k, G, 0), np.repeat(v, G, 0), fmt, True, 8.0, count=False)
    _check(ops.bfp_attention_decode(qt, shared, scale_div=8.0, group=G).cpu().numpy(), ref, keep)


def test_token_major_and_strided_head_views():
    """[1, n, H, D] projections viewed as [1, H, n, D], read in place; token-major output: the bytes of the contiguous call"""
    import torch
    from mi355q import ops
    H, D, L, M, fmt = 4, 64, 45, 5, (8, 4)
    torch.manual_seed(3)
    kp, vp = torch.randn(1, L, H, D, device=DEV), torch.randn(1, L, H, D, device=DEV)
    qp = torch.randn(1, M, H, D, device=DEV) * 3.0
    heads = lambda t: t.transpose(1, 2)
    flat = lambda t: heads(t).contiguous().view(H, t.shape[1], D)
    a = ops.MinifloatKVCache(H, 48, D, _par(fmt), _par(fmt), DEV)
    a.append(heads(kp)[:, :, :40], heads(vp)[:, :, :40])
    a.append(heads(kp)[:, :, 40:], heads(vp)[:, :, 40:])
    b = ops.MinifloatKVCache(H, 48, D, _par(fmt), _par(fmt), DEV)
    b.append(flat(kp)[:, :40], flat(vp)[:, :40])
    b.append(flat(kp)[:, 40:], flat(vp)[:, 40:])
    assert torch.equal(a.kq, b.kq) and torch.equal(a.vq, b.vq) and torch.equal(a.stage, b.stage)
    o_ref = ops.bfp_attention_decode(flat(qp), b, scale_div=8.0)
    assert float(o_ref.abs().max()) > 0
    o_tm = ops.bfp_attention_decode(heads(qp), a, scale_div=8.0, token_major=True)
    assert o_tm.shape == (1, H, M, D) and o_tm.transpose(1, 2).is_contiguous()
    assert torch.equal(o_tm[0].contiguous().view(torch.uint8), o_ref.view(torch.uint8))
    o_pl = ops.bfp_attention_decode(heads(qp), a, scale_div=8.0)
    assert o_pl.is_contiguous() and torch.equal(o_pl[0].view(torch.uint8), o_ref.view(torch.uint8))


@pytest.fixture(scope="module")
def poison():
    import ctypes
    import torch
    so = ROOT / "tools" / "lds_poison" / "liblds_poison.so"
    if not so.exists():
        pytest.fail("tools/lds_poison/liblds_poison.so is not built (__graft_entry__.build())")
    lib = ctypes.CDLL(str(so))

    def fill(pattern):
        rc = lib.lds_poison(ctypes.c_uint(pattern), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
    return fill


@pytest.mark.parametrize("B,M,L,D,splits", [
    (2, 16, 250, 128, 5),        # DC = 4: partial outputs through the workspace, the widest LDS reduction
    (3, 5, 100, 96, 1),          # DC = 3: one split
    (2, 1, 17, 64, 2),           # DC = 2: one key pair, a single split after evening out
    (2, 4, 40, 32, 2),           # DC = 1
])
def test_stale_lds(poison, B, M, L, D, splits):
    """in the manner of tests/test_gpu_decode_stale_lds.py, over each DC: every compute unit's LDS is filled with a pattern in front of each
    append + decode and the output must be the same bits under every pattern"""
    import torch
    from mi355q import ops
    torch.manual_seed(L + D)
    par = _par((8, 4))
    q, k, v = torch.randn(B, M, D, device=DEV) * 3.0, torch.randn(B, L, D, device=DEV), torch.randn(B, L, D, device=DEV)
    outs = []
    for p in PATTERNS:
        cache = ops.MinifloatKVCache(B, 256, D, par, par, DEV)
        poison(p)
        cache.append(k[:, :L - M], v[:, :L - M])
        poison(p)
        cache.append(k[:, L - M:], v[:, L - M:])
        poison(p)
        outs.append(ops.bfp_attention_decode(q, cache, causal=True, scale_div=math.sqrt(D), splits=splits).clone())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    for p, o in zip(PATTERNS[1:], outs[1:]):
        assert torch.equal(o.view(torch.uint8), outs[0].view(torch.uint8)), f"output depends on stale LDS (pattern {p:#010x})"
