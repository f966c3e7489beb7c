"""Shared by the padded-attention tests: the oracle and the bounds of tests/test_gpu_attention.py restated (its `_oracle`, `_check`,
`_cfg`, `_inputs`), the padded cases, and the per-sequence reference -- the oracle called once per sequence with
mask = broadcast(pad_row), computed once per case and cached."""
import functools

import numpy as np

FMIN = np.finfo(np.float32).min


def cfg(width, **extra):
    return dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=width, data_in_exponent_width=8,
                data_in_exponent_bias=127, data_in_block_size=[1, 16], weight_width=width, weight_exponent_width=8,
                weight_exponent_bias=127, weight_block_size=[1, 16], **extra)


def oracle(q, k, v, c0, c1, mask=None, causal=False, scale_div=None):
    """the reference's steps: bmm_0, scale, mask + clamp, softmax, bmm_1 (tests/test_gpu_attention.py:_oracle)"""
    from oracle import np_oracle as O
    w = O.matmul_quantized(q, np.swapaxes(k, -1, -2), c0)
    if scale_div:
        w = (w / np.float32(scale_div)).astype(np.float32)
    tq, tk = w.shape[-2:]
    m = np.zeros((tq, tk), np.float32)
    if causal:
        m = np.triu(np.full((tq, tk), FMIN, np.float32), 1 + tk - tq)
    if mask is not None:
        with np.errstate(over="ignore"):
            m = np.maximum(m + mask, FMIN)
    if causal or mask is not None:
        with np.errstate(over="ignore"):
            w = np.maximum(w + m, FMIN)
    e = np.exp((w - w.max(-1, keepdims=True)).astype(np.float64))
    p = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    return O.matmul_quantized(p, v, c1)


def check(out, ref):
    """the project's bounds for this path (tests/test_gpu_attention.py:_check)"""
    scale = np.abs(ref).max()
    err = np.abs(out - ref)
    print(f"max {err.max():.3e} (bound {1e-3 * scale:.3e})  mean {err.mean():.3e} (bound {3e-5 * scale:.3e})")
    assert err.max() <= 1e-3 * scale, (err.max(), scale)
    assert err.mean() <= 3e-5 * scale, (err.mean(), scale)


def key_mask(lengths, T, side):
    """[len(lengths), T] int32: `lengths[b]` real keys at the right end (side = "left": left-padded) or the left end"""
    m = np.zeros((len(lengths), T), np.int32)
    for b, n in enumerate(lengths):
        if n:
            if side == "left":
                m[b, T - n:] = 1
            else:
                m[b, :n] = 1
    return m


@functools.lru_cache(maxsize=None)
def case(T, M, hd, width, lengths, side, causal, scaled, q_scaled, heads=2):
    """(q, k, v [B, heads, ., hd], key mask [B, T], reference [B, heads, M, hd], kwargs) of one padded case; read-only arrays"""
    B = len(lengths)
    r = np.random.default_rng(1000 * T + 10 * hd + width + len(side))
    q = (r.normal(size=(B, heads, M, hd)) * np.exp(r.normal(size=(B, heads, M, 1)) * 0.5) * 0.7).astype(np.float32)
    k = (r.normal(size=(B, heads, T, hd)) * np.exp(r.normal(size=(B, heads, 1, hd)) * 0.5)).astype(np.float32)
    v = r.normal(size=(B, heads, T, hd)).astype(np.float32)
    km = key_mask(lengths, T, side)
    c = cfg(width)
    kw = {}
    if scaled:
        kw["scale_div"] = float(np.sqrt(hd))
    qs = np.float32(hd ** -0.5) if q_scaled else None
    ref = np.empty((B, heads, M, hd), np.float32)
    for b in range(B):
        add = np.broadcast_to(np.where(km[b] != 0, np.float32(0), FMIN).astype(np.float32), (M, T))
        qb = q[b] if qs is None else (q[b] * qs).astype(np.float32)
        ref[b] = oracle(qb, k[b], v[b], c, c, mask=add, causal=causal, **kw)
    for a in (q, k, v, km, ref):
        a.setflags(write=False)
    if qs is not None:
        kw["q_scale"] = float(qs)
    return q, k, v, km, ref, kw
