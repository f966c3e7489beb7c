"""Shared by the sliding-window GPU tests (tests/test_gpu_window_*.py): the oracle of tests/test_gpu_decode.py with one more np.tril --
np_oracle.matmul_quantized on the full K / V with the causal + window additive mask -- its inputs, its bounds and its cache filler."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "llm-mixed-q_amd", ROOT):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

FMIN = np.finfo(np.float32).min
DEV = "cuda:0"


def cfg(width):
    return dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=width, data_in_exponent_width=8, data_in_exponent_bias=127,
                data_in_block_size=[1, 16], weight_width=width, weight_exponent_width=8, weight_exponent_bias=127,
                weight_block_size=[1, 16])


def par(width):
    return (width, 8, 127, width, 8, 127)


def oracle(q, k, v, width, window, scale_div):
    """the last tq positions of tk keys, causal, every query bound to its last `window` keys (None: all)"""
    from oracle import np_oracle as O
    w = O.matmul_quantized(q, np.swapaxes(k, -1, -2), cfg(width))
    w = (w / np.float32(scale_div)).astype(np.float32)
    tq, tk = w.shape[-2:]
    m = np.triu(np.full((tq, tk), FMIN, np.float32), 1 + tk - tq)
    if window is not None:
        m = m + np.tril(np.full((tq, tk), FMIN, np.float32), tk - tq - window)
    with np.errstate(over="ignore"):
        w = np.maximum(w + m, FMIN)
    e = np.exp((w - w.max(-1, keepdims=True)).astype(np.float64))
    p = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    return O.matmul_quantized(p, v, cfg(width))


def inputs(B, M, T, hd, seed):
    r = np.random.default_rng(seed)
    q = (r.normal(size=(B, M, hd)) * np.exp(r.normal(size=(B, M, 1)) * 0.5) * 0.7).astype(np.float32)
    k = (r.normal(size=(B, T, hd)) * np.exp(r.normal(size=(B, 1, hd)) * 0.5)).astype(np.float32)
    v = r.normal(size=(B, T, hd)).astype(np.float32)
    return q, k, v


def check(out, ref):
    scale = np.abs(ref).max()
    print("worst", np.abs(out - ref).max() / scale, "mean", np.abs(out - ref).mean() / scale)
    assert np.abs(out - ref).max() <= 1e-3 * scale, (np.abs(out - ref).max(), scale)
    assert np.abs(out - ref).mean() <= 3e-5 * scale, (np.abs(out - ref).mean(), scale)


def filled(k, v, width, capacity=None):
    """a KVCache holding k, v [B, L, D] (numpy or tensors)"""
    import torch
    from mi355q import ops
    B, L, D = k.shape
    cache = ops.KVCache(B, capacity or (L + 15) // 16 * 16, D, par(width), par(width), DEV)
    cache.append(torch.as_tensor(k).to(DEV), torch.as_tensor(v).to(DEV))
    return cache


def i32(values):
    import torch
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


def bits(t):
    import torch
    return t.contiguous().view(torch.uint8)
