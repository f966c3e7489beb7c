"""The block_minifloat KV cache on the GPU (ops.MinifloatKVCache): its contents as BITS against the oracle's block_minifloat quantiser
rounded to bf16 -- of k^T[:, :, :L] (blocks of 16 keys at one d, the open one re-quantised on every append) and of v[:, :L] (blocks of
16 d of one key) -- after every piece of a piecewise fill, with the values planted that each branch of the in-kernel quantiser
decides: zero blocks, pass-through, the floor band below a power of two (block maxima and elements), bias 0, a clamped bias,
saturated and subnormal elements."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PIECES = (1, 1, 13, 1, 1, 16, 7)


def _below(x, ulps):
    return (np.array([x], np.float32).view(np.uint32) - np.uint32(ulps)).view(np.float32)[0]


def _inputs(B, L, D, fmt, seed):
    width, ew, bw = fmt
    r = np.random.default_rng(seed)
    k = (r.normal(size=(B, L, D)) * np.exp(r.normal(size=(B, 1, D)) * 0.5)).astype(np.float32)
    v = r.normal(size=(B, L, D)).astype(np.float32)
    k[0, 3, 5] = k[1, 20, :7] = v[2, 9, 3] = 0.0
    k[:, 18] = 0.0                                         # an all-zero key
    k[1, 33:, 9] = 0.0                                     # an all-zero open block at one d
    v[0, 5, 16:32] = 0.0                                   # an all-zero V block
    k[2, 2, 11] = v[1, 2, 7] = 3e-9                        # passes through (|x| <= 1e-8), rounded to bf16
    # the floor band: block maxima a few ulps below a power of two, where torch's fp32 log2 rounds up onto the integer
    k[0, :16, 1] *= 0.2
    k[0, 7, 1] = np.nextafter(np.float32(4), np.float32(0))
    k[0, 16:32, 2] *= 0.2
    k[0, 20, 2] = _below(8.0, 40)
    v[0, 1, :16] *= 0.2
    v[0, 1, 3] = -np.nextafter(np.float32(4), np.float32(0))
    v[0, 2, :16] *= 0.2
    v[0, 2, 9] = _below(8.0, 40)
    # elements a few ulps below a power of two, inside blocks with a larger maximum
    for i, (x, u) in enumerate(((1.0, 1), (2.0, 3), (0.5, 2), (4.0, 20), (0.25, 5), (2.0, 60))):
        k[1, 2 + i, 4] = _below(x, u) * (-1 if i % 2 else 1)
        v[1, 4, 16 + i] = _below(x, u) * (1 if i % 2 else -1)
    # a block with maximum < 1: bias 0
    k[2, 16:32, 6] = (r.uniform(-0.9, 0.9, size=16)).astype(np.float32)
    v[2, 7, :16] = (r.uniform(-0.9, 0.9, size=16)).astype(np.float32)
    # a block whose maximum exceeds 2^(2^bias_width) under bias_width 2: the bias clamps at 3; under every format here its top values lie
    # above the block's top exponent 2^exponent_width - 1 - bias and saturate
    big = np.float32(2.0 ** 16 * 1.7)
    k[2, 0:16, 8] = (r.normal(size=16) * 0.3).astype(np.float32)
    k[2, 5, 8] = big
    k[2, 6, 8] = -big * np.float32(0.93)
    v[2, 11, 16:32] = (r.normal(size=16) * 0.3).astype(np.float32)
    v[2, 11, 17] = -big
    # elements above the top exponent of their block (saturated) and at e_min / below it (the subnormal branch)
    span = 2 ** ew - 1
    k[1, 16:32, 12] = np.float32(1.5)                     # bias 0: e_max = span
    k[1, 17, 12] = np.float32(1.9)
    k[1, 18, 12] = np.float32(2.0 ** -3)                  # far below the block's e_min = 0: subnormal, rounds to a small multiple
    k[1, 19, 12] = np.float32(0.6)
    k[1, 20, 12] = np.float32(1.0)                        # exactly e_min's power of two
    v[1, 6, :16] = np.float32(2.0 ** (span + 2)) * r.uniform(0.5, 1.0, size=16).astype(np.float32)     # bias > 0: small neighbours
    v[1, 6, 2] = np.float32(1.2)
    v[1, 6, 3] = np.float32(-0.4)
    v[1, 6, 4] = np.float32(2.0 ** -20)
    return k, v


def _quantised_kv(k, v, fk, fv):
    from oracle import compare, np_oracle as O
    kq = compare.bf16_rne(O.block_minifloat_quantize(np.ascontiguousarray(np.swapaxes(k, 1, 2)), *fk, block_size=[1, 16], skip_first_dim=True))
    vq = compare.bf16_rne(O.block_minifloat_quantize(v, *fv, block_size=[1, 16], skip_first_dim=True))
    return np.ascontiguousarray(np.swapaxes(kq, 1, 2)), vq


def _same(got, want, what):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{what}: {len(bad)} values differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("D", [32, 96, 128])
@pytest.mark.parametrize("fmt", [(8, 4, 8), (6, 3, 8), (8, 3, 2)])
def test_cache_is_the_oracles_quantiser_bit_for_bit(D, fmt):
    import torch
    from mi355q import ops
    B = 3
    k, v = _inputs(B, 40, D, fmt, seed=D + sum(fmt))
    par = ((8, 4, 8) + fmt, (8, 4, 8) + fmt)              # the cached operands are the weight sides
    cache = ops.MinifloatKVCache(B, 48, D, *par, DEV)
    kt, vt = torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV)
    at = 0
    for n in PIECES:
        cache.append(kt[:, at:at + n], vt[:, at:at + n])
        at += n
        assert cache.length == at
        kd, vd = (t.cpu().numpy() for t in cache.dequantised())
        kq, vq = _quantised_kv(k[:, :at], v[:, :at], fmt, fmt)
        _same(kd, kq, f"K at length {at}")
        _same(vd, vq, f"V at length {at}")
    assert at == 40
    once = ops.MinifloatKVCache(B, 48, D, *par, DEV)
    once.append(kt, vt)
    assert torch.equal(cache.kq, once.kq) and torch.equal(cache.vq, once.vq)
    kq0, vq0 = cache.kq.clone(), cache.vq.clone()
    cache.reset()
    assert cache.length == 0
    for n in PIECES:
        cache.append(kt[:, cache.length:cache.length + n], vt[:, cache.length:cache.length + n])
    assert torch.equal(cache.kq, kq0) and torch.equal(cache.vq, vq0)


def test_ragged_append_with_a_dropped_key():
    """rows at lengths (14, 0, 30) take (3, 2, 0) of 3 input rows: each row holds what a cache of its own would, the padding row is
    never read (NaN), the untouched row keeps its bytes"""
    import torch
    from mi355q import ops
    B, D, fmt = 3, 64, (8, 4, 8)
    k, v = _inputs(B, 40, D, fmt, seed=11)
    before, counts = (14, 0, 30), (3, 2, 0)
    cache = ops.MinifloatKVCache(B, 48, D, fmt + fmt, fmt + fmt, DEV)
    kt, vt = torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV)
    lens = lambda xs: torch.tensor(xs, dtype=torch.int32, device=DEV)
    # fill the rows to their lengths, row by row (counts: the other rows take nothing)
    for b, L in enumerate(before):
        if L:
            cnt = [L if i == b else 0 for i in range(B)]
            cache.append(kt[:, :L], vt[:, :L], lengths=lens([0] * B), counts=lens(cnt), max_length=0)
    kq2 = cache.kq.clone()
    newk, newv = torch.full((B, 3, D), float("nan"), device=DEV), torch.full((B, 3, D), float("nan"), device=DEV)
    for b, (L, c) in enumerate(zip(before, counts)):
        newk[b, :c], newv[b, :c] = kt[b, L:L + c], vt[b, L:L + c]
    cache.append(newk, newv, lengths=lens(before), counts=lens(counts), max_length=max(before))
    after = [L + c for L, c in zip(before, counts)]
    kd, vd = (t.cpu().numpy() for t in cache.dequantised(lengths=lens(after), max_length=max(after)))
    for b, L in enumerate(after):
        kq, vq = _quantised_kv(k[b:b + 1, :L], v[b:b + 1, :L], fmt, fmt)
        _same(kd[b:b + 1, :L], kq, f"K of row {b}")
        _same(vd[b:b + 1, :L], vq, f"V of row {b}")
        assert not kd[b, L:].any() and not vd[b, L:].any()
    per_row = cache.kq.numel() // B
    assert torch.equal(cache.kq[2 * per_row:], kq2[2 * per_row:])      # counts[2] == 0: untouched
