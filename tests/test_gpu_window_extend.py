"""Sliding-window chunked prefill (ops.bfp_attention_extend(window=)): against the oracle with the window mask -- walks that start at
step 0, at an odd and at an even step, odd and even tile counts, ragged counts -- bit for bit against window=None when the window covers
every key and against group 1 on the repeated cache, and within the oracle bound of the windowed decode call."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from window_util import DEV, bits, check, filled, i32, inputs, oracle, par  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("W", [1, 16, 17, 40, 64])
def test_window_extend_vs_oracle_m70(W):
    """M = 70 behind L = 100 (capacity 112): two query blocks; need = 7 (odd) for the last"""
    import torch
    from mi355q import ops
    B, M, L = 2, 70, 100
    D, width = (32, 4) if W in (16, 40) else (128, 6)
    q, k, v = inputs(B, M, L, D, seed=W)
    cache = filled(k, v, width, capacity=112)
    out = ops.bfp_attention_extend(torch.from_numpy(q).to(DEV), cache, scale_div=math.sqrt(D), window=W)
    check(out.cpu().numpy(), oracle(q, k, v, width, W, math.sqrt(D)))


@pytest.mark.parametrize("L,W,D", [(160, 20, 64), (160, 33, 128), (140, 20, 32)])
def test_window_extend_three_blocks(L, W, D):
    """M = 130: three query blocks of 64, first queries at L - 130 + 0 / 64 / 128.  L = 160, W = 20: lower bounds 11, 75, 139 -- walks from
    steps 0, 2 and 4 (even); W = 33: bounds 0, 62, 126 -- from steps 0, 1 and 3 (odd).  L = 160: 6, 10 and 10 tiles (even); L = 140: 5, 9
    and 9 (odd: the last step's second tile is the clamped one)"""
    import torch
    from mi355q import ops
    B, M = 2, 130
    q, k, v = inputs(B, M, L, D, seed=L + W)
    cache = filled(k, v, 6)
    out = ops.bfp_attention_extend(torch.from_numpy(q).to(DEV), cache, scale_div=math.sqrt(D), window=W)
    again = ops.bfp_attention_extend(torch.from_numpy(q).to(DEV), cache, scale_div=math.sqrt(D), window=W)
    assert torch.equal(bits(out), bits(again))
    check(out.cpu().numpy(), oracle(q, k, v, 6, W, math.sqrt(D)))


def test_window_extend_ragged_counts():
    """counts [70, 0, 33] behind lengths [100, 40, 57]: every row against its own oracle, rows behind the count zeros"""
    import torch
    from mi355q import ops
    lengths, counts, W, D, M = [100, 40, 57], [70, 0, 33], 19, 64, 70
    B = 3
    q, k, v = inputs(B, M, 100, D, seed=5)
    cache = ops.KVCache(B, 112, D, par(6), par(6), DEV)
    cache.append(torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV), lengths=i32([0] * B), counts=i32(lengths), max_length=0)
    out = ops.bfp_attention_extend(torch.from_numpy(q).to(DEV), cache, scale_div=8.0, lengths=i32(lengths), counts=i32(counts), max_length=100,
                                   window=W).cpu().numpy()
    for b, (n, c) in enumerate(zip(lengths, counts)):
        assert not out[b, c:].any()
        if c:
            check(out[b:b + 1, :c], oracle(q[b:b + 1, :c], k[b:b + 1, :n], v[b:b + 1, :n], 6, W, 8.0))


def test_window_over_every_key_is_the_unwindowed_call():
    import torch
    from mi355q import ops
    B, M, L, D = 2, 70, 100, 64
    q, k, v = inputs(B, M, L, D, seed=9)
    cache = filled(k, v, 6, capacity=112)
    qt = torch.from_numpy(q).to(DEV)
    ref = ops.bfp_attention_extend(qt, cache, scale_div=8.0)
    for W in (L, L + 5, 10 ** 6):
        assert torch.equal(bits(ops.bfp_attention_extend(qt, cache, scale_div=8.0, window=W)), bits(ref)), W
    lens, cnts = i32([100, 64]), i32([70, 3])
    ref = ops.bfp_attention_extend(qt, cache, scale_div=8.0, lengths=lens, counts=cnts, max_length=L)
    got = ops.bfp_attention_extend(qt, cache, scale_div=8.0, lengths=lens, counts=cnts, max_length=L, window=L)
    assert torch.equal(bits(got), bits(ref))


def test_grouped_is_group_one_on_the_repeated_cache():
    import torch
    from mi355q import ops
    B, G, M, L, W, D = 2, 2, 70, 100, 23, 64
    q, k, v = inputs(B * G, M, L, D, seed=2)
    k, v = k[:B], v[:B]
    qt = torch.from_numpy(q).to(DEV)
    got = ops.bfp_attention_extend(qt, filled(k, v, 6), scale_div=8.0, group=G, window=W)
    ref = ops.bfp_attention_extend(qt, filled(np.repeat(k, G, 0), np.repeat(v, G, 0), 6), scale_div=8.0, window=W)
    assert torch.equal(bits(got), bits(ref))
    check(got.cpu().numpy(), oracle(q, np.repeat(k, G, 0), np.repeat(v, G, 0), 6, W, 8.0))


@pytest.mark.parametrize("M,L,W", [(1, 50, 13), (16, 117, 20), (7, 40, 3)])
def test_agrees_with_the_windowed_decode(M, L, W):
    """M <= 16 behind a non-empty cache, splits = 1: both calls within the oracle bound of the oracle, and of each other (not bitwise:
    the two kernels differ today)"""
    import torch
    from mi355q import ops
    B, D = 2, 64
    q, k, v = inputs(B, M, L, D, seed=M + L)
    cache = filled(k, v, 6)
    qt = torch.from_numpy(q).to(DEV)
    ref = oracle(q, k, v, 6, W, 8.0)
    ext = ops.bfp_attention_extend(qt, cache, scale_div=8.0, window=W).cpu().numpy()
    dec = ops.bfp_attention_decode(qt, cache, scale_div=8.0, splits=1, window=W).cpu().numpy()
    check(ext, ref)
    check(dec, ref)
    assert np.abs(ext - dec).max() <= 1e-3 * np.abs(ref).max()
