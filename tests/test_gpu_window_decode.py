"""Sliding-window decode on the block_fp KV cache (ops.bfp_attention_decode(window=)): against the oracle with the window mask at every
place the lower edge can fall, and bit for bit against the calls it must equal -- window=None when the window covers every key, an
unwindowed decode on a cache that holds only the window's keys, the one-row call for every row of a ragged batch, group 1 on the
repeated cache."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from window_util import DEV, bits, check, filled, i32, inputs, oracle, par  # noqa: E402

pytestmark = pytest.mark.gpu

# (B, M, L, W, splits, D, width): the lower edge lo = L - M - W + 1 of the row's first query
CASES = [(2, 1, 40, 13, None, 64, 6),      # lo = 27: inside a tile
         (2, 1, 40, 24, 1, 32, 4),         # lo = 16: at a tile edge
         (2, 1, 72, 40, None, 128, 9),     # lo = 32: at a pair edge
         (2, 1, 72, 20, 2, 64, 6),         # lo = 52: in the second tile of pair 1, whose first tile is all masked (and not read)
         (3, 1, 40, 1, None, 64, 4),       # W = 1
         (2, 4, 45, 1, 1, 128, 9),         # W = 1 with M > 1: every query its own key alone
         (2, 16, 50, 5, None, 32, 6),      # W < M
         (2, 16, 117, 20, 3, 64, 6),       # lo = 82, 82 % 32 = 18, one pair a split: the late columns see nothing of the first split
         (2, 1, 1040, 64, None, 128, 6),   # default splits
         (2, 4, 200, 100, 1, 64, 9), (2, 4, 200, 100, 2, 32, 4), (2, 4, 200, 100, 5, 128, 6)]


@pytest.mark.parametrize("B,M,L,W,splits,D,width", CASES)
def test_window_decode_vs_oracle(B, M, L, W, splits, D, width):
    import torch
    from mi355q import ops
    from oracle import compare, np_oracle as O
    q, k, v = inputs(B, M, L, D, seed=L + D + M + W)
    cache = filled(k, v, width, capacity=(L + 31) // 16 * 16)
    out = ops.bfp_attention_decode(torch.from_numpy(q).to(DEV), cache, causal=True, scale_div=math.sqrt(D), splits=splits, window=W)
    again = ops.bfp_attention_decode(torch.from_numpy(q).to(DEV), cache, causal=True, scale_div=math.sqrt(D), splits=splits, window=W)
    assert torch.equal(bits(out), bits(again)), "equal inputs, different bits"
    out = out.cpu().numpy()
    check(out, oracle(q, k, v, width, W, math.sqrt(D)))
    if W == 1:
        one = np.zeros((1, 16), np.float32)
        one[0, 0] = 1.0
        p1 = O.block_fp_quantize(one, width, 8, 127, block_size=[1, 16])[0, 0]
        assert p1 == np.float32(1.0 - 2.0 ** (1 - width))
        vq = compare.bf16_rne(O.block_fp_quantize(v, width, 8, 127, block_size=[1, 16]))
        assert np.array_equal(out, p1 * vq[:, L - M:]), "a query that sees one key must return that key's quantised V row times Q(1)"


@pytest.mark.parametrize("M,L", [(1, 75), (5, 40)])
def test_window_over_every_key_is_the_unwindowed_call(M, L):
    """W >= max_length / cache.length: klo = 0, p0 = 0, span = max_length -- the bits of window=None, uniform and ragged"""
    import torch
    from mi355q import ops
    B, D = 3, 64
    q, k, v = inputs(B, M, L, D, seed=L)
    cache = filled(k, v, 6)
    qt = torch.from_numpy(q).to(DEV)
    lens = i32([L, max(L - 17, M), M])
    for splits in (None, 1, 3):
        ref = ops.bfp_attention_decode(qt, cache, scale_div=8.0, splits=splits)
        for W in (L, L + 1, 10 ** 6):
            assert torch.equal(bits(ops.bfp_attention_decode(qt, cache, scale_div=8.0, splits=splits, window=W)), bits(ref)), (splits, W)
        ref = ops.bfp_attention_decode(qt, cache, scale_div=8.0, splits=splits, lengths=lens, max_length=L)
        got = ops.bfp_attention_decode(qt, cache, scale_div=8.0, splits=splits, lengths=lens, max_length=L, window=L)
        assert torch.equal(bits(got), bits(ref)), ("ragged", splits)


def test_truncated_twin():
    """M = 1, splits = 1, (L - W) % 128 == 0: the windowed decode is, bit for bit, the unwindowed decode on a fresh cache that holds only
    keys L - W .. L - 1 -- the same 16-key blocks, the same tiles on the same waves: skipping the tiles below the window changes no bit"""
    import torch
    from mi355q import ops
    B, L, W, D = 2, 200, 72, 128
    q, k, v = inputs(B, 1, L, D, seed=3)
    qt = torch.from_numpy(q).to(DEV)
    full, twin = filled(k, v, 6), filled(k[:, L - W:], v[:, L - W:], 6)
    got = ops.bfp_attention_decode(qt, full, scale_div=math.sqrt(D), splits=1, window=W)
    ref = ops.bfp_attention_decode(qt, twin, scale_div=math.sqrt(D), splits=1)
    assert torch.equal(bits(got), bits(ref))
    check(got.cpu().numpy(), oracle(q, k, v, 6, W, math.sqrt(D)))


def test_ragged_rows_are_the_one_row_calls():
    """lengths [33, 0, 17, 200], W = 24: every row is the one-row uniform windowed call with splits = 1; the empty row gives zeros"""
    import torch
    from mi355q import ops
    lengths, W, D, M = [33, 0, 17, 200], 24, 64, 1
    B, Lmax = len(lengths), max(lengths)
    q, k, v = inputs(B, M, Lmax, D, seed=11)
    qt, kt, vt = (torch.from_numpy(t).to(DEV) for t in (q, k, v))
    cache = ops.KVCache(B, 208, D, par(6), par(6), DEV)
    cache.append(kt, vt, lengths=i32([0] * B), counts=i32(lengths), max_length=0)
    out = ops.bfp_attention_decode(qt, cache, scale_div=8.0, splits=1, lengths=i32(lengths), max_length=Lmax, window=W)
    dflt = ops.bfp_attention_decode(qt, cache, scale_div=8.0, lengths=i32(lengths), max_length=Lmax, window=W)
    for b, n in enumerate(lengths):
        if n == 0:
            assert not out[b].any() and not dflt[b].any()
            continue
        one = filled(k[b:b + 1, :n], v[b:b + 1, :n], 6)
        ref = ops.bfp_attention_decode(qt[b:b + 1], one, scale_div=8.0, splits=1, window=W)
        assert torch.equal(bits(out[b:b + 1]), bits(ref)), f"row {b}"
        check(dflt[b:b + 1].cpu().numpy(), oracle(q[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n], 6, W, 8.0))


@pytest.mark.parametrize("G,M", [(4, 1), (2, 4)])
def test_grouped_is_group_one_on_the_repeated_cache(G, M):
    import torch
    from mi355q import ops
    B, L, W, D = 2, 90, 21, 64
    q, k, v = inputs(B * G, M, L, D, seed=G)
    k, v = k[:B], v[:B]
    qt = torch.from_numpy(q).to(DEV)
    shared, rep = filled(k, v, 6), filled(np.repeat(k, G, 0), np.repeat(v, G, 0), 6)
    for splits in (1, 2):
        got = ops.bfp_attention_decode(qt, shared, scale_div=8.0, splits=splits, group=G, window=W)
        ref = ops.bfp_attention_decode(qt, rep, scale_div=8.0, splits=splits, window=W)
        assert torch.equal(bits(got), bits(ref)), splits
    check(got.cpu().numpy(), oracle(q, np.repeat(k, G, 0), np.repeat(v, G, 0), 6, W, 8.0))
