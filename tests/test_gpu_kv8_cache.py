"""ops.PackedKVCache (int8 mantissas + one exponent byte a block, csrc/mi355q_kvp.h) holds what ops.KVCache holds: dequantised() of the
two compared as bits after every append, and against np_oracle.block_fp_quantize of k^T and of v.  Bit equality is claimed for inputs
without 0 < |x| <= 1e-8 (asserted of the seeded inputs); the planted cases show what happens at exactly those values."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from window_util import DEV, i32, inputs, par  # noqa: E402

pytestmark = pytest.mark.gpu
PIECES = (5, 16, 1, 27)         # the open tile; a tile crossing (the staging pass); one key; two crossings in one append


def _no_tiny(*arrays):
    return all(not ((np.abs(a) <= 1e-8) & (a != 0)).any() for a in arrays)


def _quantised_kv(k, v, width):
    from oracle import compare, np_oracle as O
    kq = compare.bf16_rne(O.block_fp_quantize(np.ascontiguousarray(np.swapaxes(k, 1, 2)), width, 8, 127, block_size=[1, 16]))
    vq = compare.bf16_rne(O.block_fp_quantize(v, width, 8, 127, block_size=[1, 16]))
    return np.ascontiguousarray(np.swapaxes(kq, 1, 2)), vq


def _pair(B, C, D, width):
    from mi355q import ops
    return ops.PackedKVCache(B, C, D, par(width), par(width), DEV), ops.KVCache(B, C, D, par(width), par(width), DEV)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("D", [32, 128])
@pytest.mark.parametrize("width", [4, 6, 8])
def test_contents_equal_the_bf16_caches(D, width):
    import torch
    B, L = 3, sum(PIECES)
    _, k, v = inputs(B, 1, L, D, seed=D + width)
    assert _no_tiny(k, v), "the seeded inputs hold a value 0 < |x| <= 1e-8: bit equality is not claimed for it"
    packed, plain = _pair(B, 64, D, width)
    kt, vt = torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV)
    at = 0
    for n in PIECES:
        packed.append(kt[:, at:at + n], vt[:, at:at + n])
        plain.append(kt[:, at:at + n], vt[:, at:at + n])
        at += n
        assert packed.length == plain.length == at
        (k8, v8), (k16, v16) = packed.dequantised(), plain.dequantised()
        assert k8.shape == k16.shape == (B, at, D)
        assert np.array_equal(_u32(k8), _u32(k16)), f"K differs from the bf16 cache at length {at}"
        assert np.array_equal(_u32(v8), _u32(v16)), f"V differs from the bf16 cache at length {at}"
        kq, vq = _quantised_kv(k[:, :at], v[:, :at], width)
        assert np.array_equal(_u32(k8), kq.view(np.uint32)), f"K differs from block_fp_quantize at length {at}"
        assert np.array_equal(_u32(v8), vq.view(np.uint32)), f"V differs from block_fp_quantize at length {at}"
    # one append of everything, and the same keys again behind reset(): the same bytes
    once, _ = _pair(B, 64, D, width)
    once.append(kt, vt)
    assert torch.equal(once.k8, packed.k8) and torch.equal(once.v8, packed.v8)
    packed.reset()
    packed.append(kt[:, :17], vt[:, :17])
    kq, vq = _quantised_kv(k[:, :17], v[:, :17], width)
    k8, v8 = packed.dequantised()
    assert np.array_equal(_u32(k8), kq.view(np.uint32)) and np.array_equal(_u32(v8), vq.view(np.uint32))


def test_ragged_append():
    """rows at (37, 16, 0) take (7, 0, 3) of 7 input rows; then row 0, at 44, takes 7 more of which keys 48 .. 50 lie behind the capacity
    of 48 and are dropped (the host's max_length is the caller's word and vouches for less)"""
    import torch
    B, D, C, width = 3, 64, 48, 6
    _, k, v = inputs(B, 1, 64, D, seed=11)
    assert _no_tiny(k, v)
    packed, plain = _pair(B, C, D, width)
    kt, vt = torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV)
    have = [0, 0, 0]

    def step(counts, n, max_length):
        src = np.zeros((B, n, D), np.float32), np.zeros((B, n, D), np.float32)
        for b, c in enumerate(counts):
            src[0][b, :c], src[1][b, :c] = k[b, have[b]:have[b] + c], v[b, have[b]:have[b] + c]
            src[0][b, c:] = src[1][b, c:] = np.nan                  # padding behind a row's count is never read
        for cache in (packed, plain):
            cache.append(torch.from_numpy(src[0]).to(DEV), torch.from_numpy(src[1]).to(DEV), lengths=i32(have), counts=i32(counts),
                         max_length=max_length)
        for b, c in enumerate(counts):
            have[b] = min(have[b] + c, C)
        (k8, v8), (k16, v16) = (c.dequantised(lengths=i32(have), max_length=max(have)) for c in (packed, plain))
        assert np.array_equal(_u32(k8), _u32(k16)) and np.array_equal(_u32(v8), _u32(v16)), f"differs from the bf16 cache at {have}"
        for b, l in enumerate(have):                                # each row is what a cache of its own holds
            assert not k8[b, l:].any() and not v8[b, l:].any(), f"row {b}: values behind its length"
            if l == 0:
                continue
            kq, vq = _quantised_kv(k[b:b + 1, :l], v[b:b + 1, :l], width)
            assert np.array_equal(_u32(k8[b:b + 1, :l]), kq.view(np.uint32)), f"row {b} K at {have}"
            assert np.array_equal(_u32(v8[b:b + 1, :l]), vq.view(np.uint32)), f"row {b} V at {have}"

    step((37, 16, 0), 37, 0)
    untouched = packed.k8.clone(), packed.v8.clone()
    step((7, 0, 3), 7, 37)
    # counts[b] == 0 leaves the row's bytes alone
    per_k, per_v = packed.k8.numel() // B, packed.v8.numel() // B
    assert torch.equal(packed.k8[per_k:2 * per_k], untouched[0][per_k:2 * per_k]) and torch.equal(packed.v8[per_v:2 * per_v], untouched[1][per_v:2 * per_v])
    step((7, 0, 0), 7, 41)
    assert have == [48, 16, 3]
    torch.cuda.synchronize()


def test_planted_blocks():
    """One tile of 16 keys, D = 32: a K block is the 16 keys at one d, a V block the 16 d of one key.  Planted in both: an all-zero
    block, a maximum four ulps above 1.0 (the exponent's table walk), a subnormal maximum (below bf16's smallest subnormal: both caches
    hold +0), and the values for which the packed cache differs BY DESIGN: a subnormal block above bf16's resolution and one 5e-9
    among ordinary values, 0 < |x| <= 1e-8, which the bf16 cache passes through and the packed cache stores as exactly 0."""
    import torch
    B, L, D, width = 1, 16, 32, 6
    _, k, v = inputs(B, 1, L, D, seed=5)
    assert _no_tiny(k, v)
    up4 = np.float32(1.0) + 4 * np.spacing(np.float32(1.0))
    small = (np.arange(16, dtype=np.float32) - 8) / 32
    tiny = np.float32(1e-41) * (1 + np.arange(16, dtype=np.float32) % 3)        # <= 3e-41 < 2^-134: rounds to +0 in bf16
    assert tiny.max() > 0 and tiny.max() < 2.0 ** -134 and np.float32(tiny.max()) < np.finfo(np.float32).tiny
    sub = np.float32(1e-39) * (np.arange(16, dtype=np.float32) - 7.5)           # subnormal, above bf16's resolution
    k[0, :, 3] = 0; v[0, 2, :16] = 0
    k[0, :, 5] = small; k[0, 7, 5] = up4; v[0, 4, 16:] = small; v[0, 4, 21] = -up4
    k[0, :, 7] = tiny; v[0, 6, :16] = tiny
    k[0, :, 9] = sub; v[0, 8, 16:] = sub
    k[0, 9, 11] = 5e-9; v[0, 10, 3] = -5e-9
    packed, plain = _pair(B, 16, D, width)
    for c in (packed, plain):
        c.append(torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV))
    (k8, v8), (k16, v16) = ([t.cpu().numpy() for t in c.dequantised()] for c in (packed, plain))
    dk, dv = np.zeros((B, L, D), bool), np.zeros((B, L, D), bool)          # where the two may differ: the deviation's values
    dk[0, :, 9] = dv[0, 8, 16:] = True
    dk[0, 9, 11] = dv[0, 10, 3] = True
    for name, a8, a16, dev, x in (("K", k8, k16, dk, k), ("V", v8, v16, dv, v)):
        assert np.array_equal(a8.view(np.uint32)[~dev], a16.view(np.uint32)[~dev]), f"{name}: a value outside the deviation differs"
        assert (np.abs(x[dev]) <= 1e-8).all() and (x[dev] != 0).all()
        assert (a8.view(np.uint32)[dev] == 0).all(), f"{name}: a value 0 < |x| <= 1e-8 is not stored as +0"
        assert (a16[dev] != 0).all() and (np.abs(a16[dev] - x[dev]) <= np.abs(x[dev]) * 2.0 ** -7 + 2.0 ** -133).all(), \
            f"{name}: the bf16 cache no longer passes such a value through"
    # the planted blocks that are bit-equal hold what they should: the oracle's values, zeros where planted
    kq, vq = _quantised_kv(k, v, width)
    assert np.array_equal(k8.view(np.uint32)[~dk], kq.view(np.uint32)[~dk]) and np.array_equal(v8.view(np.uint32)[~dv], vq.view(np.uint32)[~dv])
    assert not k8[0, :, 3].any() and not v8[0, 2, :16].any()
    assert (k8[0, :, 7].view(np.uint32) == 0).all() and (v8[0, 6, :16].view(np.uint32) == 0).all()
    assert k8[0, 7, 5] in (1.0, 0.96875) and k8[0, 0, 5] == -0.25                    # (the block of the maximum 1 + 4 ulps is not degenerate)
