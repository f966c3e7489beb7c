"""ops.NibbleKVCache (two 4-bit mantissas a byte + one exponent byte a block, csrc/mi355q_kvp.h) holds what ops.PackedKVCache and
ops.KVCache hold: dequantised() of the three compared as bits after every append, and against np_oracle.block_fp_quantize of k^T and of
v; the raw bytes unpacked by the numpy restatement of the documented layout (tests/kv4_util.py) give the same values.  Bit equality is
claimed for inputs without 0 < |x| <= 1e-8 (asserted of the seeded inputs); the planted cases show what happens at exactly those values
and at the places a nibble can go wrong."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import kv4_util as U  # noqa: E402
from window_util import DEV, i32, inputs, par  # noqa: E402

pytestmark = pytest.mark.gpu
PIECES = (5, 16, 1, 27)         # the open tile; a tile crossing (the staging pass); one key; two crossings in one append
WIDTHS = (2, 3, 4)


def _no_tiny(*arrays):
    return all(not ((np.abs(a) <= 1e-8) & (a != 0)).any() for a in arrays)


def _quantised_kv(k, v, width):
    from oracle import compare, np_oracle as O
    kq = compare.bf16_rne(O.block_fp_quantize(np.ascontiguousarray(np.swapaxes(k, 1, 2)), width, 8, 127, block_size=[1, 16]))
    vq = compare.bf16_rne(O.block_fp_quantize(v, width, 8, 127, block_size=[1, 16]))
    return np.ascontiguousarray(np.swapaxes(kq, 1, 2)), vq


def _three(B, C, D, width):
    from mi355q import ops
    return tuple(cls(B, C, D, par(width), par(width), DEV) for cls in (ops.NibbleKVCache, ops.PackedKVCache, ops.KVCache))


def _u32(t):
    return (t.cpu().numpy() if hasattr(t, "cpu") else t).view(np.uint32)


def _raw(cache, width):
    """the cache's bytes through the documented layout -> (K, V) float32 [B, C, D]"""
    K, V = U.unpack_cache(cache.k4.cpu().numpy(), cache.v4.cpu().numpy(), cache.B, cache.capacity, cache.D, width)
    return K.astype(np.float32), V[:, :cache.capacity].astype(np.float32)


@pytest.mark.parametrize("D", [32, 128])
@pytest.mark.parametrize("width", WIDTHS)
def test_contents_equal_the_other_caches(D, width):
    import torch
    B, L = 3, sum(PIECES)
    _, k, v = inputs(B, 1, L, D, seed=D + width)
    assert _no_tiny(k, v), "the seeded inputs hold a value 0 < |x| <= 1e-8: bit equality is not claimed for it"
    nibble, packed, plain = _three(B, 64, D, width)
    kt, vt = torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV)
    at = 0
    for n in PIECES:
        for c in (nibble, packed, plain):
            c.append(kt[:, at:at + n], vt[:, at:at + n])
        at += n
        assert nibble.length == packed.length == plain.length == at
        (k4, v4), (k8, v8), (k16, v16) = nibble.dequantised(), packed.dequantised(), plain.dequantised()
        assert k4.shape == k16.shape == (B, at, D)
        assert np.array_equal(_u32(k4), _u32(k8)) and np.array_equal(_u32(v4), _u32(v8)), f"differs from PackedKVCache at length {at}"
        assert np.array_equal(_u32(k4), _u32(k16)) and np.array_equal(_u32(v4), _u32(v16)), f"differs from KVCache at length {at}"
        kq, vq = _quantised_kv(k[:, :at], v[:, :at], width)
        assert np.array_equal(_u32(k4), kq.view(np.uint32)), f"K differs from block_fp_quantize at length {at}"
        assert np.array_equal(_u32(v4), vq.view(np.uint32)), f"V differs from block_fp_quantize at length {at}"
        # the raw bytes, read as csrc/mi355q_kvp.h words them: the same values (keys the cache does not hold yet: mantissa 0)
        K, V = _raw(nibble, width)
        assert np.array_equal(_u32(K[:, :at]), _u32(k4)) and np.array_equal(_u32(V[:, :at]), _u32(v4)), f"the documented layout at length {at}"
        assert not K[:, at:(at + 15) // 16 * 16].any(), "the open tile's keys behind the length are not mantissa 0"
    # one append of everything, and the same keys again behind reset(): the same bytes
    once = _three(B, 64, D, width)[0]
    once.append(kt, vt)
    assert torch.equal(once.k4, nibble.k4) and torch.equal(once.v4, nibble.v4)
    nibble.reset()
    once.reset()
    nibble.append(kt[:, :17], vt[:, :17])
    for n0, n1 in ((0, 5), (5, 17)):
        once.append(kt[:, n0:n1], vt[:, n0:n1])
    kq, vq = _quantised_kv(k[:, :17], v[:, :17], width)
    k4, v4 = nibble.dequantised()
    assert np.array_equal(_u32(k4), kq.view(np.uint32)) and np.array_equal(_u32(v4), vq.view(np.uint32))
    # (both held the same bytes in front of reset(): what the 17 keys do not rewrite is the same stale bytes in both)
    assert torch.equal(once.k4, nibble.k4) and torch.equal(once.v4, nibble.v4), "behind reset(): piecewise appends != one append, as bytes"


def test_ragged_append():
    """rows at (37, 16, 0) take (7, 0, 3) of 7 input rows; then row 0, at 44, takes 7 more of which keys 48 .. 50 lie behind the capacity
    of 48 and are dropped (the host's max_length is the caller's word and vouches for less)"""
    import torch
    B, D, C, width = 3, 64, 48, 4
    _, k, v = inputs(B, 1, 64, D, seed=11)
    assert _no_tiny(k, v)
    nibble, packed, plain = _three(B, C, D, width)
    have = [0, 0, 0]

    def step(counts, n, max_length):
        src = np.zeros((B, n, D), np.float32), np.zeros((B, n, D), np.float32)
        for b, c in enumerate(counts):
            src[0][b, :c], src[1][b, :c] = k[b, have[b]:have[b] + c], v[b, have[b]:have[b] + c]
            src[0][b, c:] = src[1][b, c:] = np.nan                  # padding behind a row's count is never read
        for cache in (nibble, packed, plain):
            cache.append(torch.from_numpy(src[0]).to(DEV), torch.from_numpy(src[1]).to(DEV), lengths=i32(have), counts=i32(counts),
                         max_length=max_length)
        for b, c in enumerate(counts):
            have[b] = min(have[b] + c, C)
        (k4, v4), (k8, v8), (k16, v16) = (c.dequantised(lengths=i32(have), max_length=max(have)) for c in (nibble, packed, plain))
        assert np.array_equal(_u32(k4), _u32(k8)) and np.array_equal(_u32(v4), _u32(v8)), f"differs from PackedKVCache at {have}"
        assert np.array_equal(_u32(k4), _u32(k16)) and np.array_equal(_u32(v4), _u32(v16)), f"differs from KVCache at {have}"
        for b, l in enumerate(have):                                # each row is what a cache of its own holds
            assert not k4[b, l:].any() and not v4[b, l:].any(), f"row {b}: values behind its length"
            if l == 0:
                continue
            kq, vq = _quantised_kv(k[b:b + 1, :l], v[b:b + 1, :l], width)
            assert np.array_equal(_u32(k4[b:b + 1, :l]), kq.view(np.uint32)), f"row {b} K at {have}"
            assert np.array_equal(_u32(v4[b:b + 1, :l]), vq.view(np.uint32)), f"row {b} V at {have}"

    step((37, 16, 0), 37, 0)
    untouched = nibble.k4.clone(), nibble.v4.clone()
    step((7, 0, 3), 7, 37)
    # counts[b] == 0 leaves the row's bytes alone
    per_k, per_v = nibble.k4.numel() // B, nibble.v4.numel() // B
    assert torch.equal(nibble.k4[per_k:2 * per_k], untouched[0][per_k:2 * per_k]) and torch.equal(nibble.v4[per_v:2 * per_v], untouched[1][per_v:2 * per_v])
    step((7, 0, 0), 7, 41)
    assert have == [48, 16, 3]
    torch.cuda.synchronize()


def test_planted_blocks():
    """One tile of 16 keys, D = 32, width 4 (mantissas -7 .. 7): a K block is the 16 keys at one d -- its neighbouring keys are the two
    nibbles of a byte -- and a V block the 16 d of one key -- its neighbouring d are.  Planted in both: +7 next to -7 (a sign extension
    leaking into the partner nibble would show), an all-negative block, a block whose even lanes are 0 and whose odd lanes are mantissa -1
    and the reverse (ONE lane of each holds -7: a block needs a maximum to put the others at mantissa 1), an all-zero block, and THE ONE
    DEVIATION of csrc/mi355q_kvp.h's int8 storage, carried over: |x| = 1e-8 and 1e-9 among ordinary values, which KVCache passes through unquantised,
    are stored as exactly 0."""
    import torch
    B, L, D, width = 1, 16, 32, 4
    _, k, v = inputs(B, 1, L, D, seed=5)
    assert _no_tiny(k, v)
    pm7 = np.where(np.arange(16) % 2 == 0, 1.75, -1.75).astype(np.float32)                     # mantissas +7, -7, +7, ... at exponent -2
    neg = -(4 + np.arange(16, dtype=np.float32)) / 16                                          # mantissas -1 .. -5 at exponent -2
    odd = np.where(np.arange(16) % 2 == 1, -0.25, 0).astype(np.float32); odd[15] = -1.75        # even lanes 0, odd lanes -1 (lane 15: -7)
    even = np.where(np.arange(16) % 2 == 0, -0.25, 0).astype(np.float32); even[0] = -1.75       # the reverse (lane 0: -7)
    k[0, :, 1] = pm7; v[0, 1, :16] = pm7
    k[0, :, 3] = 0; v[0, 2, :16] = 0
    k[0, :, 5] = neg; v[0, 4, 16:] = neg
    k[0, :, 7] = odd; v[0, 6, :16] = odd
    k[0, :, 8] = even; v[0, 7, 16:] = even
    k[0, 9, 11] = 1e-8; k[0, 10, 11] = -1e-9; v[0, 10, 3] = -1e-8; v[0, 10, 4] = 1e-9
    nibble, packed, plain = _three(B, 16, D, width)
    for c in (nibble, packed, plain):
        c.append(torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV))
    (k4, v4), (k8, v8), (k16, v16) = ([t.cpu().numpy() for t in c.dequantised()] for c in (nibble, packed, plain))
    dk, dv = np.zeros((B, L, D), bool), np.zeros((B, L, D), bool)          # where KVCache may differ: the deviation's values
    dk[0, 9:11, 11] = dv[0, 10, 3:5] = True
    for name, a4, a8, a16, dev, x in (("K", k4, k8, k16, dk, k), ("V", v4, v8, v16, dv, v)):
        assert np.array_equal(a4.view(np.uint32), a8.view(np.uint32)), f"{name}: differs from PackedKVCache"
        assert np.array_equal(a4.view(np.uint32)[~dev], a16.view(np.uint32)[~dev]), f"{name}: a value outside the deviation differs from KVCache"
        assert (np.abs(x[dev]) <= 1e-8).all() and (x[dev] != 0).all()
        assert (a4.view(np.uint32)[dev] == 0).all(), \
            f"{name}: the one deviation (csrc/mi355q_kvp.h: the int8 storage's, carried over by the nibble storage): 0 < |x| <= 1e-8 is stored as +0, got {a4[dev]}"
        assert (a16[dev] != 0).all(), f"{name}: the bf16 cache no longer passes such a value through"
    kq, vq = _quantised_kv(k, v, width)
    assert np.array_equal(k4.view(np.uint32)[~dk], kq.view(np.uint32)[~dk]) and np.array_equal(v4.view(np.uint32)[~dv], vq.view(np.uint32)[~dv])
    # the planted mantissas themselves, from the raw bytes
    km, kc = U.k_piece_unpack(nibble.k4.cpu().numpy()[:288])
    vm = [U.v_piece_unpack(nibble.v4.cpu().numpy()[288 * dt:288 * dt + 288])[0] for dt in range(2)]
    sign = np.where(np.arange(16) % 2 == 0, 1, -1)
    assert np.array_equal(km[:, 1], 7 * sign) and np.array_equal(vm[0][1], 7 * sign), "+7 / -7 in neighbouring nibbles"
    assert np.array_equal(k4[0, :, 1], pm7) and np.array_equal(v4[0, 1, :16], pm7)
    assert not km[:, 3].any() and not vm[0][2].any() and not k4[0, :, 3].any() and not v4[0, 2, :16].any(), "the all-zero block"
    assert (km[:, 5] < 0).all() and (vm[1][4] < 0).all() and (k4[0, :, 5] < 0).all() and (v4[0, 4, 16:] < 0).all(), "the all-negative block"
    want_odd = np.where(np.arange(16) % 2 == 1, -1, 0); want_odd[15] = -7
    want_even = np.where(np.arange(16) % 2 == 0, -1, 0); want_even[0] = -7
    assert np.array_equal(km[:, 7], want_odd) and np.array_equal(vm[0][6], want_odd), "even lanes 0, odd lanes -1"
    assert np.array_equal(km[:, 8], want_even) and np.array_equal(vm[1][7], want_even), "odd lanes 0, even lanes -1"
    assert np.array_equal(k4[0, :, 7], odd) and np.array_equal(v4[0, 6, :16], odd) and np.array_equal(k4[0, :, 8], even) and np.array_equal(v4[0, 7, 16:], even)
    assert km[9, 11] == 0 and km[10, 11] == 0 and vm[0][10, 3] == 0 and vm[0][10, 4] == 0


def test_storage_prefilled_with_0x7f():
    """stale partner nibbles and codes: every byte of k4 and v4 is 0x7F (mantissas -1 and 7, code 127) before the first append.  Inside
    the lengths the contents are those of zeroed storage; behind them every slot rebuilds to a finite value"""
    import torch
    from mi355q import ops
    B, C, D, width, have = 3, 64, 64, 4, (37, 16, 0)
    _, k, v = inputs(B, 1, max(have), D, seed=13)
    assert _no_tiny(k, v)
    kt, vt = torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV)
    stale, clean = (ops.NibbleKVCache(B, C, D, par(width), par(width), DEV) for _ in range(2))
    stale.k4.fill_(0x7F)
    stale.v4.fill_(0x7F)
    for c in (stale, clean):
        c.append(kt, vt, lengths=i32([0] * B), counts=i32(have), max_length=0)
        c.append(kt[:, :1], vt[:, :1], lengths=i32(have), counts=i32([1, 0, 0]), max_length=max(have))
    now = (38, 16, 0)
    (ks, vs), (kc, vc) = (c.dequantised(lengths=i32(now), max_length=max(now)) for c in (stale, clean))
    assert np.array_equal(_u32(ks), _u32(kc)) and np.array_equal(_u32(vs), _u32(vc)), "contents inside the lengths depend on stale bytes"
    # every slot of the storage as the kernels rebuild it: rows read up to the capacity
    ka, va = (t.cpu().numpy() for t in stale.dequantised(lengths=i32([C] * B), max_length=C))
    assert np.isfinite(ka).all() and np.isfinite(va).all(), "a slot behind a row's length does not rebuild to a finite value"
    for b, l in enumerate(now):
        assert np.array_equal(ka[b, :l].view(np.uint32), _u32(kc)[b, :l]) and np.array_equal(va[b, :l].view(np.uint32), _u32(vc)[b, :l])
    assert (va[2] == np.float32(-0.125)).any() or (va[2] == np.float32(0.875)).any(), "row 2 took no key: its V slots still hold the stale bytes"
    K, V = _raw(stale, width)
    assert np.isfinite(K).all() and np.isfinite(V).all()
