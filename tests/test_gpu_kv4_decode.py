"""ops.bfp_attention_decode on an ops.NibbleKVCache (4-bit mantissas, csrc/mi355q_kvp.hip).  Every case is held FIRST to the
fp64-softmax oracle of tests/window_util.py on each row's own keys, within its bounds (1e-3 max, 3e-5 mean of max|ref|), and only then
compared, as bits, with the same call on an ops.PackedKVCache and on an ops.KVCache filled with the same keys under the same `splits`.
Rows of (117, 41, 0) keys in a capacity of 128: a short row -- which splits = 2 leaves an empty split -- and an empty one."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import kv4_util as U  # noqa: E402
from window_util import DEV, bits, check, i32, inputs, oracle, par  # noqa: E402

pytestmark = pytest.mark.gpu
LENGTHS, CAP = (117, 41, 0), 128
WIDTHS = (2, 3, 4)
SPLITS = (1, 2, None)
_MEMO = {}


def _classes():
    from mi355q import ops
    return ops.NibbleKVCache, ops.PackedKVCache, ops.KVCache


def _caches(D, params, lengths=LENGTHS, seed=None, repeat=1):
    """(inputs k, v [B, 117, D], the nibble, the packed and the bf16 cache), each filled by one ragged append; kept per key.
    repeat = G: every row G times (the cache a grouped call is compared with at group=1)"""
    import torch
    key = (D, params, lengths, seed, repeat)
    if key not in _MEMO:
        _, k, v = inputs(len(lengths), 1, max(lengths), D, seed=D + params[3] if seed is None else seed)
        kr, vr, lr = np.repeat(k, repeat, 0), np.repeat(v, repeat, 0), [l for l in lengths for _ in range(repeat)]
        trio = []
        for cls in _classes():
            c = cls(len(lr), CAP, D, params, params, DEV)
            c.append(torch.from_numpy(kr).to(DEV), torch.from_numpy(vr).to(DEV), lengths=i32([0] * len(lr)), counts=i32(lr), max_length=0)
            trio.append(c)
        _MEMO[key] = (k, v, *trio)
    return _MEMO[key]


def _queries(rows, M, D, seed):
    return inputs(rows, M, 1, D, seed=seed)[0]


def _reference(q, k, v, lengths, ora, scale_div, causal=True, group=1):
    """per query row (cache row r // group, its own keys): the oracle, None for a row with fewer than M keys"""
    M, refs = q.shape[1], []
    for r in range(q.shape[0]):
        b = r // group
        L = lengths[b]
        if L < M:
            refs.append(None)
        elif causal:
            refs.append(ora(q[r:r + 1], k[b:b + 1, :L], v[b:b + 1, :L], scale_div)[0])
        else:   # a query that sees all L keys is the single causal query behind them (P's blocks belong to one query)
            refs.append(np.concatenate([ora(q[r:r + 1, i:i + 1], k[b:b + 1, :L], v[b:b + 1, :L], scale_div)[0] for i in range(M)]))
    return refs


def _sym(width):
    return lambda q, k, v, scale_div: oracle(q, k, v, width, None, scale_div)


def _hold(out, refs, what):
    got = out.cpu().numpy()
    for r, ref in enumerate(refs):
        if ref is None:
            assert not got[r].view(np.uint32).any(), f"{what}: row {r} has fewer keys than queries and is not exact zeros"
        else:
            assert np.isfinite(got[r]).all()
            check(got[r], ref)


def _same_bits(out, others, what, **kw):
    import torch
    from mi355q import ops
    q = kw.pop("q")
    for name, cache in others:
        want = ops.bfp_attention_decode(q, cache, **kw)
        assert want.stride() == out.stride() and torch.equal(bits(out), bits(want)), f"{what}: not {name}'s bits"


@pytest.mark.parametrize("D", [32, 64, 96, 128])
@pytest.mark.parametrize("M", [1, 7, 16])
def test_decode_against_the_oracle_then_the_other_caches(D, M):
    import torch
    from mi355q import ops
    width = WIDTHS[(D // 32 + (1, 7, 16).index(M)) % 3]
    k, v, nibble, packed, plain = _caches(D, par(width))
    lengths, sd = i32(LENGTHS), math.sqrt(D)
    q = _queries(3, M, D, seed=D + M)
    qt = torch.from_numpy(q).to(DEV)
    for kw in (dict(causal=True, scale_div=sd), dict(causal=False, scale_div=sd, q_scale=0.37)):
        refs = _reference(q * np.float32(kw.get("q_scale", 1.0)), k, v, LENGTHS, _sym(width), kw["scale_div"], causal=kw["causal"])
        assert refs[2] is None and refs[0] is not None and refs[1] is not None
        for splits in SPLITS:
            call = dict(lengths=lengths, max_length=max(LENGTHS), splits=splits, **kw)
            out = ops.bfp_attention_decode(qt, nibble, **call)
            _hold(out, refs, f"{kw} splits={splits}")
            _same_bits(out, (("PackedKVCache", packed), ("KVCache", plain)), f"{kw} splits={splits}", q=qt, **call)
    assert ops.decode_splits(3, max(LENGTHS), D, 2) == 2           # 2 pairs a split: the row of 41 keys (2 pairs) leaves split 1 empty


def test_token_major_and_the_uniform_call():
    """q as a [1, H, M, D] head view with a token-major output; and the call without lengths, which brings the cache's length"""
    import torch
    from mi355q import ops
    D, M, width, H, L = 64, 7, 4, 3, 75
    q, k, v = inputs(H, M, L, D, seed=3)
    trio = [cls(H, 80, D, par(width), par(width), DEV) for cls in _classes()]
    for c in trio:
        c.append(torch.from_numpy(k).to(DEV)[:, :70], torch.from_numpy(v).to(DEV)[:, :70])
        c.append(torch.from_numpy(k).to(DEV)[None, :, 70:], torch.from_numpy(v).to(DEV)[None, :, 70:])      # head views
    nibble, packed, plain = trio
    assert nibble.length == packed.length == plain.length == L
    refs = _reference(q, k, v, (L,) * H, _sym(width), 8.0)
    qt = torch.from_numpy(q).to(DEV)[None]
    for splits in SPLITS:
        out = ops.bfp_attention_decode(qt, nibble, scale_div=8.0, token_major=True, splits=splits)
        assert out.shape == (1, H, M, D) and out.permute(0, 2, 1, 3).is_contiguous()
        _hold(out[0], refs, "token_major")
        _same_bits(out, (("PackedKVCache", packed), ("KVCache", plain)), "token_major", q=qt, scale_div=8.0, token_major=True, splits=splits)
        flat = ops.bfp_attention_decode(qt[0], nibble, scale_div=8.0, splits=splits)
        assert torch.equal(bits(flat), bits(out[0]))


def test_a_row_with_fewer_keys_than_queries_is_zeros():
    import torch
    from mi355q import ops
    D, M, width, lengths = 64, 7, 3, (117, 5, 0)
    k, v, nibble, packed, plain = _caches(D, par(width), lengths, seed=9)
    q = _queries(3, M, D, seed=21)
    refs = _reference(q, k, v, lengths, _sym(width), 8.0)
    assert refs[1] is None and refs[2] is None
    qt = torch.from_numpy(q).to(DEV)
    for splits in SPLITS:
        call = dict(scale_div=8.0, lengths=i32(lengths), max_length=117, splits=splits)
        out = ops.bfp_attention_decode(qt, nibble, **call)
        _hold(out, refs, "short row")
        _same_bits(out, (("PackedKVCache", packed), ("KVCache", plain)), "short row", q=qt, **call)


@pytest.mark.parametrize("D", [64, 128])
def test_wide_queries_on_a_narrow_cache(D):
    """Q and P of width 8, cached K and V of width 4: the config is built here (data_in_* = the Q / P side, weight_* = the cached side)"""
    import torch
    from mi355q import ops
    M, params = 7, U.par2(8, 4)
    k, v, nibble, packed, plain = _caches(D, params, seed=31 + D)
    assert nibble.qk_params == params
    q = _queries(3, M, D, seed=D + 5)
    sd = math.sqrt(D)
    refs = _reference(q, k, v, LENGTHS, lambda q_, k_, v_, s_: U.oracle2(q_, k_, v_, 8, 4, s_), sd)
    qt = torch.from_numpy(q).to(DEV)
    for splits in SPLITS:
        call = dict(scale_div=sd, lengths=i32(LENGTHS), max_length=max(LENGTHS), splits=splits)
        out = ops.bfp_attention_decode(qt, nibble, **call)
        _hold(out, refs, f"Q / P 8, K / V 4, splits={splits}")
        _same_bits(out, (("PackedKVCache", packed), ("KVCache", plain)), "Q / P 8, K / V 4", q=qt, **call)


@pytest.mark.parametrize("G,M,gw", [(4, 4, 4), (8, 1, 8), (6, 4, 3), (4, 16, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_grouped(G, M, gw, D):
    """G query heads a cache row, the decode_group_width corners: against the oracle on the row's K / V, then as bits against group=1 on a
    cache holding each KV row G times, and against PackedKVCache(group=G)"""
    import torch
    from mi355q import ops
    assert ops.decode_group_width(G, M) == gw
    width = WIDTHS[(D // 32 + G + M) % 3]
    k, v, nibble, packed, plain = _caches(D, par(width))
    repeated = _caches(D, par(width), repeat=G)[2]
    assert repeated.B == 3 * G and type(repeated) is ops.NibbleKVCache
    q = _queries(3 * G, M, D, seed=D + G + M)
    sd = math.sqrt(D)
    refs = _reference(q, k, v, LENGTHS, _sym(width), sd, group=G)
    qt = torch.from_numpy(q).to(DEV)
    for splits in SPLITS:
        # (the default number of splits is that of the launch rows, which differ between the two calls: fix it where it is None)
        sp = splits if splits is not None else ops.decode_splits(3 * G // gw, max(LENGTHS), D)
        call = dict(scale_div=sd, max_length=max(LENGTHS), splits=sp)
        out = ops.bfp_attention_decode(qt, nibble, lengths=i32(LENGTHS), group=G, **call)
        _hold(out, refs, f"G={G} splits={splits}")
        if splits is None:
            assert torch.equal(bits(out), bits(ops.bfp_attention_decode(qt, nibble, scale_div=sd, lengths=i32(LENGTHS), max_length=max(LENGTHS), group=G)))
        one = ops.bfp_attention_decode(qt, repeated, lengths=i32([l for l in LENGTHS for _ in range(G)]), **call)
        assert torch.equal(bits(out), bits(one)), f"G={G} splits={splits}: not the bits of group=1 on the repeated rows"
        _same_bits(out, (("PackedKVCache(group=G)", packed), ("KVCache(group=G)", plain)), f"G={G} splits={splits}", q=qt, lengths=i32(LENGTHS),
                   group=G, **call)
