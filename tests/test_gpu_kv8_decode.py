"""ops.bfp_attention_decode on an ops.PackedKVCache (int8 mantissas, csrc/mi355q_kvp.hip).  Every case is held FIRST to the
fp64-softmax oracle of tests/window_util.py on each row's own keys, within its bounds, and only then compared, as bits, with the same
call on an ops.KVCache filled with the same keys under the same `splits`.  Rows of (117, 41, 0) keys in a capacity of 128: a short row
-- which splits = 2 leaves an empty split -- and an empty one."""
import ctypes
import math
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from window_util import DEV, bits, check, i32, inputs, oracle, par  # noqa: E402

pytestmark = pytest.mark.gpu
LENGTHS, CAP = (117, 41, 0), 128
WIDTHS = (4, 6, 8)
SPLITS = (1, 2, None)
_MEMO = {}


def _caches(D, width, lengths=LENGTHS, seed=None):
    """(q-less inputs k, v [B, 117, D], the packed cache, the bf16 cache), both filled by one ragged append; kept per (D, width, lengths)"""
    import torch
    from mi355q import ops
    key = (D, width, lengths)
    if key not in _MEMO:
        _, k, v = inputs(len(lengths), 1, max(lengths), D, seed=D + width if seed is None else seed)
        pair = []
        for cls in (ops.PackedKVCache, ops.KVCache):
            c = cls(len(lengths), CAP, D, par(width), par(width), DEV)
            c.append(torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV), lengths=i32([0] * len(lengths)), counts=i32(lengths), max_length=0)
            pair.append(c)
        _MEMO[key] = (k, v, pair[0], pair[1])
    return _MEMO[key]


def _queries(rows, M, D, seed):
    return inputs(rows, M, 1, D, seed=seed)[0]


def _reference(q, k, v, lengths, width, scale_div, causal=True, group=1):
    """per query row (cache row r // group, its own keys): the oracle, None for a row with fewer than M keys"""
    M, refs = q.shape[1], []
    for r in range(q.shape[0]):
        b = r // group
        L = lengths[b]
        if L < M:
            refs.append(None)
        elif causal:
            refs.append(oracle(q[r:r + 1], k[b:b + 1, :L], v[b:b + 1, :L], width, None, scale_div)[0])
        else:   # a query that sees all L keys is the single causal query behind them (P's blocks belong to one query)
            refs.append(np.concatenate([oracle(q[r:r + 1, i:i + 1], k[b:b + 1, :L], v[b:b + 1, :L], width, None, scale_div)[0]
                                        for i in range(M)]))
    return refs


def _hold(out, refs, what):
    got = out.cpu().numpy()
    for r, ref in enumerate(refs):
        if ref is None:
            assert not got[r].view(np.uint32).any(), f"{what}: row {r} has fewer keys than queries and is not exact zeros"
        else:
            assert np.isfinite(got[r]).all()
            check(got[r], ref)


@pytest.mark.parametrize("D", [32, 64, 96, 128])
@pytest.mark.parametrize("M", [1, 7, 16])
def test_decode_against_the_oracle_then_the_bf16_cache(D, M):
    import torch
    from mi355q import ops
    width = WIDTHS[(D // 32 + (1, 7, 16).index(M)) % 3]
    k, v, packed, plain = _caches(D, width)
    lengths, sd = i32(LENGTHS), math.sqrt(D)
    q = _queries(3, M, D, seed=D + M)
    variants = [dict(causal=True, scale_div=sd), dict(causal=False, scale_div=sd, q_scale=0.37)]
    for kw in variants:
        refs = _reference(q * np.float32(kw.get("q_scale", 1.0)), k, v, LENGTHS, width, kw["scale_div"], causal=kw["causal"])
        assert refs[2] is None and refs[0] is not None and refs[1] is not None
        for splits in SPLITS:
            qt = torch.from_numpy(q).to(DEV)
            out = ops.bfp_attention_decode(qt, packed, lengths=lengths, max_length=max(LENGTHS), splits=splits, **kw)
            _hold(out, refs, f"{kw} splits={splits}")
            want = ops.bfp_attention_decode(qt, plain, lengths=lengths, max_length=max(LENGTHS), splits=splits, **kw)
            assert torch.equal(bits(out), bits(want)), f"{kw} splits={splits}: not the bf16 cache's bits"
    assert ops.decode_splits(3, max(LENGTHS), D, 2) == 2           # 2 pairs a split: the row of 41 keys (2 pairs) leaves split 1 empty


def test_token_major_and_the_uniform_call():
    """q as a [1, H, M, D] head view with a token-major output; and the call without lengths, which brings the cache's length"""
    import torch
    from mi355q import ops
    D, M, width, H, L = 64, 7, 6, 3, 75
    q, k, v = inputs(H, M, L, D, seed=3)
    packed, plain = (cls(H, 80, D, par(width), par(width), DEV) for cls in (ops.PackedKVCache, ops.KVCache))
    for c in (packed, plain):
        c.append(torch.from_numpy(k).to(DEV)[:, :70], torch.from_numpy(v).to(DEV)[:, :70])
        c.append(torch.from_numpy(k).to(DEV)[None, :, 70:], torch.from_numpy(v).to(DEV)[None, :, 70:])      # head views
    assert packed.length == plain.length == L
    refs = _reference(q, k, v, (L,) * H, width, 8.0)
    qt = torch.from_numpy(q).to(DEV)[None]
    for splits in SPLITS:
        out = ops.bfp_attention_decode(qt, packed, scale_div=8.0, token_major=True, splits=splits)
        assert out.shape == (1, H, M, D) and out.permute(0, 2, 1, 3).is_contiguous()
        _hold(out[0], refs, "token_major")
        want = ops.bfp_attention_decode(qt, plain, scale_div=8.0, token_major=True, splits=splits)
        assert want.stride() == out.stride() and torch.equal(bits(out), bits(want))
        flat = ops.bfp_attention_decode(qt[0], packed, scale_div=8.0, splits=splits)
        assert torch.equal(bits(flat), bits(out[0]))


def test_a_row_with_fewer_keys_than_queries_is_zeros():
    import torch
    from mi355q import ops
    D, M, width, lengths = 64, 7, 6, (117, 5, 0)
    k, v, packed, plain = _caches(D, width, lengths, seed=9)
    q = _queries(3, M, D, seed=21)
    refs = _reference(q, k, v, lengths, width, 8.0)
    assert refs[1] is None and refs[2] is None
    for splits in SPLITS:
        qt = torch.from_numpy(q).to(DEV)
        out = ops.bfp_attention_decode(qt, packed, scale_div=8.0, lengths=i32(lengths), max_length=117, splits=splits)
        _hold(out, refs, "short row")
        assert torch.equal(bits(out), bits(ops.bfp_attention_decode(qt, plain, scale_div=8.0, lengths=i32(lengths), max_length=117, splits=splits)))


@pytest.mark.parametrize("G,M,gw", [(4, 1, 4), (6, 4, 3), (4, 16, 1)])
@pytest.mark.parametrize("D", [32, 64, 96, 128])
def test_grouped(G, M, gw, D):
    """G query heads a cache row: against the oracle on the repeated K / V, then as bits against the bf16 cache's grouped call"""
    import torch
    from mi355q import ops
    assert ops.decode_group_width(G, M) == gw
    width = WIDTHS[(D // 32 + G + M) % 3]
    k, v, packed, plain = _caches(D, width)
    q = _queries(3 * G, M, D, seed=D + G + M)
    sd, lengths = math.sqrt(D), i32(LENGTHS)
    refs = _reference(q, k, v, LENGTHS, width, sd, group=G)
    qt = torch.from_numpy(q).to(DEV)
    for splits in SPLITS:
        out = ops.bfp_attention_decode(qt, packed, scale_div=sd, lengths=lengths, max_length=max(LENGTHS), splits=splits, group=G)
        _hold(out, refs, f"G={G} splits={splits}")
        want = ops.bfp_attention_decode(qt, plain, scale_div=sd, lengths=lengths, max_length=max(LENGTHS), splits=splits, group=G)
        assert torch.equal(bits(out), bits(want)), f"G={G} splits={splits}: not the bf16 cache's grouped bits"


PATTERNS = (0x00000000, 0xFFFFFFFF, 0x7FC00000, 0x3F800000, 0x00000001, 0x80000000)


@pytest.fixture(scope="module")
def poison():
    import torch
    so = ROOT / "tools" / "lds_poison" / "liblds_poison.so"
    if not so.exists():
        pytest.fail("tools/lds_poison/liblds_poison.so is not built (__graft_entry__.build())")
    lib = ctypes.CDLL(str(so))

    def fill(pattern):
        rc = lib.lds_poison(ctypes.c_uint(pattern), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
    return fill


@pytest.mark.parametrize("B,M,L,D,splits,G", [
    (2, 16, 250, 128, 5, 1),      # partial outputs through the workspace, the widest LDS reduction
    (2, 5, 100, 96, 1, 1),        # one split, three chunks
    (2, 1, 17, 64, 2, 4),         # one key pair: a single split after evening out; grouped
    (3, 3, 70, 32, 2, 2),         # one chunk; grouped, two splits
])
def test_stale_lds(poison, B, M, L, D, splits, G):
    """tests/test_gpu_decode_stale_lds.py for the packed kernels, one case per DC: every compute unit's LDS is filled with a pattern in
    front of each append and decode, and the output must be the same bits under every pattern"""
    import torch
    from mi355q import ops
    torch.manual_seed(L + D)
    q, k, v = torch.randn(B * G, M, D, device=DEV), torch.randn(B, L, D, device=DEV), torch.randn(B, L, D, device=DEV)
    outs = []
    for p in PATTERNS:
        cache = ops.PackedKVCache(B, 256, D, par(6), par(6), DEV)
        poison(p)
        cache.append(k[:, :L - M], v[:, :L - M])
        poison(p)
        cache.append(k[:, L - M:], v[:, L - M:])
        poison(p)
        outs.append(ops.bfp_attention_decode(q, cache, causal=True, scale_div=math.sqrt(D), splits=splits, group=G).clone())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    for p, o in zip(PATTERNS[1:], outs[1:]):
        assert torch.equal(o.view(torch.uint8), outs[0].view(torch.uint8)), f"output depends on stale LDS (pattern {p:#010x})"
