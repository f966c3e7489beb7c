"""Grouped-query chunked prefill on the GPU (ops.bfp_attention_extend(group=G)): BIT-EQUAL to today's ungrouped call on a cache of
cache.B * G rows appended with repeat_interleave'd K / V (that kernel has no splits: nothing needs pinning), and against the fp64
oracle on the repeated K / V with the bounds of tests/test_gpu_decode.py (1e-3 max, 3e-5 mean, times the scale)."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))

from tests.test_gpu_gqa_decode import DEV, PAR, _bytes, _check, _oracle  # noqa: E402

pytestmark = pytest.mark.gpu
R, G, D = 2, 4, 64


def _data(M, L, seed):
    r = np.random.default_rng(seed)
    q = (r.normal(size=(R * G, M, D)) * np.exp(r.normal(size=(R * G, M, 1)) * 0.5) * 0.7).astype(np.float32)
    k = (r.normal(size=(R, L, D)) * np.exp(r.normal(size=(R, 1, D)) * 0.5)).astype(np.float32)
    v = r.normal(size=(R, L, D)).astype(np.float32)
    return q, k, v


@pytest.mark.parametrize("M,past", [(20, 30),                # one query block, two of its four waves hold queries
                                    (70, 26),                # two query blocks
                                    (20, 13)])               # 33 keys: an odd tile count, the last step's second tile does not exist
def test_grouped_extend_is_the_ungrouped_call_on_repeated_rows(M, past):
    import torch
    from mi355q import ops
    L = past + M
    q, k, v = _data(M, L, seed=M + past)
    qt, kt, vt = (torch.from_numpy(t).to(DEV) for t in (q, k, v))
    cap = (L + 15) // 16 * 16
    cache, rep = ops.KVCache(R, cap, D, PAR, PAR, DEV), ops.KVCache(R * G, cap, D, PAR, PAR, DEV)
    for n0, n1 in ((0, past), (past, L)):
        cache.append(kt[:, n0:n1], vt[:, n0:n1])
        rep.append(kt[:, n0:n1].repeat_interleave(G, 0), vt[:, n0:n1].repeat_interleave(G, 0))
    got = ops.bfp_attention_extend(qt, cache, group=G, causal=True, scale_div=math.sqrt(D))
    want = ops.bfp_attention_extend(qt, rep, causal=True, scale_div=math.sqrt(D))
    torch.cuda.synchronize()
    bad = (_bytes(got) != _bytes(want)).reshape(R * G, -1).any(1).nonzero().flatten().tolist()
    assert not bad, f"query rows {bad} differ from the ungrouped call on a private copy of their cache row"
    _check(got.cpu().numpy(), _oracle(q, np.repeat(k, G, 0), np.repeat(v, G, 0), causal=True, scale_div=math.sqrt(D)))
    # a [1, Hq, M, D] head view of a [1, M, Hq, D] buffer, token-major output
    view = qt.reshape(1, R * G, M, D).transpose(1, 2).contiguous().transpose(1, 2)
    tm = ops.bfp_attention_extend(view, cache, group=G, causal=True, scale_div=math.sqrt(D), token_major=True)
    assert tm.transpose(1, 2).is_contiguous() and torch.equal(_bytes(tm.reshape(R * G, M, D)), _bytes(want))


@pytest.mark.parametrize("lengths,counts", [([50, 19], [20, 3]),
                                            ([50, 19], [0, 3])])     # a row with count 0: its four heads return zeros
def test_ragged_lengths_and_counts_stay_per_cache_row(lengths, counts):
    import torch
    from mi355q import ops
    M = 20
    q, k, v = _data(M, 50, seed=sum(lengths) + sum(counts))
    qt, kt, vt = (torch.from_numpy(t).to(DEV) for t in (q, k, v))
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=DEV)
    rl, rc = [l for l in lengths for _ in range(G)], [c for c in counts for _ in range(G)]
    cache, rep = ops.KVCache(R, 64, D, PAR, PAR, DEV), ops.KVCache(R * G, 64, D, PAR, PAR, DEV)
    cache.append(kt, vt, lengths=i32([0] * R), counts=i32(lengths), max_length=0)
    rep.append(kt.repeat_interleave(G, 0), vt.repeat_interleave(G, 0), lengths=i32([0] * R * G), counts=i32(rl), max_length=0)
    kw = dict(causal=True, scale_div=8.0, max_length=50)
    got = ops.bfp_attention_extend(qt, cache, group=G, lengths=i32(lengths), counts=i32(counts), **kw)
    want = ops.bfp_attention_extend(qt, rep, lengths=i32(rl), counts=i32(rc), **kw)
    torch.cuda.synchronize()
    assert torch.equal(_bytes(got), _bytes(want))
    out = got.cpu().numpy()
    for r, (L, m) in enumerate(zip(lengths, counts)):
        rows = slice(r * G, (r + 1) * G)
        assert not out[rows, m:].any(), f"cache row {r}: output rows behind its count are not zeros"
        if m:
            _check(out[rows, :m], _oracle(q[rows, :m], np.repeat(k[r:r + 1, :L], G, 0), np.repeat(v[r:r + 1, :L], G, 0), causal=True,
                                          scale_div=8.0))
