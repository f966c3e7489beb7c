"""The mantissa KV caches behind their one host descriptor and one launcher an operation (csrc/mi355q_kvp.h): the same keys through the
int8 contiguous storage (ops.PackedKVCache), the int8 paged storage (ops.PagedPackedKVCache) and the nibble storage (ops.NibbleKVCache)
give the bits of the bf16 ops.KVCache, whichever storage the launchers' switch is handed -- dequantised() and bfp_attention_decode compared
as integers, at width 4 for all three and at width 8 for the two int8 storages.  One body over the storages, at their smallest
interesting shapes: two cache rows that reach (33, 17) keys of a capacity of 48 in two ragged appends, (20, 9) then (13, 8), so both rows'
open tile is quantised again and row 0 runs into a third tile; D = 32 and 128; pages of 32 keys, placed out of order (two pages a row,
the smallest whole number of pages that holds 48 keys).  Planted in K (16 keys of a tile at one d) and in V (16 d of one key): a block
whose maximum is 1 + 4 ulp -- in row 1's K the maximum arrives with the second append, so the open tile's exponent moves -- and an
all-zero block.  No input has 0 < |x| <= 1e-8 (asserted), the mantissa storages' one stated deviation from the bf16 cache.  The
per-storage files (tests/test_gpu_kv8_*.py, test_gpu_kv4_*.py) hold each storage to the oracle; this file holds the dispatch."""
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
B, CAPACITY, P = 2, 48, 32
PIECES = ((20, 9), (13, 8))                       # each row's count in the two appends
LENGTHS = (33, 17)
DECODES = [(M, G, splits) for M in (1, 7) for G in (1, 4) for splits in (1, 2)]
WIDTHS = {"int8": (4, 8), "int8_paged": (4, 8), "nibble": (4,)}
ABOVE_ONE = np.float32(1.0) + 4 * np.spacing(np.float32(1.0))
_KEYS, _BF16 = {}, {}


def _u32(t):
    return t.contiguous().cpu().numpy().view(np.uint32)


def _keys(D):
    """k, v [2, 33, D] with the planted blocks, and the queries of every decode"""
    if D not in _KEYS:
        _, k, v = inputs(B, 1, max(LENGTHS), D, seed=D)
        small = np.linspace(-0.9, 0.9, 16).astype(np.float32)
        for b, at in ((0, 5), (1, 12)):           # (row 1: key 12 comes with the second append)
            k[b, :16, 3] = small
            k[b, at, 3] = ABOVE_ONE
            v[b, 2, :16] = small
            v[b, 2, 7] = -ABOVE_ONE
        k[0, 16:32, 5] = 0                         # row 0's open tile of the first append
        k[1, :16, 6] = 0
        v[0, 20, 16:32] = 0
        v[1, 4, 16:32] = 0
        q = {(M, G): inputs(B * G, M, 1, D, seed=D + 16 * M + G)[0] for M in (1, 7) for G in (1, 4)}
        for a in (k, v, *q.values()):
            assert not ((np.abs(a) <= 1e-8) & (a != 0)).any(), "an input of magnitude 0 < |x| <= 1e-8: bit equality is not claimed for it"
        assert k[0, :16, 3].max() == ABOVE_ONE and ABOVE_ONE.view(np.uint32) == 0x3F800004
        _KEYS[D] = k, v, q
    return _KEYS[D]


def _cache(storage, D, width):
    from mi355q import ops
    if storage == "int8_paged":
        c = ops.PagedPackedKVCache(B, D, par(width), par(width), DEV, page_size=P, num_pages=6, max_pages=-(-CAPACITY // P))
        c.assign(0, [4, 1], upload=False)         # out of order, a free page between them
        c.assign(1, [2, 5])
        return c
    cls = {"bf16": ops.KVCache, "int8": ops.PackedKVCache, "nibble": ops.NibbleKVCache}[storage]
    return cls(B, CAPACITY, D, par(width), par(width), DEV)


def _run(storage, D, width):
    """the two appends, then -> (K bits, V bits, {(M, G, splits): output bits})"""
    import torch
    from mi355q import ops
    k, v, q = _keys(D)
    c = _cache(storage, D, width)
    have = [0] * B
    for counts in PIECES:
        n = max(counts)
        kin, vin = np.full((B, n, D), np.nan, np.float32), np.full((B, n, D), np.nan, np.float32)      # padding behind a count: never read
        for b, cnt in enumerate(counts):
            kin[b, :cnt], vin[b, :cnt] = k[b, have[b]:have[b] + cnt], v[b, have[b]:have[b] + cnt]
        c.append(torch.from_numpy(kin).to(DEV), torch.from_numpy(vin).to(DEV), lengths=i32(have), counts=i32(counts), max_length=max(have))
        have = [h + cnt for h, cnt in zip(have, counts)]
    assert tuple(have) == LENGTHS
    lengths = i32(LENGTHS)
    kd, vd = c.dequantised(lengths, max(LENGTHS))
    outs = {}
    for M, G, splits in DECODES:
        out = ops.bfp_attention_decode(torch.from_numpy(q[(M, G)]).to(DEV), c, scale_div=float(np.sqrt(D)), lengths=lengths,
                                       max_length=max(LENGTHS), group=G, splits=splits)
        assert out.shape == (B * G, M, D)
        outs[(M, G, splits)] = _u32(out)
    return _u32(kd), _u32(vd), outs


def _bf16(D, width):
    """ops.KVCache on the same keys: computed once a (D, width), read by every storage's case"""
    if (D, width) not in _BF16:
        _BF16[(D, width)] = _run("bf16", D, width)
    return _BF16[(D, width)]


@pytest.mark.parametrize("D", [32, 128])
@pytest.mark.parametrize("storage", ["int8", "int8_paged", "nibble"])
def test_every_storage_gives_the_bf16_caches_bits(storage, D):
    k = _keys(D)[0]
    for width in WIDTHS[storage]:
        want_k, want_v, want_out = _bf16(D, width)
        got_k, got_v, got_out = _run(storage, D, width)
        assert got_k.shape == want_k.shape == (B, max(LENGTHS), D)
        assert np.array_equal(got_k, want_k), f"width {width}: K is not KVCache's, as integers"
        assert np.array_equal(got_v, want_v), f"width {width}: V is not KVCache's, as integers"
        kf, vf = got_k.view(np.float32), got_v.view(np.float32)
        # the planted blocks: 1 + 4 ulp rounds to the block's largest mantissa or to 1 and never to 0; the zero blocks are +0
        for b, at in ((0, 5), (1, 12)):
            assert 0.5 <= kf[b, at, 3] <= 2.0 and -2.0 <= vf[b, 2, 7] <= -0.5, f"width {width}: the block whose maximum is 1 + 4 ulp"
        assert not got_k[0, 16:32, 5].any() and not got_k[1, :16, 6].any() and not got_v[0, 20, 16:32].any() and not got_v[1, 4, 16:32].any()
        assert not got_k[1, LENGTHS[1]:].any() and not got_v[1, LENGTHS[1]:].any(), "values behind row 1's length"
        assert kf[0, LENGTHS[0] - 1].any() and np.isfinite(k[0, LENGTHS[0] - 1]).all()
        for case in DECODES:
            assert np.array_equal(got_out[case], want_out[case]), f"width {width}, (M, G, splits) = {case}: the output is not KVCache's, as integers"
            assert np.isfinite(got_out[case].view(np.float32)).all() and got_out[case].any()
