"""The extend kernel stages its K and V fragments in LDS by LDS-DMA: in the manner of tests/test_gpu_decode_stale_lds.py, every
compute unit's LDS is filled with a pattern (tools/lds_poison) in front of each append + extend and the output must be the same
bits under every pattern (a fragment read before its DMA has landed would show the pattern)."""
import ctypes
import math
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
PATTERNS = (0x00000000, 0xFFFFFFFF, 0x7FC00000, 0x3F800000, 0x00000001, 0x80000000)
PAR = (6, 8, 127, 6, 8, 127)
DEV = "cuda:0"


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


def _same_bits(outs):
    import torch
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    for p, o in zip(PATTERNS[1:], outs[1:]):
        assert torch.equal(o.view(torch.uint8), outs[0].view(torch.uint8)), f"output depends on stale LDS (pattern {p:#010x})"


@pytest.mark.parametrize("B,M,L,D", [
    (2, 17, 40, 64),             # two steps, the second query tile holds one query
    (2, 65, 333, 128),           # two workgroups, 32 KiB of LDS, an odd tile count
])
def test_append_and_extend(poison, B, M, L, D):
    import torch
    from mi355q import ops
    torch.manual_seed(L + D)
    q, k, v = torch.randn(B, M, D, device=DEV), torch.randn(B, L, D, device=DEV), torch.randn(B, L, D, device=DEV)
    outs = []
    for p in PATTERNS:
        cache = ops.KVCache(B, 336, D, PAR, PAR, DEV)
        poison(p)
        cache.append(k[:, :L - M], v[:, :L - M])
        poison(p)
        cache.append(k[:, L - M:], v[:, L - M:])
        poison(p)
        outs.append(ops.bfp_attention_extend(q, cache, causal=True, scale_div=math.sqrt(D)).clone())
    torch.cuda.synchronize()
    _same_bits(outs)


def test_ragged_append_and_extend(poison):
    """B = 4, D = 64, capacity 144, lengths [45, 16, 0, 130], counts [17, 16, 0, 33], M = 33"""
    import torch
    from mi355q import ops
    B, D, C, M = 4, 64, 144, 33
    lengths, counts = [45, 16, 0, 130], [17, 16, 0, 33]
    first = [l - c for l, c in zip(lengths, counts)]
    torch.manual_seed(130)
    q, k, v = torch.randn(B, M, D, device=DEV), torch.randn(B, 130, D, device=DEV), torch.randn(B, 130, D, device=DEV)
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=DEV)
    k2, v2 = torch.zeros(B, M, D, device=DEV), torch.zeros(B, M, D, device=DEV)
    for b in range(B):
        k2[b, :counts[b]] = k[b, first[b]:lengths[b]]
        v2[b, :counts[b]] = v[b, first[b]:lengths[b]]
    zero, l1, c1, l2, c2 = i32([0] * B), i32(first), i32(first), i32(lengths), i32(counts)
    outs = []
    for p in PATTERNS:
        cache = ops.KVCache(B, C, D, PAR, PAR, DEV)
        poison(p)
        cache.append(k[:, :97].contiguous(), v[:, :97].contiguous(), lengths=zero, counts=c1, max_length=0)
        poison(p)
        cache.append(k2, v2, lengths=l1, counts=c2, max_length=97)
        poison(p)
        outs.append(ops.bfp_attention_extend(q, cache, causal=True, scale_div=8.0, lengths=l2, counts=c2, max_length=130).clone())
    torch.cuda.synchronize()
    _same_bits(outs)
    assert not outs[0][2].any() and not outs[0][0, 17:].any()
