"""The stale-LDS screen of tests/test_gpu_extend_stale_lds.py over the grouped kernels: every compute unit's LDS is filled with a
pattern (tools/lds_poison) in front of each append and each grouped call, and the output must be the same bits under every pattern
(the decode kernels exchange statistics and partial outputs through LDS, the extend kernel stages its fragments there by LDS-DMA)."""
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


def test_append_and_grouped_decode(poison):
    """2 cache rows, G = 8, M = 2 (all 16 columns), 70 keys, 3 splits, D = 128 (32 KiB of LDS in the second kernel)"""
    import torch
    from mi355q import ops
    R, G, M, L, D = 2, 8, 2, 70, 128
    torch.manual_seed(70)
    q, k, v = torch.randn(R * G, M, D, device=DEV), torch.randn(R, L, D, device=DEV), torch.randn(R, L, D, device=DEV)
    outs = []
    for p in PATTERNS:
        cache = ops.KVCache(R, 80, D, PAR, PAR, DEV)
        poison(p)
        cache.append(k[:, :L - M], v[:, :L - M])
        poison(p)
        cache.append(k[:, L - M:], v[:, L - M:])
        poison(p)
        outs.append(ops.bfp_attention_decode(q, cache, group=G, causal=True, scale_div=math.sqrt(D), splits=3).clone())
    torch.cuda.synchronize()
    _same_bits(outs)


def test_append_and_grouped_extend(poison):
    """2 cache rows, G = 4, M = 17 behind 23 keys: two steps, the second query tile holds one query"""
    import torch
    from mi355q import ops
    R, G, M, L, D = 2, 4, 17, 40, 64
    torch.manual_seed(40)
    q, k, v = torch.randn(R * G, M, D, device=DEV), torch.randn(R, L, D, device=DEV), torch.randn(R, L, D, device=DEV)
    outs = []
    for p in PATTERNS:
        cache = ops.KVCache(R, 48, D, PAR, PAR, DEV)
        poison(p)
        cache.append(k[:, :L - M], v[:, :L - M])
        poison(p)
        cache.append(k[:, L - M:], v[:, L - M:])
        poison(p)
        outs.append(ops.bfp_attention_extend(q, cache, group=G, causal=True, scale_div=math.sqrt(D)).clone())
    torch.cuda.synchronize()
    _same_bits(outs)
