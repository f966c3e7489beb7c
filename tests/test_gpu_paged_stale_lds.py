"""The stale-LDS screen of tests/test_gpu_gqa_stale_lds.py over the paged kernels: every compute unit's LDS is filled with a pattern
(tools/lds_poison) in front of each paged append and each paged attention call; the output must be the bits of a run without the
poison (the decode kernels exchange statistics and partial outputs through LDS, the extend kernel stages its fragments there by
LDS-DMA -- and the paged kernels ask for table entries ahead of those)."""
import ctypes
import math
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from paged_util import DEV, bits, grow, i32, make_paged  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
PATTERNS = (None, 0x00000000, 0xFFFFFFFF, 0x7FC00000, 0x3F800000, 0x00000001, 0x80000000)      # None: the run without the poison


@pytest.fixture(scope="module")
def poison():
    import torch
    so = ROOT / "tools" / "lds_poison" / "liblds_poison.so"
    if not so.exists():
        pytest.fail("tools/lds_poison/liblds_poison.so is not built (__graft_entry__.build())")
    lib = ctypes.CDLL(str(so))

    def fill(pattern):
        if pattern is None:
            return
        rc = lib.lds_poison(ctypes.c_uint(pattern), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
    return fill


def _same_bits(outs):
    import torch
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    for p, o in zip(PATTERNS[1:], outs[1:]):
        assert torch.equal(bits(o), bits(outs[0])), f"output depends on stale LDS (pattern {p:#010x})"


def _run(poison, attend, R, L, M, D, P):
    import torch
    torch.manual_seed(L)
    k, v = torch.randn(R, L, D, device=DEV), torch.randn(R, L, D, device=DEV)
    outs = []
    for p in PATTERNS:
        cache, plan = make_paged(R, D, P, -(-L // P))
        grow(cache, plan, [L] * R)
        poison(p)
        cache.append(k[:, :L - M].contiguous(), v[:, :L - M].contiguous(), lengths=i32([0] * R), max_length=0)
        poison(p)
        cache.append(k[:, L - M:].contiguous(), v[:, L - M:].contiguous(), lengths=i32([L - M] * R), max_length=L - M)
        poison(p)
        outs.append(attend(cache).clone())
    torch.cuda.synchronize()
    _same_bits(outs)


def test_paged_append_and_decode(poison):
    """2 cache rows, G = 8, M = 2 (all 16 columns), 70 keys in three pages of 32, 3 splits, D = 128"""
    import torch
    from mi355q import ops
    R, G, M, L, D = 2, 8, 2, 70, 128
    q = torch.randn(R * G, M, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    _run(poison, lambda c: ops.bfp_attention_decode(q, c, group=G, causal=True, scale_div=math.sqrt(D), splits=3, lengths=i32([L] * R),
                                                    max_length=L), R, L, M, D, 32)


def test_paged_append_and_extend(poison):
    """2 cache rows, G = 4, M = 17 behind 23 keys: two steps in two pages of 32, the second query tile holds one query"""
    import torch
    from mi355q import ops
    R, G, M, L, D = 2, 4, 17, 40, 64
    q = torch.randn(R * G, M, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    _run(poison, lambda c: ops.bfp_attention_extend(q, c, group=G, causal=True, scale_div=math.sqrt(D), lengths=i32([L] * R), max_length=L),
         R, L, M, D, 32)
