"""The stale-LDS screen of tests/test_gpu_paged_stale_lds.py in front of one windowed decode case and one windowed extend case: every
compute unit's LDS is filled with a pattern (tools/lds_poison) before the call; the output must be the bits of a run without it."""
import ctypes
import math
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from window_util import DEV, bits, filled, i32  # noqa: E402

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


def _screen(poison, attend):
    import torch
    outs = []
    for p in PATTERNS:
        poison(p)
        outs.append(attend().clone())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    for p, o in zip(PATTERNS[1:], outs[1:]):
        assert torch.equal(bits(o), bits(outs[0])), f"output depends on stale LDS (pattern {p:#010x})"


def test_windowed_decode(poison):
    """2 cache rows, G = 2, M = 8 (all 16 columns), 117 keys, W = 20, one pair a split: late columns with an empty first split"""
    import torch
    from mi355q import ops
    R, G, M, L, D = 2, 2, 8, 117, 128
    torch.manual_seed(1)
    cache = filled(torch.randn(R, L, D), torch.randn(R, L, D), 6)
    q = torch.randn(R * G, M, D, device=DEV)
    _screen(poison, lambda: ops.bfp_attention_decode(q, cache, group=G, scale_div=math.sqrt(D), splits=3, lengths=i32([L, L - 30]),
                                                     max_length=L, window=20))


def test_windowed_extend(poison):
    """2 cache rows, M = 70 behind 30 keys, W = 33: the second query block's walk starts at an odd step"""
    import torch
    from mi355q import ops
    R, M, L, D = 2, 70, 100, 64
    torch.manual_seed(2)
    cache = filled(torch.randn(R, L, D), torch.randn(R, L, D), 6, capacity=112)
    q = torch.randn(R, M, D, device=DEV)
    _screen(poison, lambda: ops.bfp_attention_extend(q, cache, scale_div=math.sqrt(D), window=33))
