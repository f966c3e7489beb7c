"""The decode kernels combine their waves' statistics and partial outputs through LDS: in the manner of
tests/test_gpu_small_m_stale_lds.py, every compute unit's LDS is filled with a pattern (tools/lds_poison) in front of each
append + decode and the output must be the same bits under every pattern."""
import ctypes
import math
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
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


@pytest.mark.parametrize("B,M,L,D,splits", [
    (2, 16, 250, 128, 5),        # partial outputs through the workspace, the widest LDS reduction
    (2, 1, 17, 64, 2),           # one key pair: a single split after evening out, output stored by the second phase
    (3, 5, 100, 96, 1),          # one split, three chunks
])
def test_append_and_decode(poison, B, M, L, D, splits):
    import torch
    from mi355q import ops
    dev = "cuda:0"
    torch.manual_seed(L + D)
    par = (6, 8, 127, 6, 8, 127)
    q, k, v = torch.randn(B, M, D, device=dev), torch.randn(B, L, D, device=dev), torch.randn(B, L, D, device=dev)
    outs = []
    for p in PATTERNS:
        cache = ops.KVCache(B, 256, D, par, par, dev)
        poison(p)
        cache.append(k[:, :L - M], v[:, :L - M])
        poison(p)
        cache.append(k[:, L - M:], v[:, L - M:])
        poison(p)
        outs.append(ops.bfp_attention_decode(q, cache, causal=True, scale_div=math.sqrt(D), splits=splits).clone())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    for p, o in zip(PATTERNS[1:], outs[1:]):
        assert torch.equal(o.view(torch.uint8), outs[0].view(torch.uint8)), f"output depends on stale LDS (pattern {p:#010x})"
