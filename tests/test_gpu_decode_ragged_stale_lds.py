"""The ragged decode kernels are new instantiations that combine their waves' statistics and partial outputs through LDS, and
their empty splits leave the kernel before they touch it: in the manner of tests/test_gpu_small_m_stale_lds.py, every compute
unit's LDS is filled with a pattern (tools/lds_poison) in front of each ragged append and decode, and the output must be the same
bits under every pattern."""
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


@pytest.mark.parametrize("M,D,splits,lengths", [
    (16, 128, 5, (16, 40, 250, 0)),     # partial outputs through the workspace, the widest LDS reduction, empty splits and an empty row
    (1, 64, 2, (1, 17, 33, 64)),        # two splits of one pair each
    (5, 96, 1, (5, 100, 31, 3)),        # one split, three chunks, a row shorter than its queries
])
def test_ragged_append_and_decode(poison, M, D, splits, lengths):
    import torch
    from mi355q import ops
    dev = "cuda:0"
    torch.manual_seed(D + M)
    par = (6, 8, 127, 6, 8, 127)
    B, T = len(lengths), max(lengths)
    q, k, v = torch.randn(B, M, D, device=dev), torch.randn(B, T, D, device=dev), torch.randn(B, T, D, device=dev)
    i32 = lambda xs: torch.tensor(list(xs), dtype=torch.int32, device=dev)
    first = [max(L - M, 0) for L in lengths]
    outs = []
    for p in PATTERNS:
        cache = ops.KVCache(B, 256, D, par, par, dev)
        poison(p)
        cache.append(k, v, lengths=i32([0] * B), counts=i32(first), max_length=0)
        poison(p)
        # every row's last keys: a gather of rows first[b] .. lengths[b] - 1, right-padded
        kn, vn = (torch.stack([torch.roll(t[b], -first[b], 0)[:M] for b in range(B)]) for t in (k, v))
        cache.append(kn, vn, lengths=i32(first), counts=i32([L - f for L, f in zip(lengths, first)]), max_length=max(first))
        poison(p)
        outs.append(ops.bfp_attention_decode(q, cache, causal=True, scale_div=math.sqrt(D), splits=splits, lengths=i32(lengths),
                                             max_length=T).clone())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    for p, o in zip(PATTERNS[1:], outs[1:]):
        assert torch.equal(o.view(torch.uint8), outs[0].view(torch.uint8)), f"output depends on stale LDS (pattern {p:#010x})"
