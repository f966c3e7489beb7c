"""The small-batch product on packed weights sums its waves' accumulators through LDS: in the manner of
tests/test_gpu_stale_lds.py, every compute unit's LDS is filled with a pattern (tools/lds_poison) in front of each call and
the output must be the same bits under every pattern."""
import ctypes
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


@pytest.mark.parametrize("N,K,width,flavour,M", [
    (4096, 4096, 6, "row", 16),          # 8 waves a workgroup, one chunk each
    (512, 11008, 6, "block", 4),         # 11 waves, two chunks each, a masked tail chunk
    (200, 320, 5, "block", 1),           # one wave, the halfword path
    (528, 1024, 4, "row", 7),            # two waves, exception blocks from the list
])
def test_small_m_product(poison, N, K, width, flavour, M):
    import torch
    from mi355q import ops
    dev = "cuda:0"
    torch.manual_seed(N + K)
    w = torch.randn(N, K, device=dev) * 0.05
    if flavour == "row":
        w.view(N, K // 16, 16)[::16, 5] *= 2.0 ** 10
    _, wm, we = ops.block_fp_quantize(w, width, 8, 127, [1, 16], False, want_fake=False, want_packed=True)
    if flavour == "row":
        wa = ops.bfp_align_rows(wm, we, width - 1, 127)
        assert ops.row_list_fill(wa.sparse, N)[0] == 0
        pw = ops.pack_row_aligned_weights(wm, we, wa, width, 127)
        assert bool((pw.codes == 255).any())
    else:
        pw = ops.pack_block_exponent_weights(wm, we, width, 127)
    x = torch.randn(M, K, device=dev) * torch.exp(torch.randn(M, 1, device=dev))
    bias = torch.randn(N, device=dev)
    outs = []
    for p in PATTERNS:
        poison(p)
        outs.append(ops.bfp_linear_packed_small(x, pw, width, 8, 127, bias=bias).clone())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    for p, o in zip(PATTERNS[1:], outs[1:]):
        assert torch.equal(o.view(torch.uint8), outs[0].view(torch.uint8)), f"output depends on stale LDS (pattern {p:#010x})"
