"""generate(kv_storage="int8") and harness.PackedDecodeState on the tiny Llama configs of tests/test_gpu_gqa_model.py (two layers, hidden
128, 4 heads; plain and with 2 KV heads): the int8-mantissa caches give the bf16 caches' logits bit for bit at every step, hence the
same tokens."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_gpu_gqa_model import _model  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PROMPT, NEW = 12, 24


@pytest.fixture(scope="module", params=[None, 2], ids=["plain", "grouped"])
def model(request):
    return _model(2, num_kv_heads=request.param)[0].to(DEV)


def test_generate_is_bit_equal_to_the_bf16_caches(model):
    import torch
    from mi355q import harness as H
    torch.manual_seed(4)
    prompt = torch.randint(0, 97, (2, PROMPT), device=DEV)
    ids8, logits8 = H.generate(model, prompt, NEW, kv_storage="int8")
    ids16, logits16 = H.generate(model, prompt, NEW, kv_storage=None)
    assert logits8.shape == (2, NEW, 97) and bool(torch.isfinite(logits8).all())
    for step in range(NEW):
        assert torch.equal(logits8[:, step].view(torch.uint8), logits16[:, step].view(torch.uint8)), f"logits differ at step {step}"
    assert torch.equal(ids8, ids16) and ids8.shape == (2, PROMPT + NEW)


def test_ragged_state_is_bit_equal_to_decode_state(model):
    """prompts of (12, 7, 9) tokens in one ragged prefill, then calls with counts (1, 1, 1), (1, 0, 1) and (1, 1, 1)"""
    import torch
    from mi355q import harness as H, ops
    torch.manual_seed(5)
    ids = torch.randint(0, 97, (3, 16), device=DEV)
    packed, plain = H.PackedDecodeState(model, 3, 24), H.DecodeState(model, 3, 24)
    assert all(isinstance(c, ops.PackedKVCache) for c in packed.kv) and all(type(c) is ops.KVCache for c in plain.kv)
    assert sum(c.k8.numel() + c.v8.numel() for c in packed.kv) * 32 == sum(c.kq.numel() + c.vq.numel() for c in plain.kv) * 17
    calls = [(ids[:, :12], (12, 7, 9)), (ids[:, 12:13], (1, 1, 1)), (ids[:, 13:14], (1, 0, 1)), (ids[:, 14:15], (1, 1, 1))]
    with torch.no_grad():
        for tokens, counts in calls:
            a = model(tokens, cache=packed, counts=list(counts))[0]
            b = model(tokens, cache=plain, counts=list(counts))[0]
            for row, c in enumerate(counts):
                assert torch.equal(a[row, :c].view(torch.uint8), b[row, :c].view(torch.uint8)), f"row {row} differs at counts {counts}"
            assert packed.lengths == plain.lengths
    assert packed.lengths == [15, 9, 12]
