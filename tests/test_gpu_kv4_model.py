"""generate(kv_storage="nibble") and generate(kv_storage="narrowest") on the tiny Llama of tests/test_gpu_kv8_model.py (two layers, hidden
128, 4 heads; plain and with 2 KV heads) with attention widths 4: the 4-bit-mantissa caches give the bf16 and the int8-mantissa caches'
logits bit for bit at every step, hence the same tokens; a model whose layers have cached widths 4, 8 and 9 gets a storage per layer."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import kv4_util as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PROMPT, NEW = 12, 24


@pytest.fixture(scope="module", params=[None, 2], ids=["plain", "grouped"])
def model(request):
    return U.tiny_llama((4, 4), num_kv_heads=request.param).to(DEV)


def _same(a, b, what):
    import torch
    assert a.shape == b.shape
    for step in range(a.shape[1]):
        assert torch.equal(a[:, step].view(torch.uint8), b[:, step].view(torch.uint8)), f"{what}: logits differ at step {step}"


def test_generate_nibble_is_bit_equal_to_the_other_storages(model):
    import torch
    from mi355q import harness as H
    torch.manual_seed(4)
    prompt = torch.randint(0, 97, (2, PROMPT), device=DEV)
    ids4, logits4 = H.generate(model, prompt, NEW, kv_storage="nibble")
    ids16, logits16 = H.generate(model, prompt, NEW, kv_storage=None)
    ids8, logits8 = H.generate(model, prompt, NEW, kv_storage="int8")
    assert logits4.shape == (2, NEW, 97) and bool(torch.isfinite(logits4).all())
    _same(logits4, logits16, "kv_storage=None")
    _same(logits4, logits8, "kv_storage='int8'")
    assert torch.equal(ids4, ids16) and torch.equal(ids4, ids8) and ids4.shape == (2, PROMPT + NEW)


def test_generate_nibble_on_unequal_prompts(model):
    import torch
    from mi355q import harness as H
    g = torch.Generator().manual_seed(6)
    prompts = [torch.randint(0, 97, (n,), generator=g).to(DEV) for n in (12, 7, 9)]
    rows4, logits4 = H.generate(model, prompts, 8, kv_storage="nibble")
    rows16, logits16 = H.generate(model, prompts, 8, kv_storage=None)
    rows8, logits8 = H.generate(model, prompts, 8, kv_storage="int8")
    _same(logits4, logits16, "kv_storage=None, ragged")
    _same(logits4, logits8, "kv_storage='int8', ragged")
    for a, b, c, n in zip(rows4, rows16, rows8, (12, 7, 9)):
        assert torch.equal(a, b) and torch.equal(a, c) and a.numel() == n + 8


def test_nibble_state_bytes_are_9_32(model):
    from mi355q import harness as H, ops
    nibble, plain = H.NibbleDecodeState(model, 3, 24), H.DecodeState(model, 3, 24)
    assert all(type(c) is ops.NibbleKVCache for c in nibble.kv) and all(type(c) is ops.KVCache for c in plain.kv)
    assert sum(c.k4.numel() + c.v4.numel() for c in nibble.kv) * 32 == sum(c.kq.numel() + c.vq.numel() for c in plain.kv) * 9


def test_generate_narrowest_on_a_mixed_width_model():
    """cached widths 4, 8 and 9: a NibbleKVCache, a PackedKVCache and a KVCache in one state, the logits of kv_storage=None as bits"""
    import torch
    from mi355q import harness as H, ops
    mixed = U.tiny_llama((4, 8, 9)).to(DEV)
    state = H._new_state(mixed, 2, PROMPT + NEW, "block_fp", False, None, None, "narrowest")
    assert type(state) is H.NarrowestDecodeState and state.kinds == ["nibble", "int8", "bf16"]
    assert [type(c) for c in state.kv] == [ops.NibbleKVCache, ops.PackedKVCache, ops.KVCache]
    torch.manual_seed(7)
    prompt = torch.randint(0, 97, (2, PROMPT), device=DEV)
    ids_n, logits_n = H.generate(mixed, prompt, NEW, kv_storage="narrowest")
    ids16, logits16 = H.generate(mixed, prompt, NEW, kv_storage=None)
    assert bool(torch.isfinite(logits_n).all())
    _same(logits_n, logits16, "narrowest against kv_storage=None")
    assert torch.equal(ids_n, ids16)
    g = torch.Generator().manual_seed(8)
    prompts = [torch.randint(0, 97, (n,), generator=g).to(DEV) for n in (12, 7, 9)]
    rows_n, ragged_n = H.generate(mixed, prompts, 6, kv_storage="narrowest")
    rows16, ragged16 = H.generate(mixed, prompts, 6, kv_storage=None)
    _same(ragged_n, ragged16, "narrowest against kv_storage=None, ragged")
    assert all(torch.equal(a, b) for a, b in zip(rows_n, rows16))
