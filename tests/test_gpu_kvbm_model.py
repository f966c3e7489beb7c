"""Incremental decoding of block_minifloat harness models on the block_minifloat KV cache (harness.DecodeState(mode="block")): tiny
Llama, OPT and grouped-query Llama built as tests/test_gpu_decode_model.py::_model(..., d=BM8, scale=40.0), teacher-forced 21 + 12
tokens (lengths 21 .. 33, across the 16-key block boundary at 32), against the same model under mode "fp32" -- the reference's route,
torch.cat of fp32 K / V and the four quantisers over all keys -- and, one layer, against the model's own full forward (K and V of a
one-layer model do not depend on earlier attention).  Bound: 5e-4 * max(1, max|ref|) at every step, the bound
tests/test_gpu_decode_model.py::test_declines applies to the fp32 route.  A model with one block_fp and one block_minifloat layer gets
a KVCache and a MinifloatKVCache; its block_fp layer gives the bits it gives under mode "block_fp".

Measured on an MI355X: every step of every model within 3e-5 of the mode "fp32" route (most steps bit-equal) and within 4e-7 of the full
forward.  What this file caught: with the pass-through probabilities (<= 1e-8) in the same matrix-unit accumulator as the quantised
ones, the attention output moved by one ulp where the fp32 route's does not, and the out-projection's 4-bit quantiser -- whose ties the
exact sums of a few 4-bit values often hit -- turned that into steps of up to 6.5e-2 (one layer) and 4.6e-1 (two OPT layers); the decode
kernel now accumulates the two kinds apart (csrc/mi355q_attn_dev.h: at_bm_quant_p_block)."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_gpu_decode_model import BM8, PROMPT, STEPS, W6, _ids, _model, _rel, _teacher_forced  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 5e-4


def _llama(formats, seed=0, scale=40.0, num_heads=2, num_kv_heads=None):
    """a tiny Llama whose layer i has every node in formats[i], weights scaled as _model scales them"""
    import torch
    from mi355q import harness as H
    torch.manual_seed(seed)
    layers = len(formats)
    cfg = H.TinyLlamaConfig(vocab_size=97, hidden_size=128, intermediate_size=256, num_layers=layers, num_heads=num_heads, max_positions=48,
                            num_kv_heads=num_kv_heads)
    qc = H.expand_llama_quant_config(dict(formats[0]), layers)
    for i, f in enumerate(formats):
        qc[f"model_layer_{i}"] = H.expand_llama_quant_config(dict(f), 1)["model_layer_0"]
    model = H.TinyLlamaForCausalLM(cfg, qc)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.ndim == 2 and "embed" not in n:
                p.mul_(scale)
    return model


def _err(got, ref):
    return _rel(got, ref) if np.abs(ref).max() >= 1 else float(np.abs(got - ref).max())


def _steps_against(model, ids, full_forward):
    import torch
    got = _teacher_forced(model, ids, "block")
    ref = _teacher_forced(model, ids, "fp32")
    for s in range(STEPS + 1):
        e = _err(got[:, s], ref[:, s])
        print("block vs fp32 route, step", s, e)
        assert e < BOUND, ("fp32 route", s, e)
    if full_forward:
        with torch.no_grad():
            for s, t in enumerate(range(PROMPT - 1, PROMPT + STEPS)):
                full = model(ids[:, :t + 1])[0][:, -1].cpu().numpy()
                e = _err(got[:, s], full)
                print("block vs full forward, step", s, e)
                assert e < BOUND, ("full forward", s, e)
    assert np.abs(got).max() > 0


@pytest.mark.parametrize("family", ["llama", "opt"])
@pytest.mark.parametrize("layers", [1, 2])
def test_steps_match_the_reference_route_and_the_full_forward(family, layers):
    from mi355q import harness as H, ops
    model, _ = _model(family, layers, d=BM8, scale=40.0)
    model = model.to(DEV)
    state = H.DecodeState(model, 2, 40, "block")
    assert all(type(c) is ops.MinifloatKVCache for c in state.kv)
    _steps_against(model, _ids().to(DEV), full_forward=layers == 1)


def test_grouped_query_llama():
    """4 query heads on 2 KV heads (head_dim 32): the caches hold batch x KV heads rows, the decode runs group = 2"""
    from mi355q import harness as H
    model = _llama((BM8,), num_heads=4, num_kv_heads=2).to(DEV)
    state = H.DecodeState(model, 2, 40, "block")
    assert state.kv[0].B == 4 and state.kv[0].D == 32
    _steps_against(model, _ids().to(DEV), full_forward=True)


def test_one_block_fp_and_one_block_minifloat_layer():
    import torch
    from mi355q import harness as H, ops
    model = _llama((W6, BM8)).to(DEV)
    ids = _ids().to(DEV)
    state = H.DecodeState(model, 2, 40, "block")
    assert type(state.kv[0]) is ops.KVCache and type(state.kv[1]) is ops.MinifloatKVCache
    with pytest.raises(ValueError, match="layer 1.*block_minifloat"):
        H.DecodeState(model, 2, 40, "block_fp")
    _steps_against(model, ids, full_forward=False)
    # the block_fp layer alone: the bits it gives under mode "block_fp" (the state of an all-block_fp model of the same shapes)
    fp_state = H.DecodeState(_llama((W6, W6)).to(DEV), 2, 40, "block_fp")
    blk_state = H.DecodeState(model, 2, 40, "block")
    attn = model.layers[0].self_attn
    torch.manual_seed(1)
    with torch.no_grad():
        for t0, n in ((0, PROMPT), (PROMPT, 1), (PROMPT + 1, 5), (PROMPT + 6, 1)):
            x = torch.randn(2, n, 128, device=DEV)
            pos = torch.arange(t0, t0 + n, device=DEV)[None].expand(2, n).contiguous()
            a, b = attn.decode(x, fp_state, 0, pos), attn.decode(x, blk_state, 0, pos)
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"the block_fp layer differs at length {t0}"
            for s in (fp_state, blk_state):
                s.length += n
    assert torch.equal(fp_state.kv[0].kq, blk_state.kv[0].kq) and torch.equal(fp_state.kv[0].vq, blk_state.kv[0].vq)


@pytest.mark.parametrize("family", ["llama", "opt"])
def test_generate_returns_the_reference_routes_tokens(family):
    import torch
    from mi355q import harness as H
    model, _ = _model(family, 2, d=BM8, scale=40.0)
    model = model.to(DEV)
    prompt = _ids()[:, :PROMPT].to(DEV)
    a_ids, a_logits = H.generate(model, prompt, STEPS, mode="block")
    b_ids, b_logits = H.generate(model, prompt, STEPS, mode="fp32")
    gap = torch.topk(b_logits, 2, dim=-1).values
    print("smallest top-2 gap", float((gap[..., 0] - gap[..., 1]).min()), "worst logit difference", float((a_logits - b_logits).abs().max()))
    assert torch.equal(a_ids, b_ids)
    # a ragged batch (two prompts of different lengths) runs the ragged routes of the same caches
    rows, _ = H.generate(model, [prompt[0, :9], prompt[1, :PROMPT]], 4, mode="block")
    alone, _ = H.generate(model, prompt[1:2], 4, mode="block")
    assert torch.equal(rows[1], alone[0])
