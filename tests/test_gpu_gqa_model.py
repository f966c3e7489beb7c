"""Incremental decoding of a grouped-query TinyLlama (hidden 128, 4 heads, 2 KV heads, the W6 config of
tests/test_gpu_decode_model.py).  The oracle is oracle.np_models.llama_forward on a state dict whose k_proj / v_proj rows are
repeated per group, with num_heads = 4: that multi-head twin IS the grouped model's reference (a repeated weight row gives a repeated
output column, which is what repeat_kv makes of the shared head)."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W6 = dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
          data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127,
          weight_block_size=[1, 16], bias_width=6, bias_exponent_width=8, bias_exponent_bias=127, bias_block_size=[16])
PROMPT, STEPS = 21, 12
NH, NKV, HID = 4, 2, 128


def _model(layers, seed=0, scale=4.0, num_kv_heads=NKV):
    """-> (model on the CPU, oracle forward ids -> logits); the oracle's weights are taken before PTQ overwrites them"""
    import torch
    from mi355q import harness as H
    from oracle import np_models as NM
    torch.manual_seed(seed)
    cfg = H.TinyLlamaConfig(vocab_size=97, hidden_size=HID, intermediate_size=256, num_layers=layers, num_heads=NH, max_positions=48,
                            num_kv_heads=num_kv_heads)
    model = H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(dict(W6), layers))
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.ndim == 2 and "embed" not in n:
                p.mul_(scale)
    sd = {k: v.cpu().numpy().astype(np.float32) for k, v in model.reference_state_dict().items()}
    nkv, hd = num_kv_heads or NH, HID // NH
    for k in list(sd):
        if k.endswith(("k_proj.weight", "v_proj.weight")):
            assert sd[k].shape == (nkv * hd, HID)
            sd[k] = np.ascontiguousarray(np.repeat(sd[k].reshape(nkv, hd, HID), NH // nkv, axis=0).reshape(NH * hd, HID))
    qc = H.expand_llama_quant_config(dict(W6), layers)
    return model, lambda ids: NM.llama_forward(sd, qc, ids, NH, cfg.rms_eps)[0]


def _teacher_forced(model, ids, mode):
    """-> logits [B, STEPS + 1, V]: the prompt's last position, then one teacher-forced token a step"""
    import torch
    from mi355q import harness as H
    state = H.DecodeState(model, ids.shape[0], ids.shape[1], mode)
    with torch.no_grad():
        out = [model(ids[:, :PROMPT], cache=state)[0][:, -1]]
        for t in range(PROMPT, PROMPT + STEPS):
            out.append(model(ids[:, t:t + 1], cache=state)[0][:, -1])
            assert state.length == t + 1
    if mode == "block_fp":                                    # the caches hold the KV heads, not the query heads
        assert [c.B for c in state.kv] == [ids.shape[0] * NKV] * len(state.kv)
        assert state.rows_before.numel() == state.rows_after.numel() == ids.shape[0] * NKV
    else:
        assert all(k.shape[1] == NKV and v.shape[1] == NKV for k, v in state.kv)
    return torch.stack(out, 1).cpu().numpy()


def _ids(seed=5, B=2):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 97, (B, PROMPT + STEPS + 1), generator=g)


def _oracle_steps(oracle, ids):
    idn = ids.numpy()
    return np.stack([oracle(idn[:, :t + 1])[:, -1] for t in range(PROMPT - 1, PROMPT + STEPS)], 1)


def _rel(a, ref):
    return float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max()))


@pytest.fixture(scope="module")
def one_layer():
    """(model on the GPU, ids, the oracle's step logits) -- computed once, never written"""
    model, oracle = _model(1)
    ids = _ids()
    return model.to(DEV), ids, _oracle_steps(oracle, ids)


def test_one_layer_steps_match_the_oracles_full_forward(one_layer):
    """lengths 21 .. 33 (across the 16-key block edge at 32): every step's logits, in both modes, within 1e-3 * max(1, max|ref|) of the
    oracle's last-position logits on ids[:t + 1] (the existing fixture bound)"""
    model, ids, ref = one_layer
    for mode in ("block_fp", "fp32"):
        got = _teacher_forced(model, ids.to(DEV), mode)
        for s in range(STEPS + 1):
            err = _rel(got[:, s], ref[:, s])
            print(mode, "step", s, "rel", err)
            assert err < 1e-3, (mode, s, err)


def test_full_forward_matches_the_oracle(one_layer):
    """the full forward repeats k, v right behind the head reshape: the same bound"""
    import torch
    model, ids, _ = one_layer
    _, oracle = _model(1)
    with torch.no_grad():
        got = model(ids[:, :PROMPT].to(DEV))[0].cpu().numpy()
    assert _rel(got, oracle(ids[:, :PROMPT].numpy())) < 1e-3


@pytest.fixture(scope="module")
def two_layers(one_layer):
    """(two-layer model on the GPU, ids, bound): the bound formed exactly as tests/test_gpu_decode_model.py's
    test_two_layers_cache_route_matches_the_reference_route forms it -- e1 = the worst relative logit difference of the mode "fp32"
    route from the oracle on the ONE-layer model; 2 e1, floor 1e-3"""
    m1, ids, ref1 = one_layer
    e1 = max(_rel(a, b) for a, b in zip(np.moveaxis(_teacher_forced(m1, ids.to(DEV), "fp32"), 1, 0), np.moveaxis(ref1, 1, 0)))
    bound = max(2 * e1, 1e-3)
    print("one-layer fp32 route vs oracle", e1, "bound", bound)
    model, _ = _model(2)
    return model.to(DEV), ids, bound


def test_two_layers_cache_route_matches_the_reference_route(two_layers):
    import torch
    from mi355q import harness as H
    model, ids, bound = two_layers
    a = _teacher_forced(model, ids.to(DEV), "block_fp")
    b = _teacher_forced(model, ids.to(DEV), "fp32")
    worst = max(_rel(a[:, s], b[:, s]) for s in range(STEPS + 1))
    print("bound", bound, "two-layer block_fp vs fp32", worst)
    assert worst <= bound, (worst, bound)
    prompt = ids[:, :PROMPT].to(DEV)
    ga, la = H.generate(model, prompt, STEPS, mode="block_fp")
    gb, lb = H.generate(model, prompt, STEPS, mode="fp32")
    top2 = torch.topk(lb, 2, dim=-1).values
    gap = float((top2[..., 0] - top2[..., 1]).min())
    assert gap > bound * max(1.0, float(lb.abs().max())), f"top-2 gap {gap}: pick another seed"
    assert torch.equal(ga, gb) and ga.shape == (ids.shape[0], PROMPT + STEPS)
    assert _rel(la.cpu().numpy(), lb.cpu().numpy()) <= bound


def test_ragged_generate_equals_each_row_alone(two_layers):
    """prompts of lengths 5 and 19 in one ragged batch: each row's greedy ids are those of the row alone, on top-2 gaps above the
    two-layer bound (asserted), and its logits agree within that bound (not bitwise: the Linears' route depends on the batch's shape)"""
    import torch
    from mi355q import harness as H
    model, ids, bound = two_layers
    prompts = [ids[0, :5].to(DEV), ids[1, :19].to(DEV)]
    rows, logits = H.generate(model, prompts, 6)
    for b, p in enumerate(prompts):
        alone, la = H.generate(model, p[None], 6)
        top2 = torch.topk(la[0], 2, dim=-1).values
        gap = float((top2[..., 0] - top2[..., 1]).min())
        assert gap > bound * max(1.0, float(la.abs().max())), f"row {b}: top-2 gap {gap}: pick another seed"
        err = _rel(logits[b].cpu().numpy(), la[0].cpu().numpy())
        print("row", b, "ragged batch vs alone", err)
        assert err <= bound, (b, err, bound)
        assert torch.equal(rows[b], alone[0]), f"row {b} decodes differently in the ragged batch"


def test_chunked_prefill(two_layers, monkeypatch):
    """generate(chunk=...) on a 34-token prompt: the same greedy ids as the yardstick (on a top-2 gap above the bound, asserted) and
    logits within the two-layer bound.
    chunk=16 (16 + 16 + 2) against the ONE-SHOT prompt: the chunks end on 16-key block edges, so every block of K^T is quantised from
    the keys the one-shot prompt gives it; the later calls run on the grouped DECODE kernels (16 new tokens is their limit).
    chunk=17 (17 + 17) against mode "fp32" ON THE SAME SCHEDULE: the second call runs on the grouped EXTEND kernel.  A chunk that
    ends inside a 16-key block sees that block quantised without the keys behind it, as the reference's past_key_value calls would,
    so the one-shot prompt is no yardstick there (tests/test_gpu_extend_model.py; measured 4.9e-2 from it on an MI355X).
    Every cached call reaches ops with group = 2 and a cache of batch * 2 rows, not batch * 4."""
    import torch
    from mi355q import harness as H
    from mi355q import ops
    model, ids, bound = two_layers
    seen = []
    for name in ("bfp_attention_decode", "bfp_attention_extend"):
        def spy(q, cache, _name=name, _real=getattr(ops, name), **kw):
            seen.append((_name, kw.get("group", 1), cache.B, q.shape[-2]))
            return _real(q, cache, **kw)
        monkeypatch.setattr(ops, name, spy)
    prompt = ids.to(DEV)                                      # 34 tokens
    for chunk, yardstick, route in ((16, dict(), ("bfp_attention_decode", 2, 2 * NKV, 16)),
                                    (17, dict(mode="fp32", chunk=17), ("bfp_attention_extend", 2, 2 * NKV, 17))):
        want, lw = H.generate(model, prompt, 4, **yardstick)
        top2 = torch.topk(lw, 2, dim=-1).values
        assert float((top2[..., 0] - top2[..., 1]).min()) > bound * max(1.0, float(lw.abs().max())), "top-2 gap: pick another seed"
        del seen[:]
        got, lg = H.generate(model, prompt, 4, chunk=chunk)
        err = _rel(lg.cpu().numpy(), lw.cpu().numpy())
        print("chunk", chunk, "vs", yardstick or "the one-shot prompt", err)
        assert err <= bound, (chunk, err, bound)
        assert torch.equal(got, want)
        assert route in seen and ("bfp_attention_decode", 2, 2 * NKV, 1) in seen, seen
        assert all(g == 2 and B == 2 * NKV for _, g, B, _ in seen), seen


def test_default_config_keeps_todays_logits_bit_for_bit():
    """two models from the same seed, num_kv_heads=None and num_kv_heads=num_heads: equal parameters, equal logits on one small forward"""
    import torch
    a, _ = _model(2, num_kv_heads=None)
    b, _ = _model(2, num_kv_heads=NH)
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    ids = _ids()[:, :9].to(DEV)
    with torch.no_grad():
        la, lb = a.to(DEV)(ids)[0], b.to(DEV)(ids)[0]
    assert torch.equal(la.view(torch.uint8), lb.view(torch.uint8))
