"""Incremental decoding of the harness models (harness.DecodeState, forward(cache=...), generate): one layer against the
oracle's full forward -- K and V of a one-layer model do not depend on earlier attention, so the last position's logits of the full
forward on ids[:t + 1] are the step's logits up to summation order; two layers: the block_fp cache route against the
reference-semantics route (torch.cat of fp32 K / V), both of which differ from a full forward the way the reference's own
`past_key_value` does."""
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
BM8 = dict(name="block_minifloat", is_ptq=True, bypass=False, data_in_width=8, data_in_exponent_width=4,
           data_in_exponent_bias_width=8, data_in_block_size=[1, 16], weight_width=8, weight_exponent_width=4,
           weight_exponent_bias_width=8, weight_block_size=[1, 16], bias_width=8, bias_exponent_width=4,
           bias_exponent_bias_width=8, bias_block_size=[16], mi355q_values_matmul="fp32")
PROMPT, STEPS = 21, 12


def _model(family, layers, d=W6, seed=0, scale=4.0):
    """-> (model on the CPU, oracle forward ids -> logits); the oracle's weights are taken before PTQ overwrites them"""
    import torch
    from mi355q import harness as H
    from oracle import np_models as NM
    torch.manual_seed(seed)
    if family == "llama":
        cfg = H.TinyLlamaConfig(vocab_size=97, hidden_size=128, intermediate_size=256, num_layers=layers, num_heads=2, max_positions=48)
        model = H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(dict(d), layers))
    else:
        cfg = H.TinyOPTConfig(vocab_size=97, hidden_size=128, ffn_dim=256, num_layers=layers, num_heads=2, max_positions=48)
        model = H.TinyOPTForCausalLM(cfg, H.expand_quant_config(dict(d), layers))
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.ndim == 2 and "embed" not in n:
                p.mul_(scale)
    sd = {k: v.cpu().numpy().astype(np.float32) for k, v in model.reference_state_dict().items()}
    if family == "llama":
        qc = H.expand_llama_quant_config(dict(d), layers)
        oracle = lambda ids: NM.llama_forward(sd, qc, ids, cfg.num_heads, cfg.rms_eps)[0]
    else:
        qc = H.expand_quant_config(dict(d), layers)
        oracle = lambda ids: NM.opt_forward(sd, qc, ids, cfg.num_heads)[0]
    return model, oracle


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


@pytest.mark.parametrize("family", ["llama", "opt"])
def test_one_layer_steps_match_the_oracles_full_forward(family):
    """lengths 21 .. 33 (across a 16-key block boundary at 32): every step's logits, in both modes, within
    1e-3 * max(1, max|ref|) of the oracle's last-position logits on ids[:t + 1] (tests/test_gpu_model.py's fixture bound)"""
    model, oracle = _model(family, 1)
    ids = _ids()
    ref = _oracle_steps(oracle, ids)
    model = model.to(DEV)
    for mode in ("block_fp", "fp32"):
        got = _teacher_forced(model, ids.to(DEV), mode)
        for s in range(STEPS + 1):
            err = _rel(got[:, s], ref[:, s])
            print(family, mode, "step", s, "rel", err)
            assert err < 1e-3, (mode, s, err)


@pytest.mark.parametrize("family", ["llama", "opt"])
def test_two_layers_cache_route_matches_the_reference_route(family):
    """Two layers: mode "block_fp" against mode "fp32" at every step.  The bound is formed here, from existing kernels against the
    reference's restatement: e1 = the worst relative logit difference of the mode "fp32" route from the oracle on the ONE-layer model
    (the comparison of the test above); the two-layer routes may differ by 2 e1, floor 1e-3, times max(1, max|ref|) -- a second
    layer can carry one rounding flip on (README, depth record).  Both figures are printed.  Measured on an MI355X: llama e1 = 4.4e-7,
    opt e1 = 3.9e-7, so the bound is its floor, 1e-3, for both; the two-layer block_fp / fp32 difference is 0.0 for both families
    (every step's logits byte-equal: the cache holds what the fp32 route's quantisers make of the same rows).  generate() then returns the same
    greedy ids in both modes, on a seed whose top-2 logit gap exceeds that bound at every step (asserted)."""
    import torch
    from mi355q import harness as H
    m1, oracle1 = _model(family, 1)
    ids = _ids()
    ref1 = _oracle_steps(oracle1, ids)
    e1 = max(_rel(a, b) for a, b in zip(np.moveaxis(_teacher_forced(m1.to(DEV), ids.to(DEV), "fp32"), 1, 0), np.moveaxis(ref1, 1, 0)))
    bound = max(2 * e1, 1e-3)
    model, _ = _model(family, 2)
    model = model.to(DEV)
    a = _teacher_forced(model, ids.to(DEV), "block_fp")
    b = _teacher_forced(model, ids.to(DEV), "fp32")
    worst = max(_rel(a[:, s], b[:, s]) for s in range(STEPS + 1))
    print(family, "one-layer fp32 route vs oracle", e1, "bound", bound, "two-layer block_fp vs fp32", worst)
    assert worst <= bound, (worst, bound)
    prompt = ids[:, :PROMPT].to(DEV)
    ga, la = H.generate(model, prompt, STEPS, mode="block_fp")
    gb, lb = H.generate(model, prompt, STEPS, mode="fp32")
    top2 = torch.topk(lb, 2, dim=-1).values
    gap = float((top2[..., 0] - top2[..., 1]).min())
    assert gap > bound * max(1.0, float(lb.abs().max())), f"top-2 gap {gap}: pick another seed"
    assert torch.equal(ga, gb) and ga.shape == (ids.shape[0], PROMPT + STEPS)
    assert _rel(la.cpu().numpy(), lb.cpu().numpy()) <= bound


# ---- the decode step on packed weights: mi355q_small_m = "packed" on mi355q_weight_storage = "packed" ------------------------------
PACKED = dict(W6, mi355q_weight_storage="packed", mi355q_small_m="packed", mi355q_mixed=False)
KEY_OFF = dict(W6, mi355q_weight_storage="packed", mi355q_mixed=False)
LINEARS_A_LAYER = dict(llama=7, opt=6)                    # q, k, v, o, gate, up, down / q, k, v, out, fc1, fc2: K in {128, 256}


def _layer_linears(model):
    """the quantised Linears of the decoder layers (the head is an unquantised nn.Linear)"""
    return [m for layer in model.layers for m in layer.modules() if hasattr(m, "_small_m_takes")]


def _assert_packed(linears):
    for l in linears:
        assert l._w_packed is not None and l._mixed is None, f"a Linear {l.in_features} -> {l.out_features} keeps no packed weights"


def _teacher_forced_on_the_packed_route(model, ids, family, layers):
    """_teacher_forced(mode "block_fp") with the route asserted: the prompt's 2 x 21 rows take the tile GEMMs and leave every
    Linear of the layers with packed weights; every decode step launches the small-batch product once a Linear, no more, no less"""
    import torch
    from mi355q import harness as H
    from mi355q import ops
    linears = _layer_linears(model)
    assert len(linears) == layers * LINEARS_A_LAYER[family]
    state = H.DecodeState(model, ids.shape[0], ids.shape[1], "block_fp")
    with torch.no_grad():
        before = ops.small_m_calls()
        out = [model(ids[:, :PROMPT], cache=state)[0][:, -1]]
        assert ops.small_m_calls() == before, "more than 16 rows took the small-batch route"
        _assert_packed(linears)
        for t in range(PROMPT, PROMPT + STEPS):
            before = ops.small_m_calls()
            out.append(model(ids[:, t:t + 1], cache=state)[0][:, -1])
            assert state.length == t + 1
            assert ops.small_m_calls() - before == len(linears), (t, ops.small_m_calls() - before, len(linears))
    return torch.stack(out, 1).cpu().numpy()


@pytest.mark.parametrize("family", ["llama", "opt"])
def test_one_layer_steps_on_packed_weights_match_the_oracles_full_forward(family):
    """test_one_layer_steps_match_the_oracles_full_forward with every projection of the decode steps on the small-batch product
    that reads width-bit packed weights in place (K = 128 and 256: one partial chunk, one wave), feeding the block_fp cache and the
    decode attention: every step's logits within 1e-3 * max(1, max|ref|) of the oracle's last-position logits on ids[:t + 1]"""
    _, oracle = _model(family, 1)
    model, _ = _model(family, 1, d=PACKED)                # (the same seed: the same weights)
    ids = _ids()
    ref = _oracle_steps(oracle, ids)
    got = _teacher_forced_on_the_packed_route(model.to(DEV), ids.to(DEV), family, 1)
    for s in range(STEPS + 1):
        err = _rel(got[:, s], ref[:, s])
        print(family, "packed route, step", s, "rel", err)
        assert err < 1e-3, (s, err)


@pytest.mark.parametrize("family", ["llama", "opt"])
def test_two_layers_packed_route_matches_the_key_off_model(family):
    """Two layers, mode "block_fp": the packed-route model against the model of the same weights and storage without the
    mi355q_small_m key, at every step.  The bound is the one test_two_layers_cache_route_matches_the_reference_route forms: e1 = the
    worst relative logit difference of the mode "fp32" route from the oracle on the one-layer model, measured here; 2 e1, floor 1e-3,
    times max(1, max|ref|).  Both figures are printed."""
    m1, oracle1 = _model(family, 1)
    ids = _ids()
    ref1 = _oracle_steps(oracle1, ids)
    e1 = max(_rel(a, b) for a, b in zip(np.moveaxis(_teacher_forced(m1.to(DEV), ids.to(DEV), "fp32"), 1, 0), np.moveaxis(ref1, 1, 0)))
    bound = max(2 * e1, 1e-3)
    packed, _ = _model(family, 2, d=PACKED)
    off, _ = _model(family, 2, d=KEY_OFF)
    a = _teacher_forced_on_the_packed_route(packed.to(DEV), ids.to(DEV), family, 2)
    from mi355q import ops
    before = ops.small_m_calls()
    b = _teacher_forced(off.to(DEV), ids.to(DEV), "block_fp")
    assert ops.small_m_calls() == before, "the key-off model took the small-batch route"
    worst = max(_rel(a[:, s], b[:, s]) for s in range(STEPS + 1))
    print(family, "one-layer fp32 route vs oracle", e1, "bound", bound, "two-layer packed route vs key off", worst)
    assert worst <= bound, (worst, bound)


def test_declines():
    """a block_minifloat model has no block_fp cache (ValueError naming the reason); the "fp32" route serves it and matches the
    model's own full forward at the last position, one layer, within 5e-4 * max(1, max|ref|) -- the tolerance of
    test_tiny_llama_loss_parity_other_block_arithmetics for fp32 products of that arithmetic"""
    import torch
    from mi355q import harness as H
    model, _ = _model("llama", 1, d=BM8, scale=40.0)
    model = model.to(DEV)
    with pytest.raises(ValueError, match="block_minifloat"):
        H.DecodeState(model, 2, 48, "block_fp")
    ids = _ids().to(DEV)
    got = _teacher_forced(model, ids, "fp32")
    with torch.no_grad():
        for s, t in enumerate(range(PROMPT - 1, PROMPT + STEPS)):
            ref = model(ids[:, :t + 1])[0][:, -1].cpu().numpy()
            err = _rel(got[:, s], ref) if np.abs(ref).max() >= 1 else float(np.abs(got[:, s] - ref).max())
            print("block_minifloat fp32 route step", s, err)
            assert err < 5e-4, (s, err)
    with pytest.raises(ValueError, match="batch"):
        model(ids[:1, :3], cache=H.DecodeState(model, 2, 48, "fp32"))


def test_a_refused_call_leaves_the_state_usable():
    """more than 16 new tokens behind a non-empty block_fp cache are refused BEFORE any layer's cache grows: the next call works"""
    import torch
    from mi355q import harness as H
    model, _ = _model("llama", 2)
    model = model.to(DEV)
    ids = _ids().to(DEV)
    state = H.DecodeState(model, 2, 48, "block_fp")
    with torch.no_grad():
        model(ids[:, :5], cache=state)
        with pytest.raises(NotImplementedError):
            model(ids[:, 5:25], cache=state)
        assert state.length == 5 and all(c.length == 5 for c in state.kv)
        model(ids[:, 5:6], cache=state)
    assert state.length == 6
