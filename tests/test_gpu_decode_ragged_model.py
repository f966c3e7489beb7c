"""Ragged batches through the harness models (harness.DecodeState, model(ids, cache=state, counts=[...]), generate on a list of
prompts): prompts of 5, 16 and 23 tokens decode together, twelve steps, and every sequence must come out as it does ALONE -- the
models, the configs and the bound of tests/test_gpu_decode_model.py, restated here."""
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
LENS, STEPS = (5, 16, 23), 12
PROMPT = 21                     # (of the one-layer run that forms the bound: tests/test_gpu_decode_model.py's)
SEED = 5


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


def _rel(a, ref):
    return float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max()))


_BOUND = {}


def _bound(family):
    """formed as test_two_layers_cache_route_matches_the_reference_route forms its own: e1 = the worst relative logit difference of
    the mode "fp32" route from the oracle on the ONE-layer model, teacher-forced over 21 + 12 tokens; the bound is 2 e1, floor 1e-3.
    Once a family."""
    if family not in _BOUND:
        import torch
        from mi355q import harness as H
        m1, oracle1 = _model(family, 1)
        g = torch.Generator().manual_seed(5)
        ids = torch.randint(0, 97, (2, PROMPT + STEPS + 1), generator=g)
        idn = ids.numpy()
        ref = [oracle1(idn[:, :t + 1])[:, -1] for t in range(PROMPT - 1, PROMPT + STEPS)]
        m1, ids = m1.to(DEV), ids.to(DEV)
        state = H.DecodeState(m1, 2, ids.shape[1], "fp32")
        with torch.no_grad():
            got = [m1(ids[:, :PROMPT], cache=state)[0][:, -1]]
            for t in range(PROMPT, PROMPT + STEPS):
                got.append(m1(ids[:, t:t + 1], cache=state)[0][:, -1])
        e1 = max(_rel(a.cpu().numpy(), b) for a, b in zip(got, ref))
        _BOUND[family] = (e1, max(2 * e1, 1e-3))
    return _BOUND[family]


def _prompts(seed=SEED):
    import torch
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 97, (n,), generator=g).to(DEV) for n in LENS]


def _padded(rows):
    import torch
    ids = torch.zeros(len(rows), max(r.numel() for r in rows), dtype=rows[0].dtype, device=DEV)
    for b, r in enumerate(rows):
        ids[b, :r.numel()] = r
    return ids


def _as_if_alone(family, model, what, linears=None):
    """the property below on `model`; `linears` (the layers' quantised Linears, for a model on the packed small-batch route): the ragged
    prefill's 3 x 23 rows take the tile GEMMs and leave every one of them with packed weights, and every decode step launches the
    small-batch product exactly once a Linear"""
    import torch
    from mi355q import harness as H
    from mi355q import ops
    e1, bound = _bound(family)
    prompts = _prompts()
    alone = [H.generate(model, p[None], STEPS, "block_fp") for p in prompts]
    state = H.DecodeState(model, len(LENS), max(LENS) + STEPS, "block_fp")
    worst = 0.0
    with torch.no_grad():
        calls = ops.small_m_calls()
        out = model(_padded(prompts), cache=state, counts=list(LENS))[0]
        if linears is not None:
            assert ops.small_m_calls() == calls, "more than 16 rows took the small-batch route"
            for l in linears:
                assert l._w_packed is not None and l._mixed is None, f"a Linear {l.in_features} -> {l.out_features} keeps no packed weights"
        step = torch.stack([out[b, n - 1] for b, n in enumerate(LENS)])
        for s in range(STEPS):
            assert state.lengths == [n + s for n in LENS]
            for b in range(len(LENS)):
                err = _rel(step[b].cpu().numpy(), alone[b][1][0, s].cpu().numpy())
                worst = max(worst, err)
                assert err <= bound, (family, "step", s, "row", b, err, bound)
            if s + 1 < STEPS:
                tok = torch.stack([alone[b][0][0, n + s] for b, n in enumerate(LENS)])[:, None]
                calls = ops.small_m_calls()
                step = model(tok, cache=state, counts=[1] * len(LENS))[0][:, -1]
                if linears is not None:
                    assert ops.small_m_calls() - calls == len(linears), (s, ops.small_m_calls() - calls, len(linears))
    print(family, what, "one-layer fp32 route vs oracle", e1, "bound", bound, "ragged batch vs alone, worst over rows and steps", worst)
    assert all(c.length == 0 for c in state.kv)                 # the caller -- the state -- owns the lengths
    # generate on the list
    rows, logits = H.generate(model, prompts, STEPS)
    assert [r.numel() for r in rows] == [n + STEPS for n in LENS] and logits.shape == (len(LENS), STEPS, 97)
    for b, n in enumerate(LENS):
        first = alone[b][1][0, 0]
        top2 = torch.topk(first, 2).values
        gap = float(top2[0] - top2[1])
        assert gap > bound * max(1.0, float(first.abs().max())), f"row {b}: top-2 gap {gap} of the alone run: pick another seed"
        assert torch.equal(rows[b][:n], prompts[b]) and int(rows[b][n]) == int(alone[b][0][0, n]), f"row {b}: first new token differs"
        assert _rel(logits[b, 0].cpu().numpy(), first.cpu().numpy()) <= bound


@pytest.mark.parametrize("family", ["llama", "opt"])
def test_every_sequence_of_a_ragged_batch_decodes_as_if_alone(family):
    """Two layers.  Each prompt alone through generate(..., "block_fp"); then the three together, teacher-forced with the alone
    runs' tokens: at every step each row's logits agree with its alone run within the bound above (not bitwise: the Linears' route
    depends on the batch's shape).  The rows are 5 .. 16, 16 .. 27 and 23 .. 34 keys long: they fill, start and cross a 16-key
    block, and cross the 32-key pair, at different steps.  Then generate() on the list of prompts.
    Measured on an MI355X: one-layer fp32 route against the oracle 4.4e-7 (llama), 3.9e-7 (opt), so the bound is its floor 1e-3;
    ragged batch against the alone runs, worst over rows and steps, 2.0e-7 (llama), 1.7e-7 (opt)."""
    model, _ = _model(family, 2)
    _as_if_alone(family, model.to(DEV), "default route:")


PACKED = dict(W6, mi355q_weight_storage="packed", mi355q_small_m="packed", mi355q_mixed=False)


@pytest.mark.parametrize("family", ["llama", "opt"])
def test_every_sequence_of_a_ragged_batch_on_packed_weights_decodes_as_if_alone(family):
    """The same property, the same bound, with every projection of the decode steps (3 rows a call) on the small-batch product that
    reads width-bit packed weights in place (mi355q_small_m = "packed" on mi355q_weight_storage = "packed"), feeding the ragged
    cache append and the ragged decode attention.  The alone runs of the 5- and 16-token prompts take that product in their
    prefill as well (at most 16 rows)."""
    model, _ = _model(family, 2, d=PACKED)
    model = model.to(DEV)
    linears = [m for layer in model.layers for m in layer.modules() if hasattr(m, "_small_m_takes")]
    assert len(linears) == 2 * dict(llama=7, opt=6)[family]
    _as_if_alone(family, model, "packed small-batch route:", linears)


def _cache_bytes(state):
    return [t.clone() for c in state.kv for t in (c.kq, c.vq, c.stage)]


def test_refusals_leave_every_cache_as_it_was():
    import torch
    from mi355q import harness as H
    model, _ = _model("llama", 2)
    model = model.to(DEV)
    prompts = _prompts()
    ids = _padded(prompts)
    with torch.no_grad():
        # a mixed call: row 1 has not started while rows 0 and 2 continue
        state = H.DecodeState(model, 3, 48, "block_fp")
        model(ids, cache=state, counts=[5, 0, 23])
        assert state.lengths == [5, 0, 23]
        held = _cache_bytes(state)
        with pytest.raises(NotImplementedError, match="mixed"):
            model(ids[:, :1], cache=state, counts=[1, 1, 1])
        # more than 16 tokens behind non-empty rows
        with pytest.raises(NotImplementedError, match="at most 16"):
            model(ids[:, :17], cache=state, counts=[17, 0, 17])
        # unequal counts behind non-empty rows
        with pytest.raises(NotImplementedError, match="unequal"):
            model(ids[:, :2], cache=state, counts=[2, 0, 1])
        with pytest.raises(ValueError, match="counts"):
            model(ids[:, :2], cache=state, counts=[2, 0])
        assert state.lengths == [5, 0, 23]
        for a, b in zip(held, _cache_bytes(state)):
            assert torch.equal(a, b)
        model(ids[:, :1], cache=state, counts=[1, 0, 1])           # the state is still usable; the idle row costs nothing
        assert state.lengths == [6, 0, 24]
        # mode "fp32" has no ragged route: the reference's mask route gives different numbers
        ref = H.DecodeState(model, 3, 48, "fp32")
        with pytest.raises(NotImplementedError, match="left padding"):
            model(ids, cache=ref, counts=list(LENS))
        assert ref.lengths == [0, 0, 0] and all(kv is None for kv in ref.kv)
        with pytest.raises(ValueError, match="cached call"):
            model(ids, counts=list(LENS))
