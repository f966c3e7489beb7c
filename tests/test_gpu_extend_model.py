"""Chunked prefill of the harness models (harness.DecodeState(extend=True), generate(chunk=...)): the models, configs and the bound
of tests/test_gpu_decode_model.py, restated.  The bound is formed here: e1 = the worst relative logit difference of the mode "fp32"
route from the oracle's full forward on the ONE-layer model, measured in this file; two routes of a deeper model may differ by
max(2 e1, 1e-3) times max(1, max|ref|)."""
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
SCHEDULE = (5, 20, 1, 17)


def _model(family, layers, d=W6, seed=0, scale=4.0, max_positions=48):
    """-> (model on the CPU, oracle forward ids -> logits); the oracle's weights are taken before PTQ overwrites them"""
    import torch
    from mi355q import harness as H
    from oracle import np_models as NM
    torch.manual_seed(seed)
    if family == "llama":
        cfg = H.TinyLlamaConfig(vocab_size=97, hidden_size=128, intermediate_size=256, num_layers=layers, num_heads=2,
                                max_positions=max_positions)
        model = H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(dict(d), layers))
    else:
        cfg = H.TinyOPTConfig(vocab_size=97, hidden_size=128, ffn_dim=256, num_layers=layers, num_heads=2, max_positions=max_positions)
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
    return torch.stack(out, 1).cpu().numpy()


def _ids(seed=5, B=2, T=PROMPT + STEPS + 1):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 97, (B, T), generator=g)


def _rel(a, ref):
    return float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max()))


_BOUND = {}


def _bound(family):
    """max(2 e1, 1e-3), e1 measured once a family: the one-layer mode "fp32" route against the oracle's full forward"""
    if family not in _BOUND:
        m1, oracle1 = _model(family, 1)
        ids = _ids()
        idn = ids.numpy()
        ref1 = np.stack([oracle1(idn[:, :t + 1])[:, -1] for t in range(PROMPT - 1, PROMPT + STEPS)], 1)
        got = _teacher_forced(m1.to(DEV), ids.to(DEV), "fp32")
        e1 = max(_rel(got[:, s], ref1[:, s]) for s in range(STEPS + 1))
        _BOUND[family] = max(2 * e1, 1e-3)
        print(family, "one-layer fp32 route vs oracle", e1, "bound", _BOUND[family])
    return _BOUND[family]


def _cache_bytes(state):
    return [t.clone() for c in state.kv for t in (c.kq, c.vq, c.stage)]


@pytest.mark.parametrize("family", ["llama", "opt"])
def test_chunked_prompt_two_layers(family):
    """the chunk schedule (5, 20, 1, 17) through a mode "fp32" state and through a block_fp state with extend=True (prefill, the
    uniform extend form, a decode step, the extend form again): every call's logits agree within the bound.  generate(chunk=16) and
    generate() then return the same greedy ids, on a seed whose top-2 logit gap exceeds the bound at every step (asserted); a list of
    prompts of different lengths in chunks of 7, whose third call has unequal counts, gives every row the ids of that row alone in
    chunks of 7."""
    import torch
    from mi355q import harness as H
    bound = _bound(family)
    model, _ = _model(family, 2)
    model = model.to(DEV)
    ids = _ids(T=sum(SCHEDULE)).to(DEV)
    ref, ext = H.DecodeState(model, 2, 48, "fp32"), H.DecodeState(model, 2, 48, "block_fp", extend=True)
    at = 0
    with torch.no_grad():
        for n in SCHEDULE:
            a = model(ids[:, at:at + n], cache=ext)[0].cpu().numpy()
            b = model(ids[:, at:at + n], cache=ref)[0].cpu().numpy()
            at += n
            err = _rel(a, b)
            print(family, "call of", n, "tokens at", at - n, "block_fp extend vs fp32", err)
            assert err <= bound, (n, err, bound)
            assert ext.length == at and all(c.length == at for c in ext.kv)
    prompt = _ids()[:, :PROMPT].to(DEV)
    ga, la = H.generate(model, prompt, STEPS, chunk=16)
    gb, lb = H.generate(model, prompt, STEPS)
    top2 = torch.topk(lb, 2, dim=-1).values
    gap = float((top2[..., 0] - top2[..., 1]).min())
    assert gap > bound * max(1.0, float(lb.abs().max())), f"top-2 gap {gap}: pick another seed"
    assert torch.equal(ga, gb) and ga.shape == (2, PROMPT + STEPS)
    assert _rel(la.cpu().numpy(), lb.cpu().numpy()) <= bound
    # (chunks that end inside a 16-key block see that block quantised without the keys behind it, as the reference's past_key_value
    #  calls would: the yardstick is each row ALONE on the same chunk schedule, not the one-shot prompt)
    prompts = [_ids(seed=9, B=1, T=n)[0].to(DEV) for n in (5, 16, 23)]
    ra, xa = H.generate(model, prompts, 4, chunk=7)
    for b, p in enumerate(prompts):
        rb, xb = H.generate(model, p[None], 4, chunk=7)
        top2 = torch.topk(xb, 2, dim=-1).values
        gap = float((top2[..., 0] - top2[..., 1]).min())
        assert gap > bound * max(1.0, float(xb.abs().max())), f"top-2 gap {gap}: pick another seed"
        assert torch.equal(ra[b], rb[0])
        assert _rel(xa[b].cpu().numpy(), xb[0].cpu().numpy()) <= bound


CALLS = ([5, 0, 23], [1, 7, 18], [20, 20, 20])


@pytest.mark.parametrize("family", ["llama", "opt"])
def test_mixed_and_unequal_calls(family):
    """a 3-row state: counts [5, 0, 23], then [1, 7, 18] (n = 18: row 1 starts its sequence, the counts are unequal), then
    [20, 20, 20].  Each row's logits at its real positions agree, within the bound, with the same row run alone in a B = 1 state with
    the same per-row schedule; the lengths end at [26, 27, 61]."""
    import torch
    from mi355q import harness as H
    bound = _bound(family)
    model, _ = _model(family, 2, max_positions=64)
    model = model.to(DEV)
    toks = _ids(seed=11, B=3, T=61).to(DEV)
    state = H.DecodeState(model, 3, 64, "block_fp", extend=True)
    at, got = [0, 0, 0], []
    with torch.no_grad():
        for counts in CALLS:
            n = max(counts)
            ids = torch.zeros(3, n, dtype=toks.dtype, device=DEV)
            for b, c in enumerate(counts):
                ids[b, :c] = toks[b, at[b]:at[b] + c]
                at[b] += c
            got.append(model(ids, cache=state, counts=counts)[0])
            assert state.lengths == at
        assert state.lengths == [26, 27, 61]
        for b in range(3):
            alone, p = H.DecodeState(model, 1, 64, "block_fp", extend=True), 0
            for call, counts in enumerate(CALLS):
                c = counts[b]
                if c == 0:
                    continue
                one = model(toks[b:b + 1, p:p + c], cache=alone)[0][0].cpu().numpy()
                p += c
                err = _rel(got[call][b, :c].cpu().numpy(), one)
                print(family, "row", b, "call", call, "batched vs alone", err)
                assert err <= bound, (b, call, err, bound)
            assert alone.length == state.lengths[b]


def test_the_default_state_still_refuses():
    """DecodeState(model, 3, 48, "block_fp") raises the three NotImplementedErrors as before and leaves every cache byte as it was
    (tests/test_gpu_decode_ragged_model.py's check, on purpose a second time: the default must not move)"""
    import torch
    from mi355q import harness as H
    model, _ = _model("llama", 2)
    model = model.to(DEV)
    ids = _ids(seed=11, B=3, T=23).to(DEV)
    with torch.no_grad():
        state = H.DecodeState(model, 3, 48, "block_fp")
        model(ids, cache=state, counts=[5, 0, 23])
        assert state.lengths == [5, 0, 23]
        held = _cache_bytes(state)
        with pytest.raises(NotImplementedError, match="mixed"):
            model(ids[:, :1], cache=state, counts=[1, 1, 1])
        with pytest.raises(NotImplementedError, match="at most 16"):
            model(ids[:, :17], cache=state, counts=[17, 0, 17])
        with pytest.raises(NotImplementedError, match="unequal"):
            model(ids[:, :2], cache=state, counts=[2, 0, 1])
        assert state.lengths == [5, 0, 23]
        for a, b in zip(held, _cache_bytes(state)):
            assert torch.equal(a, b)
        uniform = H.DecodeState(model, 3, 48, "block_fp")
        model(ids[:, :5], cache=uniform)
        held = _cache_bytes(uniform)
        with pytest.raises(NotImplementedError, match="at most 16"):
            model(ids[:, 5:22], cache=uniform)
        assert uniform.length == 5 and all(c.length == 5 for c in uniform.kv)
        for a, b in zip(held, _cache_bytes(uniform)):
            assert torch.equal(a, b)


def test_a_refused_call_on_an_extend_state_writes_nothing():
    import torch
    from mi355q import harness as H
    model, _ = _model("llama", 2)
    model = model.to(DEV)
    ids = _ids(seed=11, B=3, T=26).to(DEV)
    with torch.no_grad():
        state = H.DecodeState(model, 3, 48, "block_fp", extend=True)
        model(ids[:, :23], cache=state, counts=[5, 0, 23])
        held = _cache_bytes(state)
        with pytest.raises(ValueError, match="exceed the capacity"):
            model(ids, cache=state, counts=[20, 20, 26])           # 23 + 26 > 48
        assert state.lengths == [5, 0, 23] and state._call is None
        for a, b in zip(held, _cache_bytes(state)):
            assert torch.equal(a, b)
        model(ids[:, :18], cache=state, counts=[1, 7, 18])         # the state is still usable: the extend route
        assert state.lengths == [6, 7, 41]
