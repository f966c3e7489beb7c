"""A sliding-window TinyLlama (2 layers, 4 heads / 2 KV heads, 48 positions, sliding_window 12): the block_fp cache route against the
fp32 route, whose additive mask carries the window (the reference's literal route), the full forward with the window mask, paged
generation on a pool too small for the unwindowed sequence, and the configurations that must not change: a window over every position
and the default config."""
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
PROMPT, STEPS, WINDOW = 21, 14, 12


def _model(layers, window, seed=0, scale=4.0):
    import torch
    from mi355q import harness as H
    torch.manual_seed(seed)
    cfg = H.TinyLlamaConfig(vocab_size=97, hidden_size=128, intermediate_size=256, num_layers=layers, num_heads=4, max_positions=48,
                            sliding_window=window, num_kv_heads=2)
    model = H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(dict(W6), layers))
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.ndim == 2 and "embed" not in n:
                p.mul_(scale)
    return model.to(DEV)


def _ids(seed=5, B=2):
    import torch
    return torch.randint(0, 97, (B, PROMPT + STEPS + 1), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _teacher_forced(model, ids, mode):
    """-> logits [B, STEPS + 1, V]: the prompt's last position (a prompt longer than the window), then one teacher-forced token a step"""
    import torch
    from mi355q import harness as H
    state = H.DecodeState(model, ids.shape[0], ids.shape[1], mode)
    assert state.window == model.cfg.sliding_window
    with torch.no_grad():
        out = [model(ids[:, :PROMPT], cache=state)[0][:, -1]]
        for t in range(PROMPT, PROMPT + STEPS):
            out.append(model(ids[:, t:t + 1], cache=state)[0][:, -1])
    return torch.stack(out, 1).cpu().numpy()


def _full(model, ids):
    """the full forward's last-position logits on ids[:, :t + 1], per step"""
    import torch
    with torch.no_grad():
        return np.stack([model(ids[:, :t + 1])[0][:, -1].cpu().numpy() for t in range(PROMPT - 1, PROMPT + STEPS)], 1)


def _rel(a, ref):
    return float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max()))


@pytest.fixture(scope="module")
def bound():
    """as tests/test_gpu_gqa_model.py forms it: e1 = the worst relative logit difference of the mode "fp32" route from the full forward on
    the ONE-layer model; 2 e1, floor 1e-3"""
    m1, ids = _model(1, WINDOW), _ids()
    a, ref = _teacher_forced(m1, ids, "fp32"), _full(m1, ids)
    e1 = max(_rel(a[:, s], ref[:, s]) for s in range(STEPS + 1))
    print("one-layer fp32 route vs full forward", e1)
    return max(2 * e1, 1e-3)


@pytest.fixture(scope="module")
def two_layers():
    return _model(2, WINDOW), _ids()


def test_window_changes_the_logits(two_layers):
    """(the test would be empty if the window did nothing: at 21 .. 35 positions a 12-key window moves the logits)"""
    model, ids = two_layers
    a = _teacher_forced(model, ids, "block_fp")
    b = _teacher_forced(_model(2, None), ids, "block_fp")
    assert _rel(a, b) > 1e-2


def test_cached_routes_agree(two_layers, bound):
    import torch
    from mi355q import harness as H
    model, ids = two_layers
    a, b = _teacher_forced(model, ids, "block_fp"), _teacher_forced(model, ids, "fp32")
    worst = max(_rel(a[:, s], b[:, s]) for s in range(STEPS + 1))
    print("bound", bound, "block_fp vs fp32", worst)
    assert worst <= bound
    # greedy generation: equal ids wherever the fp32 route's top-2 gap exceeds twice the bound in logit units
    ia, la = H.generate(model, ids[:, :PROMPT], STEPS, mode="block_fp")
    ib, lb = H.generate(model, ids[:, :PROMPT], STEPS, mode="fp32")
    top2 = torch.topk(lb, 2, dim=-1).values
    gap = float((top2[..., 0] - top2[..., 1]).min())
    need = 2 * bound * max(1.0, float(lb.abs().max()))
    print("smallest top-2 gap", gap, "needed", need)
    assert gap > need, "the prompt does not separate the top two tokens: choose another seed"
    assert torch.equal(ia, ib)


def test_full_forward_agrees_with_the_cached_route(two_layers, bound):
    """the full forward with the window mask on T tokens against the cached route given the same T tokens in one call (T > W: the
    windowed extend kernel behind its own append), at the last position, both modes; and, on a ONE-layer model, against every
    teacher-forced step of the cached route.
    Not compared: the two-layer model's teacher-forced steps.  There the cached route and the full forward differ by 0.05 - 0.11 of
    the largest logit with sliding_window = 12 AND by 0.04 - 0.07 with sliding_window = None (measured on an MI355X, mode "fp32", steps
    1 .. 14; step 0 and the one-layer model: 0.0): a key's 16-key block of K^T is quantised with the keys the cache held when an earlier
    token's query ran, in the full forward with all T keys -- the reference's `past_key_value` semantics, window or not."""
    import torch
    from mi355q import harness as H
    model, ids = two_layers
    for T in (PROMPT, PROMPT + STEPS):
        with torch.no_grad():
            ref = model(ids[:, :T])[0][:, -1].cpu().numpy()
            for mode in ("block_fp", "fp32"):
                got = model(ids[:, :T], cache=H.DecodeState(model, ids.shape[0], T, mode))[0][:, -1].cpu().numpy()
                print("T", T, mode, "cached prompt vs full forward", _rel(got, ref))
                assert _rel(got, ref) <= bound, (T, mode)
    m1 = _model(1, WINDOW)
    a, ref = _teacher_forced(m1, ids, "block_fp"), _full(m1, ids)
    worst = max(_rel(a[:, s], ref[:, s]) for s in range(STEPS + 1))
    print("bound", bound, "one layer, block_fp cached vs full forward", worst)
    assert worst <= bound


def test_chunked_prefill_is_windowed(two_layers, bound):
    """the prompt in chunks through a state with extend=True: chunks of 8 take the windowed decode kernel, chunks of 17 the windowed
    extend kernel (the first from an empty cache, 17 > W).  The reference is mode "fp32" fed the SAME chunks: a chunked call sees K^T's
    open block as it was at its time, so the unchunked route is another computation (test_full_forward_agrees_with_the_cached_route)"""
    from mi355q import harness as H
    model, ids = two_layers
    for chunk in (8, 17):
        ref = H.generate(model, ids[:, :PROMPT + 8], 4, mode="fp32", chunk=chunk)[1].cpu().numpy()
        got = H.generate(model, ids[:, :PROMPT + 8], 4, mode="block_fp", chunk=chunk)[1].cpu().numpy()
        print("chunk", chunk, "block_fp vs fp32", _rel(got, ref))
        assert _rel(got, ref) <= bound, chunk


def test_paged_generate_on_a_small_pool(two_layers):
    """prompts of 31 and 19 tokens, 17 new ones: row 0 crosses into its second page at 33 and lets the first go at 43 (12-key window),
    row 1 needs its second page at 33, three steps later.  6 pages (2 KV heads x 3) serve that; the unwindowed model needs 8"""
    import torch
    from mi355q import harness as H
    model, ids = two_layers
    prompts = [ids[0, :31], ids[1, :19]]
    ref_ids, ref_logits = H.generate(model, prompts, 17, mode="block_fp")
    got_ids, got_logits = H.generate(model, prompts, 17, mode="block_fp", page_size=32, num_pages=6)
    assert all(torch.equal(a, b) for a, b in zip(got_ids, ref_ids))
    assert torch.equal(got_logits.view(torch.uint8), ref_logits.view(torch.uint8))
    with pytest.raises(RuntimeError, match="more pages"):
        H.generate(_model(2, None), prompts, 17, mode="block_fp", page_size=32, num_pages=6)


def test_window_over_every_position_and_default_config(two_layers):
    """sliding_window=64 >= max_positions: the logits of sliding_window=None, bit for bit, cached and full"""
    import torch
    _, ids = two_layers
    none, wide = _model(2, None), _model(2, 64)
    for mode in ("block_fp", "fp32"):
        assert np.array_equal(_teacher_forced(none, ids, mode).view(np.uint32), _teacher_forced(wide, ids, mode).view(np.uint32)), mode
    with torch.no_grad():
        assert torch.equal(none(ids[:, :40])[0], wide(ids[:, :40])[0])
