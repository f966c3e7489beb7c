"""Fork and reorder through the harness models: PagedDecodeState.fork / .reorder and harness.beam_search on the tiny Llama and OPT models
(one and two layers) and a grouped-query Llama.  A reordered batch must give every row the logits its LINEAGE gives when it is decoded
alone; the models, the configs and the bound are those of tests/test_gpu_decode_ragged_model.py (formed there, in the test run: twice
the worst difference of the one-layer fp32 route from the oracle, floor 1e-3)."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_gpu_decode_ragged_model import DEV, W6, _bound, _model, _rel  # noqa: E402

pytestmark = pytest.mark.gpu
PROMPT, STEPS, SEQS, P = 21, 14, 4, 32
# after every step: a swap, a duplication and an identity, at changing rows
BEAMS = ([1, 0, 2, 2], [0, 2, 1, 1], [3, 1, 1, 0])


def _gqa_llama():
    import torch
    from mi355q import harness as H
    torch.manual_seed(0)
    cfg = H.TinyLlamaConfig(vocab_size=97, hidden_size=128, intermediate_size=256, num_layers=2, num_heads=4, max_positions=48, num_kv_heads=2)
    model = H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(dict(W6), 2))
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.ndim == 2 and "embed" not in n:
                p.mul_(4.0)
    return model


def _build(family, layers):
    return (_gqa_llama() if family == "gqa" else _model(family, layers)[0]).to(DEV), _bound("llama" if family == "gqa" else family)


def _alone(model, tokens):
    """the lineage `tokens` (the prompt's 21, then one a step) in a one-sequence paged state -> the logits of every step"""
    import torch
    from mi355q import harness as H
    state = H.PagedDecodeState(model, 1, PROMPT + STEPS, page_size=P)
    ids = torch.tensor(tokens, device=DEV)[None]
    model(ids[:, :PROMPT], cache=state)
    return [model(ids[:, t:t + 1], cache=state)[0][0, -1] for t in range(PROMPT, len(tokens))]


@pytest.mark.parametrize("family,layers", [("llama", 1), ("llama", 2), ("opt", 1), ("opt", 2), ("gqa", 2)])
def test_every_row_of_a_reordered_batch_decodes_as_its_lineage_alone(family, layers):
    """Four sequences: a prefill of 21 planted tokens each, then 14 steps of one planted token a row, each followed by reorder(beam_idx)
    with a swap, a duplication and an identity.  The tokens are given, not picked from the logits: no tie can steer the test.  Every
    row's logits at every step against its lineage -- the prompt it descends from and the tokens fed along the way -- decoded alone in
    a one-sequence PagedDecodeState on the same schedule (21, then one a call).  The rows run 21 .. 35 keys: over the page edge at 32,
    with a partial page at every reorder but that one.  Not bitwise: the Linears' route depends on the batch's shape.
    Measured on an MI355X, worst over rows and steps: see the print below (CHANGELOG: copy-on-write)."""
    import torch
    from mi355q import harness as H
    model, (e1, bound) = _build(family, layers)
    g = torch.Generator().manual_seed(11)
    prompts = torch.randint(0, 97, (SEQS, PROMPT), generator=g)
    fed = torch.randint(0, 97, (STEPS, SEQS), generator=g)
    # (the pool: every cache row -- 4 sequences x 2 KV heads -- at its 2 pages, and the page a row a reorder draws before it gives any back)
    state = H.PagedDecodeState(model, SEQS, PROMPT + STEPS, page_size=P, num_pages=SEQS * 2 * 3)
    lineage, seen = [prompts[b].tolist() for b in range(SEQS)], {}
    with torch.no_grad():
        model(prompts.to(DEV), cache=state)
        for s in range(STEPS):
            out = model(fed[s].to(DEV)[:, None], cache=state)[0][:, -1]
            lineage = [l + [int(fed[s, b])] for b, l in enumerate(lineage)]
            assert state.lengths == [PROMPT + s + 1] * SEQS
            for b in range(SEQS):
                seen[tuple(lineage[b])] = out[b].cpu().numpy()
            idx = BEAMS[s % len(BEAMS)]
            state.reorder(idx)
            lineage = [list(lineage[i]) for i in idx]
        # every lineage alone: the longest first, which serves its ancestors' steps as well
        alone, worst = {}, 0.0
        for key in sorted(seen, key=len, reverse=True):
            if key not in alone:
                for t, logits in enumerate(_alone(model, list(key))):
                    alone[key[:PROMPT + t + 1]] = logits.cpu().numpy()
        for key, got in seen.items():
            err = _rel(got, alone[key])
            worst = max(worst, err)
            assert err <= bound, (family, layers, "step", len(key) - PROMPT - 1, err, bound)
    print(family, layers, "one-layer fp32 route vs oracle", e1, "bound", bound, "reordered batch vs lineage alone, worst over rows and steps",
          worst, "lineages", len(seen))
    assert len(seen) > STEPS * 3                                  # (the duplications leave two rows with one lineage for a step at most)
    for c in state.kv:                                            # shared pages are counted once a holder ...
        assert sum(c.refs) == sum(1 for row in c.held for p in row if p is not None)
    for b in range(SEQS):
        state.release(b)
    for c in state.kv:                                            # ... and everything comes back
        assert sorted(c.free) == list(range(c.num_pages)) and not any(c.refs)


@pytest.mark.parametrize("family", ["llama", "opt"])
def test_one_beam_is_greedy_decoding(family):
    """beam_search(num_beams=1) on a list of prompts returns generate(page_size=32)'s tokens: both take the ragged paged route"""
    import torch
    from mi355q import harness as H
    model, _ = _build(family, 2)
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(0, 97, (n,), generator=g).to(DEV) for n in (5, 16, 23)]
    rows, logits = H.generate(model, prompts, 10, page_size=P)
    ids, scores = H.beam_search(model, prompts, 10, 1, page_size=P)
    assert [tuple(i.shape) for i in ids] == [(1, n + 10) for n in (5, 16, 23)] and tuple(scores.shape) == (3, 1)
    for b, r in enumerate(rows):
        assert torch.equal(ids[b][0], r), f"prompt {b}: {ids[b][0].tolist()} is not the greedy {r.tolist()}"
    greedy = torch.log_softmax(logits.float(), -1).max(-1).values.sum(-1)
    assert torch.allclose(scores[:, 0], greedy, rtol=0, atol=1e-4)


@pytest.mark.parametrize("family,ragged", [("llama", True), ("opt", False), ("gqa", True)])
def test_beam_scores_are_the_sequences_log_probabilities(family, ragged, monkeypatch):
    """beam_search(num_beams=3), 10 new tokens: each returned score against the sum of log-probabilities of that returned sequence
    teacher-forced ALONE (a one-sequence paged state: its prompt, then one token a call), within the logit bound times the 10 steps;
    scores sorted, beams distinct, the prompts kept; and afterwards every page of every layer is free."""
    import torch
    from mi355q import harness as H
    model, (e1, bound) = _build(family, 2)
    made = []

    class Recorded(H.PagedDecodeState):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(H, "PagedDecodeState", Recorded)
    g = torch.Generator().manual_seed(7)
    new, nb = 10, 3
    prompts = [torch.randint(0, 97, (n,), generator=g).to(DEV) for n in ((7, 21) if ragged else (9, 9))]
    ids, scores = H.beam_search(model, prompts if ragged else torch.stack(prompts), new, nb, page_size=P)
    state, = made
    monkeypatch.undo()
    assert tuple(scores.shape) == (2, nb) and bool((scores[:, :-1] >= scores[:, 1:]).all()), scores
    if not ragged:
        assert tuple(ids.shape) == (2, nb, 9 + new)
    worst = 0.0
    with torch.no_grad():
        for b, p in enumerate(prompts):
            n = p.numel()
            assert tuple(ids[b].shape) == (nb, n + new) and bool((ids[b][:, :n] == p).all())
            assert len({tuple(r.tolist()) for r in ids[b]}) == nb, "two beams hold one sequence"
            for j in range(nb):
                one = H.PagedDecodeState(model, 1, n + new, page_size=P)
                seq = ids[b][j][None]
                logits = [model(seq[:, :n], cache=one)[0][0, -1]] + [model(seq[:, t:t + 1], cache=one)[0][0, -1] for t in range(n, n + new - 1)]
                logp = torch.log_softmax(torch.stack(logits).float(), -1)
                want = float(logp[torch.arange(new, device=DEV), seq[0, n:]].sum())
                err = abs(float(scores[b, j]) - want)
                worst = max(worst, err)
                assert err <= bound * new, (family, b, j, float(scores[b, j]), want, bound)
    print(family, "beam scores vs teacher-forced alone, worst", worst, "bound x steps", bound * new)
    for c in state.kv:
        assert sorted(c.free) == list(range(c.num_pages)) and not any(c.refs) and all(h == [] for h in c.held)
