"""harness.PagedPackedDecodeState and beam_search(kv_storage="int8") on the tiny models of tests/test_gpu_decode_ragged_model.py (Llama
and OPT, one and two layers) and the grouped-query Llama of tests/test_gpu_kv_fork_model.py, page_size 32: paged caches of int8 mantissas
give the logits, the tokens and the beam scores of the bf16 pages BIT FOR BIT -- the arithmetic is the same, only the storage of a
cached value and its place differ.  Every K / V row that reaches a packed cache is checked for the storage's one stated deviation, an
input 0 < |x| <= 1e-8 (none occurs), which is what makes bit equality a fair demand."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_gpu_decode_ragged_model import DEV, _model  # noqa: E402
from test_gpu_kv_fork_model import _gqa_llama  # noqa: E402

pytestmark = pytest.mark.gpu
P = 32
FAMILIES = [("llama", 1), ("llama", 2), ("opt", 1), ("opt", 2), ("gqa", 2)]
_MODELS = {}


def _build(family, layers):
    if (family, layers) not in _MODELS:
        _MODELS[(family, layers)] = (_gqa_llama() if family == "gqa" else _model(family, layers)[0]).to(DEV)
    return _MODELS[(family, layers)]


@pytest.fixture(autouse=True)
def no_tiny_inputs(monkeypatch):
    """every append into a PagedPackedKVCache: no value of magnitude 0 < |x| <= 1e-8 among its rows"""
    from mi355q import ops
    append = ops.PagedPackedKVCache.append

    def checked(self, k, v, **kw):
        for t in (k, v):
            a = t.abs()
            assert not bool(((a > 0) & (a <= 1e-8)).any()), "a K / V input of magnitude 0 < |x| <= 1e-8"
        return append(self, k, v, **kw)
    monkeypatch.setattr(ops.PagedPackedKVCache, "append", checked)


def _same(a, b, what):
    import torch
    assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), what


@pytest.mark.parametrize("family,layers", FAMILIES)
def test_ragged_prefill_decode_and_a_reused_slot(family, layers):
    """prompts of (21, 5, 16) tokens in one ragged prefill, 8 decode steps, release(1), a new sequence of 9 tokens prefilled into slot 1
    in a call where it is the only active row, and 3 more steps of all rows: at every call each row's logits are PagedDecodeState's
    bits.  The packed state holds 17/32 of the K / V bytes, and at the end every page of every layer is free."""
    import torch
    from mi355q import harness as H, ops
    model = _build(family, layers)
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, 97, (3, 40), generator=g).to(DEV)
    new, old = H.PagedPackedDecodeState(model, 3, 40, page_size=P), H.PagedDecodeState(model, 3, 40, page_size=P)
    assert all(type(c) is ops.PagedPackedKVCache for c in new.kv) and all(type(c) is ops.PagedKVCache for c in old.kv)
    for c8, c16 in zip(new.kv, old.kv):
        assert (c8.k8.numel() + c8.v8.numel()) * 32 == (c16.kq.numel() + c16.vq.numel()) * 17
    calls = [(ids[:, :21], (21, 5, 16))] + [(ids[:, 21 + s:22 + s], (1, 1, 1)) for s in range(8)]
    with torch.no_grad():
        def run(tokens, counts):
            a = model(tokens, cache=new, counts=list(counts))[0]
            b = model(tokens, cache=old, counts=list(counts))[0]
            assert bool(torch.isfinite(a).all())
            for row, c in enumerate(counts):
                _same(a[row, :c], b[row, :c], f"{family} x {layers}: row {row} differs at counts {counts}")
            assert new.lengths == old.lengths
            for c8, c16 in zip(new.kv, old.kv):
                assert c8.held == c16.held and c8.free == c16.free
        for tokens, counts in calls:
            run(tokens, counts)
        assert new.lengths == [29, 13, 24]
        for state in (new, old):
            state.release(1)
        run(ids[:, 30:39], (0, 9, 0))
        for s in range(3):
            run(ids[:, 39 - s:40 - s], (1, 1, 1))
        assert new.lengths == [32, 12, 27]
    for b in range(3):
        new.release(b)
    for c in new.kv:
        assert sorted(c.free) == list(range(c.num_pages)) and not any(c.refs) and all(h == [] for h in c.held)


@pytest.mark.parametrize("family", ["llama", "opt"])
def test_one_beam_is_greedy_decoding(family):
    """beam_search(num_beams=1, kv_storage="int8") returns generate(page_size=32)'s tokens"""
    import torch
    from mi355q import harness as H
    model = _build(family, 2)
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(0, 97, (n,), generator=g).to(DEV) for n in (5, 16, 23)]
    rows, _ = H.generate(model, prompts, 10, page_size=P)
    ids, scores = H.beam_search(model, prompts, 10, 1, page_size=P, kv_storage="int8")
    assert tuple(scores.shape) == (3, 1)
    for b, r in enumerate(rows):
        assert torch.equal(ids[b][0], r), f"prompt {b}: {ids[b][0].tolist()} is not the greedy {r.tolist()}"


@pytest.mark.parametrize("family,ragged", [("llama", True), ("opt", False), ("gqa", True)])
def test_three_beams_are_the_bf16_pages_beams(family, ragged, monkeypatch):
    """beam_search(num_beams=3), 10 new tokens: ids and scores bit-equal to the search on bf16 pages; afterwards every page of every layer
    of the packed state is free"""
    import torch
    from mi355q import harness as H, ops
    model = _build(family, 2)
    made = []

    class Recorded(H.PagedPackedDecodeState):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(H, "PagedPackedDecodeState", Recorded)
    g = torch.Generator().manual_seed(7)
    prompts = [torch.randint(0, 97, (n,), generator=g).to(DEV) for n in ((7, 21) if ragged else (9, 9))]
    given = prompts if ragged else torch.stack(prompts)
    ids8, scores8 = H.beam_search(model, given, 10, 3, page_size=P, kv_storage="int8")
    ids16, scores16 = H.beam_search(model, given, 10, 3, page_size=P)
    state, = made
    assert all(type(c) is ops.PagedPackedKVCache for c in state.kv)
    _same(scores8, scores16, f"{family}: the beam scores differ")
    for a, b in zip(ids8, ids16):
        assert torch.equal(a, b), f"{family}: the beams differ"
    for c in state.kv:
        assert sorted(c.free) == list(range(c.num_pages)) and not any(c.refs) and all(h == [] for h in c.held)
