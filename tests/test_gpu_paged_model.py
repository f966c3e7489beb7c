"""The harness models on paged caches (harness.PagedDecodeState(page_size=32)): TinyOPT, TinyLlama, and TinyLlama with 4 heads on 2 KV
heads, two layers each.  A paged state and a contiguous one are driven through the SAME counts= calls; the logits of every real
position of every call must be equal bit for bit -- paging changes where the cache's pieces lie, nothing else."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W6 = dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
          data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127,
          weight_block_size=[1, 16], bias_width=6, bias_exponent_width=8, bias_exponent_bias=127, bias_block_size=[16])
BATCH, CAPACITY, VOCAB = 3, 64, 97


@pytest.fixture(scope="module", params=["opt", "llama", "llama_gqa"])
def model(request):
    import torch
    from mi355q import harness as H
    torch.manual_seed(0)
    if request.param == "opt":
        cfg = H.TinyOPTConfig(vocab_size=VOCAB, hidden_size=128, ffn_dim=256, num_layers=2, num_heads=2, max_positions=64)
        m = H.TinyOPTForCausalLM(cfg, H.expand_quant_config(dict(W6), 2))
    else:
        heads = dict(num_heads=4, num_kv_heads=2) if request.param == "llama_gqa" else dict(num_heads=2)
        cfg = H.TinyLlamaConfig(vocab_size=VOCAB, hidden_size=128, intermediate_size=256, num_layers=2, max_positions=64, **heads)
        m = H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(dict(W6), 2))
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.ndim == 2 and "embed" not in n:
                p.mul_(4.0)
    return m.to(DEV)


def _ids(counts, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, VOCAB, (BATCH, max(counts)), generator=g).to(DEV)


def _call(model, states, counts, seed):
    """one counts= call on every state with the same tokens; asserts the real positions' logits equal bit for bit"""
    import torch
    ids = _ids(counts, seed)
    with torch.no_grad():
        outs = [model(ids, cache=s, counts=counts)[0] for s in states]
    for b, c in enumerate(counts):
        for o in outs[1:]:
            assert torch.equal(o[b, :c].contiguous().view(torch.uint8), outs[0][b, :c].contiguous().view(torch.uint8)), \
                f"call {seed}, counts {counts}: sequence {b} differs"
        assert c == 0 or bool(torch.isfinite(outs[0][b, :c]).all())
    assert states[0].lengths == states[1].lengths


def _kv_rows(state):
    return state.kv[0].B // BATCH


def test_prompts_a_chunk_and_decode_steps_bit_for_bit(model):
    """prompts of 5, 16 and 23 tokens (the ragged prefill), one chunked call of 17 tokens a row (the extend route), 12 decode steps
    that take sequence 0 over the page edge at 32 keys and sequence 1 to 45"""
    from mi355q import harness as H, ops
    paged = H.PagedDecodeState(model, BATCH, CAPACITY, extend=True, page_size=32)
    contig = H.DecodeState(model, BATCH, CAPACITY, extend=True)
    assert all(type(c) is ops.PagedKVCache for c in paged.kv) and all(type(c) is ops.KVCache for c in contig.kv)
    _call(model, (contig, paged), [5, 16, 23], 0)
    _call(model, (contig, paged), [17, 17, 17], 1)
    for t in range(12):
        _call(model, (contig, paged), [1, 1, 1], 2 + t)
    assert paged.lengths == [34, 45, 52]
    heads = _kv_rows(paged)
    assert all([len(h) for h in c.held] == [2] * (3 * heads) for c in paged.kv)


def test_continuous_batching_on_recycled_pages(model):
    """10 pages a layer where batch x capacity needs 12 (3 sequences x 2 KV rows x 2 pages).  Prompts 5 / 16 / 23, 12 steps; sequence 0
    finishes and is released; a new prompt of 20 tokens starts in slot 0 on the pages it gave back while the others take one token
    (the mixed route), then 8 more steps take sequences 1 and 2 into their second pages.  The contiguous state goes through the same
    schedule, with the same release."""
    from mi355q import harness as H
    heads = 2
    paged = H.PagedDecodeState(model, BATCH, CAPACITY, extend=True, page_size=32, num_pages=10)
    contig = H.DecodeState(model, BATCH, CAPACITY, extend=True)
    assert _kv_rows(paged) == heads and BATCH * heads * (CAPACITY // 32) > 10
    _call(model, (contig, paged), [5, 16, 23], 10)
    for t in range(12):
        _call(model, (contig, paged), [1, 1, 1], 11 + t)
    assert paged.lengths == [17, 28, 35] and all(len(c.free) == 10 - heads * 4 for c in paged.kv)
    first = [list(c.held[0]) + list(c.held[1]) for c in paged.kv]
    for s in (contig, paged):
        s.release(0)
    assert paged.lengths == contig.lengths == [0, 28, 35] and all(len(c.free) == 10 - heads * 3 for c in paged.kv)
    _call(model, (contig, paged), [20, 1, 1], 30)
    assert all(sorted(c.held[0] + c.held[1]) == sorted(f) for c, f in zip(paged.kv, first)), "slot 0 restarts on the pages it gave back"
    for t in range(8):
        _call(model, (contig, paged), [1, 1, 1], 31 + t)
    assert paged.lengths == [28, 37, 44] and all(len(c.free) == 0 for c in paged.kv)


def test_a_call_the_pool_cannot_serve_raises_before_any_cache_changes(model):
    """6 pages a layer: sequences 0 and 1 take 4; a call that gives sequence 2 a 33-token prompt needs 4 more and raises before any
    layer's table, free list or cache is touched -- the next valid call gives the logits of a contiguous state that never saw the
    refused call"""
    import torch
    from mi355q import harness as H
    paged = H.PagedDecodeState(model, BATCH, CAPACITY, extend=True, page_size=32, num_pages=6)
    contig = H.DecodeState(model, BATCH, CAPACITY, extend=True)
    _call(model, (contig, paged), [5, 30, 0], 50)
    snap = [(c.table.clone(), list(c.free), c.kq.clone(), c.vq.clone(), c.stage.clone()) for c in paged.kv]
    with pytest.raises(RuntimeError, match="need 4 more pages, 2 of 6 are free"):
        with torch.no_grad():
            model(_ids([0, 0, 33], 51), cache=paged, counts=[0, 0, 33])
    for c, (table, free, kq, vq, stage) in zip(paged.kv, snap):
        assert torch.equal(c.table, table) and torch.equal(c.block_table.cpu(), table) and c.free == free
        assert torch.equal(c.kq, kq) and torch.equal(c.vq, vq) and torch.equal(c.stage, stage)
    assert paged.lengths == [5, 30, 0] and paged._call is None
    _call(model, (contig, paged), [1, 3, 0], 52)               # sequence 1 crosses its page edge on a page that is still free
    _call(model, (contig, paged), [1, 1, 0], 53)
