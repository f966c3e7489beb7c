"""Copy-on-write for the paged block_fp KV cache on the host: the planner behind ops.PagedKVCache.fork / .reorder (pure: it reads no GPU,
so a "cpu" cache runs it), what a refused call leaves behind, the argument check of mi355q_bfp_kv_paged_copy, and the refusals of the
harness -- a machine without a GPU runs all of this, in the manner of tests/test_paged_host.py."""
import ctypes
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))

P6 = (6, 8, 127, 6, 8, 127)
W6 = dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
          data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127,
          weight_block_size=[1, 16], bias_width=6, bias_exponent_width=8, bias_exponent_bias=127, bias_block_size=[16])
LENGTHS, SRC = (37, 64, 5, 0), (2, 0, 0, 3)


def _cache(num_pages=12, lengths=LENGTHS):
    from mi355q import ops
    c = ops.PagedKVCache(4, 32, P6, P6, "cpu", page_size=32, num_pages=num_pages, max_pages=4)
    c.ensure(lengths)
    return c


def _snapshot(c):
    return c.table.clone(), c.block_table.clone(), list(c.free), list(c.refs), [list(h) for h in c.held]


def _same(c, snap):
    import torch
    return (torch.equal(c.table, snap[0]) and torch.equal(c.block_table, snap[1]) and c.free == snap[2] and c.refs == snap[3]
            and [list(h) for h in c.held] == snap[4])


def _plan(c, src_rows, lengths):
    return c._plan_copy([(b, s, lengths[s]) for b, s in enumerate(src_rows)])


def test_the_export_exists_and_the_abi_stays_25():
    from mi355q import _lib
    header = (ROOT / "include" / "mi355q.h").read_text()
    lib = _lib.load_library()
    name = "mi355q_bfp_kv_paged_copy"
    assert re.search(r"\b%s\s*\(" % name, header), f"{name} not declared"
    assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} not bound / exported"
    assert lib.mi355q_abi_version() == _lib.ABI_VERSION == 25
    assert int(re.search(r"#define MI355Q_ABI_VERSION (\d+)", header).group(1)) == 25


def test_the_export_refuses_bad_arguments_without_a_gpu():
    from mi355q import _lib
    lib = _lib.load_library()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    q = p + 1024

    def call(kq=p, vq=p, src=p, dst=q, jobs=p, n=3, B=4, num_pages=12, P=32, D=32):
        return lib.mi355q_bfp_kv_paged_copy(kq, vq, src, dst, jobs, n, B, num_pages, P, D, None)

    # nothing to do: success with every pointer NULL, and no launch (there is no GPU here to launch on)
    assert call(kq=None, vq=None, src=None, dst=None, jobs=None, n=0) == 0
    for name in ("kq", "vq", "src", "dst", "jobs"):
        assert call(**{name: None}) == _lib.E_BADARG, name
    for bad_p in (0, 16, 48, 33, -32, 96):
        assert call(P=bad_p) == _lib.E_BADARG, bad_p
        assert call(P=bad_p, n=0) == _lib.E_BADARG, bad_p
    for bad_d in (0, 16, 48, 160, -32):
        assert call(D=bad_d) == _lib.E_BADARG, bad_d
    assert call(dst=p) == _lib.E_BADARG                       # stage_src == stage_dst: never in place
    assert call(n=-1) == _lib.E_BADARG
    assert call(B=0) == call(num_pages=0) == _lib.E_BADARG
    assert call(n=65536) == _lib.E_UNSUPPORTED                # one launch: the grid's second dimension
    for name in ("kq", "vq", "src", "dst", "jobs"):
        assert call(**{name: p + 8}) == _lib.E_ALIGN, name


def test_plan_of_a_reorder_shares_full_pages_and_draws_a_private_page_per_partial_row():
    c = _cache()
    h = [list(r) for r in c.held]
    assert [len(r) for r in h] == [2, 2, 1, 0]
    snap, free = _snapshot(c), list(c.free)
    plan = _plan(c, SRC, LENGTHS)
    assert _same(c, snap), "the planner changed the cache"
    # rows 0 (<- 2: 5 keys), 1 and 2 (<- 0: 37 keys) have a partial page: three draws, from the end of the free list, in row order
    assert plan.drawn == [free[-1], free[-2], free[-3]]
    assert plan.held == {0: [plan.drawn[0]], 1: [h[0][0], plan.drawn[1]], 2: [h[0][0], plan.drawn[2]], 3: []}
    assert plan.jobs == [(h[2][0], plan.drawn[0], 2, 0), (h[0][1], plan.drawn[1], 0, 1), (h[0][1], plan.drawn[2], 0, 2)]   # row 3 (0 keys): nothing
    assert all(j[0] != j[1] for j in plan.jobs) and not {j[1] for j in plan.jobs} & {j[0] for j in plan.jobs}
    # row 0's full page is held twice; its partial page, all of row 1 and row 2's page have no holder left
    want = [0] * 12
    want[h[0][0]] = 2
    for p in plan.drawn:
        want[p] = 1
    assert plan.refs == want and plan.freed == [h[0][1], h[1][0], h[1][1], h[2][0]]
    # a page-aligned source: no page job, still a stage job; an identity row with a partial page of its own keeps it
    plan = _plan(c, (1, 1, 2, 3), LENGTHS)
    assert plan.jobs == [(-1, -1, 1, 0), (-1, -1, 1, 1), (-1, -1, 2, 2)] and plan.drawn == []
    assert plan.held == {0: h[1], 1: h[1], 2: h[2], 3: []} and plan.freed == h[0]
    assert [plan.refs[p] for p in h[1] + h[2]] == [2, 2, 1]
    # ... unless another row holds that page too (then it is no longer private: the copy is drawn)
    c.refs[h[2][0]] = 2
    assert _plan(c, (0, 1, 2, 3), LENGTHS).jobs[2] == (h[2][0], free[-1], 2, 2)
    c.refs[h[2][0]] = 1
    with pytest.raises(ValueError, match="row 2 holds 1 pages, not the 2 of 40 keys"):
        _plan(c, (2, 1, 2, 3), (37, 64, 40, 0))
    with pytest.raises(ValueError, match="not distinct dst rows"):
        c._plan_copy([(0, 1, 64), (0, 2, 5)])


def test_commit_then_release_frees_every_page_exactly_once():
    import torch
    c = _cache()
    plan = _plan(c, SRC, LENGTHS)
    c._commit_plan(plan)
    assert [list(r) for r in c.held] == [plan.held[b] for b in range(4)] and c.refs == plan.refs
    for b, row in enumerate(c.held):
        assert c.table[b, :len(row)].tolist() == row and bool((c.table[b, len(row):] == c.pad_page).all())
    assert torch.equal(c.block_table, c.table)
    used = {p for row in c.held for p in row}
    assert not used & set(c.free) and sorted(list(used) + c.free) == list(range(12)) and len(set(c.free)) == len(c.free)
    c.release(range(4))
    assert sorted(c.free) == list(range(12)) and len(c.free) == 12 and c.refs == [0] * 12 and all(r == [] for r in c.held)


def test_a_pool_short_by_one_page_refuses_before_anything_changes():
    c = _cache(num_pages=7)                                   # 5 pages held, 2 free, the reorder draws 3
    snap = _snapshot(c)
    for call in (lambda: c.reorder(SRC, LENGTHS), lambda: c.reorder(SRC, LENGTHS, dry_run=True), lambda: _plan(c, SRC, LENGTHS)):
        with pytest.raises(RuntimeError, match=r"rows \[0, 1, 2\] need 3 more pages, 2 of 7 are free"):
            call()
        assert _same(c, snap), "a refused reorder changed the table, the mirror, the free list, the counts or the held lists"
    c = _cache(num_pages=8)
    snap = _snapshot(c)
    c.reorder(SRC, LENGTHS, dry_run=True)                     # one more page: the checks pass, and a dry run changes nothing
    assert _same(c, snap)
    with pytest.raises(ValueError, match="no CPU fallback"):  # the launch is the GPU's: refused BEFORE the host state changes
        c.reorder(SRC, LENGTHS)
    assert _same(c, snap)
    with pytest.raises(ValueError, match="3 source rows and 4 lengths for 4 cache rows"):
        c.reorder((0, 1, 2), LENGTHS)
    with pytest.raises(ValueError, match="outside 0 .. 3"):
        c.reorder((0, 1, 2, 4), LENGTHS)


def test_fork_wants_an_empty_row_and_carries_a_trimmed_prefix_over():
    c = _cache()
    snap = _snapshot(c)
    with pytest.raises(ValueError, match=r"rows \[1\] hold pages"):
        c.fork(0, 1, 37)
    with pytest.raises(ValueError, match="their own source"):
        c.fork(3, 3, 0)
    with pytest.raises(ValueError, match="row 2 holds 1 pages, not the 2 of 33 keys"):
        c.fork(2, 3, 33)
    with pytest.raises(ValueError, match="no CPU fallback"):
        c.fork(0, 3, 37)
    c.fork(0, 3, 37, dry_run=True)
    assert _same(c, snap)
    h = [list(r) for r in c.held]
    plan = c._plan_copy([(3, 0, 37)], "fork")
    assert plan.held == {3: [h[0][0], c.free[-1]]} and plan.jobs == [(h[0][1], c.free[-1], 0, 3)] and plan.freed == []
    assert plan.refs[h[0][0]] == 2 and plan.refs[h[0][1]] == 1 and plan.refs[c.free[-1]] == 1
    # a sliding-window row: its first page went back to the pool (trim); the fork holds None in its place and counts nothing for it
    c.trim([37, 64, 5, 0], window=4)
    assert c.held[0] == [None, h[0][1]] and c.held[1] == [None, h[1][1]]
    plan = c._plan_copy([(3, 0, 37)], "fork")
    assert plan.held == {3: [None, c.free[-1]]} and plan.jobs == [(h[0][1], c.free[-1], 0, 3)]
    c._commit_plan(plan)
    assert c.held[3][0] is None and c.table[3].tolist() == [c.pad_page, c.held[3][1], c.pad_page, c.pad_page]
    assert sum(c.refs) == 4 and len(c.free) == 12 - 4
    c.release(range(4))
    assert sorted(c.free) == list(range(12)) and c.refs == [0] * 12
    # a trimmed PARTIAL page cannot be forked (the harness never trims it: it is the newest)
    c = _cache()
    c.held[2][0] = None
    with pytest.raises(ValueError, match="partial page .* is trimmed"):
        c._plan_copy([(3, 2, 5)], "fork")


def _tiny():
    import torch
    from mi355q import harness as H
    torch.manual_seed(3)
    cfg = H.TinyLlamaConfig(vocab_size=64, hidden_size=128, intermediate_size=256, num_layers=2, num_heads=4, max_positions=64, num_kv_heads=2)
    return H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(dict(W6), 2))


def test_an_unpaged_state_refuses_by_name_and_a_paged_one_checks_every_layer_first():
    import torch
    from mi355q import harness as H
    model = _tiny()
    for state in (H.DecodeState(model, 4, 40), H.PagedDecodeState(model, 4, 40)):
        with pytest.raises(NotImplementedError, match="page_size"):
            state.fork(0, 1)
        with pytest.raises(NotImplementedError, match="page_size"):
            state.reorder([0, 1, 2, 3])
    with pytest.raises(NotImplementedError, match="page_size"):
        H.beam_search(model, torch.zeros(2, 5, dtype=torch.long), 4, 3, page_size=None)
    with pytest.raises(ValueError, match="num_beams = 65 outside"):
        H.beam_search(model, torch.zeros(2, 5, dtype=torch.long), 4, 65)
    # 4 sequences x 2 KV heads; sequences 0 and 1 at 37 and 5 keys.  Layer 1's pool is one page short of the reorder: no layer changes
    paged = H.PagedDecodeState(model, 4, 40, page_size=32, num_pages=12)
    for c in paged.kv:
        c.ensure([37, 37, 5, 5, 0, 0, 0, 0])
    paged.lengths = [37, 5, 0, 0]
    paged.kv[1].free = paged.kv[1].free[:3]
    snaps = [_snapshot(c) for c in paged.kv]
    with pytest.raises(RuntimeError, match=r"rows \[0, 1, 2, 3\] need 4 more pages, 3 of 12 are free"):
        paged.reorder([1, 0, 2, 3])
    with pytest.raises(RuntimeError, match=r"PagedKVCache.fork: rows \[4, 5, 6, 7\] need 4 more pages, 3 of 12 are free"):
        paged.fork([0, 0], [2, 3])
    assert all(_same(c, s) for c, s in zip(paged.kv, snaps)) and paged.lengths == [37, 5, 0, 0]
    with pytest.raises(ValueError, match="must be empty"):
        paged.fork(0, 1)
    with pytest.raises(ValueError, match="3 indices for a batch of 4"):
        paged.reorder([0, 1, 2])
    with pytest.raises(ValueError, match="outside 0 .. 3"):
        paged.reorder([0, 1, 2, 4])
