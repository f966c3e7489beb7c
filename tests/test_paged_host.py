"""The paged block_fp KV cache on the host: the new C-ABI symbols and their argument checks, the reasons of the check functions, the
host allocator of ops.PagedKVCache (ensure / release / share_prefix) and the DecodeState default -- a machine without a GPU runs all
of this, in the manner of tests/test_gqa_host.py."""
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
NEW = ("mi355q_bfp_kv_paged_bytes", "mi355q_bfp_kv_append_paged", "mi355q_bfp_kv_decode_fp32_paged", "mi355q_bfp_attention_decode_paged",
       "mi355q_bfp_attention_extend_paged")


def test_the_exports_exist_and_the_abi_stays_25():
    from mi355q import _lib
    header = (ROOT / "include" / "mi355q.h").read_text()
    lib = _lib.load_library()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} not declared"
        assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} not bound / exported"
    assert lib.mi355q_abi_version() == _lib.ABI_VERSION == 25


def test_paged_bytes_against_the_formula():
    from mi355q import _lib
    lib = _lib.load_library()
    nb = [ctypes.c_int64(0) for _ in range(3)]
    a = [ctypes.addressof(n) for n in nb]
    for num_pages, P, B, D in ((7, 32, 3, 32), (100, 64, 5, 96), (9, 256, 2, 128), (1, 1024, 1, 64)):
        assert lib.mi355q_bfp_kv_paged_bytes(num_pages, P, B, D, *a) == 0
        # [num_pages][P / 16][D / 32] and [num_pages][P / 32][D / 16] pieces of 1 KiB; [B][16][D] fp32
        assert nb[0].value == num_pages * (P // 16) * (D // 32) * 1024 == num_pages * P * D * 2
        assert nb[1].value == num_pages * (P // 32) * (D // 16) * 1024 == num_pages * P * D * 2
        assert nb[2].value == B * 16 * D * 4
    for bad_p in (0, 16, 48, 33, -32, 96):
        assert lib.mi355q_bfp_kv_paged_bytes(4, bad_p, 2, 64, *a) == _lib.E_BADARG, bad_p
    assert lib.mi355q_bfp_kv_paged_bytes(4, 32, 2, 64, None, a[1], a[2]) == _lib.E_BADARG
    assert lib.mi355q_bfp_kv_paged_bytes(0, 32, 2, 64, *a) == _lib.E_BADARG
    assert lib.mi355q_bfp_kv_paged_bytes(4, 32, 2, 160, *a) == _lib.E_UNSUPPORTED


def test_c_entry_points_validate_without_a_gpu():
    from mi355q import _lib
    lib = _lib.load_library()
    pa = (ctypes.c_int32 * 6)(*P6)
    a = ctypes.addressof
    buf = ctypes.create_string_buffer(4096)
    p = (a(buf) + 15) // 16 * 16

    def app(P=32, n=4, mx=60, max_pages=2, lengths=p, table=p):
        return lib.mi355q_bfp_kv_append_paged(p, p, p, p, p, lengths, None, table, 2, max_pages, 8, P, 64, n, mx, a(pa), a(pa), None, None)

    def deq(P=32, mx=64, max_pages=2, table=p):
        return lib.mi355q_bfp_kv_decode_fp32_paged(p, p, p, table, p, p, 2, max_pages, 8, P, 64, mx, None)

    def dec(P=32, M=1, mx=64, max_pages=2, G=0, lengths=p, table=p, q=p):
        return lib.mi355q_bfp_attention_decode_paged(q, p, p, G, lengths, table, 1, 0.0, 8.0, p, p, 2, M, mx, max_pages, 8, P, 64, a(pa), a(pa),
                                                     None, 0, None)

    def ext(P=32, M=20, mx=64, max_pages=2, G=0, lengths=p, table=p, q=p):
        return lib.mi355q_bfp_attention_extend_paged(q, p, p, G, lengths, None, table, 1, 0.0, 8.0, p, 2, M, mx, max_pages, 8, P, 64, a(pa), a(pa),
                                                     None, None)
    for fn in (app, deq, dec, ext):
        for bad_p in (16, 48, 0, 100):                       # not a power of two, or below 32
            assert fn(P=bad_p) == _lib.E_BADARG, (fn.__name__, bad_p)
    # max_length > max_pages * P
    assert deq(mx=65) == dec(mx=65) == ext(mx=65) == _lib.E_BADARG
    # max_length + n > max_pages * P on the append; one key less passes the bound and meets the next check (a NULL table)
    assert app(mx=60, n=5) == _lib.E_BADARG and app(mx=61, n=4) == _lib.E_BADARG
    assert app(mx=60, n=4, table=None) == _lib.E_BADARG and app(mx=60, n=0) == 0
    # the ragged form is the only one: NULL lengths, NULL table
    assert dec(lengths=None) == dec(table=None) == ext(lengths=None) == ext(table=None) == deq(table=None) == _lib.E_BADARG
    assert dec(M=17) == _lib.E_UNSUPPORTED and dec(M=4, mx=3) == _lib.E_UNSUPPORTED and ext(M=0) == _lib.E_UNSUPPORTED
    assert dec(G=-1) == ext(G=-1) == _lib.E_BADARG
    assert dec(table=p + 2) == ext(table=p + 2) == app(table=p + 2) == _lib.E_ALIGN and dec(q=p + 4) == _lib.E_ALIGN


def _cache(**kw):
    from mi355q import ops
    args = dict(page_size=32, num_pages=8, max_pages=3)
    args.update(kw)
    return ops.PagedKVCache(3, 64, P6, P6, "cpu", **args)


def test_constructor_refusals_and_shape():
    import torch
    c = _cache()
    assert (c.capacity, c.B, c.D, c.page_size, c.num_pages, c.max_pages) == (96, 3, 64, 32, 8, 3)
    assert c.kq.numel() == c.vq.numel() == 8 * 32 * 64 * 2 and c.stage.numel() == 3 * 16 * 64 * 4
    assert not c.kq.any() and not c.vq.any()                  # zeroed pools
    assert c.block_table.dtype == torch.int32 and tuple(c.block_table.shape) == (3, 3) and sorted(c.free) == list(range(8))
    for bad in (16, 48, 0):
        with pytest.raises(ValueError, match="power of two >= 32"):
            _cache(page_size=bad)
    with pytest.raises(ValueError, match="pad_page 8 outside"):
        _cache(pad_page=8)
    c = _cache(pad_page=5)
    assert 5 not in c.free and len(c.free) == 7 and bool((c.table == 5).all())


def test_check_functions_give_the_paged_reasons():
    import torch
    from mi355q import ops
    from mi355q.quantize import get_quantized_func
    c = _cache()
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    for fn, check, M in ((ops.bfp_attention_decode, ops._decode_check, 4), (ops.bfp_attention_extend, ops._extend_check, 20)):
        q = torch.zeros(3, M, 64)
        assert "always addressed in the ragged form" in check(q, c)
        with pytest.raises(ValueError, match="paged cache is always addressed in the ragged form"):
            fn(q, c)
        with pytest.raises(ValueError, match="lengths without max_length"):
            fn(q, c, lengths=i32(40, 40, 40))
        with pytest.raises(ValueError, match="max_length = 97 outside .* the capacity 96"):
            fn(q, c, lengths=i32(40, 40, 40), max_length=97)
        with pytest.raises(ValueError, match="lengths .*one entry per cache row"):
            fn(q, c, lengths=i32(40, 40), max_length=40)
        with pytest.raises(ValueError, match=r"has 3 rows, not cache.B \* group = 3 \* 4 = 12"):
            fn(q, c, lengths=i32(40, 40, 40), max_length=40, group=4)
        assert check(q, c, lengths=i32(40, 40, 40), max_length=40).endswith("there is no CPU fallback")
        assert check(q, "a list") == "cache is not a KVCache"
    for key, M in (("attention_decode", 1), ("attention_extend", 20)):       # the registry's functions take the paged cache
        with pytest.raises(ValueError, match="always addressed in the ragged form"):
            get_quantized_func(key, dict(W6))(torch.zeros(3, M, 64), c, dict(W6), dict(W6))
        with pytest.raises(ValueError, match="no CPU fallback"):
            get_quantized_func(key, dict(W6))(torch.zeros(3, M, 64), c, dict(W6), dict(W6), lengths=i32(40, 40, 40), max_length=40)
    k = torch.zeros(3, 4, 64)
    with pytest.raises(TypeError):
        c.append(k, k)                                        # lengths is mandatory
    with pytest.raises(ValueError, match="lengths= is mandatory"):
        c.append(k, k, lengths=None)
    with pytest.raises(ValueError, match=r"max_length 93 \+ 4 new keys exceed the capacity 96"):
        c.append(k, k, lengths=i32(0, 0, 0), max_length=93)
    with pytest.raises(ValueError, match="no CPU fallback"):
        c.append(k, k, lengths=i32(0, 0, 0), max_length=92)
    with pytest.raises(ValueError, match="lengths= is mandatory"):
        c.dequantised(None)
    with pytest.raises(ValueError, match="no CPU fallback"):
        c.dequantised(i32(0, 0, 0), max_length=10)


def _snapshot(c):
    return c.table.clone(), c.block_table.clone(), list(c.free), list(c.refs), [list(h) for h in c.held]


def _same(c, snap):
    import torch
    return (torch.equal(c.table, snap[0]) and torch.equal(c.block_table, snap[1]) and c.free == snap[2] and c.refs == snap[3]
            and [list(h) for h in c.held] == snap[4])


def test_ensure_never_hands_a_page_to_two_rows_and_refuses_before_it_changes_anything():
    import torch
    c = _cache()                                              # 8 pages, 3 rows of up to 3
    c.ensure([1, 33, 0])
    assert [len(h) for h in c.held] == [1, 2, 0] and len(c.free) == 5
    c.ensure([32, 33, 64])                                    # row 0 keeps its page (32 keys: still one), row 2 takes two
    assert [len(h) for h in c.held] == [1, 2, 2]
    used = [p for h in c.held for p in h]
    assert len(set(used)) == len(used) == 5 and not set(used) & set(c.free) and sorted(used + c.free) == list(range(8))
    assert all(c.refs[p] == 1 for p in used) and all(c.refs[p] == 0 for p in c.free)
    for b, h in enumerate(c.held):
        assert c.table[b, :len(h)].tolist() == h and torch.equal(c.block_table, c.table)
    c.ensure([10, 10, 10])                                    # shorter lengths take nothing away
    assert [len(h) for h in c.held] == [1, 2, 2]
    snap = _snapshot(c)
    with pytest.raises(RuntimeError, match=r"rows \[0, 1, 2\] need 4 more pages, 3 of 8 are free"):
        c.ensure([96, 96, 96])
    assert _same(c, snap), "a refused ensure changed the table, the mirror or the free list"
    with pytest.raises(ValueError, match=r"rows \[1\] ask for more than max_pages = 3"):
        c.ensure([1, 97, 1])
    assert _same(c, snap)
    with pytest.raises(ValueError, match="2 lengths for 3 cache rows"):
        c.ensure([1, 2])
    c.ensure([96, 64, 64], dry_run=True)
    assert _same(c, snap)


def test_release_then_ensure_reuses_the_pages():
    c = _cache(num_pages=4, pad_page=0)                       # 3 usable pages
    c.ensure([64, 32, 0])
    assert c.free == []
    mine = list(c.held[0])
    with pytest.raises(RuntimeError, match=r"rows \[2\] need 1 more pages, 0 of 4 are free"):
        c.ensure([64, 32, 5])
    c.release([0])
    assert c.held[0] == [] and sorted(c.free) == sorted(mine) and c.table[0].tolist() == [0, 0, 0]
    c.ensure([0, 32, 40])
    assert sorted(c.held[2]) == sorted(mine) and c.free == [] and 0 not in c.held[2]
    c.reset()
    assert sorted(c.free) == [1, 2, 3] and all(h == [] for h in c.held) and bool((c.table == 0).all())


def test_share_prefix_counts_references():
    c = _cache()
    c.ensure([70, 0, 0])                                      # row 0: three pages, two of them full
    a = list(c.held[0])
    c.share_prefix(0, 1, 2)
    assert c.held[1] == a[:2] and c.table[1].tolist()[:2] == a[:2] and [c.refs[p] for p in a] == [2, 2, 1]
    with pytest.raises(ValueError, match="only a row that holds none can share"):
        c.share_prefix(0, 1, 1)
    with pytest.raises(ValueError, match="4 pages, row 0 holds 3"):
        c.share_prefix(0, 2, 4)
    c.ensure([70, 70, 0])                                     # row 1's own tail page
    assert c.held[1][:2] == a[:2] and c.held[1][2] not in a and len(c.free) == 4
    c.release([0])                                            # the shared pages stay alive with row 1; row 0's tail is free again
    assert [c.refs[p] for p in a] == [1, 1, 0] and a[2] in c.free and a[0] not in c.free and a[1] not in c.free
    c.ensure([0, 70, 64])
    assert not set(c.held[2]) & set(c.held[1])
    c.release([1])
    assert [c.refs[p] for p in a[:2]] == [0, 0] and a[0] in c.free and a[1] in c.free


def test_assign_places_free_pages_only():
    c = _cache()
    c.assign(1, [6, 2])
    assert c.held[1] == [6, 2] and c.table[1].tolist() == [6, 2, 0] and 6 not in c.free
    with pytest.raises(ValueError, match="not distinct free pages"):
        c.assign(0, [6])
    with pytest.raises(ValueError, match="more than max_pages"):
        c.assign(1, [0, 1])


def _tiny():
    import torch
    from mi355q import harness as H
    torch.manual_seed(3)
    cfg = H.TinyLlamaConfig(vocab_size=64, hidden_size=128, intermediate_size=256, num_layers=2, num_heads=4, max_positions=64, num_kv_heads=2)
    return H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(dict(W6), 2))


def test_decode_state_default_is_contiguous_and_paged_is_opt_in():
    from mi355q import harness as H, ops
    model = _tiny()
    state = H.DecodeState(model, 3, 40)
    assert all(type(c) is ops.KVCache for c in state.kv) and not state.paged and not state.ragged and state.capacity == 48
    paged = H.PagedDecodeState(model, 3, 40, page_size=32, num_pages=7)
    assert all(type(c) is ops.PagedKVCache for c in paged.kv) and paged.paged and paged.ragged
    assert [(c.B, c.page_size, c.max_pages, c.num_pages, c.capacity) for c in paged.kv] == [(6, 32, 2, 7, 64)] * 2
    assert H.PagedDecodeState(model, 3, 40, page_size=32).kv[0].num_pages == 12        # default: every row at its capacity
    with pytest.raises(ValueError, match="page_size belongs to mode 'block_fp'"):
        H.PagedDecodeState(model, 3, 40, "fp32", page_size=32)
    with pytest.raises(ValueError, match="num_pages without page_size"):
        H.PagedDecodeState(model, 3, 40, num_pages=4)
    # release: the sequence's rows give their pages back in every layer
    for c in paged.kv:
        c.ensure([33, 33, 1, 1, 0, 0])
    paged.lengths = [33, 1, 0]
    paged.release(0)
    assert paged.lengths == [0, 1, 0] and all(c.held[0] == c.held[1] == [] and len(c.held[2]) == 1 and len(c.free) == 5 for c in paged.kv)
    state.release(1)
    assert state.ragged and state.lengths == [0, 0, 0]


def test_paged_state_refuses_layers_with_different_kv_heads_at_construction():
    """a paged state runs every call through the ragged routes, which need one set of per-row tensors for all layers: the refusal
    comes from the constructor, not from the first forward; generate() without paging options builds the plain state"""
    from mi355q import harness as H
    model = _tiny()
    model.layers[1].self_attn.nkv = 1                         # (host bookkeeping only: nothing is launched)
    with pytest.raises(NotImplementedError, match="layers differ in their number of KV heads"):
        H.PagedDecodeState(model, 3, 40, page_size=32)
    assert type(H._new_state(_tiny(), 3, 40, "block_fp", False, None, None)) is H.DecodeState
    assert type(H._new_state(_tiny(), 3, 40, "block_fp", False, 32, None)) is H.PagedDecodeState
