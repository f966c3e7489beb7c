"""The paged int8-mantissa KV cache (ops.PagedPackedKVCache, csrc/mi355q_kvp.h: paged pools), what a machine without a GPU can say about
it: the constructor's refusals, the class's place among the cache classes, the host plans (which are PagedKVCache's, from shared code),
the refusals of the five new exports and of the entry points above them, the argument check as mi355q_debug_kv_call shows it, the byte
counts, and the ABI version."""
import ctypes as C
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from window_util import par  # noqa: E402

NAMES = ("mi355q_bfp_kv8_paged_bytes", "mi355q_bfp_kv8_append_paged", "mi355q_bfp_kv8_decode_fp32_paged", "mi355q_bfp_attention_decode_kv8_paged",
         "mi355q_bfp_kv8_paged_copy")
W9 = (6, 8, 127, 9, 8, 127)


def _new(B=4, D=32, **kw):
    from mi355q import ops
    kw = dict(dict(page_size=32, num_pages=12, max_pages=3), **kw)
    return ops.PagedPackedKVCache(B, D, par(6), par(6), "cpu", **kw)


def test_abi_stays_25_and_the_new_names_are_declared_bound_and_exported():
    from mi355q import _lib
    lib = _lib.load_library()
    assert _lib.ABI_VERSION == 25 and lib.mi355q_abi_version() == 25
    text = (ROOT / "include" / "mi355q.h").read_text()
    assert "#define MI355Q_ABI_VERSION 25" in text
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and f"int {name}(" in text, name


def test_constructor_refusals():
    from mi355q import ops
    kw = dict(page_size=32, num_pages=12, max_pages=3)
    with pytest.raises(ValueError, match="PagedPackedKVCache qk_params.*width 9 > 8.*int8"):
        ops.PagedPackedKVCache(2, 64, W9, par(6), "cpu", **kw)
    with pytest.raises(ValueError, match="PagedPackedKVCache pv_params.*width 9 > 8.*int8"):
        ops.PagedPackedKVCache(2, 64, par(6), W9, "cpu", **kw)
    ops.PagedPackedKVCache(2, 64, (9, 8, 127, 8, 8, 127), (9, 8, 127, 8, 8, 127), "cpu", **kw)      # Q and P are not stored
    for P in (16, 48, 0):
        with pytest.raises(ValueError, match="PagedPackedKVCache: page_size .* is not a power of two >= 32"):
            ops.PagedPackedKVCache(2, 64, par(6), par(6), "cpu", **dict(kw, page_size=P))
    for bad in (-1, 12):
        with pytest.raises(ValueError, match="PagedPackedKVCache: pad_page .* outside 0 .. 11"):
            ops.PagedPackedKVCache(2, 64, par(6), par(6), "cpu", pad_page=bad, **kw)
    with pytest.raises(ValueError, match="num_pages = 0"):
        ops.PagedPackedKVCache(2, 64, par(6), par(6), "cpu", **dict(kw, num_pages=0))
    with pytest.raises(ValueError, match="head_dim"):
        ops.PagedPackedKVCache(2, 48, par(6), par(6), "cpu", **kw)
    c = ops.PagedPackedKVCache(2, 64, par(6), par(6), "cpu", pad_page=5, **kw)
    assert 5 not in c.free and len(c.free) == 11 and bool((c.table == 5).all())


def test_a_class_of_its_own_with_the_paged_interface():
    import torch
    from mi355q import ops
    c = _new()
    assert not isinstance(c, (ops.PagedKVCache, ops.PackedKVCache, ops.KVCache))
    assert not isinstance(ops.PagedKVCache(4, 32, par(6), par(6), "cpu", page_size=32, num_pages=12, max_pages=3), type(c))
    assert c.k8.dtype == c.v8.dtype == torch.uint8 and not hasattr(c, "kq") and not hasattr(c, "vq")
    assert c.k8.numel() == c.v8.numel() == 12 * 32 * 32 * 17 // 16 and c.stage.numel() == c.stage_alt.numel() == 4 * 16 * 32 * 4
    assert c.capacity == 96 and c.pages_for(33) == 2 and tuple(c.block_table.shape) == (4, 3) and c.RAGGED_ONLY
    for name in ("ensure", "assign", "release", "share_prefix", "fork", "reorder", "reset", "append", "dequantised", "_plan_copy"):
        assert callable(getattr(c, name))
    # one copy of the host code: both classes run the same functions
    for name in ("ensure", "assign", "release", "share_prefix", "fork", "reorder", "reset", "_plan_copy", "_commit_plan", "_copy", "pages_for"):
        assert getattr(ops.PagedPackedKVCache, name) is getattr(ops.PagedKVCache, name), name


def test_plans_are_the_paged_caches():
    """ensure / share_prefix / fork / reorder / release for lengths (37, 64, 5, 0) and src_rows (2, 0, 0, 3): tables, counts and jobs are
    what PagedKVCache plans for the same calls"""
    import torch
    from mi355q import ops
    new = _new()
    old = ops.PagedKVCache(4, 32, par(6), par(6), "cpu", page_size=32, num_pages=12, max_pages=3)
    lengths, src = (37, 64, 5, 0), (2, 0, 0, 3)

    def same():
        assert new.held == old.held and new.free == old.free and new.refs == old.refs and torch.equal(new.table, old.table)
        assert torch.equal(new.block_table, new.table)

    for c in (new, old):
        c.ensure(lengths)
    same()
    assert new.held == [[0, 1], [2, 3], [4], []] and new.free == [11, 10, 9, 8, 7, 6, 5]
    for c in (new, old):
        c.share_prefix(1, 3, 1)
    same()
    assert new.held[3] == [2] and new.refs[2] == 2
    for c in (new, old):
        c.release(3)
    same()
    plans = [c._plan_copy([(b, s, lengths[s]) for b, s in enumerate(src)]) for c in (new, old)]
    assert vars(plans[0]) == vars(plans[1])
    # row 0 <- row 2 (5 keys: a private copy of its partial page), rows 1, 2 <- row 0 (37 keys: page 0 by reference, copies of page 1),
    # row 3 stays empty: no job
    assert plans[0].jobs == [(4, 5, 2, 0), (1, 6, 0, 1), (1, 7, 0, 2)] and plans[0].drawn == [5, 6, 7]
    assert plans[0].held == {0: [5], 1: [0, 6], 2: [0, 7], 3: []} and sorted(plans[0].freed) == [1, 2, 3, 4]
    forks = [c._plan_copy([(3, 0, 37)], "fork") for c in (new, old)]
    assert vars(forks[0]) == vars(forks[1]) and forks[0].jobs == [(1, 5, 0, 3)] and forks[0].held == {3: [0, 5]}
    for c in (new, old):
        c.fork(0, 3, 37, dry_run=True)
        c.reorder(src, lengths, dry_run=True)
    same()
    with pytest.raises(ValueError, match="PagedPackedKVCache.fork: the cache is not on a GPU"):
        new.fork(0, 3, 37)
    with pytest.raises(ValueError, match="PagedPackedKVCache.reorder: 3 source rows"):
        new.reorder((0, 1, 2), lengths)
    with pytest.raises(ValueError, match="PagedPackedKVCache.share_prefix: row 1 holds 2 pages"):
        new.share_prefix(0, 1, 1)
    for c in (new, old):
        c.reset()
    same()
    assert sorted(new.free) == list(range(12)) and not any(new.refs)


def test_a_pool_short_by_one_page_changes_nothing():
    import torch
    c = _new(num_pages=4)
    with pytest.raises(RuntimeError, match=r"PagedPackedKVCache.ensure: rows \[0, 1, 2\] need 5 more pages, 4 of 4 are free"):
        c.ensure((37, 64, 5, 0))
    assert c.free == [3, 2, 1, 0] and c.held == [[], [], [], []] and not any(c.refs) and bool((c.table == 0).all())
    c.ensure((37, 33, 0, 0))
    snap = (list(c.free), [list(h) for h in c.held], list(c.refs), c.table.clone())
    with pytest.raises(RuntimeError, match=r"PagedPackedKVCache.reorder: rows \[0, 1\] need 2 more pages, 0 of 4 are free"):
        c.reorder((1, 0, 2, 3), (37, 33, 0, 0))
    with pytest.raises(RuntimeError, match=r"PagedPackedKVCache.fork: rows \[2\] need 1 more pages, 0 of 4 are free"):
        c.fork(0, 2, 37)
    with pytest.raises(ValueError, match="PagedPackedKVCache.ensure: rows \\[0\\] ask for more than max_pages = 3"):
        c.ensure((97, 0, 0, 0))
    assert (c.free, c.held, c.refs) == snap[:3] and torch.equal(c.table, snap[3])


def test_window_trim_and_extend_are_refused_by_name():
    import torch
    from mi355q import ops
    c = _new()
    q = torch.zeros(4, 4, 32)
    lengths = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="PagedPackedKVCache.trim"):
        c.trim((0, 0, 0, 0), 8)
    with pytest.raises(NotImplementedError, match="sliding-window.*PagedPackedKVCache"):
        ops.bfp_attention_decode(q, c, lengths=lengths, max_length=8, window=8)
    with pytest.raises(NotImplementedError, match="extend.*PagedPackedKVCache"):
        ops.bfp_attention_extend(q, c, lengths=lengths, max_length=8)
    # the existing checks never take it for a bf16 cache
    assert ops._decode_check(q, c) == "cache is not a KVCache" and ops._extend_check(q, c) == "cache is not a KVCache"
    assert not ops.bfp_attention_decode_supported(q, c)
    with pytest.raises(ValueError, match="no uniform paged launch"):
        ops.bfp_attention_decode(q, c)
    with pytest.raises(ValueError, match="lengths without max_length"):
        ops.bfp_attention_decode(q, c, lengths=lengths)
    with pytest.raises(ValueError, match="outside 4 .* the capacity 96"):
        ops.bfp_attention_decode(q, c, lengths=lengths, max_length=97)
    with pytest.raises(ValueError, match="there is no CPU fallback"):
        ops.bfp_attention_decode(q, c, lengths=lengths, max_length=8)
    with pytest.raises(ValueError, match="PagedPackedKVCache.append: lengths= is mandatory"):
        c.append(torch.zeros(4, 1, 32), torch.zeros(4, 1, 32), lengths=None)
    with pytest.raises(ValueError, match="PagedPackedKVCache.append: max_length 96 \\+ 1 new keys exceed the capacity 96"):
        c.append(torch.zeros(4, 1, 32), torch.zeros(4, 1, 32), lengths=lengths, max_length=96)
    with pytest.raises(ValueError, match="there is no CPU fallback"):
        c.append(torch.zeros(4, 1, 32), torch.zeros(4, 1, 32), lengths=lengths, max_length=0)
    with pytest.raises(ValueError, match="PagedPackedKVCache.dequantised: .*not on a GPU"):
        c.dequantised(lengths, 8)


@pytest.mark.parametrize("num_pages,P,B,D", [(12, 32, 4, 32), (7, 64, 3, 128), (5, 128, 2, 96)])
def test_bytes_are_17_16_a_value_and_17_32_of_the_bf16_pools(num_pages, P, B, D):
    from mi355q import _lib
    lib = _lib.load_library()
    sizes = []
    for fn in (lib.mi355q_bfp_kv8_paged_bytes, lib.mi355q_bfp_kv_paged_bytes):
        nb = [C.c_int64(0) for _ in range(3)]
        assert fn(num_pages, P, B, D, *[C.addressof(n) for n in nb]) == 0
        sizes.append([n.value for n in nb])
    (k8, v8, s8), (k16, v16, s16) = sizes
    assert k8 == v8 == num_pages * P * D * 17 // 16 and k8 * 32 == k16 * 17 and v8 * 32 == v16 * 17 and s8 == s16 == B * 16 * D * 4
    assert (P * D * 17) % 256 == 0 and k8 // num_pages == (P * D * 17 // 256) * 16            # whole 16-byte units a page: 68 at P = D = 32
    nb = [C.addressof(C.c_int64(0)) for _ in range(3)]
    assert lib.mi355q_bfp_kv8_paged_bytes(num_pages, 48, B, D, *nb) == _lib.E_BADARG
    assert lib.mi355q_bfp_kv8_paged_bytes(num_pages, P, B, 160, *nb) == _lib.E_UNSUPPORTED
    assert lib.mi355q_bfp_kv8_paged_bytes(num_pages, P, B, D, None, nb[1], nb[2]) == _lib.E_BADARG


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


@pytest.mark.skipif(not _no_gpu(), reason="the exports are called with fake pointers: only where no GPU is visible")
def test_every_refusal_of_the_new_exports():
    """fake, never dereferenced addresses; every call below is refused, or returns 0 because there is nothing to do, before any launch"""
    from mi355q import _lib
    lib = _lib.load_library()
    BAD, UNS, ALIGN = _lib.E_BADARG, _lib.E_UNSUPPORTED, _lib.E_ALIGN
    a, odd = 0x10000, 0x10008
    good, w9 = (C.c_int32 * 6)(6, 8, 127, 6, 8, 127), (C.c_int32 * 6)(*W9)
    g, w = C.addressof(good), C.addressof(w9)

    def append(k8=a, v8=a, stage=a, k=a, v=a, lengths=a, counts=a, table=a, B=4, mp=3, num=12, P=32, D=32, n=1, L=0, qk=g, pv=g):
        return lib.mi355q_bfp_kv8_append_paged(k8, v8, stage, k, v, lengths, counts, table, B, mp, num, P, D, n, L, qk, pv, None, None)

    assert append(n=0) == 0 and append(n=0, k8=None, table=None) == 0                   # nothing to do
    assert append(n=0, qk=w) == UNS and append(n=0, pv=w) == UNS and append(pv=w) == UNS   # width 9: before the early 0
    for kw in (dict(k8=None), dict(v8=None), dict(stage=None), dict(k=None), dict(v=None), dict(lengths=None), dict(table=None), dict(qk=None),
               dict(pv=None), dict(P=48), dict(P=16), dict(B=0), dict(num=0), dict(mp=0), dict(n=-1), dict(L=-1), dict(L=96), dict(L=90, n=7)):
        assert append(**kw) == BAD, kw
    assert append(L=95, n=1, k8=None) == BAD and append(D=160) == UNS and append(D=48) == UNS
    for kw in (dict(k8=odd), dict(v8=odd), dict(stage=odd), dict(k=odd), dict(v=odd), dict(lengths=a + 2), dict(counts=a + 2), dict(table=a + 2)):
        assert append(**kw) == ALIGN, kw
    assert append(counts=None, n=0) == 0

    def dequant(k8=a, v8=a, lengths=a, table=a, ko=a, vo=a, B=4, mp=3, num=12, P=32, D=32, L=8, qk=g, pv=g):
        return lib.mi355q_bfp_kv8_decode_fp32_paged(k8, v8, lengths, table, ko, vo, B, mp, num, P, D, L, qk, pv, None)

    assert dequant(L=0) == 0 and dequant(L=0, qk=w) == UNS and dequant(pv=w) == UNS
    for kw in (dict(k8=None), dict(v8=None), dict(lengths=None), dict(table=None), dict(ko=None), dict(vo=None), dict(qk=None), dict(pv=None),
               dict(P=48), dict(L=97), dict(L=-1), dict(B=0)):
        assert dequant(**kw) == BAD, kw

    def decode(q=a, k8=a, v8=a, G=0, lengths=a, table=a, causal=1, out=a, ws=a, B=4, M=4, L=8, mp=3, num=12, P=32, D=32, qk=g, pv=g, splits=0):
        return lib.mi355q_bfp_attention_decode_kv8_paged(q, k8, v8, G, lengths, table, causal, 0.0, 0.0, out, ws, B, M, L, mp, num, P, D, qk, pv,
                                                         None, splits, None)

    for kw in (dict(q=None), dict(k8=None), dict(v8=None), dict(lengths=None), dict(table=None), dict(out=None), dict(ws=None), dict(qk=None),
               dict(pv=None), dict(P=48), dict(L=97), dict(M=-1), dict(G=-1), dict(splits=-1), dict(B=0)):
        assert decode(**kw) == BAD, kw
    for kw in (dict(M=17), dict(M=0), dict(L=3), dict(qk=w), dict(pv=w), dict(D=160), dict(B=65535, G=2, M=16)):
        assert decode(**kw) == UNS, kw
    for kw in (dict(q=odd), dict(k8=odd), dict(v8=odd), dict(out=odd), dict(ws=odd), dict(lengths=a + 2), dict(table=a + 2)):
        assert decode(**kw) == ALIGN, kw

    def copy(k8=a, v8=a, src=a, dst=a + 0x1000, jobs=a, n=3, B=4, num=12, P=32, D=32):
        return lib.mi355q_bfp_kv8_paged_copy(k8, v8, src, dst, jobs, n, B, num, P, D, None)

    assert copy(n=0) == 0 and copy(n=0, k8=None, jobs=None) == 0
    for kw in (dict(n=-1), dict(B=0), dict(B=65536), dict(num=0), dict(P=16), dict(P=48), dict(n=0, P=96), dict(D=0), dict(D=48), dict(D=160),
               dict(k8=None), dict(v8=None), dict(src=None), dict(dst=None), dict(jobs=None), dict(dst=a)):
        assert copy(**kw) == BAD, kw
    assert copy(n=65536) == UNS
    for kw in (dict(k8=odd), dict(dst=a + 0x1004), dict(jobs=odd)):
        assert copy(**kw) == ALIGN, kw


SLOTS = ("kq vq stage k v q out workspace lengths counts block_table k_bytes v_bytes stage_bytes "
         "B C max_pages num_pages P D M L n G causal window splits").split()
FIELDS = "rc go B capacity D M L n G window lg_p pages causal strides_set s0 s1 s2 s3".split()
KVX = dict(bytes=21, append=22, dequant=23, decode=24)       # the four ids behind KVX_EXTEND_WINDOW = 20


def test_the_argument_check_of_the_new_ids():
    """mi355q_debug_kv_call: what kv_call_check makes of a call of each new id, against hand-written values"""
    from mi355q import _lib
    _lib.load_library()
    fn = C.CDLL(str(_lib.library_path())).mi355q_debug_kv_call
    fn.restype = C.c_int
    fn.argtypes = [C.c_int32, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    good, w9 = (C.c_int32 * 6)(6, 8, 127, 6, 8, 127), (C.c_int32 * 6)(*W9)
    base = dict({s: 1 << 20 for s in SLOTS[:14]}, B=4, C=0, max_pages=3, num_pages=12, P=64, D=32, M=4, L=40, n=5, G=0, causal=1, window=0, splits=0)

    def check(kind, qk=good, pv=good, strides=None, **kw):
        v = dict(base, **kw)
        flat = (C.c_int64 * 27)(*[int(v[s]) for s in SLOTS])
        out = (C.c_int64 * 18)(*([-99] * 18))
        st = None if strides is None else (C.c_int64 * 4)(*strides)
        assert fn(KVX[kind], flat, qk and C.addressof(qk), pv and C.addressof(pv), st and C.addressof(st), out) == 0
        return dict(zip(FIELDS, out))

    assert fn(25, (C.c_int64 * 27)(), None, None, None, (C.c_int64 * 18)()) == _lib.E_BADARG           # 25 ids: 0 .. 24
    r = check("bytes")
    assert (r["rc"], r["go"], r["lg_p"]) == (0, 1, 6)
    assert check("bytes", P=48)["rc"] == _lib.E_BADARG and check("bytes", k_bytes=0)["rc"] == _lib.E_BADARG
    r = check("append")
    assert r == dict(rc=0, go=1, B=4, capacity=192, D=32, M=4, L=40, n=5, G=0, window=0, lg_p=6, pages=1, causal=0, strides_set=1,
                     s0=160, s1=32, s2=160, s3=32)
    assert check("append", strides=(640, 64, 320, 32))["s0"] == 640 and check("append", strides=(642, 64, 320, 32))["rc"] == _lib.E_ALIGN
    assert check("append", L=188)["rc"] == _lib.E_BADARG                                   # L + n > max_pages * P: the paged code
    assert check("append", n=0, pv=w9)["rc"] == _lib.E_UNSUPPORTED                         # the int8 check, before the early 0
    r = check("append", n=0)
    assert (r["rc"], r["go"]) == (0, 0)
    assert check("append", block_table=0)["rc"] == _lib.E_BADARG and check("append", lengths=0)["rc"] == _lib.E_BADARG
    r = check("dequant")
    assert (r["rc"], r["go"], r["capacity"], r["pages"], r["lg_p"]) == (0, 1, 192, 1, 6)
    assert check("dequant", L=193)["rc"] == _lib.E_BADARG and check("dequant", qk=None)["rc"] == _lib.E_BADARG
    assert check("dequant", L=0, qk=w9)["rc"] == _lib.E_UNSUPPORTED and check("dequant", L=0)["go"] == 0
    r = check("decode", G=1)
    assert r == dict(rc=0, go=1, B=4, capacity=192, D=32, M=4, L=40, n=5, G=0, window=0, lg_p=6, pages=1, causal=1, strides_set=0,
                     s0=0, s1=0, s2=0, s3=0)                                                # G <= 1: the ungrouped kernels
    assert check("decode", G=4)["G"] == 4 and check("decode", causal=0)["causal"] == 0 and check("decode", window=9)["window"] == 0
    assert check("decode", L=193)["rc"] == _lib.E_BADARG and check("decode", M=17)["rc"] == _lib.E_UNSUPPORTED
    assert check("decode", qk=w9)["rc"] == _lib.E_UNSUPPORTED and check("decode", workspace=0)["rc"] == _lib.E_BADARG
    assert check("decode", P=48)["rc"] == _lib.E_BADARG and check("decode", q=(1 << 20) + 8)["rc"] == _lib.E_ALIGN


def _tiny_llama(sliding_window=None):
    import torch
    from mi355q import harness as H
    W6 = dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
              data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127,
              weight_block_size=[1, 16], bias_width=6, bias_exponent_width=8, bias_exponent_bias=127, bias_block_size=[16])
    torch.manual_seed(0)
    kw = {} if sliding_window is None else dict(sliding_window=sliding_window)
    cfg = H.TinyLlamaConfig(vocab_size=97, hidden_size=128, intermediate_size=256, num_layers=1, num_heads=4, max_positions=48, **kw)
    return H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(dict(W6), 1))


def test_decode_state_and_beam_search_refusals():
    import torch
    from mi355q import harness as H, ops
    model = _tiny_llama()
    state = H.PagedPackedDecodeState(model, 2, 40, page_size=32, num_pages=20)
    assert isinstance(state, H.PagedDecodeState) and state.paged and all(type(c) is ops.PagedPackedKVCache for c in state.kv)
    assert [(c.B, c.max_pages, c.num_pages) for c in state.kv] == [(2 * 4, 2, 20)] and state.capacity == 48
    assert H.PagedPackedDecodeState(model, 2, 40, page_size=32).kv[0].num_pages == 16
    with pytest.raises(ValueError, match="PagedPackedDecodeState: page_size is mandatory"):
        H.PagedPackedDecodeState(model, 2, 40)
    with pytest.raises(ValueError, match="PagedPackedDecodeState: mode 'fp32'"):
        H.PagedPackedDecodeState(model, 2, 40, mode="fp32", page_size=32)
    with pytest.raises(NotImplementedError, match="PagedPackedDecodeState: extend=True"):
        H.PagedPackedDecodeState(model, 2, 40, extend=True, page_size=32)
    with pytest.raises(NotImplementedError, match="PagedPackedDecodeState: a sliding-window model"):
        H.PagedPackedDecodeState(_tiny_llama(sliding_window=8), 2, 40, page_size=32)
    with pytest.raises(ValueError, match="PagedPackedDecodeState: .*page_size 48"):
        H.PagedPackedDecodeState(model, 2, 40, page_size=48)
    # the routes that need the extend kernel keep DecodeState's refusals: a mixed call, more than 16 tokens behind non-empty rows
    state.lengths, state.length = [5, 0], 5
    with pytest.raises(NotImplementedError, match="a mixed call"):
        state.begin_ragged([1, 1], 1, 48)
    with pytest.raises(NotImplementedError, match="at most 16"):
        state.begin_ragged([17, 0], 17, 48)
    assert state._call is None and all(h == [] for c in state.kv for h in c.held)
    ids = torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="beam_search: kv_storage = 'int4'"):
        H.beam_search(model, ids, 2, 2, kv_storage="int4")
    with pytest.raises(NotImplementedError, match="beam_search: kv_storage='int8' with chunk"):
        H.beam_search(model, ids, 2, 2, kv_storage="int8", chunk=2)
    with pytest.raises(NotImplementedError, match="not paged"):                              # generate keeps its refusal
        H.generate(model, ids, 2, kv_storage="int8", page_size=32)
