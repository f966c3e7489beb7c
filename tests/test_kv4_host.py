"""The 4-bit-mantissa KV cache (ops.NibbleKVCache, csrc/mi355q_kvp.h), what a machine without a GPU can say about it: the class's place
among the cache classes and its refusals by name, the two decode states and generate's spellings, the byte counts, the new exports'
call check read next to the kv8 exports' through mi355q_debug_kv_call_all, and the numpy restatement of the piece layout that the GPU
tests hold the kernels to (tests/kv4_util.py)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import kv4_util as U  # noqa: E402
from window_util import par  # noqa: E402

NAMES = ("mi355q_bfp_kv4_cache_bytes", "mi355q_bfp_kv4_append", "mi355q_bfp_kv4_decode_fp32", "mi355q_bfp_attention_decode_kv4")
KV8_IDS, KV4_IDS = (15, 16, 17, 18), (28, 29, 30, 31)          # cache_bytes, append, decode_fp32, decode


def test_abi_stays_25_and_the_new_names_are_declared_bound_and_exported():
    from mi355q import _lib
    lib = _lib.load_library()
    assert _lib.ABI_VERSION == 25 and lib.mi355q_abi_version() == 25
    text = (ROOT / "include" / "mi355q.h").read_text()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and f"int {name}(" in text, name
        assert f"/* {name}:" in text, f"{name} has no comment of its own in include/mi355q.h"


def test_a_class_of_its_own_and_the_constructors_refusals():
    import torch
    from mi355q import ops
    c = ops.NibbleKVCache(3, 48, 64, par(4), par(4), "cpu")
    assert isinstance(c, ops._KVCacheBase)
    assert not isinstance(c, (ops.KVCache, ops.PackedKVCache, ops.PagedKVCache, ops.PagedPackedKVCache, ops.MinifloatKVCache))
    assert c.k4.dtype == c.v4.dtype == torch.uint8 and c.length == 0 and c.capacity == 48
    assert not c.k4.any() and not c.v4.any()
    for width in (5, 8):
        with pytest.raises(ValueError, match=f"NibbleKVCache qk_params.*width {width} > 4"):
            ops.NibbleKVCache(2, 48, 64, (4, 8, 127, width, 8, 127), par(4), "cpu")          # K is the y side of qk_params
        with pytest.raises(ValueError, match=f"NibbleKVCache pv_params.*width {width} > 4"):
            ops.NibbleKVCache(2, 48, 64, par(4), (4, 8, 127, width, 8, 127), "cpu")          # V is the y side of pv_params
    for xw in (8, 9):                                                                         # Q and P are not stored
        ops.NibbleKVCache(2, 48, 64, U.par2(xw, 4), U.par2(xw, 4), "cpu")
    for yw in (2, 3):
        ops.NibbleKVCache(2, 48, 64, par(yw), par(yw), "cpu")
    with pytest.raises(ValueError, match="outside 2 .. 9"):
        ops.NibbleKVCache(2, 48, 64, (10, 8, 127, 4, 8, 127), par(4), "cpu")
    with pytest.raises(ValueError, match="NibbleKVCache: head_dim"):
        ops.NibbleKVCache(2, 48, 48, par(4), par(4), "cpu")
    with pytest.raises(ValueError, match="NibbleKVCache: capacity"):
        ops.NibbleKVCache(2, 40, 64, par(4), par(4), "cpu")
    c.length = 5
    c.reset()
    assert c.length == 0


def test_decode_and_extend_refusals():
    import torch
    from mi355q import ops
    cache = ops.NibbleKVCache(2, 64, 64, par(4), par(4), "cpu")
    cache.length = 40
    q = torch.zeros(2, 4, 64)
    # the existing entry points never see nibble bytes: the cache is no KVCache
    assert ops._decode_check(q, cache) == "cache is not a KVCache" and ops._extend_check(q, cache) == "cache is not a KVCache"
    assert not ops.bfp_attention_decode_supported(q, cache)
    with pytest.raises(NotImplementedError, match="sliding-window.*NibbleKVCache"):
        ops.bfp_attention_decode(q, cache, window=8)
    with pytest.raises(NotImplementedError, match="extend.*NibbleKVCache"):
        ops.bfp_attention_extend(q, cache)
    with pytest.raises(ValueError, match="there is no CPU fallback"):
        ops.bfp_attention_decode(q, cache)
    with pytest.raises(ValueError, match="does not match the cache's B = 2, D = 64"):
        ops.bfp_attention_decode(torch.zeros(3, 4, 64), cache)
    with pytest.raises(ValueError, match="queries outside 1 .. 16"):
        ops.bfp_attention_decode(torch.zeros(2, 17, 64), cache)
    with pytest.raises(ValueError, match="cache.B \\* group"):
        ops.bfp_attention_decode(torch.zeros(4, 4, 64), cache, group=3)
    with pytest.raises(ValueError, match="lengths without max_length"):
        ops.bfp_attention_decode(q, cache, lengths=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="NibbleKVCache.append: fp32 tensors on cpu only.*no CPU fallback"):
        cache.append(torch.zeros(2, 1, 64), torch.zeros(2, 1, 64))
    cache.length = 64
    with pytest.raises(ValueError, match="NibbleKVCache.append: 64 \\+ 1 keys exceed the capacity"):
        cache.append(torch.zeros(2, 1, 64), torch.zeros(2, 1, 64))
    with pytest.raises(ValueError, match="NibbleKVCache.dequantised: the cache is not on a GPU"):
        cache.dequantised()


def test_nibble_decode_state_and_its_refusals():
    from mi355q import harness as H, ops
    model = U.tiny_llama((4,))
    state = H.NibbleDecodeState(model, 2, 40)
    assert isinstance(state, H.DecodeState) and not isinstance(state, H.PackedDecodeState)
    assert all(type(c) is ops.NibbleKVCache for c in state.kv) and [c.B for c in state.kv] == [2 * 4] and state.capacity == 48
    assert state.kv[0].qk_params == par(4) and state.kv[0].pv_params == par(4)
    with pytest.raises(NotImplementedError, match="NibbleDecodeState: extend=True"):
        H.NibbleDecodeState(model, 2, 40, extend=True)
    with pytest.raises(ValueError, match="NibbleDecodeState: mode 'fp32'"):
        H.NibbleDecodeState(model, 2, 40, mode="fp32")
    with pytest.raises(NotImplementedError, match="NibbleDecodeState: a sliding-window"):
        H.NibbleDecodeState(U.tiny_llama((4,), sliding_window=8), 2, 40)
    with pytest.raises(ValueError, match="NibbleDecodeState: NibbleKVCache qk_params.*width 6 > 4"):
        H.NibbleDecodeState(U.tiny_llama((4, 6)), 2, 40)


def test_narrowest_decode_state_gives_each_layer_its_storage():
    """cached widths 4, 8 and 9 (the tiny model's config takes width 9, the widest a block_fp attention operand may have)"""
    from mi355q import harness as H, ops
    model = U.tiny_llama((4, 8, 9))
    state = H.NarrowestDecodeState(model, 2, 40)
    assert state.kinds == ["nibble", "int8", "bf16"]
    assert [type(c) for c in state.kv] == [ops.NibbleKVCache, ops.PackedKVCache, ops.KVCache]
    assert [c.qk_params[3] for c in state.kv] == [4, 8, 9] and all(c.B == 8 and c.capacity == 48 for c in state.kv)
    assert H.NarrowestDecodeState(U.tiny_llama((3, 5, 2)), 1, 16).kinds == ["nibble", "int8", "nibble"]
    with pytest.raises(NotImplementedError, match="NarrowestDecodeState: extend=True"):
        H.NarrowestDecodeState(model, 2, 40, extend=True)
    with pytest.raises(ValueError, match="NarrowestDecodeState: mode 'fp32'"):
        H.NarrowestDecodeState(model, 2, 40, mode="fp32")
    with pytest.raises(NotImplementedError, match="NarrowestDecodeState: a sliding-window"):
        H.NarrowestDecodeState(U.tiny_llama((4, 8), sliding_window=8), 2, 40)
    state.reset()
    assert state.kinds == ["nibble", "int8", "bf16"]


def test_new_state_spellings():
    import torch
    from mi355q import harness as H
    model = U.tiny_llama((4,))
    assert type(H._new_state(model, 2, 40, "block_fp", False, None, None, "nibble")) is H.NibbleDecodeState
    assert type(H._new_state(model, 2, 40, "block_fp", False, None, None, "narrowest")) is H.NarrowestDecodeState
    assert type(H._new_state(model, 2, 40, "block_fp", False, None, None, "int8")) is H.PackedDecodeState
    assert type(H._new_state(model, 2, 40, "block_fp", False, None, None, None)) is H.DecodeState
    ids = torch.zeros(1, 4, dtype=torch.long)
    for name in ("nibble", "narrowest"):
        with pytest.raises(NotImplementedError, match=f"kv_storage='{name}' with page_size / num_pages.*not paged"):
            H.generate(model, ids, 2, kv_storage=name, page_size=32)
        with pytest.raises(NotImplementedError, match="extend=True"):
            H.generate(model, ids, 2, kv_storage=name, chunk=2)
    with pytest.raises(ValueError, match="kv_storage = 'int4' is neither None .* nor 'int8' .* nor 'nibble' .* nor 'narrowest'"):
        H.generate(model, ids, 2, kv_storage="int4")
    with pytest.raises(ValueError, match="beam_search: kv_storage = 'nibble'"):           # (beam_search is paged: no nibble pages)
        H.beam_search(model, ids, 2, 2, kv_storage="nibble")


def _bytes(fn, B, Cap, D):
    nb = [C.c_int64(0) for _ in range(3)]
    assert fn(B, Cap, D, *[C.addressof(n) for n in nb]) == 0
    return [n.value for n in nb]


@pytest.mark.parametrize("B,Cap,D", [(3, 64, 32), (2, 48, 96), (1, 16, 128)])
def test_byte_counts(B, Cap, D):
    from mi355q import _lib, ops
    lib = _lib.load_library()
    k4, v4, s4 = _bytes(lib.mi355q_bfp_kv4_cache_bytes, B, Cap, D)
    k8, v8, s8 = _bytes(lib.mi355q_bfp_kv8_cache_bytes, B, Cap, D)
    k16, v16, s16 = _bytes(lib.mi355q_bfp_kv_cache_bytes, B, Cap, D)
    assert k4 == B * (Cap // 16) * (D // 32) * 288 and v4 == B * -(-Cap // 32) * (D // 16) * 288
    assert k4 * 17 == k8 * 9 and v4 * 17 == v8 * 9, "not exactly 9/17 of the int8-mantissa cache"
    assert k4 * 32 == k16 * 9 and v4 * 32 == v16 * 9, "not exactly 9/32 of the bf16 cache"
    assert s4 == s8 == s16
    cache = ops.NibbleKVCache(B, Cap, D, par(4), par(4), "cpu")
    assert (cache.k4.numel(), cache.v4.numel(), cache.stage.numel()) == (k4, v4, s4)


def test_byte_counts_refuse_a_bad_shape():
    from mi355q import _lib
    lib = _lib.load_library()
    nb = [C.c_int64(0) for _ in range(3)]
    ptrs = [C.addressof(n) for n in nb]
    for fn in (lib.mi355q_bfp_kv4_cache_bytes, lib.mi355q_bfp_kv8_cache_bytes):
        assert fn(2, 40, 64, *ptrs) == _lib.E_UNSUPPORTED and fn(2, 48, 160, *ptrs) == _lib.E_UNSUPPORTED
        assert fn(0, 48, 64, *ptrs) == _lib.E_BADARG and fn(2, 48, 64, None, ptrs[1], ptrs[2]) == _lib.E_BADARG


# ---- the call check, through the debug hook: a[0 .. 13] = kq, vq, stage, k, v, q, out, workspace, lengths, counts, block_table, k_bytes,
# v_bytes, stage_bytes; a[14 .. 26] = B, C, max_pages, num_pages, P, D, M, L, n, G, causal, window, splits
ADDR = dict(kq=0, vq=1, stage=2, k=3, v=4, q=5, out=6, workspace=7, lengths=8, counts=9, block_table=10, k_bytes=11, v_bytes=12, stage_bytes=13)
NUM = dict(B=14, C=15, max_pages=16, num_pages=17, P=18, D=19, M=20, L=21, n=22, G=23, causal=24, window=25, splits=26)


def _hook():
    from mi355q import _lib
    fn = _lib.load_library().mi355q_debug_kv_call_all
    fn.restype, fn.argtypes = C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn


def _call(id_, qk=par(4), pv=par(4), strides=None, **over):
    a = [0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, 0x9000, 0, 0, 0xA000, 0xB000, 0xC000,
         2, 32, 0, 0, 0, 32, 1, 4, 1, 0, 1, 0, 0]
    for name, value in over.items():
        a[ADDR[name] if name in ADDR else NUM[name]] = value
    pa, pb, out = (C.c_int32 * 6)(*qk), (C.c_int32 * 6)(*pv), (C.c_int64 * 18)()
    st = None if strides is None else (C.c_int64 * 4)(*strides)
    assert _hook()(id_, (C.c_int64 * 27)(*a), pa, pb, st, out) == 0
    return list(out)


def test_the_valid_baseline_of_every_new_id():
    """code 0, `go`, then the normalised call: B, capacity, D, M, L, n, G, window, lg_p, pages set, causal, strides set, the four strides"""
    assert _call(28) == [0, 1, 2, 0, 32, 1, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]             # sizes: no cache is formed
    assert _call(29) == [0, 1, 2, 32, 32, 1, 4, 1, 0, 0, 0, 0, 0, 1, 32, 32, 32, 32]        # append: the contiguous strides n D, D
    assert _call(29, strides=(64, 32, 128, 64))[13:] == [1, 64, 32, 128, 64]
    assert _call(30) == [0, 1, 2, 32, 32, 1, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]            # decode_fp32
    assert _call(31) == [0, 1, 2, 32, 32, 1, 4, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0]            # decode: causal normalised, G 0
    assert _call(31, G=1)[8] == 0 and _call(31, G=4, M=4, L=4)[8] == 4                      # G <= 1 the ungrouped kernels
    assert _call(31, causal=7)[12] == 1 and _call(31, causal=0)[12] == 0
    assert _call(31, strides=(64, 32, 128, 64))[13:] == [1, 64, 32, 128, 64]
    for xw in (8, 9):                                                                        # Q and P keep 2 .. 9
        assert _call(31, qk=U.par2(xw, 4), pv=U.par2(xw, 4))[:2] == [0, 1]
    for yw in (2, 3, 4):
        for id_ in KV4_IDS:
            assert _call(id_, qk=par(yw), pv=par(yw))[:2] == [0, 1]


def test_id_27_stays_refused_and_the_recorded_hook_keeps_its_ids():
    from mi355q import _lib
    lib = _lib.load_library()
    a, qk, out = (C.c_int64 * 27)(), (C.c_int32 * 6)(*par(4)), (C.c_int64 * 18)()
    fn = _hook()
    assert fn(27, a, qk, qk, None, out) == _lib.E_BADARG and fn(32, a, qk, qk, None, out) == _lib.E_BADARG
    old = lib.mi355q_debug_kv_call
    old.restype, old.argtypes = C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for id_ in (25, 28, 31):
        assert old(id_, a, qk, qk, None, out) == _lib.E_BADARG


PERTURBATIONS = [dict(**{name: 0}) for name in ("kq", "vq", "stage", "k", "v", "q", "out", "workspace", "lengths", "k_bytes", "v_bytes",
                                                "stage_bytes")] + [
    dict(D=48), dict(D=160), dict(C=40), dict(M=17, L=20), dict(M=0), dict(M=5, L=4), dict(G=-1), dict(B=0), dict(B=65536), dict(L=33),
    dict(L=-1), dict(n=-1), dict(n=0), dict(L=32, n=1), dict(splits=-1), dict(kq=0x1008), dict(lengths=0x9002), dict(counts=0x9100, lengths=0),
    dict(G=3, B=65535, M=16, L=16), dict(strides=(32, 32, 34, 32)), dict(qk=(4, 8, 127, 9, 8, 127)), dict(pv=(4, 8, 127, 9, 8, 127)),
    dict(qk=(10, 8, 127, 4, 8, 127)), dict(qk=(4, 9, 127, 4, 8, 127)), dict(n=0, qk=(4, 8, 127, 9, 8, 127)),
]


@pytest.mark.parametrize("over", PERTURBATIONS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_one_perturbation_gives_the_kv8_exports_answer(over):
    """the code and `go` of every new id are those of its kv8 twin for the same call, read from the kv8 id in the same run"""
    for id4, id8 in zip(KV4_IDS, KV8_IDS):
        assert _call(id4, **over)[:2] == _call(id8, **over)[:2], (id4, id8, over)
    # and the perturbation is one: the list above refuses somewhere
    assert any(_call(id4, **over)[:2] != [0, 1] for id4 in KV4_IDS) or over == dict(n=0)


def test_the_one_difference_is_the_cached_width():
    from mi355q import _lib
    for width in (5, 6, 7, 8):
        for side in ("qk", "pv"):
            over = {side: (4, 8, 127, width, 8, 127)}
            for id4, id8 in zip(KV4_IDS[1:], KV8_IDS[1:]):
                assert _call(id4, **over)[:2] == [_lib.E_UNSUPPORTED, 0], (id4, over)
                assert _call(id8, **over)[:2] == [0, 1], (id8, over)
            assert _call(28, **over)[:2] == [0, 1]                                           # sizes read no widths
    # as for kv8's width 9: before the append's and the read-back's "nothing to do" return of 0
    assert _call(29, n=0, qk=(4, 8, 127, 5, 8, 127))[:2] == [_lib.E_UNSUPPORTED, 0]
    assert _call(30, L=0, pv=(4, 8, 127, 5, 8, 127))[:2] == [_lib.E_UNSUPPORTED, 0]
    assert _call(16, n=0, qk=(4, 8, 127, 5, 8, 127))[:2] == [0, 0] and _call(16, n=0, qk=(4, 8, 127, 9, 8, 127))[:2] == [_lib.E_UNSUPPORTED, 0]


def test_the_exports_themselves_refuse_width_5():
    from mi355q import _lib
    lib = _lib.load_library()
    bad, good = (C.c_int32 * 6)(4, 8, 127, 5, 8, 127), (C.c_int32 * 6)(*par(4))
    for pa, pb in ((bad, good), (good, bad)):
        assert lib.mi355q_bfp_kv4_append(None, None, None, None, None, None, None, 2, 48, 64, 1, 0, C.addressof(pa), C.addressof(pb),
                                         None, None) == _lib.E_UNSUPPORTED
        assert lib.mi355q_bfp_kv4_decode_fp32(None, None, None, None, None, 2, 48, 64, 16, C.addressof(pa), C.addressof(pb), None) == _lib.E_UNSUPPORTED
        assert lib.mi355q_bfp_attention_decode_kv4(0x6000, 0x1000, 0x2000, 0, 0x9000, 1, 0.0, 0.0, 0x7000, 0x8000, 2, 1, 4, 32, 32,
                                                   C.addressof(pa), C.addressof(pb), None, 0, None) == _lib.E_UNSUPPORTED


# ---- the layout, restated in numpy
def test_nibble_bytes_as_the_header_words_them():
    m = np.zeros((64, 8), np.int64)
    m[2, 5], m[3, 5] = -7, 7                     # lanes 2 and 3, slot 5: byte 8 * 1 + 5, low nibble lane 2
    b = U.pack_lanes(m)
    assert b[13] == ((-7) & 0xF) | (7 << 4) == 0x79 and np.count_nonzero(b) == 1
    m[:] = 0
    m[63, 7] = -1
    b = U.pack_lanes(m)
    assert b[255] == 0xF0 and np.count_nonzero(b) == 1
    assert np.array_equal(U.unpack_lanes(np.full(256, 0x7F, np.uint8)), np.tile(np.array([[-1], [7]]), (32, 8)))


def test_piece_round_trips():
    r = np.random.default_rng(0)
    km, kc = r.integers(-7, 8, size=(16, 32)), r.integers(0, 256, size=32)
    piece = U.k_piece_pack(km, kc)
    assert piece.shape == (288,) and piece.dtype == np.uint8
    m, c = U.k_piece_unpack(piece)
    assert np.array_equal(m, km) and np.array_equal(c, kc)
    assert np.array_equal(piece[256:], kc.astype(np.uint8))                                # K: byte 256 + i for d = 32 c + i
    # key 5 (lane 5, odd: high nibble) at d = 19 (g = 2, slot 3): byte 8 ((5 + 32) >> 1) + 3
    assert (int(piece[8 * ((5 + 32) >> 1) + 3]) >> 4) == (int(km[5, 19]) & 0xF)
    vm, vc = r.integers(-7, 8, size=(32, 16)), r.integers(0, 256, size=32)
    piece = U.v_piece_pack(vm, vc)
    m, c = U.v_piece_unpack(piece)
    assert np.array_equal(m, vm) and np.array_equal(c, vc)
    # key 22 = 16 * 1 + 4 * 1 + 2: h = 1, g = 1, slot j = 4 + 2 = 6; d = 9 (lane 9 + 16 = 25, odd): byte 8 (25 >> 1) + 6, code 256 + 8 + 6
    assert (int(piece[8 * (25 >> 1) + 6]) >> 4) == (int(vm[22, 9]) & 0xF) and piece[256 + 14] == vc[22]
    v4 = np.concatenate([U.v_piece_pack(vm, np.full(32, 127)), np.zeros(288, np.uint8)])    # D = 32: two V pieces a pair, the second empty
    K, V = U.unpack_cache(U.k_piece_pack(km, np.full(32, 130)), v4, 1, 16, 32, 4)
    assert np.array_equal(K[0], km * 2.0 ** (130 - 127 - 3))
    assert np.array_equal(V[0, :, :16], vm / 8.0) and not V[0, :, 16:].any()
