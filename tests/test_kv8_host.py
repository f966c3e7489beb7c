"""The int8-mantissa KV cache (ops.PackedKVCache, csrc/mi355q_kvp.h), what a machine without a GPU can say about it: byte counts,
the constructor's and the entry points' refusals, the decode state's refusals, the ABI version."""
import ctypes
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from window_util import par  # noqa: E402


def _bytes(fn, B, C, D):
    nb = [ctypes.c_int64(0) for _ in range(3)]
    assert fn(B, C, D, *[ctypes.addressof(n) for n in nb]) == 0
    return [n.value for n in nb]


@pytest.mark.parametrize("B,C,D", [(3, 48, 32), (2, 144, 128)])
def test_byte_counts_are_17_32_of_the_bf16_cache(B, C, D):
    from mi355q import _lib, ops
    lib = _lib.load_library()
    k16, v16, s16 = _bytes(lib.mi355q_bfp_kv_cache_bytes, B, C, D)
    k8, v8, s8 = _bytes(lib.mi355q_bfp_kv8_cache_bytes, B, C, D)
    assert k8 * 32 == k16 * 17 and v8 * 32 == v16 * 17 and s8 == s16
    assert k8 == B * C * D * 17 // 16                     # 1 + 1/16 bytes a value
    cache = ops.PackedKVCache(B, C, D, par(6), par(6), "cpu")
    assert (cache.k8.numel(), cache.v8.numel(), cache.stage.numel()) == (k8, v8, s8)
    assert cache.k8.dtype == cache.v8.dtype == __import__("torch").uint8 and cache.length == 0
    assert not isinstance(cache, ops.KVCache)


def test_byte_counts_refuse_a_bad_shape():
    from mi355q import _lib
    lib = _lib.load_library()
    nb = [ctypes.c_int64(0) for _ in range(3)]
    ptrs = [ctypes.addressof(n) for n in nb]
    assert lib.mi355q_bfp_kv8_cache_bytes(2, 40, 64, *ptrs) == _lib.E_UNSUPPORTED       # C % 16
    assert lib.mi355q_bfp_kv8_cache_bytes(2, 48, 160, *ptrs) == _lib.E_UNSUPPORTED      # D > 128
    assert lib.mi355q_bfp_kv8_cache_bytes(0, 48, 64, *ptrs) == _lib.E_BADARG
    assert lib.mi355q_bfp_kv8_cache_bytes(2, 48, 64, None, ptrs[1], ptrs[2]) == _lib.E_BADARG


def test_constructor_refusals():
    from mi355q import ops
    with pytest.raises(ValueError, match="width 9 > 8.*int8"):
        ops.PackedKVCache(2, 48, 64, (6, 8, 127, 9, 8, 127), par(6), "cpu")            # K is the y side of qk_params
    with pytest.raises(ValueError, match="width 9 > 8.*int8"):
        ops.PackedKVCache(2, 48, 64, par(6), (6, 8, 127, 9, 8, 127), "cpu")            # V is the y side of pv_params
    ops.PackedKVCache(2, 48, 64, (9, 8, 127, 8, 8, 127), (9, 8, 127, 8, 8, 127), "cpu")  # Q and P are not stored: 9 is theirs to take
    with pytest.raises(ValueError, match="outside 2 .. 9"):
        ops.PackedKVCache(2, 48, 64, (10, 8, 127, 8, 8, 127), par(6), "cpu")
    for D in (16, 48, 160):
        with pytest.raises(ValueError, match="head_dim"):
            ops.PackedKVCache(2, 48, D, par(6), par(6), "cpu")
    for C in (0, 8, 40):
        with pytest.raises(ValueError, match="capacity"):
            ops.PackedKVCache(2, C, 64, par(6), par(6), "cpu")
    with pytest.raises(ValueError, match="B = 0"):
        ops.PackedKVCache(0, 48, 64, par(6), par(6), "cpu")


def test_the_c_entry_points_refuse_width_9_cached_operands():
    from mi355q import _lib
    lib = _lib.load_library()
    bad = (ctypes.c_int32 * 6)(6, 8, 127, 9, 8, 127)
    good = (ctypes.c_int32 * 6)(6, 8, 127, 6, 8, 127)
    for pa, pb in ((bad, good), (good, bad)):
        rc = lib.mi355q_bfp_kv8_append(None, None, None, None, None, None, None, 2, 48, 64, 1, 0, ctypes.addressof(pa), ctypes.addressof(pb),
                                       None, None)
        assert rc == _lib.E_UNSUPPORTED
        rc = lib.mi355q_bfp_kv8_decode_fp32(None, None, None, None, None, 2, 48, 64, 16, ctypes.addressof(pa), ctypes.addressof(pb), None)
        assert rc == _lib.E_UNSUPPORTED


def test_decode_and_extend_refusals():
    import torch
    from mi355q import ops
    cache = ops.PackedKVCache(2, 64, 64, par(6), par(6), "cpu")
    cache.length = 40
    q = torch.zeros(2, 4, 64)
    # the existing entry points never see packed bytes: the cache is no KVCache
    assert ops._decode_check(q, cache) == "cache is not a KVCache" and ops._extend_check(q, cache) == "cache is not a KVCache"
    assert not ops.bfp_attention_decode_supported(q, cache)
    with pytest.raises(NotImplementedError, match="sliding-window.*PackedKVCache"):
        ops.bfp_attention_decode(q, cache, window=8)
    with pytest.raises(NotImplementedError, match="extend.*PackedKVCache"):
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
    with pytest.raises(ValueError, match="there is no CPU fallback"):
        cache.append(torch.zeros(2, 1, 64), torch.zeros(2, 1, 64))
    cache.length = 3
    with pytest.raises(ValueError, match="3 cached keys for 4 queries"):
        ops.bfp_attention_decode(q, cache)
    cache.length = 64
    with pytest.raises(ValueError, match="exceed the capacity"):
        cache.append(torch.zeros(2, 1, 64), torch.zeros(2, 1, 64))
    with pytest.raises(ValueError, match="not on a GPU"):
        cache.dequantised()


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


def test_packed_decode_state_refusals():
    from mi355q import harness as H, ops
    model = _tiny_llama()
    state = H.PackedDecodeState(model, 2, 40)
    assert isinstance(state, H.DecodeState) and all(isinstance(c, ops.PackedKVCache) for c in state.kv)
    assert [c.B for c in state.kv] == [2 * 4] and state.capacity == 48
    with pytest.raises(NotImplementedError, match="extend=True"):
        H.PackedDecodeState(model, 2, 40, extend=True)
    with pytest.raises(ValueError, match="mode 'fp32'"):
        H.PackedDecodeState(model, 2, 40, mode="fp32")
    with pytest.raises(NotImplementedError, match="sliding-window"):
        H.PackedDecodeState(_tiny_llama(sliding_window=8), 2, 40)
    import torch
    ids = torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="kv_storage = 'int4'"):
        H.generate(model, ids, 2, kv_storage="int4")
    with pytest.raises(NotImplementedError, match="not paged"):
        H.generate(model, ids, 2, kv_storage="int8", page_size=32)
    with pytest.raises(NotImplementedError, match="extend=True"):
        H.generate(model, ids, 2, kv_storage="int8", chunk=2)


def test_abi_version_is_25():
    from mi355q import _lib
    assert _lib.ABI_VERSION == 25 and _lib.load_library().mi355q_abi_version() == 25
    text = (ROOT / "include" / "mi355q.h").read_text()
    assert "#define MI355Q_ABI_VERSION 25" in text
    for name in ("mi355q_bfp_kv8_cache_bytes", "mi355q_bfp_kv8_append", "mi355q_bfp_kv8_decode_fp32", "mi355q_bfp_attention_decode_kv8"):
        assert name in _lib.SIGNATURES and f"int {name}(" in text
