"""The block_minifloat KV cache (ops.MinifloatKVCache, csrc/mi355q_kvbm.h), what a machine without a GPU can say about it: the class's
place among the cache classes, every refusal by name, the parameter bounds, the registry's decode_cache_kind, DecodeState(mode="block")
building one cache per layer of the layer's own format, and the two new exports' refusals."""
import ctypes as C
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))

BM = (8, 4, 8, 8, 4, 8)
W6 = dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
          data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127,
          weight_block_size=[1, 16], bias_width=6, bias_exponent_width=8, bias_exponent_bias=127, bias_block_size=[16])
BM8 = dict(name="block_minifloat", is_ptq=True, bypass=False, data_in_width=8, data_in_exponent_width=4,
           data_in_exponent_bias_width=8, data_in_block_size=[1, 16], weight_width=8, weight_exponent_width=4,
           weight_exponent_bias_width=8, weight_block_size=[1, 16], bias_width=8, bias_exponent_width=4,
           bias_exponent_bias_width=8, bias_block_size=[16], mi355q_values_matmul="fp32")
BL8 = dict(name="block_log", is_ptq=True, bypass=False, data_in_width=8, data_in_exponent_bias_width=8, data_in_block_size=[1, 16],
           weight_width=8, weight_exponent_bias_width=8, weight_block_size=[1, 16], bias_width=8, bias_exponent_bias_width=8,
           bias_block_size=[16])
NAMES = ("mi355q_bm_kv_append", "mi355q_bm_attention_decode")


def _mixed_model(formats=(W6, BM8), family="llama"):
    """a tiny model on the CPU whose layer i has every node in formats[i]"""
    import torch
    from mi355q import harness as H
    torch.manual_seed(0)
    layers = len(formats)
    if family == "llama":
        cfg = H.TinyLlamaConfig(vocab_size=97, hidden_size=128, intermediate_size=256, num_layers=layers, num_heads=2, max_positions=48)
        qc = H.expand_llama_quant_config(dict(formats[0]), layers)
        for i, f in enumerate(formats):
            qc[f"model_layer_{i}"] = H.expand_llama_quant_config(dict(f), 1)["model_layer_0"]
        return H.TinyLlamaForCausalLM(cfg, qc)
    cfg = H.TinyOPTConfig(vocab_size=97, hidden_size=128, ffn_dim=256, num_layers=layers, num_heads=2, max_positions=48)
    qc = H.expand_quant_config(dict(formats[0]), layers)
    for i, f in enumerate(formats):
        qc[f"model_layer_{i}"] = H.expand_quant_config(dict(f), 1)["model_layer_0"]
    return H.TinyOPTForCausalLM(cfg, qc)


def test_abi_stays_25_and_the_new_names_are_declared_bound_and_exported():
    from mi355q import _lib
    lib = _lib.load_library()
    assert _lib.ABI_VERSION == 25 and lib.mi355q_abi_version() == 25
    text = (ROOT / "include" / "mi355q.h").read_text()
    assert "#define MI355Q_ABI_VERSION 25" in text
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and f"int {name}(" in text, name


def test_a_class_of_its_own_on_kvcaches_storage():
    import torch
    from mi355q import ops
    c = ops.MinifloatKVCache(3, 48, 64, BM, BM, "cpu")
    assert isinstance(c, ops._KVCacheBase)
    assert not isinstance(c, (ops.KVCache, ops.PackedKVCache, ops.PagedKVCache, ops.PagedPackedKVCache))
    ref = ops.KVCache(3, 48, 64, (6, 8, 127, 6, 8, 127), (6, 8, 127, 6, 8, 127), "cpu")
    assert not isinstance(ref, ops.MinifloatKVCache)
    for name in ("kq", "vq", "stage"):
        assert getattr(c, name).numel() == getattr(ref, name).numel() and getattr(c, name).dtype == torch.uint8
    assert c.length == 0 and c.capacity == 48 and c.qk_params == BM and list(c._pa) == list(BM) and list(c._pb) == list(BM)
    q = torch.zeros(3, 1, 64)
    assert ops._decode_check(q, c) == "cache is not a KVCache" and not ops.bfp_attention_decode_supported(q, c)
    assert ops._extend_check(q, c) == "cache is not a KVCache"
    c.length = 5
    c.reset()
    assert c.length == 0


def test_refusals_by_name():
    import torch
    from mi355q import ops
    c = ops.MinifloatKVCache(2, 32, 32, BM, BM, "cpu")
    q = torch.zeros(2, 1, 32)
    with pytest.raises(NotImplementedError, match="no sliding-window kernel reads a MinifloatKVCache"):
        ops.bfp_attention_decode(q, c, window=4)
    with pytest.raises(NotImplementedError, match="no extend kernel reads a MinifloatKVCache"):
        ops.bfp_attention_extend(q, c)
    for name in ("fork", "reorder", "ensure", "trim"):
        with pytest.raises(NotImplementedError, match=f"MinifloatKVCache.{name}"):
            getattr(c, name)()
    # the decode's own checks, before anything touches a device
    with pytest.raises(ValueError, match="0 cached keys for 1 queries"):
        ops.bfp_attention_decode(q, c)
    c.length = 1
    with pytest.raises(ValueError, match="there is no CPU fallback"):
        ops.bfp_attention_decode(q, c)
    with pytest.raises(ValueError, match="M = 17 queries outside 1 .. 16"):
        ops.bfp_attention_decode(torch.zeros(2, 17, 32), c)
    with pytest.raises(ValueError, match="has 2 rows, not cache.B \\* group"):
        ops.bfp_attention_decode(q, c, group=2)
    with pytest.raises(ValueError, match="there is no CPU fallback"):
        c.append(torch.zeros(2, 1, 32), torch.zeros(2, 1, 32))
    with pytest.raises(ValueError, match="exceed the capacity"):
        c.append(torch.zeros(2, 40, 32), torch.zeros(2, 40, 32))
    with pytest.raises(ValueError, match="MinifloatKVCache.dequantised: the cache is not on a GPU"):
        c.dequantised()


@pytest.mark.parametrize("bad,why", [
    ((8, 0, 8), "exponent width 0 outside 1 .. 8"), ((12, 9, 8), "exponent width 9 outside 1 .. 8"),
    ((5, 4, 8), "leaves 0 mantissa bits"), ((12, 3, 8), "leaves 8 mantissa bits"),
    ((8, 4, 0), "exponent bias width 0 outside 1 .. 8"), ((8, 4, 9), "exponent bias width 9 outside 1 .. 8")])
def test_parameter_bounds(bad, why):
    from mi355q import ops
    for params in (bad + BM[3:], BM[:3] + bad):
        with pytest.raises(ValueError, match=f"MinifloatKVCache qk_params: .*{why}"):
            ops.MinifloatKVCache(2, 32, 32, params, BM, "cpu")
        with pytest.raises(ValueError, match=f"MinifloatKVCache pv_params: .*{why}"):
            ops.MinifloatKVCache(2, 32, 32, BM, params, "cpu")


def test_parameter_edges_and_shapes():
    from mi355q import ops
    for ok in ((3, 1, 1), (9, 1, 8), (16, 8, 8), (6, 3, 2)):      # mantissa bits 1 and 7, exponent widths 1 and 8
        ops.MinifloatKVCache(2, 32, 32, ok + ok, ok + ok, "cpu")
    with pytest.raises(ValueError, match="y exponent bias width\\) expected"):
        ops.MinifloatKVCache(2, 32, 32, BM[:3], BM, "cpu")
    with pytest.raises(ValueError, match="MinifloatKVCache: head_dim 48"):
        ops.MinifloatKVCache(2, 32, 48, BM, BM, "cpu")
    with pytest.raises(ValueError, match="MinifloatKVCache: capacity 40"):
        ops.MinifloatKVCache(2, 40, 32, BM, BM, "cpu")
    with pytest.raises(ValueError, match="MinifloatKVCache: B = 0"):
        ops.MinifloatKVCache(0, 32, 32, BM, BM, "cpu")


def test_decode_cache_kind():
    from mi355q.quantize import get_quantized_func
    from mi355q.quantize.quantized_functions import EXTRA_FUNC_MAP, decode_cache_kind, decode_cache_params
    assert decode_cache_kind(W6, W6, 64) == ("block_fp",) + decode_cache_params(W6, W6, 64) == ("block_fp", (6, 8, 127, 6, 8, 127), (6, 8, 127, 6, 8, 127))
    assert decode_cache_kind(BM8, BM8, 64) == ("block_minifloat", BM, BM)
    b6 = dict(BM8, data_in_width=6, data_in_exponent_width=3, weight_exponent_bias_width=2)
    assert decode_cache_kind(BM8, b6, 128) == ("block_minifloat", BM, (6, 3, 8, 8, 4, 2))
    with pytest.raises(ValueError, match="block_log and block_log"):
        decode_cache_kind(BL8, BL8, 64)
    with pytest.raises(ValueError, match="block_fp and block_minifloat"):
        decode_cache_kind(W6, BM8, 64)
    with pytest.raises(ValueError, match="bypassed and block_minifloat"):
        decode_cache_kind(dict(BM8, bypass=True), BM8, 64)
    with pytest.raises(ValueError, match="block_fp and bypassed"):
        decode_cache_kind(W6, dict(W6, bypass=True), 64)
    with pytest.raises(ValueError, match="block_minifloat KV cache: head_dim 48"):
        decode_cache_kind(BM8, BM8, 48)
    with pytest.raises(ValueError, match="block_fp KV cache: head_dim 48"):
        decode_cache_kind(W6, W6, 48)
    with pytest.raises(ValueError, match="weight_block_size \\[16, 1\\] of the second product is not \\[1, 16\\]"):
        decode_cache_kind(BM8, dict(BM8, weight_block_size=[16, 1]), 64)
    with pytest.raises(ValueError, match="data_in .*= \\(12, 3, 8\\) of the first product"):
        decode_cache_kind(dict(BM8, data_in_width=12, data_in_exponent_width=3), BM8, 64)
    # decode_cache_params itself still refuses every other format
    with pytest.raises(ValueError, match="the first attention product is block_minifloat, not block_fp"):
        decode_cache_params(BM8, BM8, 64)
    assert set(EXTRA_FUNC_MAP["attention_decode"]) == {"block_fp", "block_minifloat"} and set(EXTRA_FUNC_MAP["attention_extend"]) == {"block_fp"}
    assert get_quantized_func("attention_decode", BM8).__name__ == "attention_decode_block_minifloat"


@pytest.mark.parametrize("family", ["llama", "opt"])
def test_decode_state_mode_block_builds_each_layers_own_cache(family):
    from mi355q import harness as H, ops
    model = _mixed_model((W6, BM8), family)
    state = H.DecodeState(model, 2, 40, "block")
    assert state.mode == "block" and state.capacity == 48 and state.cached
    assert type(state.kv[0]) is ops.KVCache and type(state.kv[1]) is ops.MinifloatKVCache
    assert state.kv[0].B == state.kv[1].B == 4 and state.kv[1].qk_params == BM and state.kv[1].capacity == 48
    assert state.kv[0].qk_params == (6, 8, 127, 6, 8, 127)
    state.reset()
    # mode "block_fp" on the same model declines as before, naming the layer and the format
    with pytest.raises(ValueError, match="layer 1.*block_minifloat, not block_fp"):
        H.DecodeState(model, 2, 40, "block_fp")
    assert H.DecodeState(model, 2, 40, "fp32").kv == [None, None]
    with pytest.raises(ValueError, match="neither 'block_fp' nor 'block' nor 'fp32'"):
        H.DecodeState(model, 2, 40, "bf16")


def test_decode_state_mode_block_refusals():
    from mi355q import harness as H
    with pytest.raises(ValueError, match="DecodeState\\(mode='block'\\), layer 1: .*block_log and block_log"):
        H.DecodeState(_mixed_model((BM8, BL8)), 2, 40, "block")
    mixed_layer = _mixed_model((BM8, BM8))
    qc = mixed_layer.layers[0].self_attn.qc
    qc["matmul_1"] = dict(qc["matmul_1"], bypass=True)
    with pytest.raises(ValueError, match="layer 0: .*block_minifloat and bypassed"):
        H.DecodeState(mixed_layer, 2, 40, "block")
    model = _mixed_model((W6, BM8))
    with pytest.raises(NotImplementedError, match="mode='block'.*extend=True"):
        H.DecodeState(model, 2, 40, "block", extend=True)
    with pytest.raises(NotImplementedError, match="mode='block'.*page_size"):
        H.PagedDecodeState(model, 2, 40, "block", page_size=32)
    with pytest.raises(NotImplementedError, match="mode='block'.*page_size"):
        H._new_state(model, 2, 40, "block", False, 32, None)          # (generate(mode="block", page_size=32))
    with pytest.raises(NotImplementedError, match="only a paged state can fork"):
        H.DecodeState(model, 2, 40, "block").fork(0, 1)
    model.cfg.sliding_window = 8
    with pytest.raises(NotImplementedError, match="mode='block'.*sliding-window"):
        H.DecodeState(model, 2, 40, "block")
    model.cfg.sliding_window = None
    # the ragged routes' refusals are DecodeState's own: a mixed call, more than 16 tokens behind a non-empty row
    state = H.DecodeState(model, 2, 40, "block")
    state.lengths = [5, 0]
    with pytest.raises(NotImplementedError, match="a mixed call"):
        state.begin_ragged([1, 3], 3, 48)
    state.lengths = [5, 5]
    with pytest.raises(NotImplementedError, match="17 new tokens behind non-empty"):
        state.begin_ragged([17, 17], 17, 48)


def _call(name, **over):
    """the export with arguments that pass every check (fake, aligned addresses -- a refused call dereferences none of them)"""
    from mi355q import _lib
    lib = _lib.load_library()
    qk, pv = (C.c_int32 * 6)(*over.pop("qk", BM)), (C.c_int32 * 6)(*over.pop("pv", BM))
    a = dict(kq=0x1000, vq=0x2000, stage=0x3000, k=0x4000, v=0x5000, q=0x6000, out=0x7000, ws=0x8000, lengths=0x9000, counts=None,
             B=2, C=32, D=32, n=1, L=4, M=1, G=0, causal=1, splits=0, qk=C.addressof(qk), pv=C.addressof(pv), strides=None)
    a.update(over)
    if name == "mi355q_bm_kv_append":
        return lib.mi355q_bm_kv_append(a["kq"], a["vq"], a["stage"], a["k"], a["v"], a["lengths"], a["counts"], a["B"], a["C"], a["D"], a["n"],
                                       a["L"], a["qk"], a["pv"], a["strides"], None)
    return lib.mi355q_bm_attention_decode(a["q"], a["kq"], a["vq"], a["G"], a["lengths"], a["causal"], 0.0, 0.0, a["out"], a["ws"], a["B"], a["M"],
                                          a["L"], a["C"], a["D"], a["qk"], a["pv"], a["strides"], a["splits"], None)


def test_the_exports_refusals_without_a_gpu():
    from mi355q import _lib
    BAD, UNS, ALIGN = _lib.E_BADARG, _lib.E_UNSUPPORTED, _lib.E_ALIGN
    ap, dec = "mi355q_bm_kv_append", "mi355q_bm_attention_decode"
    for name in NAMES:
        assert _call(name, lengths=None) == BAD                       # always the ragged form
        assert _call(name, kq=None) == BAD and _call(name, B=0) == BAD
        assert _call(name, D=48) == UNS and _call(name, C=40) == UNS and _call(name, D=160) == UNS
        assert _call(name, kq=0x1008) == ALIGN and _call(name, lengths=0x9002) == ALIGN
        for bad in ((8, 0, 8), (12, 9, 8), (5, 4, 8), (12, 3, 8), (8, 4, 0), (8, 4, 9)):
            assert _call(name, qk=BM[:3] + bad) == UNS and _call(name, pv=BM[:3] + bad) == UNS, (name, bad)
        st = (C.c_int64 * 4)(32, 32, 34, 32)
        assert _call(name, strides=C.addressof(st)) == ALIGN
    assert _call(ap, n=0) == 0                                        # nothing to do
    assert _call(ap, n=-1) == BAD and _call(ap, L=32, n=1) == UNS and _call(ap, stage=None) == BAD and _call(ap, k=None) == BAD
    assert _call(ap, n=0, qk=BM[:3] + (5, 4, 8)) == 0                 # (as for the bf16 cache: the early 0 comes first)
    for bad in ((8, 0, 8), (5, 4, 8), (12, 3, 8), (8, 4, 9)):         # the decode reads all four operands' words
        assert _call(dec, qk=bad + BM[3:]) == UNS and _call(dec, pv=bad + BM[3:]) == UNS
    assert _call(dec, M=0) == UNS and _call(dec, M=17, L=20) == UNS and _call(dec, M=5, L=4) == UNS
    assert _call(dec, L=33) == BAD and _call(dec, G=-1) == BAD and _call(dec, splits=-1) == BAD and _call(dec, ws=None) == BAD
    assert _call(dec, q=None) == BAD and _call(dec, out=0x7004) == ALIGN
    assert _call(dec, G=3, B=65535, M=16, L=16) == UNS                # more than 65535 launch rows


def test_the_debug_hook_knows_the_new_ids_behind_the_old_ones():
    """ids 25 and 26 are the block_minifloat append and decode, shown by mi355q_debug_kv_call_all; the 25 ids in front keep their places
    (tests/test_kv_api_codes.py replays them) and mi355q_debug_kv_call keeps to them"""
    from mi355q import _lib
    lib = _lib.load_library()
    old = lib.mi355q_debug_kv_call
    old.restype, old.argtypes = C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    fn = lib.mi355q_debug_kv_call_all
    fn.restype, fn.argtypes = C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    qk = (C.c_int32 * 6)(*BM)
    out = (C.c_int64 * 18)()
    a = (C.c_int64 * 27)(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, 0x9000, 0, 0, 0, 0, 0,
                         2, 32, 0, 0, 0, 32, 1, 4, 1, 0, 1, 0, 0)
    for id_ in (25, 26):
        assert fn(id_, a, qk, qk, None, out) == 0 and out[0] == 0 and out[1] == 1, (id_, list(out))
    bfp = (C.c_int32 * 6)(6, 8, 127, 6, 8, 127)
    for id_ in (25, 26):                                              # block_fp's words (exponent width 8, bias 127) are not block_minifloat's
        assert fn(id_, a, bfp, bfp, None, out) == 0 and out[0] == _lib.E_UNSUPPORTED and out[1] == 0
    half = (C.c_int32 * 6)(12, 9, 0, *BM[3:])                        # the append reads the weight sides only, the decode all four
    assert fn(25, a, half, half, None, out) == 0 and out[0] == 0 and out[1] == 1
    assert fn(26, a, half, half, None, out) == 0 and out[0] == _lib.E_UNSUPPORTED and out[1] == 0
    assert fn(16, a, bfp, bfp, None, out) == 0 and out[0] == 0 and out[1] == 1        # KVX_KV8_APPEND, unchanged
    assert fn(27, a, qk, qk, None, out) == _lib.E_BADARG and old(25, a, qk, qk, None, out) == _lib.E_BADARG
    assert old(16, a, bfp, bfp, None, out) == 0 and out[0] == 0 and out[1] == 1
