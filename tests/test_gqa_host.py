"""Grouped-query attention on the host: the new C-ABI symbols, the pure group-width function, every refusal of the two check functions
that concerns `group`, and TinyLlamaConfig.num_kv_heads down to the module shapes -- a machine without a GPU runs all of this, in the
manner of tests/test_extend_host.py."""
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
NEW = ("mi355q_bfp_attention_decode_grouped", "mi355q_bfp_attention_extend_grouped", "mi355q_bfp_attention_decode_group_width")


def test_the_exports_exist_and_the_abi_stays_25():
    from mi355q import _lib
    header = (ROOT / "include" / "mi355q.h").read_text()
    lib = _lib.load_library()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} not declared"
        assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} not bound / exported"
    assert lib.mi355q_abi_version() == _lib.ABI_VERSION == 25
    assert int(re.search(r"#define MI355Q_ABI_VERSION (\d+)", header).group(1)) == 25


def test_group_width_table():
    """the largest divisor of G with gw * M <= 16, restated; the issue's four examples by value"""
    from mi355q import ops
    for G in range(1, 10):
        for M in range(1, 17):
            want = max(d for d in range(1, G + 1) if G % d == 0 and d * M <= 16)
            assert ops.decode_group_width(G, M) == want, (G, M)
    assert [ops.decode_group_width(*gm) for gm in ((8, 1), (8, 4), (6, 4), (4, 16))] == [8, 4, 3, 1]
    assert ops.decode_group_width(0, 1) == ops.decode_group_width(4, 0) == ops.decode_group_width(4, 17) == 0


def test_c_entry_points_validate_without_a_gpu():
    from mi355q import _lib
    lib = _lib.load_library()
    pa = (ctypes.c_int32 * 6)(*P6)
    a = ctypes.addressof
    buf = ctypes.create_string_buffer(4096)
    p = (a(buf) + 15) // 16 * 16

    def dec(G, M=1, mx=8, lengths=None, B=2, q=p):
        return lib.mi355q_bfp_attention_decode_grouped(q, p, p, G, lengths, 1, 0.0, 8.0, p, p, B, M, mx, 64, 64, a(pa), a(pa), None, 0, None)

    def ext(G, M=20, mx=40, lengths=None, counts=None, q=p):
        return lib.mi355q_bfp_attention_extend_grouped(q, p, p, G, lengths, counts, 1, 0.0, 8.0, p, 2, M, mx, 64, 64, a(pa), a(pa), None, None)
    assert dec(0) == dec(-1) == _lib.E_BADARG and ext(0) == ext(-2) == _lib.E_BADARG
    assert dec(4, M=17, mx=20) == _lib.E_UNSUPPORTED and dec(4, M=4, mx=3) == _lib.E_UNSUPPORTED
    assert dec(4, q=None) == _lib.E_BADARG and dec(4, lengths=p + 2) == _lib.E_ALIGN and dec(4, q=p + 4) == _lib.E_ALIGN
    # launch rows B * G / gw above the grid's 65535: M = 16 leaves gw = 1
    assert dec(4, M=16, mx=16, B=16384) == _lib.E_UNSUPPORTED
    assert ext(4, M=0) == _lib.E_UNSUPPORTED and ext(4, counts=p) == _lib.E_BADARG and ext(4, q=None) == _lib.E_BADARG
    assert ext(4, lengths=p + 2) == _lib.E_ALIGN


def test_check_functions_name_every_refusal():
    """the cache and every tensor are on the CPU: a call that got as far as the device check would say "no CPU fallback" -- each of
    these names its own reason first"""
    import torch
    from mi355q import ops
    cache = ops.KVCache(2, 32, 64, P6, P6, "cpu")
    cache.length = 20                                         # (host bookkeeping only: nothing is launched)
    rows = lambda *shape: torch.zeros(*shape)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    for fn, M in ((ops.bfp_attention_decode, 4), (ops.bfp_attention_extend, 20)):
        for bad in (0, -1, 2.0, True, None):
            with pytest.raises(ValueError, match="group = .* is not an integer >= 1"):
                fn(rows(8, M, 64), cache, group=bad)
        with pytest.raises(ValueError, match=r"has 6 rows, not cache.B \* group = 2 \* 4 = 8"):
            fn(rows(6, M, 64), cache, group=4)
        with pytest.raises(ValueError, match=r"has 8 rows, not cache.B \* group = 2 \* 2 = 4"):
            fn(rows(1, 8, M, 64), cache, group=2)
        with pytest.raises(ValueError, match="does not match the cache's B = 2, D = 64"):
            fn(rows(8, M, 32), cache, group=4)
        with pytest.raises(ValueError, match="does not match the cache's B = 2, D = 64"):
            fn(rows(8, M, 64), cache)                         # (group = 1: today's message)
        # lengths / counts stay one entry per CACHE row
        with pytest.raises(ValueError, match="lengths .*one entry per cache row"):
            fn(rows(8, M, 64), cache, group=4, lengths=i32(*[20] * 8), max_length=20)
        with pytest.raises(ValueError, match="no CPU fallback"):
            fn(rows(8, M, 64), cache, group=4, lengths=i32(20, 20), max_length=20)
        with pytest.raises(ValueError, match="no CPU fallback"):
            fn(rows(2, 4, M, 64), cache, group=4)
    with pytest.raises(ValueError, match="counts .*one entry per cache row"):
        ops.bfp_attention_extend(rows(8, 20, 64), cache, group=4, lengths=i32(20, 20), counts=i32(*[20] * 8), max_length=20)
    with pytest.raises(ValueError, match="outside 1 .. 16"):
        ops.bfp_attention_decode(rows(8, 17, 64), cache, group=4)
    with pytest.raises(ValueError, match="splits = 0 < 1"):
        ops.bfp_attention_decode(rows(8, 4, 64), cache, group=4, splits=0)
    assert ops._decode_check(rows(8, 4, 64), cache, group=4).endswith("there is no CPU fallback")
    assert ops._extend_check(rows(8, 20, 64), cache, group=4).endswith("there is no CPU fallback")
    assert "group = 0" in ops._decode_check(rows(8, 4, 64), cache, group=0)
    assert "group = 0" in ops._extend_check(rows(8, 20, 64), cache, group=0)


def test_registry_functions_pass_group_through():
    import torch
    from mi355q import ops
    from mi355q.quantize import get_quantized_func
    cache = ops.KVCache(2, 32, 64, P6, P6, "cpu")
    cache.length = 20
    for key, M in (("attention_decode", 1), ("attention_extend", 20)):
        with pytest.raises(ValueError, match=r"has 6 rows, not cache.B \* group = 2 \* 4 = 8"):
            get_quantized_func(key, dict(W6))(torch.zeros(6, M, 64), cache, dict(W6), dict(W6), group=4)


def _tiny(**kw):
    import torch
    from mi355q import harness as H
    torch.manual_seed(3)
    cfg = H.TinyLlamaConfig(vocab_size=64, hidden_size=128, intermediate_size=256, num_layers=2, num_heads=4, max_positions=48, **kw)
    return H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(dict(W6), 2)), cfg


def test_config_default_and_value_error():
    import dataclasses
    from mi355q import harness as H
    fields = [f.name for f in dataclasses.fields(H.TinyLlamaConfig)]
    assert fields[-1] == "num_kv_heads" and H.TinyLlamaConfig().num_kv_heads is None
    for bad in (3, 0, 8, -2):
        with pytest.raises(ValueError, match=f"num_kv_heads = {bad} does not divide num_heads = 4"):
            H.TinyLlamaConfig(num_heads=4, num_kv_heads=bad)
    for ok in (1, 2, 4):
        assert H.TinyLlamaConfig(num_heads=4, num_kv_heads=ok).num_kv_heads == ok


def test_projection_shapes_and_state_dict_round_trip():
    import torch
    mha, _ = _tiny()
    gqa, _ = _tiny(num_kv_heads=2)
    same, _ = _tiny(num_kv_heads=4)
    assert {k: tuple(v.shape) for k, v in mha.state_dict().items()} == {k: tuple(v.shape) for k, v in same.state_dict().items()}
    assert all(torch.equal(a, b) for a, b in zip(mha.state_dict().values(), same.state_dict().values()))    # (the same seed)
    for layer in gqa.layers:
        a = layer.self_attn
        assert (a.nh, a.nkv, a.hd) == (4, 2, 32)
        assert tuple(a.k_proj.weight.shape) == tuple(a.v_proj.weight.shape) == (64, 128)
        assert tuple(a.q_proj.weight.shape) == tuple(a.o_proj.weight.shape) == (128, 128)
    assert mha.layers[0].self_attn.nkv == 4 and tuple(mha.layers[0].self_attn.k_proj.weight.shape) == (128, 128)
    sd = gqa.reference_state_dict()
    assert tuple(sd["model.layers.1.self_attn.k_proj.weight"].shape) == (64, 128)
    other, _ = _tiny(num_kv_heads=2)
    with torch.no_grad():
        for p in other.parameters():
            p.add_(1.0)
    other.load_reference_state_dict(sd)
    assert all(torch.equal(a, b) for a, b in zip(gqa.state_dict().values(), other.state_dict().values()))
    with pytest.raises(RuntimeError, match="size mismatch"):
        mha.load_reference_state_dict(sd)


def test_repeat_kv_is_head_j_from_kv_head_j_over_g():
    import torch
    from mi355q import harness as H
    t = torch.arange(2 * 3 * 5 * 4, dtype=torch.float32).reshape(2, 3, 5, 4)
    r = H._repeat_kv(t, 2)
    assert r.shape == (2, 6, 5, 4) and torch.equal(r, t.repeat_interleave(2, dim=1))


def test_shard_model_refuses_grouped_queries():
    from mi355q import sharded
    gqa, _ = _tiny(num_kv_heads=2)
    with pytest.raises(NotImplementedError, match="grouped-query"):
        sharded.shard_model(gqa)
