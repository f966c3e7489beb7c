"""Chunked prefill on the host: the new C-ABI symbol, the argument errors of ops.bfp_attention_extend (every one a ValueError raised
before anything is launched), and the pure route choice of harness.DecodeState.begin_ragged with extend=True on a stub state -- a
machine without a GPU runs all of this, in the manner of tests/test_decode_ragged_host.py."""
import ctypes
import inspect
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


def test_the_export_exists_and_the_abi_stays_25():
    from mi355q import _lib
    header = (ROOT / "include" / "mi355q.h").read_text()
    lib = _lib.load_library()
    name = "mi355q_bfp_attention_extend"
    assert re.search(r"\b%s\s*\(" % name, header), f"{name} not declared"
    assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} not bound / exported"
    assert "modeling_llama.py:301-344" in header and "modeling_llama.py:53-79" in header
    assert lib.mi355q_abi_version() == _lib.ABI_VERSION == 25
    assert int(re.search(r"#define MI355Q_ABI_VERSION (\d+)", header).group(1)) == 25


def test_c_entry_point_validates_without_a_gpu():
    from mi355q import _lib
    lib = _lib.load_library()
    pa = (ctypes.c_int32 * 6)(*P6)
    a = ctypes.addressof
    buf = ctypes.create_string_buffer(4096)
    p = (a(buf) + 15) // 16 * 16

    def ext(M, mx, lengths=p, counts=None, D=64, q=p, strides=None):
        return lib.mi355q_bfp_attention_extend(q, p, p, lengths, counts, 1, 0.0, 8.0, p, 2, M, mx, 64, D, a(pa), a(pa), strides, None)
    assert ext(0, 8) == _lib.E_UNSUPPORTED and ext(4, 3) == _lib.E_UNSUPPORTED and ext(1, 8, D=48) == _lib.E_UNSUPPORTED
    assert ext(-1, 8) == _lib.E_BADARG and ext(17, 65) == _lib.E_BADARG and ext(17, 64, q=None) == _lib.E_BADARG
    assert ext(17, 64, lengths=None, counts=p) == _lib.E_BADARG             # counts without lengths
    assert ext(17, 64, lengths=p + 2) == _lib.E_ALIGN and ext(17, 64, counts=p + 1) == _lib.E_ALIGN and ext(17, 64, q=p + 4) == _lib.E_ALIGN
    st = (ctypes.c_int64 * 4)(64 * 17, 64, 64 * 17, 66)
    assert ext(17, 64, strides=a(st)) == _lib.E_ALIGN


def test_extend_arguments_are_rejected_before_any_launch():
    """the cache and every tensor are on the CPU: a call that got as far as the device check would say "no CPU fallback" -- each of
    these names its own reason first"""
    import torch
    from mi355q import ops
    cache = ops.KVCache(2, 32, 64, P6, P6, "cpu")
    rows = lambda B, n, D: torch.zeros(B, n, D)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    ext = ops.bfp_attention_extend
    with pytest.raises(ValueError, match="M = 0 queries"):
        ext(rows(2, 0, 64), cache, lengths=i32(1, 2), max_length=8)
    with pytest.raises(ValueError, match="does not match the cache's B = 2, D = 64"):
        ext(rows(3, 20, 64), cache, lengths=i32(1, 2), max_length=20)
    with pytest.raises(ValueError, match="does not match the cache's B = 2, D = 64"):
        ext(rows(2, 20, 32), cache, lengths=i32(1, 2), max_length=20)
    with pytest.raises(ValueError, match="cache is not a KVCache"):
        ext(rows(2, 20, 64), None)
    with pytest.raises(ValueError, match="counts without lengths"):
        ext(rows(2, 20, 64), cache, counts=i32(1, 2))
    with pytest.raises(ValueError, match="ragged"):
        ext(rows(2, 20, 64), cache, max_length=20)
    with pytest.raises(ValueError, match="without max_length"):
        ext(rows(2, 20, 64), cache, lengths=i32(20, 20))
    with pytest.raises(ValueError, match="max_length = 19 outside 20"):
        ext(rows(2, 20, 64), cache, lengths=i32(19, 19), max_length=19)
    with pytest.raises(ValueError, match="max_length = 33"):
        ext(rows(2, 20, 64), cache, lengths=i32(20, 20), max_length=33)
    for bad, why in ((torch.tensor([1, 2]), "must be an int32 tensor"), ([1, 2], "must be an int32 tensor"),
                     (i32(1, 2, 3), "one entry per cache row"), (torch.zeros(2, dtype=torch.int32, device="meta"), "is on meta")):
        with pytest.raises(ValueError, match="lengths .*" + why):
            ext(rows(2, 20, 64), cache, lengths=bad, max_length=20)
        with pytest.raises(ValueError, match="counts .*" + why):
            ext(rows(2, 20, 64), cache, lengths=i32(20, 20), counts=bad, max_length=20)
    # the uniform form asks for the queries' own keys; the ragged form does not look at cache.length
    assert cache.length == 0
    with pytest.raises(ValueError, match="0 cached keys for 20 queries"):
        ext(rows(2, 20, 64), cache)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ext(rows(2, 20, 64), cache, lengths=i32(20, 20), counts=i32(20, 3), max_length=20)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ext(rows(2, 20, 64).double(), cache, lengths=i32(20, 20), max_length=20)
    assert ops._extend_check(rows(2, 20, 64), cache, i32(20, 20), i32(20, 3), 20).endswith("there is no CPU fallback")
    # the decode op keeps its limit
    assert ops.DECODE_MAX_QUERIES == 16
    with pytest.raises(ValueError, match="outside 1 .. 16"):
        ops.bfp_attention_decode(rows(2, 17, 64), cache, lengths=i32(20, 20), max_length=20)


def test_the_registry_entry():
    from mi355q.quantize import quantized_functions as QF
    assert QF.EXTRA_FUNC_MAP["attention_extend"]["block_fp"] is QF.attention_extend_block_fp
    assert "attention_extend" not in QF.QUANTIZED_FUNC_MAP
    from mi355q.quantize import get_quantized_func
    assert get_quantized_func("attention_extend", dict(W6)) is QF.attention_extend_block_fp


def _tiny():
    import torch
    from mi355q import harness as H
    torch.manual_seed(0)
    cfg = H.TinyLlamaConfig(vocab_size=97, hidden_size=128, intermediate_size=256, num_layers=1, num_heads=2, max_positions=48)
    return H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(dict(W6), 1))


def test_default_state_is_unchanged():
    from mi355q import harness as H
    sig = inspect.signature(H.DecodeState.__init__)
    assert list(sig.parameters) == ["self", "model", "batch", "capacity", "mode", "extend"]
    assert sig.parameters["mode"].default == "block_fp" and sig.parameters["extend"].default is False
    assert inspect.signature(H.generate).parameters["chunk"].default is None
    model = _tiny()
    s = H.DecodeState(model, 3, 40)
    assert (s.mode, s.batch, s.length, s.lengths, s.ragged, s._call, s.capacity, s.heads) == ("block_fp", 3, 0, [0, 0, 0], False, None, 48, 2)
    assert s.extend is False and len(s.kv) == 1 and s.kv[0].B == 6 and s.kv[0].capacity == 48
    assert H.DecodeState(model, 3, 40, "block_fp", extend=True).extend is True
    f = H.DecodeState(model, 3, 40, "fp32", extend=True)               # accepted and ignored: that route has no limit
    assert f.extend is False and f.kv == [None]


def _stub(before, extend, capacity=64, heads=2):
    """a DecodeState without a model: what begin_ragged reads and writes"""
    import torch
    from mi355q import harness as H
    s = H.DecodeState.__new__(H.DecodeState)
    s.mode, s.batch, s.capacity, s.heads, s.extend = "block_fp", len(before), capacity, heads, extend
    s.lengths, s.length, s.ragged, s._call = list(before), max(before), True, None
    s.rows_before, s.rows_after, s._rows_counts = (torch.zeros(len(before) * heads, dtype=torch.int32) for _ in range(3))
    return s


ROUTES = [  # before, counts, n, route with extend=True, what the default state says
    ([0, 0, 0], [5, 0, 23], 23, "prefill", None),
    ([0, 0, 0], [40, 40, 40], 40, "prefill", None),
    ([5, 7, 23], [1, 1, 1], 1, "decode", None),
    ([5, 0, 23], [16, 0, 16], 16, "decode", None),
    ([5, 7, 23], [3, 0, 3], 3, "decode", None),
    ([5, 0, 23], [1, 1, 1], 1, "extend", "mixed"),
    ([5, 0, 23], [1, 7, 18], 18, "extend", "mixed"),
    ([5, 7, 23], [17, 17, 17], 17, "extend", "at most 16"),
    ([5, 0, 23], [17, 0, 17], 17, "extend", "at most 16"),
    ([5, 7, 23], [2, 0, 1], 2, "extend", "unequal"),
    ([5, 7, 23], [20, 3, 1], 20, "extend", "at most 16"),
    ([5, 7, 23], [1, 1, 0], 4, "extend", "unequal"),          # every count below n: padded columns
]


@pytest.mark.parametrize("before,counts,n,route,refusal", ROUTES)
def test_route_choice(before, counts, n, route, refusal):
    s = _stub(before, extend=True)
    pos = s.begin_ragged(counts, n, 64)
    assert s._call["route"] == route
    after = [l + c for l, c in zip(before, counts)]
    assert s._call["after"] == after and s._call["max_after"] == max(after) and s._call["max_before"] == max(before)
    assert s.rows_before.tolist() == [l for l in before for _ in range(2)]
    assert s.rows_after.tolist() == [a if c else 0 for a, c in zip(after, counts) for _ in range(2)]
    assert s._rows_counts.tolist() == [c for c in counts for _ in range(2)]
    assert [p[0] for p in pos] == [min(l, max(l + c - 1, 0)) for l, c in zip(before, counts)] and all(len(p) == n for p in pos)
    s.end_ragged()
    assert s.lengths == after and s._call is None
    d = _stub(before, extend=False)
    if refusal is None:
        d.begin_ragged(counts, n, 64)
        assert d._call["route"] == route
    else:
        with pytest.raises(NotImplementedError, match=refusal):
            d.begin_ragged(counts, n, 64)
        assert d._call is None and d.lengths == before and not d.rows_before.any()


def test_refusals_that_remain():
    """capacity, positions and bad counts are refused with extend=True as before, and before anything is written"""
    for counts, n, max_positions, why in (([20, 0, 42], 42, 64, "exceed the capacity"),       # 23 + 42 > 64
                                          ([1, 7, 18], 18, 64, None),
                                          ([30, 0, 1], 42, 64, "exceed the capacity"),        # max(before) + n > 64: the append's bound
                                          ([1, 7, 18], 18, 40, "positions"),                  # 23 + 18 > 40
                                          ([1, 7], 18, 64, "counts"),
                                          ([1, 7, 19], 18, 64, "counts"),
                                          ([1, -1, 18], 18, 64, "counts")):
        s = _stub([5, 0, 23], extend=True)
        if why is None:
            s.begin_ragged(counts, n, max_positions)
            assert s._call["route"] == "extend"
            continue
        with pytest.raises(ValueError, match=why):
            s.begin_ragged(counts, n, max_positions)
        assert s._call is None and s.lengths == [5, 0, 23]
        assert not s.rows_before.any() and not s.rows_after.any() and not s._rows_counts.any()
    # the fp32 route still has no ragged form
    f = _stub([5, 0, 23], extend=False)
    f.mode = "fp32"
    with pytest.raises(NotImplementedError, match="left padding"):
        f.begin_ragged([1, 1, 1], 1, 64)
