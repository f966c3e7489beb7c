"""Incremental decoding on the host: the new C-ABI symbols, the pinned ABI version, argument errors of ops.KVCache /
ops.bfp_attention_decode raised before anything is launched (a machine without a GPU runs all of this), and the split function."""
import ctypes
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))

NEW = ("mi355q_bfp_kv_cache_bytes", "mi355q_bfp_kv_append", "mi355q_bfp_kv_decode_fp32", "mi355q_bfp_attention_decode_splits",
       "mi355q_bfp_attention_decode_workspace_bytes", "mi355q_bfp_attention_decode")
P6 = (6, 8, 127, 6, 8, 127)


def test_new_symbols_are_declared_exported_and_bound():
    from mi355q import _lib
    header = (ROOT / "include" / "mi355q.h").read_text()
    lib = _lib.load_library()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} not declared"
        assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} not bound / exported"
    assert lib.mi355q_abi_version() == 25 == _lib.ABI_VERSION


def test_c_entry_points_validate_without_a_gpu():
    from mi355q import _lib
    lib = _lib.load_library()
    pa = (ctypes.c_int32 * 6)(*P6)
    pw = (ctypes.c_int32 * 6)(10, 8, 127, 10, 8, 127)
    a = ctypes.addressof
    buf = ctypes.create_string_buffer(4096)
    p = (a(buf) + 15) // 16 * 16
    n = [ctypes.c_int64(0) for _ in range(3)]
    assert lib.mi355q_bfp_kv_cache_bytes(2, 64, 64, a(n[0]), a(n[1]), a(n[2])) == 0
    assert [x.value for x in n] == [2 * 64 * 64 * 2, 2 * 64 * 64 * 2, 2 * 16 * 64 * 4]
    assert lib.mi355q_bfp_kv_cache_bytes(2, 48, 64, a(n[0]), a(n[1]), a(n[2])) == 0 and n[1].value == 2 * 64 * 64 * 2
    assert lib.mi355q_bfp_kv_cache_bytes(2, 40, 64, a(n[0]), a(n[1]), a(n[2])) == _lib.E_UNSUPPORTED      # C % 16
    assert lib.mi355q_bfp_kv_cache_bytes(2, 64, 48, a(n[0]), a(n[1]), a(n[2])) == _lib.E_UNSUPPORTED      # D % 32
    # append: past the capacity, width 10 -- before any pointer is used
    assert lib.mi355q_bfp_kv_append(p, p, p, p, p, 2, 64, 64, 60, 5, a(pa), a(pa), None, None) == _lib.E_UNSUPPORTED
    assert lib.mi355q_bfp_kv_append(p, p, p, p, p, 2, 64, 64, 0, 5, a(pw), a(pa), None, None) == _lib.E_UNSUPPORTED
    assert lib.mi355q_bfp_kv_append(None, p, p, p, p, 2, 64, 64, 0, 5, a(pa), a(pa), None, None) == _lib.E_BADARG
    assert lib.mi355q_bfp_kv_append(p, p, p, p, p, 2, 64, 64, 7, 0, a(pa), a(pa), None, None) == 0       # nothing to append
    dec = lambda M, L, D=64, par=pa, q=p: lib.mi355q_bfp_attention_decode(q, p, p, 1, 0.0, 8.0, p, p, 2, M, L, 64, D, a(par), a(pa), None, 0, None)
    assert dec(0, 8) == _lib.E_UNSUPPORTED and dec(17, 32) == _lib.E_UNSUPPORTED and dec(4, 3) == _lib.E_UNSUPPORTED
    assert dec(1, 8, D=48) == _lib.E_UNSUPPORTED and dec(1, 8, D=160) == _lib.E_UNSUPPORTED and dec(1, 8, par=pw) == _lib.E_UNSUPPORTED
    assert dec(1, 65) == _lib.E_BADARG and dec(1, 8, q=None) == _lib.E_BADARG and dec(1, 8, q=p + 4) == _lib.E_ALIGN


def test_kv_cache_and_decode_reject_bad_arguments_before_any_launch():
    import torch
    from mi355q import ops
    with pytest.raises(ValueError, match="head_dim"):
        ops.KVCache(2, 64, 48, P6, P6, "cpu")
    with pytest.raises(ValueError, match="width"):
        ops.KVCache(2, 64, 64, (10, 8, 127, 6, 8, 127), P6, "cpu")
    with pytest.raises(ValueError, match="width"):
        ops.KVCache(2, 64, 64, P6, (6, 8, 127, 10, 8, 127), "cpu")
    with pytest.raises(ValueError, match="capacity"):
        ops.KVCache(2, 40, 64, P6, P6, "cpu")
    cache = ops.KVCache(2, 32, 64, P6, P6, "cpu")
    assert cache.length == 0
    rows = lambda B, n, D: torch.zeros(B, n, D)
    with pytest.raises(ValueError, match="capacity"):
        cache.append(rows(2, 33, 64), rows(2, 33, 64))
    with pytest.raises(ValueError, match="does not match"):
        cache.append(rows(3, 4, 64), rows(3, 4, 64))
    with pytest.raises(ValueError, match="does not match"):
        cache.append(rows(2, 4, 32), rows(2, 4, 32))
    with pytest.raises(ValueError, match="rows"):
        cache.append(rows(2, 4, 64), rows(2, 5, 64))
    with pytest.raises(ValueError, match="no CPU fallback"):
        cache.append(rows(2, 4, 64), rows(2, 4, 64))                 # a CPU tensor
    assert cache.length == 0
    cache.length = 20                                                  # (as if 20 keys had been appended)
    for q, why in ((rows(2, 0, 64), "M = 0"), (rows(2, 17, 64), "M = 17"), (rows(3, 1, 64), "does not match"),
                   (rows(2, 1, 32), "does not match"), (rows(2, 1, 64), "no CPU fallback")):
        assert not ops.bfp_attention_decode_supported(q, cache)
        with pytest.raises(ValueError, match=why):
            ops.bfp_attention_decode(q, cache)
    cache.length = 3
    with pytest.raises(ValueError, match="cached keys"):
        ops.bfp_attention_decode(rows(2, 4, 64), cache)
    with pytest.raises(ValueError, match="splits"):
        cache.length = 20
        ops.bfp_attention_decode(rows(2, 4, 64), cache, splits=0)


def test_split_function_is_pure_and_bounded():
    from mi355q import ops
    for B in (1, 2, 8, 32, 64, 512):
        for L in (1, 15, 16, 17, 33, 250, 512, 1040, 2048, 4096, 100000):
            for D in (32, 64, 128):
                blocks = (L + 15) // 16
                s = ops.decode_splits(B, L, D)
                assert s == ops.decode_splits(B, L, D) and 1 <= s <= blocks, (B, L, D, s)
                for ask in (1, 2, 3, 5, 64, 1000):
                    so = ops.decode_splits(B, L, D, ask)
                    assert 1 <= so <= min(ask, blocks), (B, L, D, ask, so)
    assert ops.decode_splits(32, 4096, 128) >= 8        # B x S fills 256 compute units at B = 32
    assert ops.decode_splits(32, 16, 128) == 1
