"""Ragged batches on the host: the new C-ABI symbols, and the argument errors of the ragged forms of ops.KVCache.append /
dequantised and ops.bfp_attention_decode, every one a ValueError raised before anything is launched (a machine without a GPU runs
all of this, in the manner of tests/test_small_m_host.py).  The split function is the one it was."""
import ctypes
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))

NEW = ("mi355q_bfp_kv_append_ragged", "mi355q_bfp_kv_decode_fp32_ragged", "mi355q_bfp_attention_decode_ragged")
P6 = (6, 8, 127, 6, 8, 127)


def test_new_symbols_are_declared_exported_and_bound():
    from mi355q import _lib
    header = (ROOT / "include" / "mi355q.h").read_text()
    lib = _lib.load_library()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} not declared"
        assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} not bound / exported"
    assert "BEFORE the append" in header and "INCLUDING the M queries' own keys" in header


def test_c_entry_points_validate_without_a_gpu():
    from mi355q import _lib
    lib = _lib.load_library()
    pa = (ctypes.c_int32 * 6)(*P6)
    a = ctypes.addressof
    buf = ctypes.create_string_buffer(4096)
    p = (a(buf) + 15) // 16 * 16
    app = lambda n, mx, lengths=p, kq=p: lib.mi355q_bfp_kv_append_ragged(kq, p, p, p, p, lengths, None, 2, 64, 64, n, mx, a(pa), a(pa), None, None)
    assert app(5, 60) == _lib.E_UNSUPPORTED                      # max_length + n > C: nothing is written
    assert app(0, 64) == 0                                       # nothing to append
    assert app(5, 10, lengths=None) == _lib.E_BADARG and app(5, 10, kq=None) == _lib.E_BADARG
    assert app(5, 10, lengths=p + 2) == _lib.E_ALIGN and app(5, -1) == _lib.E_BADARG
    dec = lambda M, mx, lengths=p, D=64: lib.mi355q_bfp_attention_decode_ragged(p, p, p, lengths, 1, 0.0, 8.0, p, p, 2, M, mx, 64, D, a(pa), a(pa),
                                                                                None, 0, None)
    assert dec(0, 8) == _lib.E_UNSUPPORTED and dec(17, 32) == _lib.E_UNSUPPORTED and dec(4, 3) == _lib.E_UNSUPPORTED
    assert dec(1, 8, D=48) == _lib.E_UNSUPPORTED
    assert dec(1, 65) == _lib.E_BADARG and dec(1, 8, lengths=None) == _lib.E_BADARG and dec(1, 8, lengths=p + 1) == _lib.E_ALIGN
    deq = lambda mx, lengths=p: lib.mi355q_bfp_kv_decode_fp32_ragged(p, p, lengths, p, p, 2, 64, 64, mx, None)
    assert deq(65) == _lib.E_BADARG and deq(0) == 0 and deq(8, lengths=None) == _lib.E_BADARG


def test_ragged_arguments_are_rejected_before_any_launch():
    """the cache and every tensor are on the CPU: a call that got as far as the device check would say "no CPU fallback" -- each of
    these names its own reason first"""
    import torch
    from mi355q import ops
    cache = ops.KVCache(2, 32, 64, P6, P6, "cpu")
    rows = lambda B, n, D: torch.zeros(B, n, D)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    k = rows(2, 4, 64)
    bad = ((torch.tensor([1, 2]), "lengths must be an int32 tensor"), (torch.tensor([1.0, 2.0]), "lengths must be an int32 tensor"),
           ([1, 2], "lengths must be an int32 tensor"), (i32(1, 2, 3), "one entry per cache row"), (i32(1, 2)[None], "one entry per cache row"),
           (torch.zeros(2, dtype=torch.int32, device="meta"), "is on meta"))
    for lengths, why in bad:
        with pytest.raises(ValueError, match=why):
            cache.append(k, k, lengths=lengths, max_length=8)
        with pytest.raises(ValueError, match=why):
            ops.bfp_attention_decode(rows(2, 1, 64), cache, lengths=lengths, max_length=8)
        with pytest.raises(ValueError, match=why):
            cache.dequantised(lengths=lengths, max_length=8)
        with pytest.raises(ValueError, match=why.replace("lengths", "counts")):
            cache.append(k, k, lengths=i32(1, 2), counts=lengths, max_length=8)
    # the host bound
    with pytest.raises(ValueError, match="without max_length"):
        cache.append(k, k, lengths=i32(1, 2))
    with pytest.raises(ValueError, match="without max_length"):
        ops.bfp_attention_decode(rows(2, 1, 64), cache, lengths=i32(1, 2))
    with pytest.raises(ValueError, match="without max_length"):
        cache.dequantised(lengths=i32(1, 2))
    with pytest.raises(ValueError, match="exceed the capacity"):
        cache.append(k, k, lengths=i32(1, 2), max_length=29)          # 29 + 4 > 32
    with pytest.raises(ValueError, match="no CPU fallback"):
        cache.append(k, k, lengths=i32(1, 2), max_length=28)          # 28 + 4 fits: on to the device check
    with pytest.raises(ValueError, match="max_length = 33"):
        ops.bfp_attention_decode(rows(2, 1, 64), cache, lengths=i32(1, 2), max_length=33)
    with pytest.raises(ValueError, match="max_length = 3 outside 4"):
        ops.bfp_attention_decode(rows(2, 4, 64), cache, lengths=i32(4, 4), max_length=3)
    with pytest.raises(ValueError, match="max_length = 33"):
        cache.dequantised(lengths=i32(1, 2), max_length=33)
    # counts / max_length without lengths are not silently dropped
    with pytest.raises(ValueError, match="ragged"):
        cache.append(k, k, counts=i32(1, 2))
    with pytest.raises(ValueError, match="ragged"):
        cache.append(k, k, max_length=8)
    with pytest.raises(ValueError, match="ragged"):
        ops.bfp_attention_decode(rows(2, 1, 64), cache, max_length=8)
    # a ragged decode does not look at cache.length (0 here): it gets as far as the device check
    assert cache.length == 0
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.bfp_attention_decode(rows(2, 1, 64), cache, lengths=i32(1, 2), max_length=8)
    assert not ops.bfp_attention_decode_supported(rows(2, 1, 64), cache)      # the uniform form still asks for its keys
    assert cache.length == 0


def test_decode_splits_is_unchanged():
    """the function of (B, L, D) it was, restated: 512 / B workgroups wanted, at least two key pairs each, at most 64, evened out"""
    from mi355q import ops

    def want(B, L, override=0):
        NP = (L + 31) // 32
        w = override if override > 0 else (512 + B - 1) // B
        if override <= 0 and w > NP // 2:
            w = NP // 2
        w = max(1, min(w, 64, NP))
        pps = (NP + w - 1) // w
        return (NP + pps - 1) // pps

    for B in (1, 2, 8, 32, 64, 512):
        for L in (1, 15, 16, 17, 33, 250, 257, 512, 1040, 2048, 4096, 100000):
            for D in (32, 64, 128):
                assert ops.decode_splits(B, L, D) == want(B, L), (B, L, D)
                for ask in (1, 2, 3, 4, 5, 64, 1000):
                    assert ops.decode_splits(B, L, D, ask) == want(B, L, ask), (B, L, D, ask)
    assert ops.decode_splits(32, 4096, 128) == 16 and ops.decode_splits(32, 512, 64) == 8 and ops.decode_splits(8, 257, 64, 4) == 3
