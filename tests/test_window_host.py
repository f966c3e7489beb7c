"""Sliding-window attention, everything a machine without a GPU can check: the new exports and their argument errors, the reasons
ops._decode_check / ops._extend_check give for a window, TinyLlamaConfig.sliding_window, and the page trim of ops.PagedKVCache on its
host mirror (which pages go, reference counts, ensure / release after a trim, the free list)."""
import ctypes
import dataclasses
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))

PAR = (6, 8, 127, 6, 8, 127)
NAMES = ("mi355q_bfp_attention_decode_window", "mi355q_bfp_attention_extend_window", "mi355q_bfp_attention_decode_window_span",
         "mi355q_bfp_attention_decode_window_workspace_bytes")


def test_exports_and_abi():
    from mi355q import _lib
    lib = _lib.load_library()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} not bound / exported"
    assert lib.mi355q_abi_version() == _lib.ABI_VERSION == 25


def test_span_and_workspace():
    """span = min(max_length, W + M - 1 + 31); the workspace and the default splits are those of span keys"""
    from mi355q import _lib, ops
    lib = _lib.load_library()
    span = lib.mi355q_bfp_attention_decode_window_span
    assert span(1, 8192, 1024) == 1024 + 31 and span(16, 8192, 64) == 64 + 15 + 31
    assert span(1, 100, 100) == 100 and span(1, 100, 5000) == 100 and span(4, 40, 20) == 40 and span(1, 40, 1) == 32
    assert span(0, 40, 8) == 0 and span(1, 0, 8) == 0 and span(1, 40, 0) == 0
    ws = lib.mi355q_bfp_attention_decode_window_workspace_bytes
    for splits in (0, 1, 5):
        assert ws(8, 1, 32768, 1024, 128, splits) == lib.mi355q_bfp_attention_decode_workspace_bytes(8, 1055, 128, splits)
    assert ws(8, 1, 32768, 0, 128, 0) == 0 and ws(8, 17, 32768, 8, 128, 0) == 0
    assert ops.decode_splits(8, 1055, 128) < ops.decode_splits(8, 32768, 128)


def _call(lib, which, **over):
    """one *_window call with valid scalars and 16-byte aligned fake addresses, `over` on top; argument errors come before any launch"""
    par = (ctypes.c_int32 * 6)(*PAR)
    a = dict(q=4096, kq=8192, vq=12288, G=0, lengths=16384, counts=0, table=0, causal=1, window=8, out=20480, ws=24576, B=2, M=4,
             max_length=40, max_pages=1, num_pages=1, P=64, D=64)
    a.update(over)
    pp = ctypes.addressof(par)
    if which == "decode":
        return lib.mi355q_bfp_attention_decode_window(a["q"], a["kq"], a["vq"], a["G"], a["lengths"], a["table"], a["causal"], a["window"], 0.0,
                                                      8.0, a["out"], a["ws"], a["B"], a["M"], a["max_length"], a["max_pages"], a["num_pages"],
                                                      a["P"], a["D"], pp, pp, None, 0, None)
    return lib.mi355q_bfp_attention_extend_window(a["q"], a["kq"], a["vq"], a["G"], a["lengths"], a["counts"], a["table"], a["causal"],
                                                  a["window"], 0.0, 8.0, a["out"], a["B"], a["M"], a["max_length"], a["max_pages"],
                                                  a["num_pages"], a["P"], a["D"], pp, pp, None, None)


@pytest.mark.parametrize("which", ["decode", "extend"])
def test_badarg_before_any_launch(which):
    from mi355q import _lib
    lib = _lib.load_library()
    bad = _lib.E_BADARG
    assert _call(lib, which, window=0) == bad and _call(lib, which, window=-3) == bad
    assert _call(lib, which, causal=0) == bad
    assert _call(lib, which, lengths=0) == bad                       # always the ragged form
    assert _call(lib, which, q=0) == bad and _call(lib, which, out=0) == bad
    assert _call(lib, which, max_length=65) == bad                   # above the contiguous capacity max_pages * P
    assert _call(lib, which, G=-1) == bad
    # the paged forms' checks, with a table
    assert _call(lib, which, table=28672, P=48, max_pages=2, num_pages=4) == bad          # no power of two
    assert _call(lib, which, table=28672, P=32, max_pages=1, num_pages=4) == bad          # max_length 40 > max_pages * P
    assert _call(lib, which, table=28672, P=32, max_pages=2, num_pages=0) == bad
    assert _call(lib, which, table=28674, P=32, max_pages=2, num_pages=4) == _lib.E_ALIGN
    assert _call(lib, which, M=0) == _lib.E_UNSUPPORTED
    if which == "decode":
        assert _call(lib, which, ws=0) == bad and _call(lib, which, M=17) == _lib.E_UNSUPPORTED


def test_check_reasons():
    import torch
    from mi355q import ops
    cache = ops.KVCache(2, 64, 64, PAR, PAR, "cpu")
    cache.length = 40
    rows = lambda M: torch.zeros(2, M, 64)
    for check, M in ((ops._decode_check, 4), (ops._extend_check, 20)):
        assert check(rows(M), cache, window=8).endswith("there is no CPU fallback")       # taken, up to the device
        assert check(rows(M), cache).endswith("there is no CPU fallback")
        assert "window = 0" in check(rows(M), cache, window=0)
        assert "window = -1" in check(rows(M), cache, window=-1)
        assert "window = 8.0" in check(rows(M), cache, window=8.0)
        assert "window = True" in check(rows(M), cache, window=True)
        assert "causal=False" in check(rows(M), cache, causal=False, window=8)
        assert check(rows(M), cache, causal=False).endswith("there is no CPU fallback")
    for fn, M in ((ops.bfp_attention_decode, 4), (ops.bfp_attention_extend, 20)):
        with pytest.raises(ValueError, match="window = 0"):
            fn(rows(M), cache, window=0)
        with pytest.raises(ValueError, match="causal=False"):
            fn(rows(M), cache, causal=False, window=3)
        with pytest.raises(TypeError):
            fn(rows(M), cache, True, None, None, False, None, None, None, 1, 8)            # (keyword-only)
    import inspect
    for fn in (ops.bfp_attention_decode, ops.bfp_attention_extend):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "window" and last.default is None and last.kind is inspect.Parameter.KEYWORD_ONLY


def test_registry_passes_window():
    import inspect
    from mi355q.quantize import quantized_functions as QF
    for fn in (QF.attention_decode_block_fp, QF.attention_extend_block_fp):
        p = inspect.signature(fn).parameters["window"]
        assert p.default is None and list(inspect.signature(fn).parameters)[-1] == "window"


def test_config_field():
    from mi355q import harness as H
    fields = [f.name for f in dataclasses.fields(H.TinyLlamaConfig)]
    assert fields[-2:] == ["sliding_window", "num_kv_heads"] and H.TinyLlamaConfig().sliding_window is None
    assert H.TinyLlamaConfig(sliding_window=1).sliding_window == 1
    for bad in (0, -4, 2.0, True):
        with pytest.raises(ValueError, match="sliding_window"):
            H.TinyLlamaConfig(sliding_window=bad)
    assert not hasattr(H.TinyOPTConfig(), "sliding_window")


def test_mask_is_the_window_mask():
    """query i of n at p = L - n + i: finfo.min above p and below p - W + 1, 0 between; window None: the causal mask as it was"""
    import torch
    from mi355q import harness as H
    fmin = torch.finfo(torch.float32).min
    for n, L, W in ((5, 12, 3), (12, 12, 1), (4, 9, 20), (1, 7, 4)):
        m = H._causal_mask(n, L, W, torch.float32, "cpu")
        for i in range(n):
            p = L - n + i
            want = [0.0 if max(0, p - W + 1) <= j <= p else fmin for j in range(L)]
            assert m[i].tolist() == want, (n, L, W, i)
        assert torch.equal(H._causal_mask(n, L, None, torch.float32, "cpu"), torch.full((n, L), fmin).triu(1 + L - n))


def _paged(P, num_pages=12, max_pages=6, B=3, pad_page=None):
    from mi355q import ops
    return ops.PagedKVCache(B, 64, PAR, PAR, "cpu", page_size=P, num_pages=num_pages, max_pages=max_pages, pad_page=pad_page)


def _sound(c):
    held = [p for row in c.held for p in row if p is not None]
    assert len(c.free) == len(set(c.free)), "a page is twice in the free list"
    assert not set(c.free) & set(held), "a held page is free"
    assert all(c.refs[p] == held.count(p) for p in set(held)) and all(c.refs[p] == 0 for p in c.free)
    for b, row in enumerate(c.held):
        assert c.table[b, :len(row)].tolist() == [c.pad_page if p is None else p for p in row]
        assert bool((c.table[b, len(row):] == c.pad_page).all())


@pytest.mark.parametrize("P", [32, 64])
def test_trim_which_pages_go(P):
    """page i goes when (i + 1) P <= length - W + 1: lengths on both sides of every edge"""
    W = 10
    for length in (W - 1, P + W - 2, P + W - 1, P + W, 2 * P + W - 2, 2 * P + W - 1, 3 * P):
        c = _paged(P, pad_page=11)
        c.ensure([length, 3 * P, 1])
        before = [list(r) for r in c.held]
        c.trim([length, 0, 1], W)
        gone = max(length - W + 1, 0) // P
        assert c.held[0] == [None] * gone + before[0][gone:], (P, length)
        assert c.held[1] == before[1] and c.held[2] == before[2]
        assert set(before[0][:gone]) <= set(c.free) and not set(before[0][gone:]) & set(c.free)
        assert bool((c.table[0, :gone] == 11).all())
        _sound(c)
    c = _paged(P)
    c.ensure([3 * P, 3 * P, 3 * P])
    c.trim([3 * P] * 3, 1)                                   # W = 1: every full page
    assert all(row == [None, None, None] for row in c.held) and len(c.free) == 12
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="window"):
            c.trim([0, 0, 0], bad)
    with pytest.raises(ValueError, match="lengths"):
        c.trim([0, 0], 4)


def test_trim_respects_shared_pages():
    c = _paged(32)
    c.ensure([100, 0, 0])
    shared = list(c.held[0][:2])
    c.share_prefix(0, 1, 2)
    c.trim([100, 34, 0], 4)                                  # row 0 gives back pages 0 .. 2, row 1 nothing yet (34 - 4 + 1 < 32)
    assert c.held[0][:3] == [None] * 3 and c.held[1] == shared
    assert all(c.refs[p] == 1 for p in shared) and not set(shared) & set(c.free)
    _sound(c)
    c.trim([100, 70, 0], 4)                                  # now row 1 lets them go: back to the pool
    assert c.held[1] == [None, None] and set(shared) <= set(c.free)
    _sound(c)
    with pytest.raises(ValueError, match="trimmed"):
        c.share_prefix(0, 2, 1)


def test_ensure_and_release_after_trim():
    c = _paged(32, num_pages=8)
    c.ensure([64, 64, 0])
    c.trim([64, 64, 0], 8)                                   # page 0 of rows 0 and 1
    free = len(c.free)
    c.ensure([64, 64, 0])                                    # nothing to do: a trimmed entry is never refilled
    assert len(c.free) == free and c.held[0][0] is None and c.held[1][0] is None
    c.ensure([65, 64, 0])                                    # the next LOGICAL page
    assert len(c.held[0]) == 3 and c.held[0][0] is None and c.held[0][2] is not None and len(c.free) == free - 1
    _sound(c)
    still = [p for p in c.held[0] if p is not None]
    free = list(c.free)
    c.release(0)
    assert c.held[0] == [] and sorted(c.free) == sorted(free + still)
    _sound(c)
    c.reset()
    assert sorted(c.free) == list(range(8)) and all(r == 0 for r in c.refs)


def test_trimmed_rows_live_in_a_small_pool():
    """W + 16 keys a row plus one page: a row grows by one key a step for 6 P steps; without trim the pool runs out"""
    P, W, B = 32, 24, 2
    pages = -(-(W + 16) // P) + 1
    for trim in (True, False):
        c = _paged(P, num_pages=B * pages, max_pages=8, B=B)
        try:
            for n in range(1, 6 * P + 1):
                c.ensure([n] * B)
                if trim:
                    c.trim([n] * B, W)
                _sound(c)
            assert trim
            assert all(sum(p is not None for p in row) <= pages for row in c.held)
        except RuntimeError as e:
            assert not trim and "more pages" in str(e)
