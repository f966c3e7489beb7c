"""Attention sinks, everything a machine without a GPU can check: the Python refusals, the two exports' argument check through the debug
hook against hand-written values, PagedKVCache.trim(..., sinks=S) on its host mirror, harness._causal_mask against a mask written out by
loops, and the table of sink kernel forms (tests/sink_util.py) against the launch lines of csrc/mi355q_sink.hip and the ISA profile."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import sink_util as U  # noqa: E402

CSRC = ROOT / "llm-mixed-q_amd" / "csrc"
PAR = (6, 8, 127, 6, 8, 127)
DECODE_SINK, EXTEND_SINK = 33, 34


# ---- Python refusals ------------------------------------------------------------------------------------------------------------
def test_exports_and_abi():
    from mi355q import _lib
    lib = _lib.load_library()
    for name in ("mi355q_bfp_attention_decode_sink", "mi355q_bfp_attention_extend_sink"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} not bound / exported"
    assert lib.mi355q_abi_version() == _lib.ABI_VERSION == 25


def test_window_check_reasons():
    from mi355q import ops
    chk = ops._window_check
    assert chk(8, True, None) is None and chk(8, True, 0) is None and chk(8, True, 16) is None and chk(None, True, None) is None
    assert "without window" in chk(None, True, 4) and "without window" in chk(None, True, 0)
    for bad in (17, -1, True, 2.0, "4"):
        assert "0 .. 16" in chk(8, True, bad), bad
    assert "causal=False" in chk(8, False, 4)
    assert "integer >= 1" in chk(0, True, 4)                    # (the window's own refusal comes first)


def test_the_calls_refuse_before_the_device():
    import torch
    from mi355q import ops
    q = torch.zeros(2, 4, 64)
    cache = ops.KVCache(2, 64, 64, PAR, PAR, "cpu")
    cache.length = 40
    for fn in (ops.bfp_attention_decode, ops.bfp_attention_extend):
        with pytest.raises(ValueError, match="without window"):
            fn(q, cache, sinks=4)
        with pytest.raises(ValueError, match="0 .. 16"):
            fn(q, cache, window=8, sinks=17)
        with pytest.raises(ValueError, match="0 .. 16"):
            fn(q, cache, window=8, sinks=True)
        with pytest.raises(ValueError, match="causal=False"):
            fn(q, cache, window=8, sinks=4, causal=False)
    assert ops._decode_check(q, cache, window=8, sinks=4) is not None and "fp32 tensors on" in ops._decode_check(q, cache, window=8, sinks=4)
    # the mantissa and minifloat caches refuse sinks with their window refusal
    for kind, par in ((ops.PackedKVCache, PAR), (ops.NibbleKVCache, (4, 8, 127, 4, 8, 127)), (ops.MinifloatKVCache, (8, 4, 8, 8, 4, 8))):
        other = kind(2, 64, 64, par, par, "cpu")
        for kw in (dict(window=8, sinks=4), dict(sinks=4)):
            with pytest.raises(NotImplementedError, match="no sliding-window kernel"):
                ops.bfp_attention_decode(q, other, **kw)
    paged8 = ops.PagedPackedKVCache(2, 64, PAR, PAR, "cpu", page_size=32, num_pages=4, max_pages=2)
    with pytest.raises(NotImplementedError):
        paged8.trim([40, 40], 8, sinks=4)


def test_the_route_takes_the_sink_export_only_for_truthy_sinks():
    import inspect
    from mi355q import ops
    src = inspect.getsource(ops._cached_attention)
    assert src.index('"_sink" if windowed and sinks') < src.index('"_window" if windowed')
    assert 'if form == "_sink"' in src


def test_config():
    from mi355q import harness as H
    assert H.TinyLlamaConfig().attention_sinks is None
    assert H.TinyLlamaConfig(sliding_window=8, attention_sinks=2).attention_sinks == 2
    assert H.TinyLlamaConfig(sliding_window=8, attention_sinks=0).attention_sinks == 0
    for bad in (17, -1, True, 2.0):
        with pytest.raises(ValueError, match="attention_sinks"):
            H.TinyLlamaConfig(sliding_window=8, attention_sinks=bad)
    with pytest.raises(ValueError, match="without sliding_window"):
        H.TinyLlamaConfig(attention_sinks=2)


# ---- the exports' argument check, through the debug hook ---------------------------------------------------------------------------
# a[0 .. 13] = kq, vq, stage, k, v, q, out, workspace, lengths, counts, block_table, k_bytes, v_bytes, stage_bytes;
# a[14 .. 27] = B, C, max_pages, num_pages, P, D, M, L, n, G, causal, window, splits, sinks (the 28th word: ids 33 and 34 only)
IDX = dict(kq=0, vq=1, q=5, out=6, workspace=7, lengths=8, counts=9, block_table=10, B=14, max_pages=16, num_pages=17, P=18, D=19, M=20, L=21,
           G=23, causal=24, window=25, splits=26, sinks=27)


def _call(id_, **over):
    from mi355q import _lib
    fn = _lib.load_library().mi355q_debug_kv_call_all
    fn.restype, fn.argtypes = C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    a = [0x1000, 0x2000, 0, 0, 0, 0x6000, 0x7000, 0x8000, 0x9000, 0, 0xD000, 0, 0, 0,
         2, 0, 2, 8, 32, 32, 1, 40, 0, 0, 1, 8, 0, 4]
    for name, value in over.items():
        a[IDX[name]] = value
    par, out = (C.c_int32 * 6)(*PAR), (C.c_int64 * 18)()
    assert fn(id_, (C.c_int64 * 28)(*a), par, par, None, out) == 0
    return list(out)


@pytest.mark.parametrize("id_", [DECODE_SINK, EXTEND_SINK])
def test_the_argument_check(id_):
    """code, `go`, then B, capacity, D, M, L, sinks (in n's place), G, window, lg_p, pages set, causal, strides set, the four strides"""
    from mi355q import _lib
    BAD, UNS, ALIGN = _lib.E_BADARG, _lib.E_UNSUPPORTED, _lib.E_ALIGN
    assert _call(id_) == [0, 1, 2, 64, 32, 1, 40, 4, 0, 8, 5, 1, 1, 0, 0, 0, 0, 0]
    assert _call(id_, sinks=16)[:2] == [0, 1] and _call(id_, sinks=16)[7] == 16
    assert _call(id_, sinks=0) == [0, 1, 2, 64, 32, 1, 40, 0, 0, 8, 5, 1, 1, 0, 0, 0, 0, 0]
    for over in (dict(sinks=17), dict(sinks=-1), dict(window=0), dict(window=0, sinks=0), dict(causal=0), dict(lengths=0), dict(q=0),
                 dict(G=-1), dict(L=65), dict(P=48), dict(num_pages=0)):
        assert _call(id_, **over)[:2] == [BAD, 0], over
    assert _call(id_, window=1000)[9] == 40                       # the window is clamped to L as in the *_window exports
    assert _call(id_, G=1)[8] == 0 and _call(id_, G=2, M=4)[8] == 2
    assert _call(id_, M=0)[:2] == [UNS, 0] and _call(id_, D=48)[:2] == [UNS, 0]
    assert _call(id_, block_table=0xD002)[:2] == [ALIGN, 0]
    # block_table == NULL: the contiguous cache of max_pages * P keys
    assert _call(id_, block_table=0, max_pages=1, P=64) == [0, 1, 2, 64, 32, 1, 40, 4, 0, 8, 0, 0, 1, 0, 0, 0, 0, 0]
    if id_ == DECODE_SINK:
        assert _call(id_, M=17)[:2] == [UNS, 0] and _call(id_, workspace=0)[:2] == [BAD, 0] and _call(id_, splits=-1)[:2] == [BAD, 0]
    else:
        assert _call(id_, M=17, L=40)[:2] == [0, 1] and _call(id_, counts=0x9100)[:2] == [0, 1]
    # every refusal of the windowed export for the same call is this export's
    for over in (dict(window=0), dict(causal=0), dict(lengths=0), dict(L=65), dict(M=0), dict(block_table=0xD002)):
        assert _call(id_, **over)[:2] == _call(id_ - 14, **over)[:2], over


def test_the_ids_sit_behind_the_old_ones():
    from mi355q import _lib
    lib = _lib.load_library()
    a, par, out = (C.c_int64 * 28)(), (C.c_int32 * 6)(*PAR), (C.c_int64 * 18)()
    for name in ("mi355q_debug_kv_call", "mi355q_debug_kv_call_all"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for id_ in (27, 32, 35):
        assert lib.mi355q_debug_kv_call_all(id_, a, par, par, None, out) == _lib.E_BADARG
    for id_ in (DECODE_SINK, EXTEND_SINK):
        assert lib.mi355q_debug_kv_call_all(id_, a, par, par, None, out) == 0
        assert lib.mi355q_debug_kv_call(id_, a, par, par, None, out) == _lib.E_BADARG           # the recorded hook keeps its 25 ids
    assert lib.mi355q_debug_kv_call(24, a, par, par, None, out) == 0 and lib.mi355q_debug_kv_call(25, a, par, par, None, out) == _lib.E_BADARG


def test_the_exports_refuse_before_any_launch():
    from mi355q import _lib
    lib = _lib.load_library()
    par = (C.c_int32 * 6)(*PAR)
    pp = C.addressof(par)

    def dec(window=8, sinks=4, causal=1):
        return lib.mi355q_bfp_attention_decode_sink(4096, 8192, 12288, 0, 16384, None, causal, window, 0.0, 8.0, 20480, 24576, 2, 4, 40, 1, 1, 64,
                                                    64, pp, pp, None, 0, None, sinks)

    def ext(window=8, sinks=4, causal=1):
        return lib.mi355q_bfp_attention_extend_sink(4096, 8192, 12288, 0, 16384, None, None, causal, window, 0.0, 8.0, 20480, 2, 4, 40, 1, 1, 64, 64,
                                                    pp, pp, None, None, sinks)
    for fn in (dec, ext):
        assert fn(sinks=17) == fn(sinks=-1) == fn(window=0) == fn(window=0, sinks=0) == fn(causal=0) == _lib.E_BADARG


# ---- trim -----------------------------------------------------------------------------------------------------------------------
def test_trim_keeps_page_zero():
    from mi355q import ops
    P = 32
    cache = ops.PagedKVCache(3, 64, PAR, PAR, "cpu", page_size=P, num_pages=20, max_pages=6)
    start = len(cache.free)
    cache.ensure([170, 100, 20])
    held = [list(r) for r in cache.held]
    free0 = len(cache.free)
    assert [len(r) for r in held] == [6, 4, 1]
    with pytest.raises(ValueError, match="sinks"):
        cache.trim([170, 100, 20], 8, sinks=17)
    with pytest.raises(ValueError, match="sinks"):
        cache.trim([170, 100, 20], 8, sinks=True)
    cache.trim([170, 100, 20], 8, sinks=4)         # row 0: pages 0 .. 4 lie wholly below key 163 -- page 0 stays; row 1: pages 0, 1 below key 93
    assert cache.held[0] == held[0][:1] + [None] * 4 + held[0][5:]
    assert cache.held[1] == held[1][:1] + [None] + held[1][2:]
    assert cache.held[2] == held[2]
    assert len(cache.free) == free0 + 5 and set(cache.free[free0:]) == set(held[0][1:5]) | {held[1][1]}
    for b, row in enumerate(cache.held):
        for i, p in enumerate(row):
            assert int(cache.table[b, i]) == (cache.pad_page if p is None else p)
    assert all(cache.refs[p] == 1 for row in cache.held for p in row if p is not None)
    assert all(cache.refs[p] == 0 for p in held[0][1:5])
    cache.trim([170, 100, 20], 8, sinks=4)         # idempotent
    assert len(cache.free) == free0 + 5
    cache.ensure([171, 130, 20])                   # a trimmed page is never refilled; row 1 grows by one page
    assert cache.held[0][1:5] == [None] * 4 and len(cache.held[1]) == 5 and cache.held[1][1] is None
    # sinks=0 is the plain trim: page 0 goes as well
    cache.trim([171, 130, 20], 8)
    assert cache.held[0][0] is None and cache.held[1][0] is None and cache.held[2] == held[2]
    cache.release(range(3))
    assert len(cache.free) == len(set(cache.free)) == start and not any(cache.refs)


def test_trim_leaves_a_shared_page_to_its_other_holder():
    from mi355q import ops
    cache = ops.PagedKVCache(2, 64, PAR, PAR, "cpu", page_size=32, num_pages=12, max_pages=4)
    cache.ensure([128, 0])
    cache.share_prefix(0, 1, 3)
    shared = list(cache.held[0][:3])
    assert cache.held[1] == shared and all(cache.refs[p] == 2 for p in shared)
    free0 = list(cache.free)
    cache.trim([128, 0], 8, sinks=2)               # row 0 gives back pages 1, 2 (row 1 still holds them) and keeps page 0
    assert cache.held[0][:3] == [shared[0], None, None] and cache.held[1] == shared
    assert cache.refs[shared[0]] == 2 and cache.refs[shared[1]] == cache.refs[shared[2]] == 1 and cache.free == free0


# ---- the mask -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,L,W,S", [(1, 40, 8, 4), (5, 40, 8, 4), (40, 40, 8, 2), (7, 20, 1, 4), (7, 20, 3, 16), (3, 10, 4, 0), (6, 6, 2, 4),
                                     (4, 30, 50, 4)])
def test_causal_mask_against_loops(n, L, W, S):
    import torch
    from mi355q import harness as H
    got = H._causal_mask(n, L, W, torch.float32, "cpu", sinks=S).numpy()
    want = U.loop_mask(n, L, W, S)
    assert np.array_equal(got == 0, want == 0)
    assert (got[want != 0] <= np.finfo(np.float32).min).all()
    if not S:
        assert torch.equal(H._causal_mask(n, L, W, torch.float32, "cpu"), H._causal_mask(n, L, W, torch.float32, "cpu", sinks=None))
    # the oracle's mask is the same one
    ones = np.ones((1, n, 32), np.float32)
    k = np.zeros((1, L, 32), np.float32)
    v = np.broadcast_to(np.arange(L, dtype=np.float32)[None, :, None] % 4, (1, L, 32)).copy()
    out = U.oracle(ones, k, v, 8, W, 1.0, S)       # equal scores: the output is the mean of v over the visible keys
    for i in range(n):
        vis = [key for key in range(L) if U.visible(L - n + i, key, W, S)]
        assert abs(float(out[0, i, 0]) - float(np.mean([key % 4 for key in vis]))) <= 0.05, (i, vis)


# ---- the table of forms against the launcher's text -------------------------------------------------------------------------------
def _bools(text):
    vals = [w.strip() for w in text.split(",") if w.strip()]
    assert all(v in ("true", "false") for v in vals) and len(vals) == 2, text
    return tuple(v == "true" for v in vals)


def _chunk_counts(body, macro):
    body = body[body.index("switch (c.D / 32)"):]
    body = body[:body.index("default:")]
    labels = re.findall(r"case (\d+): %s\((\d+)\); break;" % macro, body)
    assert labels and all(a == b for a, b in labels), labels
    assert len(labels) == len(re.findall(r"\bcase\b", body)), "a case label of the switch does not expand the launch macro"
    return [int(a) for a, _ in labels]


def _launcher(src, name):
    body = src[src.index("int " + name + "("):]
    return body[:body.index("\n}\n")]


def dispatched(kind):
    src = (CSRC / "mi355q_sink.hip").read_text()
    if kind == "decode":
        body = _launcher(src, "launch_bfp_attention_decode_sink")
        lists = [m for m in re.findall(r"MI355Q_SINK_DECODE_GO2\(DC_, ([^)]*)\)", body) if "GQ_" not in m]
        return {(dc,) + _bools(m) for dc in _chunk_counts(body, "MI355Q_SINK_DECODE_GO") for m in lists}, len(lists)
    body = _launcher(src, "launch_bfp_attention_extend_sink")
    lists = re.findall(r"bfp_attention_extend_sink_kernel<DC_, ([^>]*)>", body)
    return {(dc,) + _bools(m) for dc in _chunk_counts(body, "MI355Q_SINK_EXTEND_GO") for m in lists}, len(lists)


@pytest.mark.parametrize("kind", ["decode", "extend"])
def test_table_is_what_the_launcher_dispatches(kind):
    want, per_dc = dispatched(kind)
    assert len(want) == 16 == 4 * per_dc, "two launch lines of the launcher name the same form"
    assert U.forms(kind) == want
    assert len([c for c in U.CASES if c.kind == kind]) == 16


def test_the_old_launchers_have_no_sink_line():
    for name in ("mi355q_decode.hip", "mi355q_extend.hip"):
        assert "sink" not in (CSRC / name).read_text().lower()


def test_profile_lists_the_same_kernels_without_spills():
    text = (ROOT / "profiles" / "decode_sink_isa.txt").read_text()
    rows = re.findall(r"^\s*(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+"
                      r"(decode_scores_sink_kernel|decode_pv_sink_kernel|bfp_attention_extend_sink_kernel)<([^>]*)>", text, re.M)
    found = {}
    for *cols, name, args in rows:
        dc, rest = args.split(",", 1)
        found.setdefault(name, set()).add((int(dc),) + _bools(rest))
        assert cols[3] == cols[4] == cols[5] == "0", f"{name}<{args}> spills or uses scratch"
    assert found == {"decode_scores_sink_kernel": U.forms("decode"), "decode_pv_sink_kernel": U.forms("decode"),
                     "bfp_attention_extend_sink_kernel": U.forms("extend")}
    assert not re.search(r"^\s+\d.*\s+no\s+\S*_kernel", text, re.M) and "FAIL" not in text and text.count(" yes ") == 122


def test_cases_reach_the_new_code():
    """row 0 of every case has a sink piece, row 1 has its sinks inside the window's first pair, row 2 is empty"""
    for c in U.CASES:
        if c.kind == "decode":
            lo = U.LENGTHS[0] - c.M - U.WINDOW + 1
            assert lo // 32 == 1 and (lo // 16) % 2 == 1, "p0 = 1 with the lower edge in the pair's second tile"
            assert U.p0_of(U.LENGTHS[1], c.M, U.WINDOW) == 0 and c.queries(2) == 0 and c.queries(1) == c.M
        else:
            L, m = U.LENGTHS[0], c.counts[0]
            assert m == 70 and max(L - m + 64 - U.WINDOW + 1, 0) // 32 >= 1 and ((L - m + 69) // 16 + 1) % 2 == 1
            assert c.queries(1) == 10 and c.queries(2) == 0
        assert 1 <= U.SINKS <= 16 and U.PAGE == 32
