"""The table of cached-attention launch forms (tests/attn_forms_util.py) against the launchers' own text and the ISA profile, its
predicates, and its oracle -- everything a machine without a GPU can say about tests/test_gpu_attn_forms.py before a GPU runs it."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import attn_forms_util as U  # noqa: E402

CSRC = ROOT / "llm-mixed-q_amd" / "csrc"


def _bools(text, n):
    """'true, false, true' -> the n template booleans, the trailing defaults (WN = false) filled in"""
    vals = [w.strip() for w in text.split(",") if w.strip()]
    assert all(v in ("true", "false") for v in vals) and len(vals) <= n, text
    return tuple(v == "true" for v in vals) + (False,) * (n - len(vals))


def _chunk_counts(src, macro):
    """the DC values of the `switch (c.D / 32)` whose cases expand `macro`"""
    body = src[src.index("switch (c.D / 32)"):]
    body = body[:body.index("default:")]
    labels = re.findall(r"case (\d+): %s\((\d+)\); break;" % macro, body)
    assert labels and all(a == b for a, b in labels), labels
    assert len(labels) == len(re.findall(r"\bcase\b", body)), "a case label of the switch does not expand the launch macro"
    return [int(a) for a, _ in labels]


def dispatched_decode():
    src = (CSRC / "mi355q_decode.hip").read_text()
    lists = [m for m in re.findall(r"MI355Q_DECODE_GO2\(DC_, ([^)]*)\)", src) if "RG_" not in m]
    return {(dc,) + _bools(m, 4) for dc in _chunk_counts(src, "MI355Q_DECODE_GO") for m in lists}, len(lists)


def dispatched_extend():
    src = (CSRC / "mi355q_extend.hip").read_text()
    lists = re.findall(r"bfp_attention_extend_kernel<DC_, ([^>]*)>", src)
    return {(dc,) + _bools(m, 3) for dc in _chunk_counts(src, "MI355Q_EXTEND_GO") for m in lists}, len(lists)


def _names(forms):
    return sorted("<%s>" % ", ".join(str(x).lower() for x in f) for f in forms)


@pytest.mark.parametrize("kind,dispatched,count", [("decode", dispatched_decode, 40), ("extend", dispatched_extend, 32)])
def test_table_is_what_the_launcher_dispatches(kind, dispatched, count):
    want, per_dc = dispatched()
    assert len(want) == count == 4 * per_dc, "two launch lines of the launcher name the same form"
    have = U.forms(kind)
    assert not want - have, f"{kind} forms the launcher dispatches and no case launches: {_names(want - have)}"
    assert not have - want, f"{kind} cases for forms the launcher does not dispatch: {_names(have - want)}"
    # no uniform paged and no uniform windowed kernel
    if kind == "decode":
        assert not [f for f in want if not f[1] and (f[3] or f[4])]


def test_profile_lists_the_same_kernels():
    text = (ROOT / "profiles" / "decode_window_isa.txt").read_text()
    found = {name: set() for name in ("decode_scores_kernel", "decode_pv_kernel", "bfp_attention_extend_kernel")}
    for name, args in re.findall(r"\b(decode_scores_kernel|decode_pv_kernel|bfp_attention_extend_kernel)<([^>]*)>", text):
        dc, rest = args.split(",", 1)
        found[name].add((int(dc),) + _bools(rest, 4 if name.startswith("decode") else 3))
    for name, have in found.items():
        want = U.forms("extend" if name.startswith("bfp") else "decode")
        assert have == want, f"{name}: profile only {_names(have - want)}, table only {_names(want - have)}"


def test_form_of():
    f = U.form_of
    assert f("decode", 64, None, 1, False, None) == (2, False, False, False, False)
    assert f("decode", 64, None, 4, False, None) == (2, False, True, False, False)
    assert f("decode", 96, (5, 5), 1, False, None) == (3, True, False, False, False)
    assert f("decode", 32, None, 1, False, 8) == (1, True, False, False, True), "the uniform windowed call launches RG = true"
    assert f("decode", 128, (5,), 2, True, 8) == (4, True, True, True, True)
    assert f("extend", 64, None, 1, False, 8) == (2, False, False, True)
    assert f("extend", 96, (5,), 2, True, None) == (3, True, True, False)
    for kind in ("decode", "extend"):
        with pytest.raises(ValueError, match="uniform paged"):
            f(kind, 64, None, 1, True, None)
        with pytest.raises(ValueError, match="head dim"):
            f(kind, 160, None, 1, False, None)
    for c in U.CASES:
        assert f(c.kind, c.D, c.lengths if c.ragged else None, c.group, c.paged, c.window) == c.form
        assert c.form[0] == c.D // 32 and c.id.startswith(c.kind + "<") and U.BY_ID[c.id] is c


def test_form_of_follows_ops():
    """the two facts form_of takes from ops.py, read there: group == 1 never reaches a grouped entry point with G = 1 (the *_grouped route
    sits behind `group != 1` and behind the windowed and paged routes, whose entry points turn G <= 1 into 0 -- one line of the exports'
    shared check, which spares only the *_grouped exports), and a windowed call always brings lengths"""
    import inspect
    import torch
    from mi355q import ops
    src = inspect.getsource(ops._cached_attention)
    assert src.index('"_window" if windowed') < src.index('"_paged" if paged') < src.index('"_grouped" if group != 1')
    assert "_window_lengths(cache, lengths, max_length)" in src
    for fn in (ops.bfp_attention_decode, ops.bfp_attention_extend):
        assert "_cached_attention(" in inspect.getsource(fn)
    check = (CSRC / "mi355q_kv_call.h").read_text()
    assert len(re.findall(r"k\.G = \(d\.form & KV_GROUPED\) \|\| d\.G > 1 \? d\.G : 0;", check)) == 1       # decode / extend x paged / window / kv8
    api = (CSRC / "mi355q_api.hip").read_text()
    assert len(re.findall(r"KV_EXPORTS\[KVX_(?:DECODE|EXTEND)_(?:PAGED|WINDOW)\]", api)) == 4 and "G = 0" not in api
    cache = ops.KVCache(2, 64, 64, U.par(6), U.par(6), "cpu")
    cache.length = 40
    lengths, max_length = ops._window_lengths(cache, None, None)
    assert lengths.dtype == torch.int32 and lengths.tolist() == [40, 40] and max_length == 40
    for check in (ops._decode_check, ops._extend_check):
        paged = ops.PagedKVCache(2, 64, U.par(6), U.par(6), "cpu", page_size=32, num_pages=4, max_pages=2)
        assert "no uniform paged launch" in check(torch.zeros(2, 4, 64), paged)


def test_host_arithmetic_is_the_librarys():
    from mi355q import _lib, ops
    span = _lib.load_library().mi355q_bfp_attention_decode_window_span
    for G in range(1, 9):
        for M in range(1, 17):
            assert U.group_width(G, M) == ops.decode_group_width(G, M)
    for M, L, W in ((7, 117, 20), (4, 117, 20), (1, 40, 1), (7, 75, 75), (16, 8192, 64)):
        assert U.window_span(M, L, W) == span(M, L, W)
    for rows in (1, 2, 3, 6, 12, 600):
        for L in (1, 32, 57, 75, 117, 131, 1040):
            for override in (None, 1, 2, 3, 5, 70):
                assert U.splits_of(rows, L, override)[0] == ops.decode_splits(rows, L, 64, override), (rows, L, override)


@pytest.mark.parametrize("c", U.CASES, ids=lambda c: c.id)
def test_predicates_hold(c):
    dc, (rg, gq, pg, wn) = c.form[0], c.form[1:] if c.kind == "decode" else (c.ragged,) + c.form[1:]
    assert c.D == 32 * dc and c.width in U.WIDTHS and U.scaling_ok(c) and U.fill_ok(c)
    assert c.L <= 131 and c.B <= 3 and c.L <= c.capacity and all(0 <= n for n in c.lengths)
    if c.ragged:
        assert U.rg_ok(c)
    else:
        assert len(set(c.lengths)) == 1 and c.counts is None and c.M <= c.L
    assert (c.group > 1) == gq and (not gq or U.gq_ok(c))
    assert c.paged == pg and (not pg or U.pg_ok(c))
    if wn:
        assert U.wn_decode_ok(c) if c.kind == "decode" else U.wn_extend_ok(c)
    elif c.kind == "decode":
        assert U.plain_decode_ok(c)
    if c.kind == "decode":
        assert 1 <= c.M <= 16 and rg == (c.ragged or wn)
    else:
        assert c.M == 70 and c.splits == ()


def test_widths_and_scalings_rotate():
    for kind in ("decode", "extend"):
        base = [c for c in U.CASES if c.kind == kind and not c.note]
        for switches in {c.form[1:] for c in base}:
            assert {c.width for c in base if c.form[1:] == switches} == set(U.WIDTHS), (kind, switches)
        for dc in (1, 2, 3, 4):
            assert {c.width for c in base if c.form[0] == dc} == set(U.WIDTHS), (kind, dc)
            # one non-causal q_scale case for the non-window paged grouped form, at every DC
            extra = [c for c in U.CASES if c.kind == kind and not c.causal and c.form[0] == dc]
            assert len(extra) == 1 and extra[0].paged and extra[0].group > 1 and extra[0].window is None
    assert all(c.causal for c in U.CASES if c.window is not None)


def test_the_stale_lds_screen_covers_eight_forms():
    assert sorted(c.form for c in U.ALL_ON if c.kind == "decode") == [(dc, True, True, True, True) for dc in (1, 2, 3, 4)]
    assert sorted(c.form for c in U.ALL_ON if c.kind == "extend") == [(dc, True, True, True) for dc in (1, 2, 3, 4)]
    assert all(2 in c.splits for c in U.ALL_ON if c.kind == "decode")


def test_a_predicate_notices_a_spoiled_case():
    """the predicates are not vacuous: one edit to a good case's numbers fails the predicate that guards that switch"""
    import dataclasses
    dec = U.BY_ID["decode<2,true,true,true,true>"]
    ext = U.BY_ID["extend<2,true,true,true>"]
    assert not U.wn_decode_ok(dataclasses.replace(dec, window=30))                     # lo = 81: the first tile of its pair
    assert not U.wn_decode_ok(dataclasses.replace(dec, splits=(1, None)))               # never one pair a split
    assert not U.gq_ok(dataclasses.replace(dec, group=2)) and not U.gq_ok(dataclasses.replace(dec, M=16))
    assert not U.rg_ok(dataclasses.replace(dec, lengths=(117, 64, 3))) and not U.rg_ok(dataclasses.replace(dec, lengths=(117, 70, 7)))
    assert not U.pg_ok(dataclasses.replace(dec, lengths=(64, 41, 3))) and not U.pg_ok(dataclasses.replace(dec, P=128))
    assert not U.wn_extend_ok(dataclasses.replace(ext, window=20)) and not U.wn_extend_ok(dataclasses.replace(ext, lengths=(116, 57, 40)))
    assert not U.plain_decode_ok(dataclasses.replace(U.BY_ID["decode<2,true,false,false,false>"], lengths=(64, 41, 3)))
    assert not U.fill_ok(dataclasses.replace(dec, lengths=(122, 70, 3)))


@pytest.mark.parametrize("c", U.CASES, ids=lambda c: c.id)
def test_oracle_is_not_degenerate(c):
    refs = U.reference(c)
    q, k, v = U.arrays(c)
    assert q.shape == (c.B * c.group, c.M, c.D) and k.shape == v.shape == (c.B, c.L, c.D)
    assert any(r is not None for r in refs)
    for b, ref in enumerate(refs):
        if c.queries(b) == 0:
            assert ref is None
            continue
        assert ref.shape == (c.group, c.queries(b), c.D) and ref.dtype == np.float32
        assert np.isfinite(ref).all()
        assert (np.abs(ref).reshape(-1, c.D).max(-1) > 0).all(), f"row {b}: a query whose reference output is all zeros"
