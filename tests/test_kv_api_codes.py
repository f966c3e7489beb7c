"""CPU tests of the KV-cache exports' argument check (csrc/mi355q_kv_call.h) through the diagnostic hook mi355q_debug_kv_call, which
calls the function the 21 exports call and never launches: every row of tests/golden/kv_api_codes.json / .npz -- the return code of
an export under one perturbation of a valid call or under two, recorded from the exports of the commit before the descriptor existed
(the fixture's header says how; tools/record_kv_api_codes.py) -- gives the same code; where no GPU is visible the exports themselves
are replayed too (the pointers are fake: a lost check must not become a launch on a shared card); and the normalised descriptor of
every baseline and of the variants whose handling differs between exports is held to hand-written values."""
import ctypes as C
import json
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden" / "kv_api_codes.json"
# mi355q_debug_kv_call's flat arguments: 14 addresses, then 13 integers
SLOTS = ("kq vq stage k v q out workspace lengths counts block_table k_bytes v_bytes stage_bytes "
         "B C max_pages num_pages P D M L n G causal window splits").split()
FIELDS = "rc go B capacity D M L n G window lg_p pages causal strides_set s0 s1 s2 s3".split()


@pytest.fixture(scope="module")
def table():
    import numpy as np
    doc = json.loads(GOLDEN.read_text())
    doc["rows"] = np.load(GOLDEN.with_suffix(".npz"))["rows"].tolist()
    return doc


def arguments(export, perts):
    """{argument: value} of a call of `export` under the perturbations [[argument, index or None, value], ...]"""
    values = {a: list(v) if isinstance(v, list) else v for a, v in zip(export["args"], export["baseline"])}
    for name, i, v in perts:
        if i is None:
            values[name] = v
        else:
            values[name][i] = v
    return values


def host_arrays(table, values):
    """the real host arrays of a call (or None): the quantiser parameters, the strides, the int64 a *_bytes export writes"""
    made = {}
    for a, v in values.items():
        if a in table["sizes"]:
            made[a] = None if v is None else C.c_int64(0)
        elif a in table["host"]:
            made[a] = None if v is None else ((C.c_int64 * 4) if a == "strides" else (C.c_int32 * 6))(*v)
    return made


@pytest.fixture(scope="module")
def hook(table):
    from mi355q import _lib
    fn = C.CDLL(str(_lib.library_path())).mi355q_debug_kv_call
    fn.restype = C.c_int
    fn.argtypes = [C.c_int32, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]

    def check(e, perts=()):
        values = arguments(table["exports"][e], perts)
        made = host_arrays(table, values)
        flat = [(0 if values.get(a) is None else 1 << 20) if a in table["sizes"] else int(values.get(a) or 0) for a in SLOTS]
        out = (C.c_int64 * 18)(*([-99] * 18))
        assert fn(e, (C.c_int64 * 27)(*flat), *[None if made.get(a) is None else C.addressof(made[a]) for a in table["host"]], out) == 0
        return list(out)
    return check


def perturbed(table, row):
    e, i, j, code = row
    perts = table["exports"][e]["perturbations"]
    return perts[i][1] + (perts[j][1] if j >= 0 else []), perts[i][0] + (" + " + perts[j][0] if j >= 0 else "")


def test_the_table_covers_every_export_and_holds_only_codes(table):
    assert [x["name"] for x in table["exports"]][::10] == ["mi355q_bfp_kv_cache_bytes", "mi355q_bfp_kv_paged_bytes", "mi355q_bfp_attention_extend_window"]
    assert len(table["exports"]) == 21 and {r[0] for r in table["rows"]} == set(range(21)) and len(table["rows"]) > 20000
    assert {r[3] for r in table["rows"]} == {0, -1, -2, -3}
    for e, export in enumerate(table["exports"]):       # every perturbation that does not launch alone is recorded alone
        alone = {r[1] for r in table["rows"] if r[0] == e and r[2] < 0}
        assert alone == {i for i, (label, _) in enumerate(export["perturbations"]) if label not in export["launches"]}


def test_every_recorded_code_comes_out_of_the_check(table, hook):
    wrong = []
    for row in table["rows"]:
        perts, label = perturbed(table, row)
        got = hook(row[0], perts)
        if got[0] != row[3] or got[1] != 0:
            wrong.append((table["exports"][row[0]]["name"], label, row[3], got[:2]))
    assert not wrong, f"{len(wrong)} of {len(table['rows'])} rows differ; first (export, perturbations, recorded code, (code, go)): {wrong[:5]}"


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


@pytest.mark.skipif(not _no_gpu(), reason="the exports are called with fake pointers: only where no GPU is visible")
def test_every_recorded_code_comes_out_of_the_exports(table):
    from mi355q import _lib
    lib = _lib.load_library()
    wrong = []
    for row in table["rows"]:
        export = table["exports"][row[0]]
        perts, label = perturbed(table, row)
        values = arguments(export, perts)
        made = host_arrays(table, values)
        got = getattr(lib, export["name"])(*[(None if made[a] is None else C.addressof(made[a])) if a in made else values[a] for a in export["args"]])
        if got != row[3]:
            wrong.append((export["name"], label, row[3], got))
    assert not wrong, f"{len(wrong)} of {len(table['rows'])} rows differ; first (export, perturbations, recorded, returned): {wrong[:5]}"


# the normalised call of each export's baseline (B = 2, D = 64, capacity 64 = 2 pages of 32, M = 2, n = 1, L = 8, G = 2, window 4, strides
# 128, 64, 128, 64): G, window, lg_p, pages set, causal, strides set -- by hand, from the exports' contracts in include/mi355q.h
BASELINES = {
    "mi355q_bfp_kv_cache_bytes": dict(capacity=0), "mi355q_bfp_kv8_cache_bytes": dict(capacity=0), "mi355q_bfp_kv_paged_bytes": dict(capacity=0, lg_p=5),
    "mi355q_bfp_kv_append": dict(strides_set=1), "mi355q_bfp_kv_append_ragged": dict(strides_set=1), "mi355q_bfp_kv8_append": dict(strides_set=1),
    "mi355q_bfp_kv_append_paged": dict(strides_set=1, lg_p=5, pages=1),
    "mi355q_bfp_kv_decode_fp32": {}, "mi355q_bfp_kv_decode_fp32_ragged": {}, "mi355q_bfp_kv8_decode_fp32": {},
    "mi355q_bfp_kv_decode_fp32_paged": dict(lg_p=5, pages=1),
    "mi355q_bfp_attention_decode": dict(causal=1, strides_set=1), "mi355q_bfp_attention_decode_ragged": dict(causal=1, strides_set=1),
    "mi355q_bfp_attention_extend": dict(causal=1, strides_set=1),
    "mi355q_bfp_attention_decode_grouped": dict(G=2, causal=1, strides_set=1), "mi355q_bfp_attention_extend_grouped": dict(G=2, causal=1, strides_set=1),
    "mi355q_bfp_attention_decode_kv8": dict(G=2, causal=1, strides_set=1),
    "mi355q_bfp_attention_decode_paged": dict(G=2, causal=1, strides_set=1, lg_p=5, pages=1),
    "mi355q_bfp_attention_extend_paged": dict(G=2, causal=1, strides_set=1, lg_p=5, pages=1),
    "mi355q_bfp_attention_decode_window": dict(G=2, window=4, causal=1, strides_set=1, lg_p=5, pages=1),
    "mi355q_bfp_attention_extend_window": dict(G=2, window=4, causal=1, strides_set=1, lg_p=5, pages=1),
}


def expected(export, **over):
    """a passed call's words: what the export's own arguments give, zeros elsewhere, then `over`"""
    values = dict(zip(export["args"], export["baseline"]))
    want = dict.fromkeys(FIELDS, 0)
    want.update(go=1, B=2, D=64, capacity=64, M=values.get("M", 0), L=values.get("L", 0), n=values.get("n", 0))
    want.update(over)
    if want["strides_set"] and "s0" not in over:
        want.update(s0=128, s1=64, s2=128, s3=64)
    return [want[f] for f in FIELDS]


def test_the_baselines_pass_with_the_normalised_call_of_their_contract(table, hook):
    assert set(BASELINES) == {x["name"] for x in table["exports"]}
    for e, export in enumerate(table["exports"]):
        assert hook(e) == expected(export, **BASELINES[export["name"]]), export["name"]


def test_the_variants_the_exports_treat_differently(table, hook):
    index = {x["name"]: e for e, x in enumerate(table["exports"])}

    def held(name, perts, **over):
        e = index[f"mi355q_bfp_{name}"]
        assert hook(e, perts) == expected(table["exports"][e], **{**BASELINES[f"mi355q_bfp_{name}"], **over}), (name, perts)
    # G = 1: the *_grouped exports run the grouped form, every other export the ungrouped kernels (G = 0); so does G = 0 where it is taken
    for name in ("attention_decode_grouped", "attention_extend_grouped"):
        held(name, [["G", None, 1]], G=1)
    for name in ("attention_decode_paged", "attention_extend_paged", "attention_decode_kv8", "attention_decode_window", "attention_extend_window"):
        held(name, [["G", None, 1]], G=0)
        held(name, [["G", None, 0]], G=0)
    # a window over more keys than the call can hold is clamped to max_length; causal goes on as 1
    for name in ("attention_decode_window", "attention_extend_window"):
        held(name, [["window", None, 100]], window=8)
        held(name, [["window", None, 8]], window=8)
        # block_table == NULL: the contiguous cache of max_pages * P keys, no pages -- also where num_pages or P would not do for pools
        held(name, [["block_table", None, None]], pages=0, lg_p=0)
        held(name, [["block_table", None, None], ["num_pages", None, 0]], pages=0, lg_p=0)
        held(name, [["block_table", None, None], ["P", None, 48], ["max_pages", None, 1]], pages=0, lg_p=0, capacity=48)
    # causal = 0 is passed on where there is no window
    for name in ("attention_decode", "attention_decode_ragged", "attention_extend", "attention_decode_grouped", "attention_decode_paged", "attention_decode_kv8"):
        held(name, [["causal", None, 0]], causal=0)
    # NULL strides: the append's contiguous rows {n D, D, n D, D}; decode and extend hand NULL on to fill_qo_strides
    for name in ("kv_append", "kv_append_ragged", "kv_append_paged", "kv8_append"):
        held(name, [["strides", None, None]], s0=64, s1=64, s2=64, s3=64)
        held(name, [["strides", None, None], ["n", None, 3], ["L", None, 0]], n=3, L=0, s0=192, s1=64, s2=192, s3=64)
    for name in ("attention_decode", "attention_decode_grouped", "attention_decode_paged", "attention_decode_kv8", "attention_decode_window",
                 "attention_extend", "attention_extend_grouped", "attention_extend_paged", "attention_extend_window"):
        held(name, [["strides", None, None]], strides_set=0)
    # extend takes lengths == NULL (the uniform form) with counts == NULL, any M, and no workspace; decode_grouped takes lengths == NULL
    held("attention_extend", [["lengths", None, None], ["counts", None, None]])
    held("attention_extend_grouped", [["lengths", None, None], ["counts", None, None], ["M", None, 17], ["L", None, 64]], M=17, L=64)
    held("attention_decode_grouped", [["lengths", None, None]])
