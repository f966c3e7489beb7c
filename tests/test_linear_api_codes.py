"""CPU tests of the Linear-side exports' argument checks against tests/golden/linear_api_codes.json / .npz: the return code of each
of the 21 exports under one perturbation of a valid call or under two, recorded from the exports of the commit before
csrc/mi355q_linear_call.h existed (the fixture's header says how; tools/record_linear_api_codes.py).  Where no GPU is visible every
row is replayed through the exports themselves (the pointers are fake: a lost check must not become a launch on a shared card)."""
import ctypes as C
import json
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden" / "linear_api_codes.json"


@pytest.fixture(scope="module")
def table():
    import numpy as np
    doc = json.loads(GOLDEN.read_text())
    doc["rows"] = np.load(GOLDEN.with_suffix(".npz"))["rows"].tolist()
    return doc


def arguments(entry, perts):
    """{argument: value} of a call of `entry` under the perturbations [[[argument, (index,) (field)], value], ...]"""
    values = json.loads(json.dumps(dict(zip(entry["args"], entry["baseline"]))))
    for key, v in perts:
        at = values
        for k in key[:-1]:
            at = at[k]
        at[key[-1]] = v
    return values


def host_memory(table, values):
    """the real host memory of a call: {argument: ctypes object or None} for the operand structs and _multi's arrays, and what keeps it alive"""
    from mi355q import _lib
    struct = lambda f: _lib.BfpOperand(*[f[name] for name in table["fields"]])
    made, keep = {}, []
    for a, v in values.items():
        if a in table["structs"]:
            made[a] = None if v is None else struct(v)
        elif a in table["arrays"]:
            items = None if v is None else [None if e is None else struct(e) if a == "wos" else e for e in v]
            keep.append(items)
            made[a] = None if v is None else (C.c_void_p * 3)(*[C.addressof(e) if isinstance(e, C.Structure) else e for e in items])
    return made, keep


def perturbed(table, row):
    e, i, j, code = row
    perts = table["entries"][e]["perturbations"]
    return perts[i][1] + (perts[j][1] if j >= 0 else []), perts[i][0] + (" + " + perts[j][0] if j >= 0 else "")


def test_the_table_covers_every_export_and_holds_only_codes(table):
    names = [x["name"] for x in table["entries"]]
    assert len(set(names)) == 21 and names[0] == "mi355q_block_fp_quantize_aligned_rows" and names[-1] == "mi355q_mx_gemm"
    assert [x["id"] for x in table["entries"]] == sorted(x["id"] for x in table["entries"]) and {x["id"] for x in table["entries"]} == set(range(21))
    for name in ("mi355q_bfp_gemm_aligned", "mi355q_bfp_gemm_aligned_res", "mi355q_bfp_gemm_aligned_multi"):
        assert [x["variant"] for x in table["entries"] if x["name"] == name] == [0, 2, 8]
    assert {r[0] for r in table["rows"]} == set(range(len(table["entries"]))) and len(table["rows"]) > 20000
    assert {r[3] for r in table["rows"]} == {0, -1, -2, -3}
    assert len(table["header"]["commit"]) == 40
    for e, entry in enumerate(table["entries"]):       # every perturbation that does not launch alone is recorded alone
        alone = {r[1] for r in table["rows"] if r[0] == e and r[2] < 0}
        assert alone == {i for i, (label, _) in enumerate(entry["perturbations"]) if label not in entry["launches"]}


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


@pytest.mark.skipif(not _no_gpu(), reason="the exports are called with fake pointers: only where no GPU is visible")
def test_every_recorded_code_comes_out_of_the_exports(table):
    from mi355q import _lib
    lib = _lib.load_library()
    wrong = []
    try:
        for row in table["rows"]:
            entry = table["entries"][row[0]]
            perts, label = perturbed(table, row)
            values = arguments(entry, perts)
            made, keep = host_memory(table, values)
            lib.mi355q_bfp_gemm_set_variant(entry["variant"])
            got = getattr(lib, entry["name"])(*[(None if made[a] is None else C.addressof(made[a])) if a in made else values[a] for a in entry["args"]])
            if got != row[3]:
                wrong.append((entry["name"], entry["variant"], label, row[3], got))
        # K = 0 makes the row flags optional for the check, and the launch PLANNER behind it answers -1 to lists without flags: listed as
        # launching in the table, so held here (the code is ABI all the same; the planner launches nothing)
        lib.mi355q_bfp_gemm_set_variant(0)
        for e, entry in enumerate(table["entries"]):
            if entry["name"] in ("mi355q_bfp_gemm_aligned", "mi355q_bfp_gemm_aligned_res") and entry["variant"] == 0:
                for operand in ("xo", "wo"):
                    assert f"K=0 + {operand}.rowflag=NULL" in entry["launches"]
                    values = arguments(entry, [[["K"], 0], [[operand, "rowflag"], None]])
                    made, keep = host_memory(table, values)
                    assert getattr(lib, entry["name"])(*[C.addressof(made[a]) if a in made else values[a] for a in entry["args"]]) == -1
    finally:
        lib.mi355q_bfp_gemm_set_variant(0)
    assert not wrong, f"{len(wrong)} of {len(table['rows'])} rows differ; first (export, variant, perturbations, recorded, returned): {wrong[:5]}"
