#!/usr/bin/env python3
"""Records tests/golden/kv_api_codes.json / .npz: the return code of each of the 21 KV-cache exports (mi355q_bfp_kv_cache_bytes ..
mi355q_bfp_attention_extend_window) for every single perturbation of a valid baseline call and for every pair of perturbations --
the pairs fix the ORDER of the checks, which is ABI.  tests/test_kv_api_codes.py replays the table.

A host-only job for a machine WITHOUT a GPU: the data pointers are fake (non-null, 16-byte aligned integers), so a call must end in
the argument checks.  The tool refuses to run where torch sees a GPU.  The baseline and every case listed in LAUNCHES -- the
perturbations that leave a call valid, such as G = 1 or NULL strides -- are never called, nor is a pair of two of them.  Every
recorded code is 0, -1, -2 or -3; any other result means that the case reached a launch: the tool stops and names it, and it goes
into LAUNCHES (an entry "a + b" for a pair).

    MI355Q_LIBRARY=<libmi355q.so of the commit to record> python tools/record_kv_api_codes.py --commit <that commit>

--dump N prints N evenly spaced rows of the recorded table as the lines tools/kv_call_check/kv_call_rows.cpp reads (no library, no call).
"""
import argparse
import ctypes as C
import itertools
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
GOLDEN = ROOT / "tests" / "golden" / "kv_api_codes.json"

PTR16 = ("kq", "vq", "stage", "k", "v", "q", "out", "workspace")            # device data: 16-byte aligned
PTR4 = ("lengths", "counts", "block_table")                                  # device int32 arrays: 4-byte aligned
SIZES = ("k_bytes", "v_bytes", "stage_bytes")                                # host int64 the *_bytes exports write: real, or NULL
HOST = ("qk_params", "pv_params", "strides")                                 # host arrays the checks read: real, or NULL
# the exports in the order of include/mi355q.h and of csrc/mi355q_kv_call.h's KvExport, with their arguments in order.  One name per
# role: kq / vq the cache or the pools (k8 / v8), k / v the new rows or the fp32 outputs, L the host length (L or max_length)
EXPORTS = [
    ("mi355q_bfp_kv_cache_bytes", "B C D k_bytes v_bytes stage_bytes"),
    ("mi355q_bfp_kv_append", "kq vq stage k v B C D L n qk_params pv_params strides stream"),
    ("mi355q_bfp_kv_decode_fp32", "kq vq k v B C D L stream"),
    ("mi355q_bfp_attention_decode", "q kq vq causal q_scale scale_div out workspace B M L C D qk_params pv_params strides splits stream"),
    ("mi355q_bfp_kv_append_ragged", "kq vq stage k v lengths counts B C D n L qk_params pv_params strides stream"),
    ("mi355q_bfp_kv_decode_fp32_ragged", "kq vq lengths k v B C D L stream"),
    ("mi355q_bfp_attention_decode_ragged", "q kq vq lengths causal q_scale scale_div out workspace B M L C D qk_params pv_params strides splits stream"),
    ("mi355q_bfp_attention_extend", "q kq vq lengths counts causal q_scale scale_div out B M L C D qk_params pv_params strides stream"),
    ("mi355q_bfp_attention_decode_grouped", "q kq vq G lengths causal q_scale scale_div out workspace B M L C D qk_params pv_params strides splits stream"),
    ("mi355q_bfp_attention_extend_grouped", "q kq vq G lengths counts causal q_scale scale_div out B M L C D qk_params pv_params strides stream"),
    ("mi355q_bfp_kv_paged_bytes", "num_pages P B D k_bytes v_bytes stage_bytes"),
    ("mi355q_bfp_kv_append_paged", "kq vq stage k v lengths counts block_table B max_pages num_pages P D n L qk_params pv_params strides stream"),
    ("mi355q_bfp_kv_decode_fp32_paged", "kq vq lengths block_table k v B max_pages num_pages P D L stream"),
    ("mi355q_bfp_attention_decode_paged", "q kq vq G lengths block_table causal q_scale scale_div out workspace B M L max_pages num_pages P D "
                                          "qk_params pv_params strides splits stream"),
    ("mi355q_bfp_attention_extend_paged", "q kq vq G lengths counts block_table causal q_scale scale_div out B M L max_pages num_pages P D "
                                          "qk_params pv_params strides stream"),
    ("mi355q_bfp_kv8_cache_bytes", "B C D k_bytes v_bytes stage_bytes"),
    ("mi355q_bfp_kv8_append", "kq vq stage k v lengths counts B C D n L qk_params pv_params strides stream"),
    ("mi355q_bfp_kv8_decode_fp32", "kq vq lengths k v B C D L qk_params pv_params stream"),
    ("mi355q_bfp_attention_decode_kv8", "q kq vq G lengths causal q_scale scale_div out workspace B M L C D qk_params pv_params strides splits stream"),
    ("mi355q_bfp_attention_decode_window", "q kq vq G lengths block_table causal window q_scale scale_div out workspace B M L max_pages num_pages P D "
                                           "qk_params pv_params strides splits stream"),
    ("mi355q_bfp_attention_extend_window", "q kq vq G lengths counts block_table causal window q_scale scale_div out B M L max_pages num_pages P D "
                                           "qk_params pv_params strides stream"),
]
CAP = 64                                                                      # C, and max_pages * P
BASE = dict(B=2, C=CAP, D=64, P=32, max_pages=2, num_pages=5, M=2, n=1, L=8, G=2, causal=1, window=4, splits=0, q_scale=0.0, scale_div=8.0,
            qk_params=[6, 8, 127, 6, 8, 127], pv_params=[6, 8, 127, 6, 8, 127], strides=[128, 64, 128, 64], stream=0,
            k_bytes="int64", v_bytes="int64", stage_bytes="int64")
BASE.update({name: 0x10000 * (i + 1) for i, name in enumerate(PTR16 + PTR4)})
BIAS_DEFAULT = -2 ** 31
# perturbations that leave the call of an export valid: it would launch.  Never called; "a + b": a pair that only launches together.
LAUNCHES = {
    "mi355q_bfp_kv_append": ["strides=NULL", "L=1", "qk_params[0]=1", "qk_params[0]=9", "qk_params[0]=10", "qk_params[1]=0", "qk_params[1]=9", "qk_params[3]=9",
        "qk_params[2]=default", "pv_params[0]=1", "pv_params[0]=9", "pv_params[0]=10", "pv_params[1]=0", "pv_params[1]=9", "pv_params[3]=9",
        "pv_params[2]=default"],
    "mi355q_bfp_kv_decode_fp32": ["kq+4", "vq+4", "k+4", "v+4", "L=1", "L=64"],
    "mi355q_bfp_attention_decode": ["strides=NULL", "causal=0", "L=64", "qk_params[0]=9", "qk_params[3]=1", "qk_params[3]=9", "qk_params[3]=10", "qk_params[4]=0",
        "qk_params[4]=9", "qk_params[2]=default", "pv_params[0]=9", "pv_params[3]=1", "pv_params[3]=9", "pv_params[3]=10", "pv_params[4]=0",
        "pv_params[4]=9", "pv_params[2]=default"],
    "mi355q_bfp_kv_append_ragged": ["counts=NULL", "strides=NULL", "L=1", "qk_params[0]=1", "qk_params[0]=9", "qk_params[0]=10", "qk_params[1]=0", "qk_params[1]=9",
        "qk_params[3]=9", "qk_params[2]=default", "pv_params[0]=1", "pv_params[0]=9", "pv_params[0]=10", "pv_params[1]=0", "pv_params[1]=9",
        "pv_params[3]=9", "pv_params[2]=default"],
    "mi355q_bfp_kv_decode_fp32_ragged": ["kq+4", "vq+4", "lengths+2", "k+4", "v+4", "L=1", "L=64"],
    "mi355q_bfp_attention_decode_ragged": ["strides=NULL", "causal=0", "L=64", "qk_params[0]=9", "qk_params[3]=1", "qk_params[3]=9", "qk_params[3]=10", "qk_params[4]=0",
        "qk_params[4]=9", "qk_params[2]=default", "pv_params[0]=9", "pv_params[3]=1", "pv_params[3]=9", "pv_params[3]=10", "pv_params[4]=0",
        "pv_params[4]=9", "pv_params[2]=default"],
    "mi355q_bfp_attention_extend": ["counts=NULL", "strides=NULL", "causal=0", "L=64", "qk_params[0]=9", "qk_params[3]=1", "qk_params[3]=9", "qk_params[3]=10",
        "qk_params[4]=0", "qk_params[4]=9", "qk_params[2]=default", "pv_params[0]=9", "pv_params[3]=1", "pv_params[3]=9", "pv_params[3]=10",
        "pv_params[4]=0", "pv_params[4]=9", "pv_params[2]=default", "lengths=NULL + counts=NULL", "M=17 + L=64"],
    "mi355q_bfp_attention_decode_grouped": ["lengths=NULL", "strides=NULL", "G=1", "causal=0", "L=64", "qk_params[0]=9", "qk_params[3]=1", "qk_params[3]=9", "qk_params[3]=10",
        "qk_params[4]=0", "qk_params[4]=9", "qk_params[2]=default", "pv_params[0]=9", "pv_params[3]=1", "pv_params[3]=9", "pv_params[3]=10",
        "pv_params[4]=0", "pv_params[4]=9", "pv_params[2]=default"],
    "mi355q_bfp_attention_extend_grouped": ["counts=NULL", "strides=NULL", "G=1", "G=65537", "causal=0", "L=64", "qk_params[0]=9", "qk_params[3]=1", "qk_params[3]=9",
        "qk_params[3]=10", "qk_params[4]=0", "qk_params[4]=9", "qk_params[2]=default", "pv_params[0]=9", "pv_params[3]=1", "pv_params[3]=9",
        "pv_params[3]=10", "pv_params[4]=0", "pv_params[4]=9", "pv_params[2]=default", "lengths=NULL + counts=NULL", "M=17 + L=64"],
    "mi355q_bfp_kv_append_paged": ["counts=NULL", "strides=NULL", "L=1", "qk_params[0]=1", "qk_params[0]=9", "qk_params[0]=10", "qk_params[1]=0", "qk_params[1]=9",
        "qk_params[3]=9", "qk_params[2]=default", "pv_params[0]=1", "pv_params[0]=9", "pv_params[0]=10", "pv_params[1]=0", "pv_params[1]=9",
        "pv_params[3]=9", "pv_params[2]=default"],
    "mi355q_bfp_kv_decode_fp32_paged": ["kq+4", "vq+4", "lengths+2", "block_table+2", "k+4", "v+4", "L=1", "L=64"],
    "mi355q_bfp_attention_decode_paged": ["strides=NULL", "G=0", "G=1", "causal=0", "L=64", "qk_params[0]=9", "qk_params[3]=1", "qk_params[3]=9", "qk_params[3]=10",
        "qk_params[4]=0", "qk_params[4]=9", "qk_params[2]=default", "pv_params[0]=9", "pv_params[3]=1", "pv_params[3]=9", "pv_params[3]=10",
        "pv_params[4]=0", "pv_params[4]=9", "pv_params[2]=default"],
    "mi355q_bfp_attention_extend_paged": ["counts=NULL", "strides=NULL", "G=0", "G=1", "G=65537", "causal=0", "L=64", "qk_params[0]=9", "qk_params[3]=1", "qk_params[3]=9",
        "qk_params[3]=10", "qk_params[4]=0", "qk_params[4]=9", "qk_params[2]=default", "pv_params[0]=9", "pv_params[3]=1", "pv_params[3]=9",
        "pv_params[3]=10", "pv_params[4]=0", "pv_params[4]=9", "pv_params[2]=default", "M=17 + L=64"],
    "mi355q_bfp_kv8_append": ["counts=NULL", "strides=NULL", "L=1", "qk_params[0]=1", "qk_params[0]=9", "qk_params[0]=10", "qk_params[1]=0", "qk_params[1]=9",
        "qk_params[2]=default", "pv_params[0]=1", "pv_params[0]=9", "pv_params[0]=10", "pv_params[1]=0", "pv_params[1]=9",
        "pv_params[2]=default"],
    "mi355q_bfp_kv8_decode_fp32": ["kq+4", "vq+4", "lengths+2", "k+4", "v+4", "L=1", "L=64", "qk_params[0]=1", "qk_params[0]=9", "qk_params[0]=10", "qk_params[1]=0",
        "qk_params[1]=9", "qk_params[2]=default", "pv_params[0]=1", "pv_params[0]=9", "pv_params[0]=10", "pv_params[1]=0", "pv_params[1]=9",
        "pv_params[2]=default"],
    "mi355q_bfp_attention_decode_kv8": ["strides=NULL", "G=0", "G=1", "causal=0", "L=64", "qk_params[0]=9", "qk_params[2]=default", "pv_params[0]=9", "pv_params[2]=default"],
    "mi355q_bfp_attention_decode_window": ["block_table=NULL", "strides=NULL", "G=0", "G=1", "window=100", "L=64", "qk_params[0]=9", "qk_params[3]=1", "qk_params[3]=9",
        "qk_params[3]=10", "qk_params[4]=0", "qk_params[4]=9", "qk_params[2]=default", "pv_params[0]=9", "pv_params[3]=1", "pv_params[3]=9",
        "pv_params[3]=10", "pv_params[4]=0", "pv_params[4]=9", "pv_params[2]=default", "block_table=NULL + P=16", "block_table=NULL + P=48",
        "block_table=NULL + num_pages=0"],
    "mi355q_bfp_attention_extend_window": ["counts=NULL", "block_table=NULL", "strides=NULL", "G=0", "G=1", "G=65537", "window=100", "L=64", "qk_params[0]=9", "qk_params[3]=1",
        "qk_params[3]=9", "qk_params[3]=10", "qk_params[4]=0", "qk_params[4]=9", "qk_params[2]=default", "pv_params[0]=9", "pv_params[3]=1",
        "pv_params[3]=9", "pv_params[3]=10", "pv_params[4]=0", "pv_params[4]=9", "pv_params[2]=default", "block_table=NULL + P=16",
        "block_table=NULL + P=48", "block_table=NULL + num_pages=0", "M=17 + L=64"],
}


def baseline(args):
    return [BASE[a] for a in args]


def perturbations(args):
    """[(label, {argument or (argument, index): value})] of one export: every perturbation whose arguments the export has"""
    out = []
    for a in args:
        if a in PTR16 + PTR4 + SIZES + HOST:
            out.append((f"{a}=NULL", {a: None}))
        if a in PTR16:
            out.append((f"{a}+4", {a: BASE[a] + 4}))
        if a in PTR4:
            out.append((f"{a}+2", {a: BASE[a] + 2}))
    scalars = dict(B=(0, 65536), C=(0, 40, 2 ** 30 + 16), D=(16, 48, 160), M=(-1, 0, 17), n=(-1, 0), splits=(-1,), G=(-1, 0, 1, 65537),
                   P=(16, 48), max_pages=(0,), num_pages=(0,), window=(0, 100), causal=(0,), L=(-1, 1, CAP, CAP + 1))
    for a, values in scalars.items():
        if a in args:
            out += [(f"{a}={v}", {a: v}) for v in values]
    if "L" in args and "n" in args:
        out.append((f"L+n={CAP + 1}", {"L": CAP - 4, "n": 5}))
    for a in ("qk_params", "pv_params"):
        if a in args:
            for i in (0, 3):
                out += [(f"{a}[{i}]={w}", {(a, i): w}) for w in (1, 9, 10)]
                out += [(f"{a}[{i + 1}]={e}", {(a, i + 1): e}) for e in (0, 9)]
            out.append((f"{a}[2]=default", {(a, 2): BIAS_DEFAULT}))
    if "strides" in args:
        out.append(("strides[1]=66", {("strides", 1): 66}))
    return out


def apply(args, perts):
    """the argument list of a call under some perturbations, None when two of them set the same argument"""
    values, seen = [list(v) if isinstance(v, list) else v for v in baseline(args)], set()
    for p in perts:
        for key, v in p.items():
            name, i = key if isinstance(key, tuple) else (key, None)
            if (name, i) in seen or (name, None) in seen or (i is None and any(s[0] == name for s in seen)):
                return None
            seen.add((name, i))
            if i is None:
                values[args.index(name)] = v
            elif values[args.index(name)] is None:
                return None
            else:
                values[args.index(name)][i] = v
    return values


def marshal(args, values):
    """ctypes arguments of one call; `keep` holds the host arrays alive"""
    keep, out = [], []
    for a, v in zip(args, values):
        if a in SIZES:
            v = None if v is None else C.c_int64(0)
        elif a in HOST:
            v = None if v is None else ((C.c_int64 * 4) if a == "strides" else (C.c_int32 * 6))(*v)
        if a in SIZES + HOST:
            keep.append(v)
            out.append(None if v is None else C.addressof(v))
        else:
            out.append(v)
    return out, keep


def cases(export, args):
    """(i, j, values) for every single (j = -1) and every pair i < j of perturbations that is to be called"""
    perts = perturbations(args)
    launches = set(LAUNCHES.get(export, ()))
    benign = {i for i, (label, _) in enumerate(perts) if label in launches}
    for i, (label, p) in enumerate(perts):
        if i not in benign:
            yield i, -1, apply(args, [p])
    for (i, (li, pi)), (j, (lj, pj)) in itertools.combinations(enumerate(perts), 2):
        values = apply(args, [pi, pj])
        if values is None or (i in benign and j in benign) or f"{li} + {lj}" in launches:
            continue
        yield i, j, values


# mi355q_debug_kv_call's flat arguments (csrc/mi355q_api.hip): 14 addresses, then 13 integers
SLOTS = ("kq vq stage k v q out workspace lengths counts block_table k_bytes v_bytes stage_bytes "
         "B C max_pages num_pages P D M L n G causal window splits").split()


def dump(count):
    import numpy as np
    rows = np.load(GOLDEN.with_suffix(".npz"))["rows"].tolist()
    for e, i, j, code in rows[::max(1, len(rows) // count)]:
        args = EXPORTS[e][1].split()
        perts = perturbations(args)
        values = dict(zip(args, apply(args, [perts[i][1]] + ([perts[j][1]] if j >= 0 else []))))
        flat = [(0 if values.get(a) is None else 1 << 20) if a in SIZES else int(values.get(a) or 0) for a in SLOTS]
        host = [w for a, n in zip(HOST, (6, 6, 4)) for w in [int(values.get(a) is not None)] + list(values.get(a) or [0] * n)]
        print(e, code, *flat, *host)


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="the commit the loaded library was built from (the fixture's header)")
    ap.add_argument("--dump", type=int, metavar="N", help="print N recorded rows for tools/kv_call_check and call nothing")
    ap.add_argument("--discover", action="store_true", help="print the cases that reach a launch (for LAUNCHES) and write nothing")
    opt = ap.parse_args()
    if opt.dump:
        return dump(opt.dump)
    if not opt.commit and not opt.discover:
        ap.error("--commit is required to record")
    import torch
    if torch.cuda.is_available():
        sys.exit("record_kv_api_codes: a GPU is visible; the calls carry fake pointers and are for a machine without one")
    from mi355q import _lib
    lib = _lib.load_library()
    rows, found = [], {}
    for e, (export, names) in enumerate(EXPORTS):
        args = names.split()
        types = _lib.SIGNATURES[export][1]
        assert len(types) == len(args) and all((t is C.c_void_p) == (a in PTR16 + PTR4 + SIZES + HOST + ("stream",)) for a, t in zip(args, types)), export
        labels = [label for label, _ in perturbations(args)]
        assert set(LAUNCHES.get(export, ())) <= set(labels) | {f"{a} + {b}" for a, b in itertools.combinations(labels, 2)}, export
        for i, j, values in cases(export, args):
            call, keep = marshal(args, values)
            code = getattr(lib, export)(*call)
            what = labels[i] if j < 0 else f"{labels[i]} + {labels[j]}"
            if code not in (0, -1, -2, -3):
                found.setdefault(export, []).append(what)
                continue
            rows.append((e, i, j, code))
    if opt.discover:
        print(json.dumps(found, indent=1))
        return
    assert not found, f"these cases reached a launch (code outside 0, -1, -2, -3): list them in LAUNCHES\n{json.dumps(found, indent=1)}"
    doc = {"header": {"commit": opt.commit, "how": "tools/record_kv_api_codes.py with MI355Q_LIBRARY = the library built at that commit, on a machine "
                                                   "without a GPU; rows (tests/golden/kv_api_codes.npz): export, perturbation, second perturbation "
                                                   "or -1, code"},
           "ptr16": PTR16, "ptr4": PTR4, "sizes": SIZES, "host": HOST,
           "exports": [{"name": export, "args": names.split(), "baseline": baseline(names.split()),
                        "perturbations": [[label, [[*(k if isinstance(k, tuple) else (k, None)), v] for k, v in p.items()]]
                                          for label, p in perturbations(names.split())],
                        "launches": LAUNCHES.get(export, [])} for export, names in EXPORTS]}
    GOLDEN.write_text(json.dumps(doc, indent=None, separators=(",", ":")).replace('{"name"', '\n{"name"') + "\n")
    np.savez_compressed(GOLDEN.with_suffix(".npz"), rows=np.asarray(rows, dtype=np.int32))
    print(f"{len(rows)} rows of {len(EXPORTS)} exports -> {GOLDEN}")


if __name__ == "__main__":
    main()
