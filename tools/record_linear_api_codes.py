#!/usr/bin/env python3
"""Records tests/golden/linear_api_codes.json / .npz: the return code of each Linear-side export (the row and tiled quantisers and the
products, mi355q_block_fp_quantize_aligned_rows .. mi355q_mx_gemm) for every single perturbation of a valid baseline call and for
every pair of perturbations -- the pairs fix the ORDER of the checks, which is ABI.  The `aligned` products and _multi are recorded
under mi355q_bfp_gemm_set_variant 0, 2 and 8: one entry each.  tests/test_linear_api_codes.py replays the table.

A host-only job for a machine WITHOUT a GPU: the data pointers are fake (non-null, 16-byte aligned integers; the operand structs and
_multi's arrays are real host memory with fake pointers inside), so a call must end in the argument checks.  The tool refuses to run
where torch sees a GPU.  The baseline and every case listed in the fixture's "launches" -- the perturbations that leave a call valid --
are never called when recording; --discover finds them (a code outside 0, -1, -2, -3: the case reached a launch) and writes them
into the fixture, where recording reads them.  Recording stops at any such code and names the case.

    MI355Q_LIBRARY=<libmi355q.so of the commit to record> python tools/record_linear_api_codes.py --discover
    MI355Q_LIBRARY=<the same>                             python tools/record_linear_api_codes.py --commit <that commit>
"""
import argparse
import ctypes as C
import itertools
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
GOLDEN = ROOT / "tests" / "golden" / "linear_api_codes.json"

# every argument an export can have: addresses, then integers (and the float eps)
PTRS = ("x x2 x3 colmap mant exp rowflag rowscale list list_to_clear p0 p1 p2 p3 p4 p5 y y_tiled workspace xo wo wos x1 w1 bias biases out outs "
        "resid").split()
INTS = "pre_op M N K seg_len seg_stride n0 n1 width exponent_width exponent_bias bucket_cap ldy ldr K1 x_seg_stride count x_segs".split()
STRUCTS = ("xo", "wo")                       # mi355q_bfp_operand: real host memory
ARRAYS = ("wos", "biases", "outs")           # _multi's host arrays (three entries each)
FIELDS = "mant exp rowflag gscale list list_cap mbits exp_bias row_aligned".split()
FAKE = [a for a in PTRS if a not in STRUCTS + ARRAYS]
MAX_K, CAP_MAX, BIAS_DEFAULT = 16384, 1016, -2 ** 31
ROWS = "mant exp rowflag rowscale list list_to_clear M K"
QUANT = "width exponent_width exponent_bias"
# the exports in the order of csrc/mi355q_api.hip, with their arguments in order.  One name per role: M the rows,
# p0 .. p5 the MX planes, list / list_to_clear also MX's bad words, out the product (or the epilogues' scratch), y_tiled every tiled
# bf16 output, x1 / w1 the tiled operands; what an export sets itself on the way to the check comes third
EXPORTS = [
    ("mi355q_block_fp_quantize_aligned_rows", f"x {ROWS} {QUANT} bucket_cap stream", {}),
    ("mi355q_block_fp_quantize_aligned_rows_pre", f"x x2 pre_op {ROWS} {QUANT} bucket_cap stream", {}),
    ("mi355q_block_fp_quantize_aligned_rows_norm", f"x x2 x3 pre_op eps {ROWS} {QUANT} bucket_cap stream", {}),
    ("mi355q_block_fp_quantize_aligned_rows_seg", f"x x2 x3 pre_op eps {ROWS} seg_len seg_stride {QUANT} bucket_cap stream", {}),
    ("mi355q_block_fp_quantize_classes", f"x colmap n0 n1 mant exp rowflag rowscale list list_to_clear y_tiled M K {QUANT} bucket_cap stream", {}),
    ("mi355q_block_fp_quantize_mx", f"x p0 p1 p2 list list_to_clear M K {QUANT} stream", {}),
    ("mi355q_block_fp_quantize_bf16_tiled", f"x y y_tiled M K {QUANT} workspace stream", {}),
    ("mi355q_block_fp_quantize_bf16_tiled_pre", f"x x2 pre_op y y_tiled M K {QUANT} workspace stream", {}),
    ("mi355q_block_fp_quantize_bf16_tiled_norm", f"x x2 pre_op eps y y_tiled M K {QUANT} workspace stream", {}),
    ("mi355q_block_minifloat_quantize_bf16_tiled", f"x y_tiled M K {QUANT} workspace stream", {}),
    ("mi355q_bf16_tile", "x y_tiled M K stream", {}),
    ("mi355q_bfp_gemm_aligned", "xo wo bias out M N K ldy stream", {}),
    ("mi355q_bfp_gemm_aligned_res", "xo wo bias resid ldr out M N K ldy stream", {}),
    ("mi355q_bfp_gemm_mixed", "xo wo x1 w1 bias out M N K K1 ldy stream", {}),
    ("mi355q_bfp_gemm_aligned_gated", f"xo wo bias out y_tiled M N K {QUANT} stream", {}),
    ("mi355q_bfp_gemm_aligned_relu", f"xo wo bias out y_tiled M N K {QUANT} stream", {}),
    ("mi355q_bfp_gemm_aligned_multi", "xo wos biases outs count M N K ldy stream", {}),
    ("mi355q_bf16_gemm_tiled", "x1 w1 bias out M N K ldy stream", {"x_segs": 1}),
    ("mi355q_bf16_gemm_tiled_res", "x1 w1 bias resid ldr out M N K ldy stream", {"x_segs": 1}),
    ("mi355q_bf16_gemm_tiled_seg", "x1 w1 bias out M N K ldy x_segs x_seg_stride stream", {}),
    ("mi355q_mx_gemm", f"p0 p1 p2 p3 p4 p5 list x w1 bias out M N K ldy {QUANT} stream", {}),
]
VARIANTS = {"mi355q_bfp_gemm_aligned": (0, 2, 8), "mi355q_bfp_gemm_aligned_res": (0, 2, 8), "mi355q_bfp_gemm_aligned_multi": (0, 2, 8)}
# cases that pass the argument check and are answered -1 by the launch PLANNER behind it (K = 0 makes the row flags optional for the
# check; the planner wants them with the lists): launching cases whatever --discover sees, never called when recording
PLANNER_REFUSES = {f"{name}@0": ["K=0 + xo.rowflag=NULL", "K=0 + wo.rowflag=NULL"] for name in ("mi355q_bfp_gemm_aligned", "mi355q_bfp_gemm_aligned_res")}
ENTRIES = [(i, v) for i, (name, _, _) in enumerate(EXPORTS) for v in VARIANTS.get(name, (0,))]      # (export id, variant)

SEG_STRIDE = 128 * 256                       # mi355q_bfp_tiled_bytes(M, 2 * K / x_segs): one segment of the baseline, tiled
BASE = dict(pre_op=0, eps=1e-5, M=4, N=64, K=256, seg_len=0, seg_stride=0, n0=8, n1=8, width=6, exponent_width=8, exponent_bias=127, bucket_cap=0,
            ldy=64, ldr=64, K1=128, x_seg_stride=SEG_STRIDE, count=2, x_segs=2, stream=0)
BASE.update({name: 0x10000 * (i + 1) for i, name in enumerate(FAKE)})


def operand(seed):
    return dict({f: 0x1000000 * seed + 0x10000 * (i + 1) for i, f in enumerate(FIELDS[:5])}, list_cap=0, mbits=5, exp_bias=127, row_aligned=1)


BASE.update(xo=operand(1), wo=operand(2), wos=[operand(3), operand(4), operand(5)], biases=[0x7100000, 0x7200000, 0x7300000],
            outs=[0x8100000, 0x8200000, 0x8300000])
OWN = {"mi355q_block_fp_quantize_mx": dict(width=4), "mi355q_mx_gemm": dict(width=4),
       "mi355q_block_minifloat_quantize_bf16_tiled": dict(width=8, exponent_width=4, exponent_bias=8)}


def baseline(export, args):
    return [dict(BASE, **OWN.get(export, {}))[a] for a in args]


def perturbations(export, args):
    """[(label, {argument or (argument, field) or (argument, index, field): value})]: every perturbation whose arguments the export has"""
    out = []
    for a in args:
        if a in PTRS:
            out.append((f"{a}=NULL", {a: None}))
        if a in FAKE:
            out.append((f"{a}+4", {a: BASE[a] + 4}))
    if "list_to_clear" in args:
        out.append(("list_to_clear=list", {"list_to_clear": BASE["list"]}))
    caps = (-2, -1, 0, 120, CAP_MAX, CAP_MAX + 1)
    scalars = dict(M=(0, -1), N=(0, -1, 48), K=(0, -1, 48, 64, 192, MAX_K + 64), ldy=(63,), ldr=(63, 65), width=(1, 5, 6, 8, 9, 10, 26),
                   exponent_width=(0, 9), exponent_bias=(BIAS_DEFAULT, -1), bucket_cap=caps, pre_op=(0, 1, 2, 3, 4, 5), eps=(-1.0, float("nan")),
                   seg_len=(0, -1, 63, 48, 64, 256), seg_stride=(0, -1, 255, 256), n0=(0, -1, 6, 12), n1=(0, -1, 7, 4), count=(0, 1, 2, 3, 4),
                   x_segs=(0, 1, 2, 3), x_seg_stride=(0, 8, SEG_STRIDE - 16), K1=(0, -1, 64, 128, 96, MAX_K + 64))
    if export == "mi355q_bfp_gemm_mixed":
        scalars["K"] = (0, -1, 128, 256, 320, MAX_K + 128)
    for a, values in scalars.items():
        if a in args:
            out += [(f"{a}={'default' if v == BIAS_DEFAULT else v}", {a: v}) for v in values]
    if "seg_len" in args:           # a valid split, a stride too short for the rows, a stride that is no multiple of 4
        out += [(f"seg={n}/{s}", {"seg_len": n, "seg_stride": s}) for n, s in ((64, 256), (64, 252), (64, 258), (256, 1024))]
    for a in args:
        fields = [(a,)] if a in STRUCTS else [(a, 0), (a, 1)] if a == "wos" else []
        for key in fields:
            label = ".".join(str(k) for k in key)
            out += [(f"{label}.{f}=NULL", {key + (f,): None}) for f in FIELDS[:5]]
            out.append((f"{label}.mant+4", {key + ("mant",): 4 + (BASE[a] if a in STRUCTS else BASE[a][key[1]])["mant"]}))
            out += [(f"{label}.list_cap={v}", {key + ("list_cap",): v}) for v in caps]
            out += [(f"{label}.row_aligned={v}", {key + ("row_aligned",): v}) for v in (0, 1, 2)]
            out += [(f"{label}.mbits={v}", {key + ("mbits",): v}) for v in (0, 4, 8)]
            out.append((f"{label}.exp_bias=126", {key + ("exp_bias",): 126}))
        if a in ("wos", "outs"):
            out += [(f"{a}.{i}=NULL", {(a, i): None}) for i in (0, 1)]
    return out


def apply(export, args, perts):
    """{argument: value} of a call under some perturbations, None when two of them set the same thing"""
    values = json.loads(json.dumps(dict(zip(args, baseline(export, args)))))
    seen = set()
    for p in perts:
        for key, v in p.items():
            key = key if isinstance(key, tuple) else (key,)
            if any(key[:n] in seen for n in range(1, len(key) + 1)) or any(s[:len(key)] == key for s in seen):
                return None
            seen.add(key)
            at = values
            for k in key[:-1]:
                at = at[k]
                if at is None:
                    return None
            at[key[-1]] = v
    return values


def struct(fields):
    from mi355q import _lib
    return _lib.BfpOperand(*[fields[f] for f in FIELDS])


def marshal(args, values):
    """ctypes arguments of one call; `keep` holds the host memory alive"""
    keep, out = [], []
    for a in args:
        v = values[a]
        if v is not None and a in STRUCTS:
            v = struct(v)
        elif v is not None and a in ARRAYS:
            made = [None if e is None else struct(e) if a == "wos" else e for e in v]
            keep.append(made)
            v = (C.c_void_p * 3)(*[C.addressof(e) if isinstance(e, C.Structure) else e for e in made])
        if a in STRUCTS + ARRAYS and v is not None:
            keep.append(v)
            v = C.addressof(v)
        out.append(v)
    return out, keep


def cases(export, args, launches):
    """(i, j, values) for every single (j = -1) and every pair i < j of perturbations that is to be called"""
    perts = perturbations(export, args)
    benign = {i for i, (label, _) in enumerate(perts) if label in launches}
    for i, (label, p) in enumerate(perts):
        if i not in benign:
            yield i, -1, apply(export, args, [p])
    for (i, (li, pi)), (j, (lj, pj)) in itertools.combinations(enumerate(perts), 2):
        values = apply(export, args, [pi, pj])
        if values is None or (i in benign and j in benign) or f"{li} + {lj}" in launches:
            continue
        yield i, j, values


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="the commit the loaded library was built from (the fixture's header)")
    ap.add_argument("--discover", action="store_true", help="find the cases that reach a launch and write them into the fixture")
    opt = ap.parse_args()
    if not opt.commit and not opt.discover:
        ap.error("--commit is required to record")
    import torch
    if torch.cuda.is_available():
        sys.exit("record_linear_api_codes: a GPU is visible; the calls carry fake pointers and are for a machine without one")
    from mi355q import _lib
    lib = _lib.load_library()
    known = {} if opt.discover else {f"{x['name']}@{x['variant']}": x["launches"] for x in json.loads(GOLDEN.read_text())["entries"]}
    rows, found = [], {}
    for e, (x, variant) in enumerate(ENTRIES):
        export, names, _ = EXPORTS[x]
        args = names.split()
        types = _lib.SIGNATURES[export][1]
        assert len(types) == len(args) and all((t is C.c_void_p) == (a in PTRS + ["stream"]) for a, t in zip(args, types)), export
        labels = [label for label, _ in perturbations(export, args)]
        assert len(set(labels)) == len(labels), export
        entry = f"{export}@{variant}"
        lib.mi355q_bfp_gemm_set_variant(variant)
        try:
            for i, j, values in cases(export, args, set(known.get(entry, ()))):
                call, keep = marshal(args, values)
                code = getattr(lib, export)(*call)
                if code not in (0, -1, -2, -3):
                    found.setdefault(entry, []).append(labels[i] if j < 0 else f"{labels[i]} + {labels[j]}")
                    continue
                rows.append((e, i, j, code))
        finally:
            lib.mi355q_bfp_gemm_set_variant(0)
    if opt.discover:
        # a pair of two perturbations that each launch alone is never called: only the others are kept
        for entry, labels in found.items():
            alone = {w for w in labels if " + " not in w}
            found[entry] = [w for w in labels if " + " not in w or not set(w.split(" + ")) <= alone]
        for entry, labels in PLANNER_REFUSES.items():
            found[entry] = found.get(entry, []) + labels
        print(f"{sum(len(v) for v in found.values())} launching cases -> {GOLDEN}; now record")
        known, rows = found, []
    assert opt.discover or not found, f"these cases reached a launch (code outside 0, -1, -2, -3): run --discover\n{json.dumps(found, indent=1)}"
    listed = lambda p: [[list(k) if isinstance(k, tuple) else [k], v] for k, v in p.items()]
    doc = {"header": {"commit": opt.commit, "how": "tools/record_linear_api_codes.py with MI355Q_LIBRARY = the library built at that commit, on a "
                                                   "machine without a GPU; rows (tests/golden/linear_api_codes.npz): entry, perturbation, second "
                                                   "perturbation or -1, code"},
           "structs": STRUCTS, "arrays": ARRAYS, "fields": FIELDS,
           "entries": [{"name": EXPORTS[x][0], "id": x, "variant": v, "args": EXPORTS[x][1].split(), "fixed": EXPORTS[x][2],
                        "baseline": baseline(EXPORTS[x][0], EXPORTS[x][1].split()),
                        "perturbations": [[label, listed(p)] for label, p in perturbations(EXPORTS[x][0], EXPORTS[x][1].split())],
                        "launches": known.get(f"{EXPORTS[x][0]}@{v}", [])} for x, v in ENTRIES]}
    GOLDEN.write_text(json.dumps(doc, indent=None, separators=(",", ":")).replace('{"name"', '\n{"name"') + "\n")
    if opt.discover:
        return
    np.savez_compressed(GOLDEN.with_suffix(".npz"), rows=np.asarray(rows, dtype=np.int32))
    singles = sum(1 for r in rows if r[2] < 0)
    print(f"{len(rows)} rows ({singles} single perturbations, {len(rows) - singles} pairs) of {len(ENTRIES)} entries, {len(EXPORTS)} exports -> {GOLDEN}")


if __name__ == "__main__":
    main()
