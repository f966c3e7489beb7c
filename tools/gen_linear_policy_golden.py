"""Record the route decisions of the quantised Linear as they were BEFORE quantized_modules/linear_policy.py existed, into
tests/golden/linear_policy.json and .npz (tests/test_linear_policy.py holds linear_policy.py to every row).

    git show <parent>:llm-mixed-q_amd/mi355q/quantize/quantized_modules/linear.py > parent_linear.py
    python tools/gen_linear_policy_golden.py parent_linear.py --commit <parent>

The parent's linear.py is loaded next to the package's modules and its OWN methods are called on layers built on the meta device
(no storage), with stand-in inputs that carry only what the predicates read (is_cuda, dtype, ndim, shape, numel, requires_grad).
The measuring calls of `ops` are stubs that return prescribed fills, `_try_mixed` (where the row / block decision calls it) a stub
that notes that it was asked and answers as prescribed.  Needs no GPU; never imports linear_policy."""
import argparse
import importlib.util
import io
import json
import sys
import zipfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "llm-mixed-q_amd"), str(ROOT)]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mi355q import ops  # noqa: E402

BASE = dict(name="block_fp", is_ptq=True, bypass=False)
for _p in ("data_in", "weight", "bias"):
    BASE.update({f"{_p}_width": 6, f"{_p}_exponent_width": 8, f"{_p}_exponent_bias": 127, f"{_p}_exponent_bias_width": 8,
                 f"{_p}_frac_width": 3, f"{_p}_block_size": [16] if _p == "bias" else [1, 16]})
SHAPE_K = [48, 64, 96, 512, 4096, 16384, 16512]
SHAPE_MN = [(2048, 4096), (2048, 11008)]
ALIGNS = ["auto", "rows", "rows_post", "blocks", "groups"]
ARITHS = ["block_fp", "block_minifloat", "block_log", "integer", "minifloat_ieee", "minifloat_denorm", "log"]
FAST, SLOW = ops.ROW_TILE_ENTRIES_FAST, ops.ROW_TILE_ENTRIES_SLOW


class Standin:
    """what the predicates read of a tensor, and nothing else"""
    def __init__(self, *shape, is_cuda=True, dtype=torch.float32):
        self.shape, self.ndim, self.is_cuda, self.dtype, self.requires_grad, self.device = tuple(shape), len(shape), is_cuda, dtype, False, "standin"

    def numel(self):
        n = 1
        for d in self.shape:
            n *= d
        return n

    def reshape(self, *shape):
        return self


class Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class StubOps:
    """the real `ops` (constants, pure helpers) with the measuring / packing calls replaced"""
    def __init__(self, **stubs):
        self.__dict__.update(stubs)

    def __getattr__(self, name):
        return getattr(ops, name)


class Stop(Exception):
    pass


def load_parent(path):
    spec = importlib.util.spec_from_file_location("mi355q.quantize.quantized_modules._parent_linear", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def layer(P, K, N, over=None, arith="block_fp"):
    cfg = dict(BASE, **(over or {}))
    cls = {c.arith: c for c in (P.LinearBlockFP, P.LinearBlockMinifloat, P.LinearBlockLog, P.LinearInteger, P.LinearMinifloatIEEE,
                                P.LinearMinifloatDenorm, P.LinearLog)}[arith]
    return cls(K, N, bias=True, device="meta", config=cfg)


def x_of(ndim, K, rows=4):
    return Standin(*{1: (K,), 2: (rows, K), 3: (2, rows, K), 4: (2, 2, rows, K)}[ndim])


def either_side(key, values):
    return [{f"{p}_{key}": v} for p in ("data_in", "weight") for v in values]


def rec_int8_plan(P):
    overs = ([{}] + either_side("width", [1, 2, 8, 9, 10]) + either_side("exponent_width", [0, 1, 8, 9])
             + either_side("exponent_bias", [None, "none", -3, 127]) + either_side("block_size", [[1, 32], [16]])
             + [{"data_in_exponent_bias": None, "data_in_exponent_width": 1}, {"weight_exponent_bias": "None", "weight_exponent_width": 5}])
    rows = []
    for K in SHAPE_K:
        for _, N in SHAPE_MN:
            cases = [("block_fp", o, 2) for o in overs] + [("block_fp", {}, nd) for nd in (1, 3, 4)] + [(a, {}, 2) for a in ARITHS[1:]]
            cases += [("block_fp", {"data_in_block_size": [1, 32]}, 3), ("block_fp", {"data_in_block_size": [16]}, 3)]
            for arith, over, nd in cases:
                lin, x = layer(P, K, N, over, arith), x_of(nd, K)
                plan = lin._int8_plan(x)
                if arith == "block_fp" and 2 <= nd:
                    assert plan == lin._int8_plan_uncached(x)
                rows.append([over, arith, K, N, nd, x.shape[-2] if nd == 3 else 0, None if plan is None else list(plan)])
    return dict(fields=["config", "arith", "K", "N", "x_ndim", "x_rows_dim", "plan"], rows=rows)


def rec_exponent_bias(P):
    rows = []
    for bias in (None, "none", "None", -3, 0, 127):
        for ew in (0, 1, 8, 9):
            lin = layer(P, 64, 64, {"weight_exponent_bias": bias, "weight_exponent_width": ew})
            rows.append([bias, ew, lin._weight_bias_value()])
    return dict(fields=["bias", "exponent_width", "value"], rows=rows)


def rec_initial_x_cap(P):
    rows = []
    for align in ALIGNS + ["other", None]:
        lin = layer(P, 64, 64, {} if align is None else {"mi355q_align": align})
        first = lin._x_cap
        lin._x_cap = 7
        lin.requantize()
        assert lin._x_cap == first
        rows.append([lin.align, first])
    return dict(fields=["align", "x_cap"], rows=rows)


def x_fullest_around(w_max, tile_rows):
    """the activations' fullest buckets at which a tile's entries reach 47 .. 49 and 87 .. 89, by the parent's own formula"""
    f = 0.5 * 1.15 if tile_rows == 128 else 1.0
    return [0] + [x for x in range(1, 200) if w_max + int(x * f + 0.999) in (FAST - 1, FAST, FAST + 1, SLOW - 9, SLOW - 8, SLOW - 7)]


def rec_align(P):
    rows = []
    for K in SHAPE_K:
        for M, N in SHAPE_MN:
            tile_rows = ops.gemm_tile_rows(M, N)
            assert tile_rows == (128 if N == 4096 else 256)
            for align in ALIGNS:
                full = align == "auto" and ops.row_align_supported(K)
                w_fills = [(0, 0), (0, 10), (0, FAST - 1), (0, FAST), (0, FAST + 1), (1, 0), (1, FAST)] if full else [(0, 0), (1, FAST + 1)]
                for w_fill in w_fills:
                    x_fills = ([None, (1, 0)] + [(0, x) for x in x_fullest_around(w_fill[1], tile_rows)]) if full else [None, (0, 0), (1, 200)]
                    for x_fill in x_fills:
                        for answer in (False, True):
                            rows.append([K, N, M, align, list(w_fill), x_fill and list(x_fill), answer,
                                         choose_align(P, K, N, M, align, w_fill, x_fill, answer)])
    return dict(fields=["K", "N", "M", "align", "w_fill", "x_fill (null: no sample)", "mixed_answer", "[x_cap, mixed_asked, returned] or the error"],
                rows=rows)


def choose_align(P, K, N, M, align, w_fill, x_fill, answer):
    lin, asked = layer(P, K, N, {"mi355q_align": align}), []
    P.ops = StubOps(bfp_align_rows=lambda *a, **k: Obj(sparse=None, tiled=None),
                    block_fp_quantize_aligned_rows=lambda *a, **k: Obj(sparse=None, rows=M, list_cap=k["bucket_cap"]),
                    row_list_fill=lambda *a: tuple(w_fill) if len(a) == 2 else tuple(x_fill))
    lin._try_mixed = lambda wm, we, xs: (asked.append(1), answer)[1]
    try:
        mode = lin._choose_align_mode(None, None, None if x_fill is None else Standin(M, K))
    except ValueError as e:
        return f"ValueError: {e}"
    finally:
        P.ops = ops
    return [lin._x_cap, len(asked), mode]


def try_mixed(P, K, over, sample, n_outlier=0, w_fill=(0, 0), x_fill=(0, 0), stop_at_classes=False):
    """the parent's _try_mixed on prescribed measurements -> (result, quantiser launched?, class-1 blocks handed to ColumnClasses)"""
    N, nb, seen = 4, K // 16, dict(quantised=False, n1=0)
    lin = layer(P, K, N, over)
    share = torch.zeros(max(nb, 1))
    share[:n_outlier] = 1.0

    def classes(K_, blocks1, device):
        seen["n1"] = len(blocks1)
        if stop_at_classes:
            raise Stop
        b1 = sorted(blocks1)
        b0 = [b for b in range(nb) if b not in set(b1)]
        cols = lambda bs: [16 * b + i for b in bs for i in range(16)]  # noqa: E731
        return Obj(blocks0=b0, cols0=cols(b0), cols1=cols(b1), K1=16 * len(b1))
    P.ops = StubOps(block_fp_quantize=lambda *a, **k: (seen.update(quantised=True), (None, None, torch.zeros(2 * max(nb, 1), dtype=torch.uint8)))[1],
                    ColumnClasses=classes, bfp_align_rows=lambda *a, **k: Obj(sparse=None),
                    row_list_fill=lambda *a: tuple(w_fill) if len(a) == 2 else tuple(x_fill),
                    block_fp_quantize_classes=lambda *a, **k: (Obj(sparse=None, rows=2, list_cap=k["bucket_cap"]), None),
                    bf16_tile=lambda t: "tiled")
    lin._outlier_share = lambda codes, spare: share
    wm, we = torch.zeros(N * K, dtype=torch.int8), torch.zeros(N * max(nb, 1), dtype=torch.uint8)
    try:
        got = lin._try_mixed(wm, we, Standin(2, K) if sample else None)
        assert (lin._mixed is not None) == got
    except Stop:
        got = None
    finally:
        P.ops = ops
    return got, seen["quantised"], seen["n1"]


def rec_mixed_gate(P):
    rows, Ks = [], [48, 64, 96, 384, 512, 640, 4096, 16384, 16512]
    cases = [(K, align, {"mi355q_mixed": knob} if knob != "absent" else {}, True)
             for K in Ks for align in ALIGNS for knob in ("absent", "auto", False, "off", None)]
    cases += [(K, "auto", dict(o, mi355q_weight_storage=st), True) for K in Ks for st in ("int8", "packed", "hybrid")
              for o in [{}] + either_side("width", [8, 9])]
    cases += [(K, "auto", {}, False) for K in Ks]
    for K, align, over, sample in cases:
        got, quantised, _ = try_mixed(P, K, dict(over, mi355q_align=align), sample)
        assert got is False
        rows.append([over, K, align, sample, quantised])
    return dict(fields=["config", "K", "align", "sample given", "past the gate (the activations' exponents were read)"], rows=rows)


def rec_mixed_size(P):
    rows = []
    for nb in (32, 64, 256):
        half = nb // 2
        counts = range(nb + 1) if nb < 256 else sorted({0, 1, 8, 9, *range(half - 9, half + 10), *range(nb - 16 - 9, nb - 16 + 10)})
        for n in counts:
            got, _, n1 = try_mixed(P, 16 * nb, {}, True, n_outlier=n, stop_at_classes=True)
            assert (got is False and n1 == 0) or (got is None and n1 > 0)
            rows.append([n, nb, n1])
    return dict(fields=["outlier columns", "nb = K // 16", "class-1 blocks (0: no split)"], rows=rows)


def rec_mixed_fits(P):
    rows = []
    for w_fill in [(0, 0), (0, 10), (0, FAST - 1), (0, FAST), (0, FAST + 1), (1, 0)]:
        for x_fill in [(1, 0)] + [(0, x) for x in sorted({0, *(max(0, FAST - w_fill[1] + d) for d in (-1, 0, 1))})]:
            got, _, n1 = try_mixed(P, 512, {}, True, n_outlier=8, w_fill=w_fill, x_fill=x_fill)
            assert n1 == 8
            rows.append([list(w_fill), list(x_fill), got])
    return dict(fields=["class-0 w_fill", "class-0 x_fill", "split taken"], rows=rows)


def rec_routes(P):
    bf16, rides = [], []
    for K in SHAPE_K:
        for x_cap in (ops.ROW_NO_ALIGN, ops.ROW_BUCKET_CAP, ops.ROW_BUCKET_CAP_MAX):
            for over in [{}] + either_side("width", [9, 10]):
                for knob in ("absent", "bf16", "int8"):
                    o = dict(over) if knob == "absent" else dict(over, mi355q_blocks_gemm=knob)
                    lin = layer(P, K, 64, o)
                    lin._align_mode, lin._x_cap = "rows", x_cap
                    bf16.append([o, K, x_cap, lin._uses_bf16_route()])
            lin = layer(P, K, 64)
            lin._align_mode, lin._x_cap, lin._packed = "rows", x_cap, (None, None, 0, 0)
            rides.append([K, x_cap, lin._residual_rides_the_int8_product()])
    small = []
    for knob in ("absent", "off", "packed"):
        for rows in (0, 1, ops.SMALL_M_MAX, ops.SMALL_M_MAX + 1):
            o = {} if knob == "absent" else {"mi355q_small_m": knob}
            lin = layer(P, 64, 64, o)
            lin._w_packed = object()
            small.append([o, 64, rows * 64, lin._small_m_takes(Standin(rows, 64))])
    return (dict(fields=["config", "K", "x_cap", "uses_bf16_route (_align_mode = rows)"], rows=bf16),
            dict(fields=["K", "x_cap", "rides (packed, not mixed)"], rows=rides),
            dict(fields=["config", "K", "numel", "takes (weights at rest, not mixed)"], rows=small))


def rec_values_exact(P):
    rows = []
    for arith in ARITHS:
        overs = [{}, {"mi355q_values_gemm": "fp32"}, {"mi355q_values_gemm": "bf16"}]
        for p in ("data_in", "weight"):
            overs += [{f"{p}_width": 8, f"{p}_exponent_width": 8 - 1 - m} for m in (-1, 0, 7)] + [{f"{p}_width": 12, f"{p}_exponent_width": 3}]
            overs += [{f"{p}_width": w} for w in (1, 2, 9, 10)]
        for over in overs:
            for K in (48, 64):
                lin = layer(P, K, 64, dict(over, is_ptq=True), arith)
                lin.weight_requires_quantisation = False
                rows.append([over, arith, K, lin._values_exact_in_bf16(x_of(2, K))])
    return dict(fields=["config", "arith", "K", "exact (input on the device, weights quantised)"], rows=rows)


def rec_qat(P):
    rows = []
    shapes = [(2048, 4096, 2048), (2016, 4096, 2048), (2048, 4096, 2016), (1024, 4096, 4096), (2040, 4096, 2048), (0, 4096, 2048),
              (2048, 48, 2048), (2048, 4096, 40), (64, 64, 64)]
    assert shapes[0][0] * shapes[0][1] * shapes[0][2] == 1 << 34 and shapes[1][0] % 32 == 0
    for M, K, N in shapes:
        for knob in ("absent", "bf16", "bf16_always", "fp32"):
            cases = [("block_fp", o) for o in [{}] + either_side("width", [1, 2, 9, 10])] + [("integer", {}), ("integer", {"weight_width": 12}), ("log", {})]
            for arith, over in cases:
                o = dict(over, is_ptq=False) if knob == "absent" else dict(over, is_ptq=False, mi355q_qat_gemm=knob)
                lin = layer(P, K, N, o, arith)
                exact = arith != "block_fp" and lin._values_exact_in_bf16(Standin(M, K))
                rows.append([o, arith, K, N, M, exact, lin._qat_on_tile_gemm(Standin(M, K))])
    return dict(fields=["config", "arith", "K", "N", "M", "values exact in bf16 (not block_fp)", "on the tile GEMM"], rows=rows)


def rec_padded(P):
    rows = []
    for K in (16, 40, 48, 64, 80, 96, 112, 128):
        cases = [("block_fp", o, 2) for o in [{}, {"mi355q_pad_k": False}, {"mi355q_pad_k": True}] + either_side("width", [1, 2, 9, 10])
                 + either_side("block_size", [[1, 32]])]
        cases += [("block_fp", {}, nd) for nd in (1, 3, 4)] + [("integer", {}, 2), ("block_fp", {"data_in_block_size": [16]}, 3)]
        for arith, over, nd in cases:
            lin, x = layer(P, K, 96, over, arith), x_of(nd, K)
            lin.weight_requires_quantisation = False
            rows.append([over, arith, K, 96, nd, x.shape[-2] if nd == 3 else 0, lin._padded_block_fp_ok(x)])
    return dict(fields=["config", "arith", "K", "N", "x_ndim", "x_rows_dim", "padded route (fp32 operands on the device, weights quantised)"], rows=rows)


def rec_mx(P):
    conf, takes = [], []
    for K in (48, 512, 16384, 16512):
        for knob in ("absent", "auto", True, False, "off", None):
            cases = [("block_fp", o) for o in either_side("width", [1, 2, 4, 5, 6]) + [{"data_in_width": 4, "weight_width": 4}, {"data_in_width": 5, "weight_width": 5}]]
            cases += [("block_fp", {"data_in_width": 4, "weight_width": 4, "mi355q_weight_storage": st}) for st in ("int8", "packed", "hybrid")]
            cases += [("block_fp", {"data_in_width": 4, "weight_width": 4, "is_ptq": False}), ("block_fp", {"data_in_width": 4, "weight_width": 4, "bypass": True}),
                      ("integer", {"data_in_width": 4, "weight_width": 4})]
            for arith, over in cases:
                o = dict({"data_in_width": 4, "weight_width": 4}, **over)
                if knob != "absent":
                    o["mi355q_mx"] = knob
                lin = layer(P, K, 64, o, arith)
                lin.__dict__["weight"] = Standin(64, K)
                conf.append([o, arith, lin.is_ptq, lin.bypass, K, lin._mx_config_ok()])
    for knob in ("absent", "auto", True):
        for M, N in [(256 * 191, 256), (256 * 191 + 1, 256), (256 * 192, 256), (2048, 256 * 24 - 256), (2048, 256 * 24 - 255), (2048, 256 * 24), (1, 1)]:
            o = {} if knob == "absent" else {"mi355q_mx": knob}
            lin = layer(P, 128, N, o)
            lin._mx_w, lin._mx_version = Obj(c16=Obj(device="standin")), lin.weight._version
            takes.append([o, M, N, lin._mx_takes(Standin(M, 128))])
    return (dict(fields=["config", "arith", "is_ptq", "bypass", "K", "config ok (fp32 weights on the device, not released)"], rows=conf),
            dict(fields=["config", "M", "N", "takes (operand current, input on the device)"], rows=takes))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent_linear", help="a copy of the parent commit's quantized_modules/linear.py")
    ap.add_argument("--commit", required=True, help="the parent commit the copy was taken from (recorded in the header)")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "linear_policy.json"))
    a = ap.parse_args()
    P = load_parent(a.parent_linear)
    assert not hasattr(P, "policy"), "this is not the linear.py from before linear_policy.py"
    bf16, rides, small = rec_routes(P)
    mx_conf, mx_takes = rec_mx(P)
    sections = dict(int8_plan=rec_int8_plan(P), exponent_bias=rec_exponent_bias(P), initial_x_cap=rec_initial_x_cap(P), align=rec_align(P),
                    mixed_gate=rec_mixed_gate(P), mixed_class1_blocks=rec_mixed_size(P), mixed_fits=rec_mixed_fits(P), uses_bf16_route=bf16,
                    residual_rides_the_int8_product=rides, small_m_takes=small, values_exact_in_bf16=rec_values_exact(P),
                    qat_on_tile_gemm=rec_qat(P), padded_block_fp_ok=rec_padded(P), mx_config_ok=mx_conf, mx_takes=mx_takes)
    assert not torch.cuda.is_initialized()
    doc = dict(header=dict(what="route decisions of quantized_modules/linear.py's own methods, recorded by tools/gen_linear_policy_golden.py",
                           recorded_from_commit=a.commit, base_config=BASE,
                           constants={k: getattr(ops, k) for k in ("ROW_TILE_ENTRIES_FAST", "ROW_TILE_ENTRIES_SLOW", "ROW_BUCKET_CAP", "ROW_BUCKET_CAP_MAX",
                                                                  "ROW_NO_ALIGN", "ACTIVATION_BUCKET_CAP", "SMALL_M_MAX", "ROW_ALIGN_MAX_K")}),
               grid={k: dict(fields=v["fields"], rows=len(v["rows"])) for k, v in sections.items()})
    # the rows go next to the JSON as integers (as tests/golden/gemm_plan.npz does): every cell an index into "values", the distinct
    # JSON values in order of first appearance; "outcomes" lists the distinct outcomes each section recorded
    values, index, arrays = [], {}, {}
    for k, v in sections.items():
        arrays[k] = np.array([[index.setdefault(json.dumps(cell, sort_keys=True), len(index)) for cell in r] for r in v["rows"]], dtype=np.int32)
    values = [json.loads(t) for t in index]
    doc.update(values=values, outcomes={k: [values[i] for i in sorted(set(arr[:, -1].tolist()))] for k, arr in arrays.items()})
    out = Path(a.out)
    out.write_text("{\n" + ",\n".join(f' "{k}": {json.dumps(v)}' for k, v in doc.items()) + "\n}\n")
    with zipfile.ZipFile(out.with_suffix(".npz"), "w") as z:          # (fixed timestamps: the same bytes on every run)
        for k, arr in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, arr)
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print(out, {k: len(arr) for k, arr in arrays.items()}, out.stat().st_size, "+", out.with_suffix(".npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
