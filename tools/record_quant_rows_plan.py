#!/usr/bin/env python3
"""Records tests/golden/quant_rows_plan.json / .npz: which build of the row quantiser a launch takes and on how many workgroups,
for a grid of shapes and environment sets -- from the LAUNCHER BODIES of a commit that still has them (the commit before
csrc/mi355q_quant_plan.h existed), not from the planner.  tests/test_quant_rows_plan.py holds the planner to the table.

Method: the host bodies of launch_quant_align_rows, launch_quant_mx_rows (csrc/mi355q_quant.hip) and launch_quant_classes
(csrc/mi355q_quant_cls.hip) are cut verbatim out of `git show <commit>:...` and compiled into a host-only program in which
hipLaunchKernelGGL is a stub that notes the kernel as spelled -- name and template arguments -- and the grid; one fresh process per
environment set, the environment in place before it starts, so that the latched read of MI355Q_QROWS_SHORT sees it.  Template
arguments a launch line leaves out are filled in from the kernel's declaration in the same commit.  No GPU, no library.

    python tools/record_quant_rows_plan.py --commit <the commit to record>
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "quant_rows_plan.json"
CSRC = "llm-mixed-q_amd/csrc/"

KINDS = ("int8", "mx", "classes")
COLS = (64, 320, 1024, 1088, 2048, 2112, 4096, 4160, 5120, 8192, 8256, 11008, 12288, 12352, 16384, 16448)
ROWS = (1, 7, 128, 1024, 1025, 1536, 1537, 4096, 65536, 70000)
CLASS_EDGE = ((262143, 4096), (262144, 4096), (131071, 8192), (131072, 8192))        # either side of rows * cols = 2^30
PRE_OPS = (0, 1, 2, 3, 4)
ENVS = [{}, {"MI355Q_QROWS_GRID": "0"}, {"MI355Q_QROWS_GRID": "7"}, {"MI355Q_QROWS_GRID": "512"}, {"MI355Q_QROWS_GRID": "2000"}, {"MI355Q_QROWS_GRID": "100000"},
        {"MI355Q_QROWS_VARIANT": "0"}, {"MI355Q_QROWS_VARIANT": "1"}, {"MI355Q_QROWS_SHORT": "0"},
        {"MI355Q_QROWS_GRID": "7", "MI355Q_QROWS_VARIANT": "0"}, {"MI355Q_QROWS_SHORT": "0", "MI355Q_QROWS_VARIANT": "0"}]
SHAPE_FIELDS = ["kind", "rows", "cols", "pre_op", "segmented"]
PLAN_FIELDS = ["maxit", "full", "seg", "mx", "pre", "st16", "wps", "grid", "rc"]

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "mi355q.h"
typedef void* hipStream_t;
struct QuantArgs { long long rows, cols, seg_len; int pre_op; };
struct MxOut { uint8_t *c16, *c8, *sc; int *bad, *bad_clear; };
static const char* kernel;
static unsigned grid_launched;
#define hipLaunchKernelGGL(k, g, ...) (kernel = #k, grid_launched = (g))
static int hipGetLastError() { return 0; }
%s
int main() {
    long long kind, rows, cols, pre_op, segmented;
    while (scanf("%%lld %%lld %%lld %%lld %%lld", &kind, &rows, &cols, &pre_op, &segmented) == 5) {
        const QuantArgs a{rows, cols, segmented ? 64 : 0, (int)pre_op};
        kernel = "";
        grid_launched = 0;
        const int rc = kind == 0   ? launch_quant_align_rows(a, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0)
                       : kind == 1 ? launch_quant_mx_rows(a, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)
                                   : launch_quant_classes(a, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0);
        printf("%%s|%%u|%%d\n", kernel, grid_launched, rc);
    }
    return 0;
}
"""


def show(commit, path):
    return subprocess.run(["git", "-C", str(ROOT), "show", f"{commit}:{path}"], capture_output=True, text=True, check=True).stdout


def body(source, name):
    """the definition of function `name`, from its first line to the closing brace in column 0"""
    start = re.search(rf"^int {name}\(", source, re.M).start()
    return source[start:source.index("\n}\n", start) + 3]


def defaults(source, kernel):
    """the kernel's template parameters as declared: [(name, default or None)]"""
    decl = re.search(rf"template <([^>]*)>\s*__global__[^\n]*\b{kernel}\(", source).group(1)
    return [(p.split("=")[0].split()[-1], p.split("=")[1].strip() if "=" in p else None) for p in decl.split(",")]


def shapes():
    out = [(k, r, c, p, s) for k in range(3) for c in COLS for r in ROWS for p in PRE_OPS for s in (0, 1)]
    return out + [(2, r, c, 0, 0) for r, c in CLASS_EDGE]


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="a commit whose launchers still hold their own ladders")
    opt = ap.parse_args()
    commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", opt.commit], capture_output=True, text=True, check=True).stdout.strip()
    quant, cls = show(commit, CSRC + "mi355q_quant.hip"), show(commit, CSRC + "mi355q_quant_cls.hip")
    bodies = [body(quant, "launch_quant_align_rows"), body(quant, "launch_quant_mx_rows"), body(cls, "launch_quant_classes")]
    params = {"bfp_quant_align_rows_kernel": defaults(quant, "bfp_quant_align_rows_kernel"),
              "bfp_quant_classes_kernel": defaults(cls, "bfp_quant_classes_kernel")}
    assert [n for n, _ in params["bfp_quant_align_rows_kernel"]] == ["MAXIT", "FULL", "SEG", "MX", "PRE", "ST16", "WPS"]
    assert [n for n, _ in params["bfp_quant_classes_kernel"]] == ["MAXIT", "FULL", "WPS"]

    def plan_words(line):
        spelled, grid, rc = line.split("|")
        if int(rc):
            assert not spelled
            return [0] * 8 + [int(rc)]
        name, args = re.fullmatch(r"\((\w+)<(.*)>\)", spelled).groups()
        args = [a.strip() for a in args.split(",")]
        args += [d for _, d in params[name][len(args):]]
        t = {n: int({"true": 1, "false": 0}.get(a, a)) for (n, _), a in zip(params[name], args)}
        return [t["MAXIT"], t["FULL"], t.get("SEG", 0), t.get("MX", 0), t.get("PRE", 0), t.get("ST16", 0), t["WPS"], int(grid), 0]

    sh = shapes()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        (tmp / "mi355q.h").write_text(show(commit, "include/mi355q.h"))
        (tmp / "rows.cpp").write_text(PROGRAM % "\n".join(bodies))
        subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-w", "-I", str(tmp), str(tmp / "rows.cpp"), "-o", str(tmp / "rows")], check=True)
        clean = {k: v for k, v in os.environ.items() if not k.startswith("MI355Q_QROWS")}
        for e, env in enumerate(ENVS):
            out = subprocess.run([str(tmp / "rows")], input="".join("%d %d %d %d %d\n" % s for s in sh), env=dict(clean, **env),
                                 capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
            assert len(out) == len(sh)
            rows += [[e, *s, *plan_words(line)] for s, line in zip(sh, out)]
    builds = sorted({(r[1], *r[6:13]) for r in rows if r[-1] == 0})
    doc = {"header": {"parent": commit,
                      "method": "Recorded from the parent commit, not from the planner (tools/record_quant_rows_plan.py): the host bodies of "
                                "launch_quant_align_rows, launch_quant_mx_rows and launch_quant_classes copied verbatim into a host-only program, with "
                                "hipLaunchKernelGGL replaced by a stub that notes the kernel as spelled and the grid; template arguments a launch "
                                "line leaves out filled in from the kernel's declaration; one fresh process per environment set, the environment "
                                "in place before start, so that the latched read of MI355Q_QROWS_SHORT sees it.  rc != 0: nothing was launched, "
                                "every other plan word 0.",
                      "rows": f"quant_rows_plan.npz, array `rows`: int32 [{len(rows)}, {len(rows[0])}], columns as `row_fields`; env = index into `envs`"},
           "kinds": KINDS, "shape_fields": SHAPE_FIELDS, "plan_fields": PLAN_FIELDS, "row_fields": ["env"] + SHAPE_FIELDS + PLAN_FIELDS,
           "build_fields": ["kind"] + PLAN_FIELDS[:7], "envs": ENVS, "builds": builds}
    GOLDEN.write_text("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in doc.items()) + "\n}\n")      # (a key a line)
    np.savez_compressed(GOLDEN.with_suffix(".npz"), rows=np.asarray(rows, dtype=np.int32))
    print(f"{len(rows)} rows, {len(ENVS)} environment sets, {len(builds)} builds -> {GOLDEN}")


if __name__ == "__main__":
    sys.exit(main())
