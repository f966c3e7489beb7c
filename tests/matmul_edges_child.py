"""Child process of tests/test_gpu_matmul_edges.py (a plain script, not collected by pytest): the product kernels latch
MI355Q_MATMUL_TILE and MI355Q_MATMUL_RW in function-local statics at their first launch, so a route other than the default needs an
interpreter of its own.  Runs the case list of tests/matmul_edges_util.py under the environment it was started with and writes every
output to one .npz, key by key; the parent compares them with the same expected values.

usage: matmul_edges_child.py OUT.npz [--short-only] [--kinds bfp,bm,bl]"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "llm-mixed-q_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--short-only", action="store_true")
    ap.add_argument("--kinds", default="bfp,bm,bl")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from mi355q import ops
    from tests import matmul_edges_util as U
    out = {}
    for key, fmt, x, y in U.all_cases(short_only=a.short_only, kinds=tuple(a.kinds.split(","))):
        out[key] = U.run_case(ops, torch, fmt, x, y)
    np.savez(a.out, **out)
    print(f"{len(out)} products")
    return 0


if __name__ == "__main__":
    sys.exit(main())
