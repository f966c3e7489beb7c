"""The full-tile unit of the 256 x 256 tile GEMM (csrc/mi355q_gemm_v9f.hip) against the general kernel and the oracle.

The unit must give the general kernel's BITS: same arithmetic, same order of summation.  The switch MI355Q_V9_FULL is read
once per process, so the cases (tests/full_tile_cases.py) run in two fresh child interpreters, one per setting, once for the
whole module, side by side, while the oracle's references are computed here (threads: numpy's integer products release
the interpreter lock); the tests only compare.  Shapes: one to four tiles; K = 256 is the shortest loop the 256 x 256 kernel
takes (four K-steps: no turn of the main loop, the last requests go out while the ring still fills), 384 one turn, 768 twelve
K-steps = one full rotation of the four A slots against the three B slots; K = 128 is two K-steps, which the planner keeps on
another kernel -- both children then run the same code, and the case only shows that the unit is not taken.  One tile has,
in turn, no exception entries, x entries only, w entries only, rows with several entries, more vectors than fit beside the
rings, and an overflowed bucket (the grid-uniform blockwise fallback).  Each with and without bias.

Bound against oracle.np_oracle.bfp_linear_int: 1e-5 of the output scale, the bound smoke() and the other tile GEMM tests hold
this product to."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

from tests import full_tile_cases as cases

pytestmark = pytest.mark.gpu

CFG6 = dict(name="block_fp", data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
            data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127,
            weight_block_size=[1, 16], bias_width=6, bias_exponent_width=8, bias_exponent_bias=127,
            bias_block_size=[16])
HERE = Path(__file__).resolve().parent


ALL = [(M, N, K, v) for M, N in cases.SHAPES for K in cases.KS for v in cases.VARIANTS]


def _start_child(tmp, switch):
    out = tmp / f"full_{switch}.npz"
    env = dict(os.environ, MI355Q_V9_FULL=switch, MI355Q_V8_TILE_ROWS="256")      # the 256 x 256 tile at these small shapes
    for name in ("MI355Q_V9", "MI355Q_V9_FIX", "MI355Q_V9_DBG", "MI355Q_V10", "MI355Q_V8_SPLITS", "MI355Q_V8_STAMPS", "MI355Q_V8_CLOCK"):
        env.pop(name, None)
    return out, subprocess.Popen([sys.executable, str(HERE / "full_tile_cases.py"), str(out)], env=env, stdout=subprocess.PIPE,
                                 stderr=subprocess.STDOUT, text=True)


def _references(case):
    from oracle import np_oracle as O
    x, w, b = cases.operands(*case)
    return O.bfp_linear_int(x, w, None, CFG6), O.bfp_linear_int(x, w, b, CFG6)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(what the full-tile child wrote, what the general-kernel child wrote, {case: (oracle without bias, with bias)})"""
    tmp = tmp_path_factory.mktemp("full_tile")
    children = [_start_child(tmp, "1"), _start_child(tmp, "0")]
    try:
        with ThreadPoolExecutor(12) as pool:
            refs = dict(zip(ALL, pool.map(_references, ALL)))
        loaded = []
        for out, proc in children:
            text, _ = proc.communicate(timeout=300)
            assert proc.returncode == 0, text[-4000:]
            loaded.append(np.load(out))
    finally:
        for _, proc in children:
            if proc.poll() is None:
                proc.kill()
    return loaded[0], loaded[1], refs


@pytest.mark.parametrize("M,N,K,variant", ALL, ids=[cases.case_id(*c) for c in ALL])
def test_full_tile_unit_gives_the_general_kernels_bits_and_the_oracles_values(runs, M, N, K, variant):
    full, general, refs = runs
    key = cases.case_id(M, N, K, variant)
    ovx, ovw, tx, tw, nx, nw, taken = (int(v) for v in full[key + "/info"])
    assert int(general[key + "/info"][6]) == 0, "MI355Q_V9_FULL=0 must keep every launch on the general kernel"
    assert np.array_equal(full[key + "/info"][:6], general[key + "/info"][:6])
    # the case is what it says it is
    if variant == "none":
        assert (nx, nw, ovx, ovw) == (0, 0, 0, 0)
    elif variant == "x_only":
        assert tx == nx == 3 and nw == 0 and not ovx
    elif variant == "w_only":
        assert tw == nw == 3 and nx == 0 and not ovw
    elif variant == "several_per_row":
        assert (tx, tw, ovx, ovw) == (4, 3, 0, 0)
    elif variant == "slow_vectors":
        assert tx + tw == 40 > cases.V9_FAST_MAX and not ovx and not ovw
    else:
        assert ovx != 0, "the bucket did not overflow"
    # ... and ran where it should: both launches (without, with bias) on the full-tile unit from four K-steps on
    assert taken == (2 if K >= 256 else 0), f"{taken} of 2 launches took the full-tile unit"
    ref0, ref1 = refs[(M, N, K, variant)]
    for tag, ref in (("y0", ref0), ("y1", ref1)):
        yf, yg = full[f"{key}/{tag}"], general[f"{key}/{tag}"]
        assert yf.shape == (M, N) and np.isfinite(yf).all()
        diff = int((yf.view(np.uint32) != yg.view(np.uint32)).sum())
        err = np.abs(yf - ref).max() / np.abs(ref).max()
        print(f"{key} {tag}: {diff} words differ from the general kernel, rel err to the oracle {err:.3e}")
        assert diff == 0, f"{diff} of {yf.size} words differ from the general kernel"
        assert err < 1e-5
