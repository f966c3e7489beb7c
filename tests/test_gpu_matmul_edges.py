"""The fused quantisers of the values-matmul kernels (csrc/mi355q_matmul.hip) held to the reference's edge set, bit for bit, by an
exact read-back through the product: one operand is the edge set, the other a selector with one non-zero per column (or row), so
every output element is ONE exact product and shows the quantised value (tests/matmul_edges_util.py; what the inputs hold and that the
oracle is the reference on them: tests/test_matmul_edges_host.py).  Every comparison is an integer equality of fp32 words, a zero's
sign aside (the oracle does not pin it).  Elements 0 < |x| <= 1e-8 are expected as the kernels document them: rounded to bf16.

Template instantiations reached, from launch_qmatmul_fmt / launch_bfp_qmatmul (FMT = block_fp, block_minifloat: PLANES 1; block_log:
PLANES 3, y through bfp_quant_pack_t_kernel<FMT_RAW> and x through bl_block_stats_kernel / bl_zero_fill):

  default route (this process): bfp_quant_pack_t_kernel<FMT, LANE = true>, bfp_qmatmul_tile_kernel<STREAM, NTNS, FMT, PLANES, RW>
    K = 64, 128, 192 (Kp = 1, 2, 3)       <false, 1 / 2 / 3, FMT, PLANES, RW = 1> (block_fp, block_minifloat), RW = 2 (block_log)
    K = 208 x N = 208                     <true, 8, ...>: a last 64-step that is not whole (blocks behind K), two groups of 8 tiles
    K = 256 x N = 64 (four selectors)     <true, 4, ...>;  K = 320 x N = 64 (the clamped exponent_width 4 / bias 7 case): the same
    K = 256 x N = 128 (two selectors)     <true, 8, ...>
    y side: y [64, 464] (<false, 1>, eight 64-column chunks, the last not whole), y [208, 144] (<true, 8>, the k < K guard of
    kernel 1, two tile groups)
  MI355Q_MATMUL_TILE=0 (child): bfp_quant_pack_t_kernel<FMT, LANE = false>, bfp_qmatmul_kernel<RESIDENT, NT, false, FMT, PLANES>
    K = 64, 128, 192                      <true, 1 / 2 / 3>
    K = 208 x 208, K = 256 x 128          <false, 8> (block_log: <false, 4>, column chunks of 64)
    K = 256 x 64, K = 320 x 64            <false, 4>
  MI355Q_MATMUL_RW=2 (child)              bfp_qmatmul_tile_kernel<false, 1 / 2 / 3, block_fp / block_minifloat, 1, RW = 2>
  MI355Q_MATMUL_RW=1 (child)              bfp_qmatmul_tile_kernel<false, 1 / 2 / 3, block_log, 3, RW = 1>

NOT reached: the softmax forms (bfp_qmatmul_kernel<false, 4 / 8, SOFTMAX = true>, block_fp and block_minifloat).  They have no exact
read-back: the probabilities are formed in-kernel to ~1 ulp (exp_neg, div_fast), so a tie of the quantiser moves with the last bit of
its input.  They use quantise_xblk, the quantiser the MI355Q_MATMUL_TILE=0 child holds here.  Neither reached:
bfp_qmatmul_tile_kernel<..., CW = 4>, which no launch names."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import matmul_edges_util as U

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
CHILD_TIMEOUT = 240

_EXPECTED = {}


def expected(key, fmt, x, y):
    if key not in _EXPECTED:
        _EXPECTED[key] = U.expected_of(key, fmt, x, y)
    return _EXPECTED[key]


@pytest.fixture(scope="module")
def lib():
    import torch
    from mi355q import ops
    return ops, torch


def _check(lib, cases):
    failed = []
    for key, fmt, x, y in cases:
        got = U.run_case(*lib, fmt, x, y)
        try:
            U.same(got, expected(key, fmt, x, y), key)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, f"{len(failed)} of {len(cases)} products differ:\n" + "\n".join(failed[:6])


@pytest.mark.parametrize("B", U.BATCHES)
@pytest.mark.parametrize("kind", U.ORDERS)
@pytest.mark.parametrize("s", U.SETS_A, ids=U.set_id)
def test_x_side(lib, s, kind, B):
    """construction A: the edge set as x, every launch branch of the tile route, rows whole and cut into two batch entries"""
    name, fmt = s
    _check(lib, [(key, fmt, x, y) for key, x, y, K, N, sel in U.cases_a(name, fmt, kind, B)])


@pytest.mark.parametrize("B", U.BATCHES)
def test_x_side_clamped_exponents(lib, B):
    """exponent_width 4 / bias 7 on row_edges_util.clamp_layout(): blocks at both exponent clamps and in between"""
    _check(lib, [(key, U.CLAMP_FMT, x, y) for key, x, y, K, N, sel in U.cases_clamp(B)])


@pytest.mark.parametrize("kind", U.ORDERS)
@pytest.mark.parametrize("s", U.SETS_B, ids=U.set_id)
def test_y_side(lib, s, kind):
    """construction B: the edge set as y (kernel 1's quantiser), x = d I"""
    name, fmt = s
    _check(lib, [(key, fmt, x, y) for key, x, y, K, N in U.cases_b(name, fmt, kind)])


def test_block_log_zero_blocks(lib):
    """the statistics pass's fill in the output: planted and padding all-zero blocks, and a tensor of zeros (fill 1)"""
    cases = U.bl_extra_cases()
    _check(lib, [(key, fmt, x, y) for key, x, y, K, N, sel, fmt in cases])
    key, x, y, K, N, sel, fmt = cases[0]
    fill = expected(key, fmt, x, y)[0, 3, 16:32] / y[0, sel[16:32], np.arange(16, 32)]
    assert (fill == fill[0]).all() and 2.0 ** -125 <= fill[0] < 1, "the planted block does not show a fill other than 1's"


@pytest.mark.parametrize("s", [s for s in U.SETS_A if s[1][0] != "bl" and s[1] != U.bfp(2)], ids=U.set_id)
def test_representable_operand_comes_back_unchanged(lib, s):
    """blocks that are fixed points of the oracle's quantiser come back as they went in, times q (33 .. 1291 blocks of the set per
    format, tests/test_matmul_edges_host.py; block_fp width 2 has none: its only non-zero mantissa makes every maximum 2^(e - 1))"""
    name, fmt = s
    x, keep = U.fixed_point_case(name, fmt)
    assert keep > 0
    y, sel = U.selectors(64, 64)[0]
    got = U.run_case(*lib, fmt, x, y)
    q = U.single_q(y, fmt)
    U.same(got, (x.astype(np.float64) * np.float64(q)).astype(np.float32), f"fixed points of {U.set_id(s)}")


@pytest.mark.parametrize("s", [s for s in U.SETS_A if s[1][0] != "bl"], ids=U.set_id)
def test_batch_of_two_is_two_single_calls(lib, s):
    """B = 2 against its two entries run alone, bit for bit (block_log is left out: its fill is tensor-wide, so an entry alone is
    another input)"""
    name, fmt = s
    for key, x, y, K, N, sel in U.cases_a(name, fmt, "strided", 2):
        if K not in (128, 208):
            continue
        both = U.run_case(*lib, fmt, x, y)
        for b in range(2):
            one = U.run_case(*lib, fmt, x[b:b + 1], y[b:b + 1])
            assert np.array_equal(both[b].view(np.int32), one[0].view(np.int32)), (key, b)


# ---------------------------------------------------------------------------------------------------
# the latched routes: one child process each
# ---------------------------------------------------------------------------------------------------
ROUTES = {"tile0": (dict(MI355Q_MATMUL_TILE="0"), []),
          "rw2": (dict(MI355Q_MATMUL_RW="2"), ["--short-only", "--kinds", "bfp,bm"]),
          "rw1": (dict(MI355Q_MATMUL_RW="1"), ["--short-only", "--kinds", "bl"])}


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """{route: {key: output}}: three fresh interpreters, one after another, each under its own time limit; a child that ends by a
    signal or at its limit fails the fixture and no further child is started"""
    d = tmp_path_factory.mktemp("matmul_edges")
    out = {}
    for route, (env, args) in ROUTES.items():
        path = d / f"{route}.npz"
        e = {k: v for k, v in os.environ.items() if k not in ("MI355Q_MATMUL_TILE", "MI355Q_MATMUL_RW")}
        try:
            p = subprocess.run([sys.executable, str(ROOT / "tests" / "matmul_edges_child.py"), str(path), *args], cwd=ROOT, env=dict(e, **env),
                               capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.fail(f"child {route} did not end within {CHILD_TIMEOUT} s; no further child started")
        if p.returncode < 0:
            pytest.fail(f"child {route} ended by signal {-p.returncode}; no further child started\n{p.stderr[-2000:]}")
        assert p.returncode == 0, f"child {route}: exit {p.returncode}\n{p.stderr[-2000:]}"
        with np.load(path) as z:
            out[route] = {k: z[k] for k in z.files}
    return out


def _route_cases(route):
    args = ROUTES[route][1]
    kinds = tuple(args[args.index("--kinds") + 1].split(",")) if "--kinds" in args else ("bfp", "bm", "bl")
    return U.all_cases(short_only="--short-only" in args, kinds=kinds)


def _groups(route):
    """the sets a route's child runs"""
    cases = _route_cases(route)
    return sorted({key.split("/")[1] for key, *_ in cases})


@pytest.mark.parametrize("route,group", [(r, g) for r in ROUTES for g in _groups(r)])
def test_latched_route(children, route, group):
    """kernel 2 (all its non-softmax builds), the two-row-group tile builds of block_fp / block_minifloat and the one-row-group
    builds of block_log against the same expected values"""
    got = children[route]
    cases = [c for c in _route_cases(route) if c[0].split("/")[1] == group]
    assert cases and all(key in got for key, *_ in cases)
    failed = []
    for key, fmt, x, y in cases:
        try:
            U.same(got[key], expected(key, fmt, x, y), f"{route} {key}")
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, f"{len(failed)} of {len(cases)} products differ:\n" + "\n".join(failed[:6])


def test_kernel_2_and_kernel_3_agree(lib, children):
    """the two K permutations (mm_kperm, mm_kperm_lane) feed the same sums: kernel 2's outputs are kernel 3's, bit for bit"""
    got = children["tile0"]
    n = 0
    for key, fmt, x, y in U.all_cases():
        if "/sorted/" in key and "/B1/" in key or key.startswith(("B/", "A/bl-extra", "A/clamp")):
            here = U.run_case(*lib, fmt, x, y)
            assert np.array_equal(here.view(np.int32), got[key].view(np.int32)), key
            n += 1
    assert n >= 100
