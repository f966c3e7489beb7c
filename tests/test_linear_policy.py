"""CPU tests of the quantised Linear's route policy (quantized_modules/linear_policy.py): every row of tests/golden/linear_policy.json / .npz
-- the decisions of linear.py's own methods at the commit before the policy was split out, recorded by
tools/gen_linear_policy_golden.py (the fixture's header says from where) -- is decided the same; and the policy is pure: importing
and calling it leaves CUDA untouched."""
import json
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden" / "linear_policy.json"


@pytest.fixture(scope="module")
def table():
    return load_table()


def load_table():
    """header, grid and the vocabulary from the JSON; the rows -- indices into "values" -- from the .npz next to it"""
    import numpy as np
    doc, rows = json.loads(GOLDEN.read_text()), np.load(GOLDEN.with_suffix(".npz"))
    rows = {name: rows[name].tolist() for name in doc["grid"]}
    assert all([doc["values"][i] for i in sorted({r[-1] for r in rows[name]})] == doc["outcomes"][name] for name in rows)
    recorded = {name: [[doc["values"][i] for i in r] for r in rows[name]] for name in rows}
    return dict(doc, outcomes=recorded)


@pytest.fixture(scope="module")
def policy():
    from mi355q.quantize.quantized_modules import linear_policy
    return linear_policy


def _fill(f):
    return None if f is None else tuple(f)


def _align(P, K, N, M, align, w_fill, x_fill, answer):
    """what the layer does with the decision (`_choose_align_mode`): -> [x_cap, mixed asked, "rows"] from the starting value"""
    try:
        d = P.align_decision(K, N, M, align, _fill(w_fill), _fill(x_fill))
    except ValueError as e:
        return f"ValueError: {e}"
    cap = P.initial_x_cap(align) if d.x_cap is None else d.x_cap
    if d.try_mixed:
        after = d.x_cap_if_mixed if answer else d.x_cap_if_not
        cap = cap if after is None else after
    return [cap, int(d.try_mixed), "rows"]


def _decide(P, base):
    """section -> (recorded row without its outcome) -> what linear_policy answers"""
    def cfg(over):
        return dict(base, **over)

    def plan(over, arith, K, N, nd, rows_dim):
        got = P.int8_plan(cfg(over), arith, K, N, nd, rows_dim)
        return None if got is None else list(got)
    return dict(
        int8_plan=plan,
        exponent_bias=P.exponent_bias,
        initial_x_cap=P.initial_x_cap,
        align=lambda *row: _align(P, *row),
        mixed_gate=lambda over, K, align, sample: sample and P.mixed_config_ok(cfg(over), K, align),
        mixed_class1_blocks=P.mixed_class1_blocks,
        mixed_fits=lambda w, x: P.rows_fit(_fill(w)) and P.mixed_fits(_fill(w), _fill(x)),
        uses_bf16_route=lambda over, K, x_cap: P.uses_bf16_route(cfg(over), K, x_cap),
        residual_rides_the_int8_product=P.residual_rides_the_int8_product,
        small_m_takes=lambda over, K, numel: P.small_m_takes(cfg(over), K, numel),
        values_exact_in_bf16=lambda over, arith, K: P.values_exact_in_bf16(cfg(over), arith, K),
        qat_on_tile_gemm=lambda over, arith, K, N, M, exact: P.qat_on_tile_gemm(cfg(over), arith, K, N, M, exact),
        padded_block_fp_ok=lambda over, arith, K, N, nd, rows_dim: P.padded_block_fp_ok(cfg(over), arith, K, N, nd, rows_dim),
        mx_config_ok=lambda over, arith, is_ptq, bypass, K: P.mx_config_ok(cfg(over), arith, is_ptq, bypass, K),
        mx_takes=lambda over, M, N: P.mx_takes(cfg(over), M, N))


def test_every_recorded_decision_is_decided_the_same(table, policy):
    decide = _decide(policy, table["header"]["base_config"])
    assert set(decide) == set(table["outcomes"]) == set(table["grid"])
    total = 0
    for name, rows in table["outcomes"].items():
        assert len(rows) == table["grid"][name]["rows"] and all(len(r) == len(table["grid"][name]["fields"]) for r in rows)
        wrong = [(r, got) for r in rows for got in [decide[name](*r[:-1])] if got != r[-1] or type(got) is not type(r[-1])]
        assert not wrong, f"{name}: {len(wrong)} of {len(rows)} rows differ; first (recorded row, decided): {wrong[0]}"
        total += len(rows)
    assert total > 4000


def test_the_grid_crosses_the_thresholds_from_both_sides(table, policy):
    """every section records both answers (the plan: both None and a plan), and the row / block decision every kind of outcome"""
    from mi355q import ops
    for name, rows in table["outcomes"].items():
        if name not in ("exponent_bias", "initial_x_cap", "mixed_class1_blocks", "align"):
            assert {r[-1] is None or r[-1] is False for r in rows} == {True, False}, name
    align = table["outcomes"]["align"]
    assert {r[-1][0] for r in align if isinstance(r[-1], list)} == {ops.ROW_NO_ALIGN, ops.ROW_BUCKET_CAP, ops.ROW_BUCKET_CAP_MAX}
    assert {r[-1][1] for r in align if isinstance(r[-1], list)} == {0, 1} and any(isinstance(r[-1], str) for r in align)
    for N, tile_rows in ((4096, 128), (11008, 256)):                 # both tile heights, fits and does not fit on either side of 48 and 88
        assert ops.gemm_tile_rows(2048, N) == tile_rows
        f = 0.5 * 1.15 if tile_rows == 128 else 1.0
        seen = {(r[4][1] + int(r[5][1] * f + 0.999), r[-1][0]) for r in align
                if r[1] == N and r[3] == "auto" and r[0] == 4096 and r[5] is not None and r[5][0] == 0 and r[4][0] == 0 and r[4][1] <= 48 and not r[6]}
        fast, slow = ops.ROW_TILE_ENTRIES_FAST, ops.ROW_TILE_ENTRIES_SLOW - 8
        assert (fast, ops.ROW_BUCKET_CAP) in seen and (fast + 1, ops.ROW_BUCKET_CAP if tile_rows == 256 else ops.ROW_NO_ALIGN) in seen
        assert (slow, ops.ROW_BUCKET_CAP if tile_rows == 256 else ops.ROW_NO_ALIGN) in seen and (slow + 1, ops.ROW_NO_ALIGN) in seen
    sizes = {(r[1], r[0]): r[2] for r in table["outcomes"]["mixed_class1_blocks"]}
    assert sizes[(32, 8)] == 8 and sizes[(32, 9)] == 16 and sizes[(32, 17)] == 0 and sizes[(64, 32)] == 32 and sizes[(64, 33)] == 0
    assert sizes[(256, 128)] == 128 and sizes[(256, 129)] == 0 and sizes[(256, 1)] == 8 and sizes[(256, 0)] == 0


def test_the_policy_touches_no_device(table):
    """a fresh interpreter: import the policy, decide every recorded row, and CUDA is still not initialised"""
    import subprocess
    import sys
    code = ("import sys, json, torch; sys.path[:0] = [{tests!r}, {pkg!r}]; import test_linear_policy as T\n"
            "from mi355q.quantize.quantized_modules import linear_policy as P\n"
            "table = T.load_table(); T.test_every_recorded_decision_is_decided_the_same(table, P)\n"
            "assert not torch.cuda.is_initialized(); print('pure')").format(tests=str(Path(__file__).resolve().parent), pkg=str(Path(__file__).resolve().parents[1] / "llm-mixed-q_amd"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(Path(__file__).resolve().parents[1]))
    assert out.returncode == 0 and out.stdout.strip().endswith("pure"), out.stderr[-2000:]
