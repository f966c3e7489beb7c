"""CPU tests of the row quantiser's launch planner (csrc/mi355q_quant_plan.h) through the diagnostic hooks
mi355q_debug_quant_rows_plan / _builds: every row of the route table in tests/golden/quant_rows_plan.json / .npz -- recorded from the
launcher bodies of the commit before the planner existed (the fixture's header says how) -- gives the same plan; the builds the
launchers can look up are exactly the builds that table reaches; the switches tests set in-process are read per launch; and the calls
of tests/test_gpu_row_quantiser_edges.py reach the builds that file claims."""
import ctypes as C
import json
from pathlib import Path

import pytest

from tests import row_edges_util as U

GOLDEN = Path(__file__).resolve().parent / "golden" / "quant_rows_plan.json"
INT8, MX, CLASSES = 0, 1, 2
PRE_RELU = 1


@pytest.fixture(scope="module")
def table():
    import numpy as np
    doc = json.loads(GOLDEN.read_text())
    doc["rows"] = np.load(GOLDEN.with_suffix(".npz"))["rows"].tolist()
    return doc


@pytest.fixture(scope="module")
def dispatch_builds():
    """(kind, maxit, full, seg, mx, pre, st16, wps) of every entry of the launchers' lookup tables"""
    from mi355q import _lib
    fn = C.CDLL(str(_lib.library_path())).mi355q_debug_quant_rows_builds
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_int32), C.c_int32]
    n = fn(None, 0)
    out = (C.c_int32 * (8 * n))()
    assert fn(out, n) == n
    return [tuple(out[8 * i:8 * i + 8]) for i in range(n)]


def test_every_recorded_route_is_planned_the_same(table):
    assert table["row_fields"] == ["env"] + table["shape_fields"] + table["plan_fields"] and len(table["rows"]) > 40000
    assert table["plan_fields"] == ["maxit", "full", "seg", "mx", "pre", "st16", "wps", "grid", "rc"]
    wrong = [(table["envs"][r[0]], r[1:6], r[6:], got) for r in table["rows"] for got in [U.rows_plan(*r[1:6], env=table["envs"][r[0]])] if got != r[6:]]
    assert not wrong, f"{len(wrong)} of {len(table['rows'])} rows differ; first (env, shape, recorded, planned): {wrong[0]}"


def test_the_table_covers_what_it_is_meant_to(table):
    rows = table["rows"]
    assert {r[1] for r in rows} == {INT8, MX, CLASSES} and {r[4] for r in rows} == {0, 1, 2, 3, 4} and {r[5] for r in rows} == {0, 1}
    assert {r[3] for r in rows} >= {64, 320, 1024, 1088, 2048, 2112, 4096, 4160, 5120, 8192, 8256, 11008, 12288, 12352, 16384, 16448}
    assert {r[2] for r in rows} >= {1, 7, 128, 1024, 1025, 1536, 1537, 4096, 65536, 70000}
    edge = {(r[2] * r[3] >= 2 ** 30, r[14]) for r in rows if r[1] == CLASSES and r[3] == 4096 and abs(r[2] * r[3] - 2 ** 30) <= 4096}
    assert edge == {(False, 0), (True, -2)}
    envs = table["envs"]
    for env in ([{}] + [{"MI355Q_QROWS_GRID": g} for g in "0 7 512 2000".split()] + [{"MI355Q_QROWS_VARIANT": v} for v in "01"] + [{"MI355Q_QROWS_SHORT": "0"}]
                + [{"MI355Q_QROWS_GRID": "7", "MI355Q_QROWS_VARIANT": "0"}, {"MI355Q_QROWS_SHORT": "0", "MI355Q_QROWS_VARIANT": "0"}]):
        assert env in envs
    assert {r[0] for r in rows} == set(range(len(envs)))


def test_the_dispatch_tables_hold_the_reachable_builds_and_no_other(table, dispatch_builds):
    assert table["build_fields"] == ["kind", "maxit", "full", "seg", "mx", "pre", "st16", "wps"]
    assert len(set(dispatch_builds)) == len(dispatch_builds), "an instantiation is named once"
    planned = {(r[1], *U.rows_plan(*r[1:6], env=table["envs"][r[0]])[:7]) for r in table["rows"] if r[14] == 0}
    assert planned == {tuple(b) for b in table["builds"]} == set(dispatch_builds)
    # the instantiations the launcher ladders compiled and no launch could reach: the segmented builds (any pre-op) and round 5's build
    # at one, two and twelve slabs a lane
    removed = {(INT8, maxit, 0, 1, 0, pre, 0, 1) for maxit in (1, 2, 12) for pre in (0, 2, 3, 4)} | {(INT8, maxit, 0, 0, 0, 1, 0, 1) for maxit in (1, 2, 12)}
    assert len(removed) == 15 and not removed & planned and not removed & set(dispatch_builds)


def test_grid_and_variant_are_read_on_every_call(monkeypatch):
    for name in ("MI355Q_QROWS_GRID", "MI355Q_QROWS_VARIANT"):
        monkeypatch.delenv(name, raising=False)
    shape = (INT8, 4096, 4096)
    default = U.rows_plan(*shape)
    assert default == [4, 1, 0, 0, 0, 1, 1, 1536, 0]
    for env, plan in (({"MI355Q_QROWS_GRID": "7"}, [4, 1, 0, 0, 0, 1, 1, 7, 0]), ({"MI355Q_QROWS_VARIANT": "0"}, [4, 1, 0, 0, 1, 0, 1, 1024, 0]),
                      ({"MI355Q_QROWS_GRID": "7", "MI355Q_QROWS_VARIANT": "0"}, [4, 1, 0, 0, 1, 0, 1, 7, 0])):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            assert U.rows_plan(*shape) == plan == U.rows_plan(*shape, env=env), env
    assert U.rows_plan(*shape) == default


# ---- the calls of tests/test_gpu_row_quantiser_edges.py: (K, pre-op, segmented, kind, env) -----------------------------------------
def _params(test, name):
    """the values a GPU edge test is parametrised with for `name`"""
    return next(list(m.args[1]) for m in test.pytestmark if m.name == "parametrize" and m.args[0] == name)


def edge_calls():
    from tests import test_gpu_row_quantiser_edges as G
    grid7, round5 = {"MI355Q_QROWS_GRID": "7"}, {"MI355Q_QROWS_VARIANT": "0"}
    calls = [(K, 0, 0, INT8, {}) for K in _params(G.test_elements_in_every_build, "K")]
    calls += [(K, 0, 0, INT8, grid7) for K, _ in _params(G.test_elements_when_a_workgroup_walks_many_rows, "K,rows")]
    calls += [(K, 0, 0, INT8, round5) for K in _params(G.test_elements_in_the_round5_build, "K")]
    calls += [(K, 0, 0, INT8, {}) for K in _params(G.test_elements_beside_blocks_below_2_pow_minus_23, "K")]
    calls += [(U.clamp_layout().shape[1], 0, 0, INT8, {}), (U.OVERFLOW_K, 0, 0, INT8, {})]
    calls += [(K, 0, 0, INT8, {}) for K in _params(G.test_aligned_operand_denotes_the_oracle_values, "K")]
    calls += [(K, 0, 0, INT8, {}) for K in _params(G.test_product_with_identity_returns_the_oracle_values, "K")]
    calls += [(2048, 0, 0, INT8, {}), (2048, 0, 1, INT8, {})]                                  # test_segmented_rows
    calls += [(K, PRE_RELU, 0, INT8, {}) for K in _params(G.test_relu_in_front, "K")]
    calls += [(1024, 0, 0, CLASSES, {})]                                                       # test_column_classes
    calls += [(K, 0, 0, MX, {}) for K in _params(G.test_mx_operand, "K")]
    return calls


# reachable builds that no call of the GPU edge tests runs: (kind, MAXIT, FULL, SEG, MX, PRE, ST16, WPS)
NOT_RUN_BY_THE_EDGE_SET = sorted(
    # behind a pre-op: relu (PRE 4) runs at K = 1024 and 4096 only, LlamaRMSNorm (2) and LayerNorm (3) nowhere
    [(INT8, 2, 0, 0, 0, 4, 0, 1), (INT8, 4, 0, 0, 0, 4, 0, 1), (INT8, 8, 0, 0, 0, 4, 0, 1), (INT8, 8, 1, 0, 0, 4, 1, 1), (INT8, 12, 0, 0, 0, 4, 0, 1),
     (INT8, 16, 0, 0, 0, 4, 0, 1), (INT8, 16, 1, 0, 0, 4, 1, 1)]
    + [(INT8, 1, 0, 0, 0, 2, 0, 1), (INT8, 2, 0, 0, 0, 2, 0, 1), (INT8, 4, 0, 0, 0, 2, 0, 1), (INT8, 4, 1, 0, 0, 2, 1, 1), (INT8, 8, 0, 0, 0, 2, 0, 1),
       (INT8, 8, 1, 0, 0, 2, 1, 1), (INT8, 12, 0, 0, 0, 2, 0, 1), (INT8, 16, 0, 0, 0, 2, 0, 1), (INT8, 16, 1, 0, 0, 2, 1, 1)]
    + [(INT8, 1, 0, 0, 0, 3, 0, 1), (INT8, 2, 0, 0, 0, 3, 0, 1), (INT8, 4, 0, 0, 0, 3, 0, 1), (INT8, 4, 1, 0, 0, 3, 1, 1), (INT8, 8, 0, 0, 0, 3, 0, 1),
       (INT8, 8, 1, 0, 0, 3, 1, 1), (INT8, 12, 0, 0, 0, 3, 0, 1), (INT8, 16, 0, 0, 0, 3, 0, 1), (INT8, 16, 1, 0, 0, 3, 1, 1)]
    # segmented rows: K = 2048 without a pre-op only
    + [(INT8, 4, 0, 1, 0, 2, 0, 1), (INT8, 4, 0, 1, 0, 3, 0, 1), (INT8, 4, 0, 1, 0, 4, 0, 1)]
    + [(INT8, maxit, 0, 1, 0, pre, 0, 1) for maxit in (8, 16) for pre in (0, 2, 3, 4)]
    # round 5's build beyond four slabs
    + [(INT8, 8, 0, 0, 0, 1, 0, 1), (INT8, 8, 1, 0, 0, 1, 0, 1), (INT8, 16, 0, 0, 0, 1, 0, 1), (INT8, 16, 1, 0, 0, 1, 0, 1)]
    # MX rows of other widths than MX_ROWS; the class-aware kernel beyond K = 1024
    + [(MX, 2, 0, 0, 1, 0, 0, 1), (MX, 4, 0, 0, 1, 0, 0, 1), (MX, 8, 0, 0, 1, 0, 0, 1), (MX, 8, 1, 0, 1, 0, 0, 1), (MX, 16, 0, 0, 1, 0, 0, 1), (MX, 16, 1, 0, 1, 0, 0, 1)]
    + [(CLASSES, 4, 1, 0, 0, 0, 0, 1), (CLASSES, 8, 0, 0, 0, 0, 0, 1), (CLASSES, 16, 0, 0, 0, 0, 0, 1)])


def test_the_edge_set_runs_the_builds_it_claims(dispatch_builds):
    lean = lambda maxit, full: (INT8, maxit, full, 0, 0, 0, full, 1)                 # plain rows: no pre-op code, 16-byte stores where FULL
    # what ELEMENT_SHORT_K and ELEMENT_LONG_K are there for, K by K
    assert [U.planned_build(K) for K in U.ELEMENT_SHORT_K] == [lean(1, 0)] * 3
    assert [U.planned_build(K) for K in U.ELEMENT_LONG_K] == [lean(2, 0), lean(2, 0), lean(4, 0), lean(4, 1), lean(8, 0), lean(8, 1), lean(12, 0),
                                                               lean(16, 0), lean(16, 1)]
    run = {U.planned_build(*call) for call in edge_calls()}
    assert run >= {lean(m, f) for m, f in ((1, 0), (2, 0), (4, 0), (4, 1), (8, 0), (8, 1), (12, 0), (16, 0), (16, 1))}
    assert run >= {(INT8, 4, 0, 0, 0, 1, 0, 1), (INT8, 4, 1, 0, 0, 1, 0, 1)}, "round 5's build, guarded and full"
    assert {U.planned_build(K, kind=MX) for K in U.MX_ROWS} == {(MX, 1, 0, 0, 1, 0, 0, 1), (MX, 4, 1, 0, 1, 0, 0, 1)} <= run
    assert {(INT8, 4, 0, 1, 0, 0, 0, 1), (INT8, 1, 0, 0, 0, 4, 0, 1), (INT8, 4, 1, 0, 0, 4, 1, 1), (CLASSES, 4, 0, 0, 0, 0, 0, 1)} <= run, "segmented, relu, classes"
    # the grid walk: seven workgroups over the layouts' rows
    assert U.rows_plan(INT8, U.GRID_WALK_ROWS, 64, env={"MI355Q_QROWS_GRID": "7"})[7] == 7
    assert U.rows_plan(INT8, U.ELEMENT_LONG_ROWS, 4096, env={"MI355Q_QROWS_GRID": "7"})[7] == 7
    assert run <= set(dispatch_builds)
    assert sorted(set(dispatch_builds) - run) == NOT_RUN_BY_THE_EDGE_SET
