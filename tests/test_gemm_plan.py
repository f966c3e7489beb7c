"""CPU tests of the tile GEMM's launch planner (csrc/mi355q_gemm_plan.h) through the diagnostic hook
mi355q_debug_gemm_plan: every row of the route table in tests/golden/gemm_plan.json / .npz -- recorded from the launcher bodies
of the commit before the planner existed (the fixture's header says how) -- gives the same plan; every launch line that
was reachable there is still covered and the removed instantiations are not; the switches tests pin in-process are read
per launch."""
import ctypes as C
import json
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden" / "gemm_plan.json"
PINS = ("MI355Q_V10", "MI355Q_V10_NS", "MI355Q_V10_AUTO", "MI355Q_V10_KG", "MI355Q_V8_TILE_ROWS", "MI355Q_V8_SPLITS", "MI355Q_V9", "MI355Q_V9_FIX",
        "MI355Q_V9_DBG", "MI355Q_V8_CLOCK", "MI355Q_V8_STAMPS")


@pytest.fixture(scope="module")
def table():
    import numpy as np
    doc = json.loads(GOLDEN.read_text())
    doc["rows"] = np.load(GOLDEN.with_suffix(".npz"))["rows"].tolist()
    return doc


@pytest.fixture(scope="module")
def hook():
    from mi355q import _lib
    fn = C.CDLL(str(_lib.library_path())).mi355q_debug_gemm_plan
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32)]

    def plan(shape, env, workspace_ok):
        out = (C.c_int32 * 16)(*([-99] * 16))
        words = None if env is None else (C.c_int32 * 13)(*env)
        assert fn((C.c_int64 * 8)(*shape), words, workspace_ok, out) == 0
        assert out[14] == 0 and out[15] == 0
        return [out[i] & 0xFFFFFFFF if i == 12 else out[i] for i in range(14)]
    return plan


def env_words(env):
    """the 13 words of TileEnv for a set of environment strings (what read_tile_env() makes of them)"""
    def num(name, unset):
        return int(env[name]) if name in env else unset
    return [num("MI355Q_V10", 0), num("MI355Q_V10_NS", 0), num("MI355Q_V10_AUTO", 1), num("MI355Q_V10_KG", 1), num("MI355Q_V8_TILE_ROWS", 0),
            num("MI355Q_V8_SPLITS", 0), num("MI355Q_V9", 1), num("MI355Q_V9_FIX", 1), num("MI355Q_V9_DBG", 0), int("MI355Q_V8_SPLITS" in env),
            int("MI355Q_V8_CLOCK" in env), int("MI355Q_V8_STAMPS" in env), int("MI355Q_V8_TILE_ROWS" in env)]


def shape_of(row):
    bf16, M, N, K, ngroup, lists, flags, x_segs = row[1:9]
    return [M, N, K, ngroup, lists, flags, x_segs, bf16]


def outcome(row):
    return [row[1], row[10], row[11]] + row[14:20] + [int(row[20] > 1)]


def test_every_recorded_route_is_planned_the_same(table, hook):
    assert table["row_fields"][10:] == table["plan_fields"] and len(table["rows"]) > 1000
    words = [env_words(e) for e in table["envs"]]
    wrong = [(table["envs"][r[0]], r[1:10], r[10:], got) for r in table["rows"] for got in [hook(shape_of(r), words[r[0]], r[9])] if got != r[10:]]
    assert not wrong, f"{len(wrong)} of {len(table['rows'])} rows differ; first (env, shape + workspace_ok, recorded, planned): {wrong[0]}"


def test_a_split_plan_has_its_unsplit_twin(table):
    """workspace_ok = 0 is recorded for every row whose plan splits, and never splits"""
    rows = {(r[0], tuple(r[1:9]), r[9]): r for r in table["rows"]}
    split = [k for k, r in rows.items() if r[20] > 1]
    assert split and all(k[2] == 1 for k in split)
    for env, shape, _ in split:
        assert rows[(env, shape, 0)][20] == 1


def test_reachable_launch_lines_are_covered_and_the_removed_ones_are_not(table, hook):
    words = [env_words(e) for e in table["envs"]]
    planned = {tuple(outcome(r[:10] + hook(shape_of(r), words[r[0]], r[9]))) for r in table["rows"] if r[23] == 0}
    assert planned == {tuple(o) for o in table["outcomes"]}
    fields = table["outcome_fields"]
    assert fields == ["bf16", "family", "geom", "ti", "sched", "fixmode", "ns", "occ", "kg", "split"]
    v8 = {(o[0], o[5], o[3], o[4]) for o in table["outcomes"] if o[1] == 8}          # (bf16, FIXMODE, TI, SCHED)
    assert v8 == {(0, 1, 4, 2), (0, 0, 4, 2), (0, 1, 4, 1), (0, 0, 4, 1), (0, 3, 8, 2), (0, 1, 8, 2), (0, 2, 8, 2), (0, 0, 8, 2), (0, 0, 8, 0),
                  (1, 0, 4, 2), (1, 0, 4, 1), (1, 0, 8, 2), (1, 0, 8, 0)}
    assert not v8 & {(0, 3, 8, 0), (0, 1, 8, 0), (0, 2, 8, 0)}                      # bfp_gemm_v8<3, 8>, <1, 8>, <2, 8>: gone
    v10 = {(o[2], o[6], o[7], o[8]) for o in table["outcomes"] if o[1] == 10}        # (geometry, NS, OCC, KG)
    for bf16 in (0, 1):
        assert {(o[2], o[6], o[7], o[8]) for o in table["outcomes"] if o[1] == 10 and o[0] == bf16} == v10
    assert v10 == {(1, 6, 1, 1), (1, 4, 1, 1), (1, 3, 2, 1), (2, 4, 1, 1), (2, 3, 2, 1), (3, 8, 1, 1), (3, 6, 1, 1), (3, 4, 2, 1), (4, 6, 1, 1), (4, 4, 2, 1),
                   (5, 4, 1, 2), (6, 3, 1, 2)}
    assert {o[0] for o in table["outcomes"] if o[1] == 9} == {0, 1}
    assert any(o[1] == 9 and o[9] for o in table["outcomes"]) and any(o[1] == 8 and o[9] for o in table["outcomes"]) and any(o[1] == 10 and o[9] for o in table["outcomes"])


def test_the_process_environment_is_read_on_every_call(table, hook, monkeypatch):
    for name in PINS:
        monkeypatch.delenv(name, raising=False)
    int8, bf16 = [4096, 512, 4096, 0, 1, 1, 1, 0], [2048, 2048, 16384, 0, 0, 0, 1, 1]
    for shape in (int8, bf16):
        assert hook(shape, None, 1) == hook(shape, env_words({}), 1)
    # one switch after the other in one process, each against the same setting passed explicitly -- and every setting moves the plan
    default = [hook(shape, None, 1) for shape in (int8, bf16)]
    for env in ({"MI355Q_V10": "3"}, {"MI355Q_V10": "1", "MI355Q_V10_NS": "6"}, {"MI355Q_V10": "3", "MI355Q_V10_NS": "8"},
                {"MI355Q_V10": "3", "MI355Q_V8_SPLITS": "2"}, {"MI355Q_V10": "3", "MI355Q_V8_SPLITS": "4"}, {"MI355Q_V8_SPLITS": "4"}, {"MI355Q_V8_SPLITS": "2"},
                {"MI355Q_V8_SPLITS": "0"}, {"MI355Q_V8_TILE_ROWS": "128"}, {"MI355Q_V8_TILE_ROWS": "256"}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            got = [hook(shape, None, 1) for shape in (int8, bf16)]
        assert got == [hook(shape, env_words(env), 1) for shape in (int8, bf16)], env
        assert got[0] != default[0] and got[1] != default[1], env
    assert [hook(shape, None, 1) for shape in (int8, bf16)] == default
