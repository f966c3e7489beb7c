"""Which C export every KV-cache call of mi355q.ops reaches, and with which arguments: one call of append, dequantised,
bfp_attention_decode and bfp_attention_extend for every legal combination of cache kind, uniform / ragged, group, window, token_major and
splits, through a recorder around the loaded library that forwards every call and notes (export name, integer and float arguments;
a pointer only as "null" / "ptr").  Every recorded call equals tests/golden/kv_routes.json, which this file wrote at the commit its
header names (MI355Q_KV_ROUTES_RECORD=<path> records instead of comparing).  Every output is finite and bit-equal on a second call."""
import ctypes as C
import json
import os
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden" / "kv_routes.json"
RECORD = os.environ.get("MI355Q_KV_ROUTES_RECORD")
DEV = "cuda:0"
B, D, CAP, LENGTHS, MAXLEN = 2, 32, 64, (5, 40), 40
P, MAX_PAGES, NUM_PAGES = 32, 2, 5
M_DECODE, M_EXTEND, WINDOW, SPLITS = 2, 3, 8, 2
PAR = (6, 8, 127, 6, 8, 127)
KINDS = [("KVCache", False), ("KVCache", True), ("PagedKVCache", True), ("PackedKVCache", False), ("PackedKVCache", True)]
_RECORDED = {}


class Recorder:
    """the loaded library with every call noted in `calls` while `on`"""

    def __init__(self, lib, signatures):
        self._lib, self._signatures, self.calls, self.on = lib, signatures, [], True

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        types = self._signatures[name][1]

        def call(*args):
            if self.on:
                assert len(args) == len(types), name
                self.calls.append([name, [("null" if not a else "ptr") if t is C.c_void_p else (float(a) if t is C.c_float else int(a))
                                          for a, t in zip(args, types)]])
            return fn(*args)
        return call

    def take(self):
        calls, self.calls = self.calls, []
        return calls


@pytest.fixture(scope="module")
def recorder():
    from mi355q import _lib
    lib = _lib.load_library()
    rec = _lib._LIB = Recorder(lib, _lib.SIGNATURES)
    yield rec
    _lib._LIB = lib
    if RECORD:
        header = {"commit": os.environ.get("MI355Q_KV_ROUTES_COMMIT", "unknown"),
                  "how": "MI355Q_KV_ROUTES_RECORD=<path> pytest -m gpu tests/test_gpu_kv_routes.py on an MI355X at that commit",
                  "call": "[export, arguments in the export's order; a pointer is \"null\" or \"ptr\"]"}
        kinds = ",\n".join(f"{json.dumps(name)}: {{\n" + ",\n".join(f"{json.dumps(case)}: {json.dumps(calls)}" for case, calls in cases.items()) + "\n}"
                           for name, cases in _RECORDED.items())
        Path(RECORD).parent.mkdir(parents=True, exist_ok=True)
        Path(RECORD).write_text(f"{{\"header\": {json.dumps(header)},\n\"cases\": {{\n{kinds}\n}}}}\n")


@pytest.fixture(scope="module")
def golden():
    return None if RECORD else json.loads(GOLDEN.read_text())["cases"]


def _i32(values):
    import torch
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


def _twice(rec, fn):
    """fn's output and the calls it made; the output is finite, and a second, unrecorded call gives its bits"""
    import torch
    first, calls = fn(), rec.take()
    rec.on = False
    second = fn()
    rec.on = True
    for a, b in zip(first, second) if isinstance(first, tuple) else [(first, second)]:
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    return calls


@pytest.mark.parametrize("kind,ragged", KINDS, ids=[f"{k}-{'ragged' if r else 'uniform'}" for k, r in KINDS])
def test_every_call_reaches_the_recorded_export_with_the_recorded_arguments(recorder, golden, kind, ragged):
    import torch
    from mi355q import ops
    gen = torch.Generator(device="cpu").manual_seed(7)
    k, v = (torch.randn(B, MAXLEN, D, generator=gen).to(DEV) for _ in range(2))
    cases, name = {}, f"{kind}-{'ragged' if ragged else 'uniform'}"
    recorder.take()
    if kind == "PagedKVCache":
        cache = ops.PagedKVCache(B, D, PAR, PAR, DEV, page_size=P, num_pages=NUM_PAGES, max_pages=MAX_PAGES)
        cache.ensure(LENGTHS)
    else:
        cache = getattr(ops, kind)(B, CAP, D, PAR, PAR, DEV)
    cases["construct"] = recorder.take()
    lengths = _i32(LENGTHS) if ragged else None
    rag = dict(lengths=lengths, max_length=MAXLEN) if ragged else {}
    if ragged:
        cache.append(k, v, lengths=_i32([0] * B), counts=lengths, max_length=0)
    else:
        cache.append(k, v)
    cases["append"] = recorder.take()
    cases["dequantised"] = _twice(recorder, lambda: cache.dequantised(**rag))
    for group in (1, 2):
        qd, qe = (torch.randn(1, B * group, m, D, generator=gen).to(DEV) for m in (M_DECODE, M_EXTEND))
        for window in ((None,) if kind == "PackedKVCache" else (None, WINDOW)):
            for tm in (False, True):
                for splits in (None, SPLITS):
                    cases[f"decode/g{group}-w{window}-tm{int(tm)}-s{splits}"] = _twice(recorder, lambda: ops.bfp_attention_decode(
                        qd, cache, scale_div=2.0, token_major=tm, splits=splits, group=group, window=window, **rag))
                if kind != "PackedKVCache":
                    cases[f"extend/g{group}-w{window}-tm{int(tm)}"] = _twice(recorder, lambda: ops.bfp_attention_extend(
                        qe, cache, scale_div=2.0, token_major=tm, group=group, window=window, **rag))
    assert all(len(c) >= 1 for c in cases.values())
    if RECORD:
        _RECORDED[name] = cases
        return
    assert set(cases) == set(golden[name])
    wrong = [(case, golden[name][case], got) for case, got in cases.items() if got != golden[name][case]]
    assert not wrong, f"{len(wrong)} of {len(cases)} calls of {name} differ; first (case, recorded, made): {wrong[0]}"
