"""Shared by the attention-sink tests (tests/test_sink_host.py, tests/test_gpu_sink.py): the oracle of tests/window_util.py with the sink
columns unmasked -- np_oracle.matmul_quantized on the full K / V, fp64 softmax under the causal + window additive mask whose lower part
is lifted for keys 0 .. S - 1 -- the same mask written out by loops, and the table of one small case per compiled sink kernel form."""
import sys
from dataclasses import dataclass
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from window_util import FMIN, cfg  # noqa: E402,F401


def visible(p, key, window, sinks):
    """the semantics, word for word: the query at absolute position p sees keys {0 .. min(S, p + 1) - 1} u {max(0, p - W + 1) .. p}"""
    return key < min(sinks, p + 1) or max(0, p - window + 1) <= key <= p


def loop_mask(tq, tk, window, sinks):
    """[tq, tk] additive mask of the last tq of tk positions, by loops: 0 where visible, finfo.min elsewhere"""
    m = np.zeros((tq, tk), np.float32)
    for i in range(tq):
        for key in range(tk):
            if not visible(tk - tq + i, key, window, sinks):
                m[i, key] = FMIN
    return m


def oracle(q, k, v, width, window, scale_div, sinks):
    """window_util.oracle with the sink columns unmasked: the last tq positions of tk keys, causal, every query bound to its last
    `window` keys and the first `sinks`"""
    from oracle import np_oracle as O
    w = O.matmul_quantized(q, np.swapaxes(k, -1, -2), cfg(width))
    w = (w / np.float32(scale_div)).astype(np.float32)
    tq, tk = w.shape[-2:]
    m = np.triu(np.full((tq, tk), FMIN, np.float32), 1 + tk - tq)
    below = np.tril(np.full((tq, tk), FMIN, np.float32), tk - tq - window)
    below[:, :sinks] = 0
    m = m + below
    with np.errstate(over="ignore"):
        w = np.maximum(w + m, FMIN)
    e = np.exp((w - w.max(-1, keepdims=True)).astype(np.float64))
    p = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    return O.matmul_quantized(p, v, cfg(width))


# ---- one case per compiled form: <DC, GQ, PG> of decode_scores_sink_kernel / decode_pv_sink_kernel and of bfp_attention_extend_sink_kernel
# Three cache rows: 80 keys (decode: lo = 56, p0 = 1, lo in the pair's second tile; extend: the second query block has st0 = 1 and
# need = 5), 18 keys (the sinks inside the window's first pair) and an empty row.  W = 20, S = 4, P = 32.
WINDOW, SINKS, PAGE = 20, 4, 32
LENGTHS = (80, 18, 0)


@dataclass(frozen=True)
class Case:
    kind: str           # "decode" / "extend"
    form: tuple         # (DC, GQ, PG)
    M: int              # decode: queries a row; extend: the host's M
    counts: tuple       # extend: m_b per cache row; decode: None

    @property
    def D(self):
        return 32 * self.form[0]

    @property
    def group(self):
        return 2 if self.form[1] else 1

    @property
    def paged(self):
        return self.form[2]

    @property
    def id(self):
        return "%s_sink<%s>" % (self.kind, ",".join(str(x).lower() for x in self.form))

    def queries(self, b):
        if self.kind == "decode":
            return self.M if LENGTHS[b] >= self.M else 0
        return self.counts[b] if 0 < self.counts[b] <= LENGTHS[b] else 0


CASES = [Case(kind, (dc, gq, pg), 5 if kind == "decode" else 70, None if kind == "decode" else (70, 10, 0))
         for kind in ("decode", "extend") for dc in (1, 2, 3, 4) for gq in (False, True) for pg in (False, True)]


def forms(kind):
    return {c.form for c in CASES if c.kind == kind}


def p0_of(L, M, W):
    return max(L - M - W + 1, 0) // 32
