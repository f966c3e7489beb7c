"""Shared by tests/test_attention_bm_host.py and tests/test_gpu_attention_bm.py: block_minifloat configs, the oracle of the one-pass
block_minifloat attention (ops.bm_attention) and the case table.

Oracle: the reference's steps on oracle.np_oracle -- matmul_quantized with the block_minifloat configs, an fp64 softmax -- the recipe of
tests/test_gpu_kvbm_decode.py::_oracle / _reference, restated here (with a config a product, so the two products and the two sides of a
product may differ).

Inputs.  With bias 0 every probability below 1 is a subnormal step of 2^(1 - mantissa bits): flat inputs give an oracle output that is
exactly 0 in every row, on which any kernel passes.  The queries are that file's peaked ones (factor 3.0).  Asserted on the oracle's own
values before any GPU comparison (reference()): at least 75 % of the rows are non-zero in the oracle's output (every row sees a key),
and a row may be left out only if the oracle ITSELF moves by more than 1e-6 max|ref| when its probabilities are scaled by 1 +- 2^-20
(a probability on a quantiser boundary) -- at most 2 % of all rows.  The seeds of CASES were picked on a CPU for both to hold.
Bounds on the rows kept, the project's own for this arithmetic: worst <= 1e-3 max|ref|, mean <= 3e-5 max|ref|."""
import math
from functools import lru_cache

import numpy as np

FMIN = np.finfo(np.float32).min
F848, F634, F423, F735 = (8, 4, 8), (6, 3, 4), (4, 2, 3), (7, 3, 5)       # (width, exponent_width, exponent_bias_width)


def cfg(x_fmt, y_fmt=None, **knobs):
    """the config of one product: data_in (x side) in x_fmt, weight (y side) in y_fmt (default: x_fmt)"""
    y_fmt = y_fmt or x_fmt
    return dict(name="block_minifloat", is_ptq=True, bypass=False, data_in_width=x_fmt[0], data_in_exponent_width=x_fmt[1],
                data_in_exponent_bias_width=x_fmt[2], data_in_block_size=[1, 16], weight_width=y_fmt[0], weight_exponent_width=y_fmt[1],
                weight_exponent_bias_width=y_fmt[2], weight_block_size=[1, 16], **knobs)


def par(x_fmt, y_fmt=None):
    return tuple(x_fmt) + tuple(y_fmt or x_fmt)


def oracle(q, k, v, c0, c1, causal=False, scale_div=None, p_scale=None):
    from oracle import np_oracle as O
    w = O.matmul_quantized(q, np.swapaxes(k, -1, -2), c0)
    if scale_div:
        w = (w / np.float32(scale_div)).astype(np.float32)
    tq, tk = w.shape[-2:]
    if causal:
        m = np.triu(np.full((tq, tk), FMIN, np.float32), 1 + tk - tq)
        with np.errstate(over="ignore"):
            w = np.maximum(w + m, FMIN)
    e = np.exp((w - w.max(-1, keepdims=True)).astype(np.float64))
    p = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    if p_scale is not None:
        p = (p * np.float32(p_scale)).astype(np.float32)
    return O.matmul_quantized(p, v, c1)


def inputs(B, M, T, hd, seed):
    r = np.random.default_rng(seed)
    q = (r.normal(size=(B, M, hd)) * np.exp(r.normal(size=(B, M, 1)) * 0.5) * 3.0).astype(np.float32)
    k = (r.normal(size=(B, T, hd)) * np.exp(r.normal(size=(B, 1, hd)) * 0.5)).astype(np.float32)
    v = r.normal(size=(B, T, hd)).astype(np.float32)
    return q, k, v


def conditions(ref, moved, count=True):
    """-> keep [rows]; the two conditions of the header, asserted when `count`"""
    scale = np.abs(ref).max()
    keep = np.ones(ref.shape[:-1], bool)
    for m in moved:
        keep &= np.abs(m - ref).max(-1) <= 1e-6 * scale
    nonzero = np.abs(ref).max(-1) > 0
    print("rows", keep.size, "left out", int((~keep).sum()), "non-zero", int(nonzero.sum()))
    if count:
        assert nonzero.mean() >= 0.75, f"only {nonzero.mean():.0%} of the oracle's rows are non-zero: the inputs are not peaked enough"
        assert (~keep).mean() <= 0.02, f"{int((~keep).sum())} of {keep.size} rows sit on a quantiser boundary of the oracle"
    return keep


def reference_of(q, k, v, c0, c1, causal, scale_div, count=True):
    """-> (ref, keep) for given inputs: the oracle's output and the rows it does not itself move under a 2^-20 scaling of its probabilities"""
    ref = oracle(q, k, v, c0, c1, causal=causal, scale_div=scale_div)
    moved = [oracle(q, k, v, c0, c1, causal=causal, scale_div=scale_div, p_scale=s) for s in (1.0 + 2.0 ** -20, 1.0 - 2.0 ** -20)]
    return ref, conditions(ref, moved, count)


def check(out, ref, keep):
    scale = np.abs(ref).max()
    d = np.abs(out - ref)[keep]
    print("worst", d.max() / scale, "mean", d.mean() / scale)
    assert d.max() <= 1e-3 * scale, (d.max(), scale)
    assert d.mean() <= 3e-5 * scale, (d.mean(), scale)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# (B, M, T, D, causal, (qk x, qk y, pv x, pv y) formats, scale: "div" scale_div = sqrt(D) / "q" q_scale = D^-0.5 / "both" / None, seed)
# T = 16: one tile, the pair's second tile missing.  48: an odd tile count.  80.  272: more than four steps, a second buffer wrap, five
# query blocks with the last one partial.  M = T causal; M = 1; M = 17 behind T = 48 causal (offset horizon); M = 70 with T = 48
# non-causal (more queries than keys); M = 65 (a wave wholly behind M).
def _same(f):
    return (f, f, f, f)


def _case(B, M, T, D, causal=True, fmts=_same(F848), scale="div", seed=None):
    return (B, M, T, D, causal, fmts, scale, T + D + M if seed is None else seed)


CASES = (
    # every head_dim x every T, M = T causal
    [_case(1, T, T, D) for D in (32, 64, 96, 128) for T in (16, 48, 80, 272)]
    # the query shapes
    + [_case(1, 1, 48, 64), _case(1, 1, 48, 128, seed=1177)]
    + [_case(1, 17, 48, D) for D in (32, 64, 96, 128)]
    + [_case(1, 70, 48, D, causal=False) for D in (64, 128)]
    + [_case(1, 65, 80, D) for D in (32, 64, 96, 128)]
    + [_case(1, 65, 272, D) for D in (64, 128)]
    + [_case(1, 1, 16, 32), _case(2, 1, 272, 96)]
    # B = 3
    + [_case(3, 80, 80, 64), _case(3, 17, 48, 128), _case(3, 272, 272, 32), _case(3, 16, 16, 96)]
    # the formats ((4, 2, 3) has ONE mantissa bit: a probability below 0.5 is 0, so its cases run unscaled scores -- under scale_div
    # the oracle's output is zero in three rows of four and its own condition above refuses the case)
    + [_case(1, M, T, D, fmts=_same(f)) for f in (F634, F735) for (M, T, D) in ((48, 48, 64), (272, 272, 128), (17, 48, 96))]
    + [_case(1, M, T, D, fmts=_same(F423), scale=None) for (M, T, D) in ((48, 48, 64), (272, 272, 128), (17, 48, 96))]
    # different formats for Q / K and P / V; different x and y sides within a product
    + [_case(1, 80, 80, 64, fmts=(F848, F848, F634, F634)), _case(2, 48, 48, 128, fmts=(F735, F735, F848, F848)),
       _case(1, 80, 80, 64, fmts=(F848, F634, F735, F848)), _case(2, 17, 48, 32, fmts=(F634, F848, F848, F735))]
    # scale_div off with q_scale on (OPT), both off; non-causal M = T.  (Both ON scales the scores twice: 28 % of the oracle's rows are
    # non-zero at [80, 80, 64], which the oracle's own condition refuses; the two multiplications are each covered.)
    + [_case(1, T, T, D, scale="q") for (T, D) in ((48, 64), (272, 128), (80, 96), (16, 32))]
    + [_case(1, 48, 48, 64, scale=None), _case(1, 65, 80, 128, scale=None)]
    + [_case(1, T, T, D, causal=False) for (T, D) in ((48, 32), (80, 64), (272, 128))]
    + [_case(2, 70, 48, 96, causal=False, scale="q")]
)


def case_id(c):
    B, M, T, D, causal, fmts, scale, _ = c
    f = "-".join("".join(str(x) for x in fm) for fm in fmts) if len(set(fmts)) > 1 else "".join(str(x) for x in fmts[0])
    return f"B{B}-M{M}-T{T}-D{D}-{'causal' if causal else 'full'}-{f}-{scale}"


def case_scales(c):
    """-> (scale_div, q_scale) of the op's call"""
    D, scale = c[3], c[6]
    return (math.sqrt(D) if scale in ("div", "both") else None, float(np.float32(D ** -0.5)) if scale in ("q", "both") else None)


@lru_cache(maxsize=None)
def case_reference(c, count=True):
    """-> (q, k, v, ref, keep) of a case, computed once and shared (the arrays are not to be written)"""
    B, M, T, D, causal, fmts, _, seed = c
    q, k, v = inputs(B, M, T, D, seed)
    scale_div, q_scale = case_scales(c)
    qs = q if q_scale is None else (q * np.float32(q_scale)).astype(np.float32)
    ref, keep = reference_of(qs, k, v, cfg(fmts[0], fmts[1]), cfg(fmts[2], fmts[3]), causal, scale_div, count)
    for a in (q, k, v, ref, keep):
        a.setflags(write=False)
    return q, k, v, ref, keep
