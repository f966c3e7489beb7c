"""Checker-side helpers for the fused paths that write a CONSUMER's quantised operand (tests/test_gpu_fused_oracle.py).

TEST INFRASTRUCTURE ONLY, like the rest of ``oracle/``: the product path never imports it.  Pure numpy: nothing here calls
the kernels it is used to check.

* ``decode_bf16_tiled``: the tiled bf16 operand (csrc/mi355q_split.hip header, ``gated_offset`` in csrc/mi355q_gemm_v9.hip)
  back to a [rows, cols] fp32 array.  1-KiB pieces of 16 rows x 32 values, [8-value group 0..3][row 0..15][8 bf16] inside;
  piece (row / 16, col / 32) at index (row / 16) * (cols / 32) + col / 32.
* ``match_quantised``: the exact-or-ambiguous rule.  A kernel that computes h in fp32 (products, epilogue op) and then
  quantises it may land on the other side of a rounding boundary than the fp64 value does -- but only where h moved by
  its own fp32 rounding could.  So every quantised element must equal the oracle's quantisation of h * (1 - delta), of h,
  or of h * (1 + delta); where those three disagree the element is AMBIGUOUS, and callers bound the ambiguous fraction so
  the rule cannot pass by being vacuous.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import np_oracle as O


def _as_numpy(a) -> np.ndarray:
    if hasattr(a, "detach"):                        # (a torch tensor: duck-typed, so that this module needs numpy only)
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a)


def bf16_bits_to_f32(u16: np.ndarray) -> np.ndarray:
    return (np.asarray(u16, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def decode_bf16_tiled(buf, rows: int, cols: int) -> np.ndarray:
    """the first `rows` rows of a tiled bf16 operand [>= rows, cols] as fp32 (cols % 32 == 0; the buffer may hold padding
    rows behind them)"""
    assert cols % 32 == 0, cols
    u = _as_numpy(buf).reshape(-1).view(np.uint16)
    rt, kp = (rows + 15) // 16, cols // 32
    assert u.size >= rt * 16 * cols, (u.size, rows, cols)
    t = u[: rt * 16 * cols].reshape(rt, kp, 4, 16, 8).transpose(0, 3, 1, 2, 4).reshape(rt * 16, cols)
    return bf16_bits_to_f32(t[:rows])


def encode_bf16_tiled(x: np.ndarray) -> np.ndarray:
    """the inverse (x exact in bf16, [rows, cols], cols % 32 == 0): uint16 pieces, the last piece row padded with zeros"""
    x = np.asarray(x, dtype=np.float32)
    rows, cols = x.shape
    assert cols % 32 == 0
    rt, kp = (rows + 15) // 16, cols // 32
    u = np.zeros((rt * 16, cols), dtype=np.uint16)
    bits = x.view(np.uint32)
    assert not (bits & 0xFFFF).any(), "not exact in bf16"
    u[:rows] = (bits >> 16).astype(np.uint16)
    return np.ascontiguousarray(u.reshape(rt, 16, kp, 4, 8).transpose(0, 2, 3, 1, 4)).reshape(-1)


class Match(NamedTuple):
    mismatched: int
    ambiguous: int
    total: int
    first: str                      # where the first mismatch is, what it got and what was allowed ("" when none)

    @property
    def ambiguous_fraction(self) -> float:
        return self.ambiguous / max(self.total, 1)


def bf16_rne(x: np.ndarray) -> np.ndarray:
    """fp32 -> the nearest bf16 (ties to even), as fp32; finite inputs"""
    b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def match_quantised(got, h64, width: int, exponent_width: int, exponent_bias, delta: float, block_size=(1, 16),
                    bf16: bool = False, slack=None) -> Match:
    """`got` [rows, cols]: a kernel's fake-quantised values; `h64`: the fp64 value the operation should produce before the
    quantiser.  Each element must equal O.block_fp_quantize (activation blocking: skip_first_dim) of h64 * (1 - delta),
    h64 or h64 * (1 + delta), compared as values (-0 == +0).  `bf16`: `got` was stored as bf16 -- the quantised values are
    exact in bf16 (width <= 9), the ones the quantiser passes through (|h| <= 1e-8) are compared after the same rounding.
    `slack` (fp64, h's shape): an absolute allowance for the pass-through values -- an fp32 sum's rounding scales with the
    magnitude of its terms, not of its result, and a value below 1e-8 out of terms of magnitude ~1 is all cancellation."""
    got = np.asarray(_as_numpy(got), dtype=np.float32)
    h64 = np.asarray(h64, dtype=np.float64)
    assert got.shape == h64.shape, (got.shape, h64.shape)
    q = [O.block_fp_quantize((h64 * s).astype(np.float32), width, exponent_width, exponent_bias, list(block_size), True)
         for s in (1.0 - delta, 1.0, 1.0 + delta)]
    dev = delta * np.abs(h64)
    if bf16:
        q = [bf16_rne(v) for v in q]
    ok = (got == q[0]) | (got == q[1]) | (got == q[2])
    amb = (q[0] != q[1]) | (q[1] != q[2])
    # values the quantiser passes through unquantised (|h| <= 1e-8 whichever way h moves) are fp32 results themselves, not
    # points of a grid: with a `slack`, held to the interval h -/+ (dev + slack) (and the bf16 store's rounding); never ambiguous
    passed = np.abs(h64) + dev <= float(O._ATOL)
    if passed.any():
        if slack is not None:
            tol = dev + (2.0 ** -8 * np.abs(h64) if bf16 else 0.0) + np.asarray(slack, dtype=np.float64)
            ok = np.where(passed, ok | (np.abs(got.astype(np.float64) - h64) <= tol), ok)
        amb = amb & ~passed
    bad = ~ok
    first = ""
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        first = f"at {i}: got {got[i]!r}, allowed {q[0][i]!r} / {q[1][i]!r} / {q[2][i]!r} (h = {h64[i]!r})"
    return Match(int(bad.sum()), int(amb.sum()), int(got.size), first)
