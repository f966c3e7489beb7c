"""Which kernels a quantised `Linear` runs, as pure functions of ints, bools and the config dict: no tensor, no device call, no
environment, no state.  `linear.py` measures (exception-bucket fills, outlier columns), asks here, and applies the answer; the
placement half of every predicate (is_cuda, dtype, versions, devices) stays on the layer.  tests/golden/linear_policy.json holds
the decisions of the commit before this file existed; tests/test_linear_policy.py holds every function here to them."""
from __future__ import annotations

from typing import NamedTuple, Optional

from ... import ops

_OFF = (False, "off", None)


def exponent_bias(bias, exponent_width: int):
    """the quantisers' default bias (2^(e-1) - 1) where the config gives none"""
    return 2 ** (exponent_width - 1) - 1 if bias in (None, "none", "None") else bias


def weight_bias(c: dict):
    return exponent_bias(c["weight_exponent_bias"], c["weight_exponent_width"])


def initial_x_cap(align: str) -> int:
    """exception entries per 256 activation rows a layer starts with: "rows_post" the post-pass's large buckets, "blocks" no
    alignment at all, everything else the GEMM's in-LDS add-back"""
    return {"rows_post": ops.ROW_BUCKET_CAP_MAX, "blocks": ops.ROW_NO_ALIGN}.get(align, ops.ACTIVATION_BUCKET_CAP)


def _blocks_1x16(c: dict, K: int, N: int, x_ndim: int, x_rows_dim: int) -> bool:
    """both operands in [1, 16] blocks along in_features"""
    xs = [1, K] if x_ndim == 2 else [1, x_rows_dim, K]
    return (ops.resolve_blocking(xs, c["data_in_block_size"], True)[3:] == (1, 16)
            and ops.resolve_blocking([N, K], c["weight_block_size"], False)[3:] == (1, 16))


def int8_plan(c: dict, arith: str, K: int, N: int, x_ndim: int, x_rows_dim: int):
    """(x_mbits, w_mbits, x_bias, w_bias) when the contraction is an int8 x int8 block dot on the MFMA path: block_fp both sides,
    [1,16] blocks along in_features, widths <= 8.  `x_rows_dim`: x.shape[-2] of a 3-d input."""
    if arith != "block_fp" or K % 64 or not (2 <= c["data_in_width"] <= 8 and 2 <= c["weight_width"] <= 8):
        return None
    if not (1 <= c["data_in_exponent_width"] <= 8 and 1 <= c["weight_exponent_width"] <= 8):
        return None
    if not 2 <= x_ndim <= 3 or not _blocks_1x16(c, K, N, x_ndim, x_rows_dim):
        return None
    xb, wb = exponent_bias(c["data_in_exponent_bias"], c["data_in_exponent_width"]), weight_bias(c)
    if xb < 0 or wb < 0:
        return None                  # packed operands store biased uint8 exponent codes: non-negative biases only
    return c["data_in_width"] - 1, c["weight_width"] - 1, xb, wb


# ---- rows / per-block / mixed: decided once per packing ----------------------------------------------------------------------
class Align(NamedTuple):
    """what `_x_cap` becomes now (None: it stays), whether the mixed split is to be attempted, and what `_x_cap` becomes once
    that attempt succeeded / failed (None: it stays)"""
    x_cap: Optional[int]
    try_mixed: bool = False
    x_cap_if_mixed: Optional[int] = None
    x_cap_if_not: Optional[int] = None


def align_is_measured(K: int, align: str) -> bool:
    """does the decision read the operands' exception buckets (one-off host reads at pack time)?"""
    if align == "groups":
        raise ValueError('mi355q_align = "groups" was removed in round 5 (use "auto", "rows", "rows_post" or "blocks")')
    return ops.row_align_supported(K) and align not in ("rows", "rows_post", "blocks")


def rows_fit(fill) -> bool:
    """fill = (overflow word, fullest bucket) of an operand's exception list: it fits a tile's in-LDS add-back on its own"""
    return fill[0] == 0 and fill[1] <= ops.ROW_TILE_ENTRIES_FAST


def align_decision(K: int, N: int, M: int, align: str, w_fill, x_fill) -> Align:
    """`w_fill` / `x_fill`: (overflow, fullest) of the weights' and of the sample activations' [M, K] exception lists (None: not
    measured -- `align_is_measured`, no sample, or weights that do not fit).  Rows pay off while a 256 x 256 tile's entries
    (x bucket + w bucket) fit the GEMM's in-LDS add-back."""
    if not align_is_measured(K, align):
        # contractions past the row format's 16384 (Llama-30B/65B down_proj): every block keeps its exponent
        return Align(None if ops.row_align_supported(K) else ops.ROW_NO_ALIGN)
    if not rows_fit(w_fill):
        # weights whose exception blocks do not fit a tile's LDS add-back (outlier input channels put one in every
        # row): the outlier block columns as class 1 of the mixed contraction if that leaves a class 0 that fits, else no
        # alignment -- the blockwise / bf16 product does not care how exponents are distributed
        return Align(None, True, None, ops.ROW_NO_ALIGN)
    if x_fill is None:
        return Align(None)
    # activations: the GEMM's in-LDS add-back while a tile's entries fit it; otherwise (post-activation inputs:
    # hundreds of exception blocks per 256 rows after a ReLU, no usable row window at all after a SiLU gate) no
    # alignment -- measured faster than the row post-pass wherever that one applies (tools/timing/time_linear_modes.py;
    # "rows_post" remains available explicitly)
    # (a 128-row tile carries about half of its 256-row bucket's activation entries; 15 % margin for the busier
    # half.  Measured at 2048 x 4096 -> 4096, tools/timing/time_exception_density.py: the row-scale route wins up to a
    # fullest activation bucket of ~60 there, the per-block route beyond ~85)
    # Between 48 and 96 entries a tile forms its vectors behind the K loop: still ahead of the per-block route where
    # that one runs 256-row tiles (2048 x 4096 -> 11008: 163 vs 208 us at a fullest bucket of 87), behind it on
    # 128-row tiles (2048 x 4096 -> 4096: 100 vs 91 us).
    tile_rows = ops.gemm_tile_rows(M, N)
    n_tile = w_fill[1] + int(x_fill[1] * (0.5 * 1.15 if tile_rows == 128 else 1.0) + 0.999)
    if x_fill[0] == 0 and (n_tile <= ops.ROW_TILE_ENTRIES_FAST or (tile_rows == 256 and n_tile <= ops.ROW_TILE_ENTRIES_SLOW - 8)):
        return Align(ops.ROW_BUCKET_CAP)
    return Align(ops.ROW_NO_ALIGN, True, ops.ROW_BUCKET_CAP, ops.ROW_NO_ALIGN)


def mixed_config_ok(c: dict, K: int, align: str) -> bool:
    """the mixed contraction is on, the route is the layer's to choose, and the shape / storage / widths are ones it takes"""
    return not (c.get("mi355q_mixed", "auto") in _OFF or align != "auto" or K % 128 or K < 512 or not ops.row_align_supported(K)
                or c.get("mi355q_weight_storage", "int8") == "packed" or c["data_in_width"] > 8 or c["weight_width"] > 8)


MIXED_OUTLIER_SHARE = 0.25       # a block column is class 1 when it lies outside its rows' exponent window in more of the rows


def mixed_class1_blocks(n_outlier: int, nb: int) -> int:
    """block columns of class 1 for `n_outlier` outlier columns out of nb = K // 16 (0: no split): whole pairs of 64-byte
    K-steps in both classes, at most half of the columns, and a class 0 of at least 16 blocks"""
    n1 = -(-n_outlier // 8) * 8
    return 0 if n1 == 0 or n1 > nb // 2 or nb - n1 < 16 else n1


def mixed_fits(w_fill, x_fill) -> bool:
    """class 0 of both operands fits the row-scale route's in-LDS add-back"""
    return rows_fit(w_fill) and x_fill[0] == 0 and w_fill[1] + x_fill[1] <= ops.ROW_TILE_ENTRIES_FAST


# ---- routes: the config and shape half of the layer's predicates -----------------------------------------------------------------
def bf16_operands_ok(c: dict, K: int) -> bool:
    """block_fp values of width <= 9 are exact in bf16; the tile GEMM's K-step is 32 of them"""
    return K % 32 == 0 and c["data_in_width"] <= 9 and c["weight_width"] <= 9


def uses_bf16_route(c: dict, K: int, x_cap: int) -> bool:
    """every block keeps its exponent and the product is the bf16 flavour of the tile GEMM (mi355q_blocks_gemm = "int8": the
    blockwise-exact int8 kernel instead, where the row format takes K at all)"""
    return (x_cap == ops.ROW_NO_ALIGN and (c.get("mi355q_blocks_gemm", "bf16") == "bf16" or not ops.row_align_supported(K))
            and bf16_operands_ok(c, K))


def residual_rides_the_int8_product(K: int, x_cap: int) -> bool:
    """ops.bfp_gemm_aligned(residual=...): 120-entry activation buckets, K a multiple of 128"""
    return x_cap == ops.ROW_BUCKET_CAP and K % 128 == 0


def small_m_takes(c: dict, K: int, numel: int) -> bool:
    return c.get("mi355q_small_m", "off") == "packed" and numel // K <= ops.SMALL_M_MAX and numel > 0


def values_exact_in_bf16(c: dict, arith: str, K: int) -> bool:
    """minifloats with at most 7 mantissa bits, signed powers of two, fixed point of at most 9 bits: exact in bf16, a product of
    two of them exact in fp32.  config["mi355q_values_gemm"] = "fp32" keeps F.linear."""
    if c.get("mi355q_values_gemm", "bf16") != "bf16":
        return False
    if arith in ("block_minifloat", "minifloat_ieee", "minifloat_denorm"):     # <= 7 mantissa bits
        if not all(0 <= c[f"{p}_width"] - c[f"{p}_exponent_width"] - 1 <= 7 for p in ("data_in", "weight")):
            return False
    elif arith == "integer":                          # fixed point of <= 9 bits: <= 8 significant bits
        if not all(2 <= c[f"{p}_width"] <= 9 for p in ("data_in", "weight")):
            return False
    elif arith != "block_log":                        # (signed powers of two)
        return False
    return K % 32 == 0


def _widths_2_to_9(c: dict) -> bool:
    return 2 <= c["data_in_width"] <= 9 and 2 <= c["weight_width"] <= 9


def qat_on_tile_gemm(c: dict, arith: str, K: int, N: int, M: int, values_exact: bool) -> bool:
    """`values_exact`: the layer's `_values_exact_in_bf16` (not asked for block_fp, whose widths decide)"""
    knob = c.get("mi355q_qat_gemm", "bf16")
    if knob not in ("bf16", "bf16_always") or not (_widths_2_to_9(c) if arith == "block_fp" else values_exact):
        return False
    if not (K % 32 == 0 and N % 32 == 0 and M % 32 == 0 and M > 0):
        return False
    # three products + the tiling / plane-split launches around them: ahead of the fp32 library GEMM from ~2^34 multiply-adds a
    # product (profiles/r05_qat_gemm.jsonl: 2048 x 1024 x 4096 0.97-1.09x, 2048 x 4096 x 4096 2.0x, 512 x 1024 x 4096 0.4-0.6x);
    # mi355q_qat_gemm = "bf16_always" takes it regardless (tests)
    return knob == "bf16_always" or M * K * N >= (1 << 34)


def padded_block_fp_ok(c: dict, arith: str, K: int, N: int, x_ndim: int, x_rows_dim: int) -> bool:
    """in_features a multiple of the block (16) but not of the tile kernels' K-step (64).  config["mi355q_pad_k"] = False keeps
    F.linear."""
    if arith != "block_fp" or not c.get("mi355q_pad_k", True) or K % 16 or K % 64 == 0:
        return False
    return 2 <= x_ndim <= 3 and _widths_2_to_9(c) and _blocks_1x16(c, K, N, x_ndim, x_rows_dim)


def mx_config_ok(c: dict, arith: str, is_ptq: bool, bypass: bool, K: int) -> bool:
    """config["mi355q_mx"]: "auto" (default) -- block_fp operands of <= 4 bits each (every mantissa exact in FP6 e2m3 with
    three exponents of reach inside a 32-group; at 5 bits the reach is two and Gaussian data already trips it), [1,16] blocks
    along in_features, in_features % 128 == 0; True -- every launch that fits the format (<= 5 bits); False -- never"""
    knob = c.get("mi355q_mx", "auto")
    if knob in _OFF or arith != "block_fp" or not is_ptq or bypass:
        return False
    wmax = 5 if knob is True else 4
    return (ops.mx_supported(K, c["data_in_width"], c["weight_width"]) and c["data_in_width"] <= wmax and c["weight_width"] <= wmax
            and c.get("mi355q_weight_storage", "int8") != "packed")


def mx_takes(c: dict, M: int, N: int) -> bool:
    """"auto": launches of >= 192 tiles of 256 x 256 (below that the small-tile int8 kernel wins: profiles/r05_mx_w4a4.txt)"""
    return c.get("mi355q_mx", "auto") is True or -(-M // 256) * -(-N // 256) >= 192
