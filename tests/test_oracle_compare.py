"""CPU self-tests of the checker the fused-path tests use (oracle/compare.py): the tiled-bf16 decoder and the
exact-or-ambiguous comparator must themselves be right -- and strict enough to catch the errors they exist for -- before
anything is held to them.  Also: the switch set the model tests call "config3" is the one the config-3 tool turns on."""
import numpy as np

from oracle import compare as C
from oracle import np_oracle as O

W, EW, EB = 6, 8, 127                                    # the consumer quantiser of the W6A6 configs (mbits = 5)


def _bf16_exact(r, shape):
    x = r.normal(size=shape).astype(np.float32)
    return (x.view(np.uint32) & 0xFFFF0000).view(np.float32)


def _encode_by_formula(x):
    """a host encoder written from the documented byte offset alone (gated_offset, mi355q_gemm_v9.hip): value (row, col) at
    ((row >> 4) * (cols / 32) + (col >> 5)) * 1024 + ((col & 31) >> 3) * 256 + (row & 15) * 16 + (col & 7) * 2"""
    rows, cols = x.shape
    buf = np.zeros(((rows + 15) // 16) * 16 * cols * 2, dtype=np.uint8)
    u = (x.view(np.uint32) >> 16).astype(np.uint16)
    for row in range(rows):
        for col in range(cols):
            off = ((row >> 4) * (cols // 32) + (col >> 5)) * 1024 + ((col & 31) >> 3) * 256 + (row & 15) * 16 + (col & 7) * 2
            buf[off:off + 2] = np.frombuffer(u[row, col].tobytes(), dtype=np.uint8)
    return buf


def test_decoder_round_trips_the_formula_encoder():
    r = np.random.default_rng(0)
    for rows, cols in ((16, 32), (17, 64), (1, 96), (45, 128)):
        x = _bf16_exact(r, (rows, cols))
        buf = _encode_by_formula(x)
        assert np.array_equal(C.decode_bf16_tiled(buf, rows, cols), x)
        assert np.array_equal(C.encode_bf16_tiled(x).view(np.uint8), buf)
        assert np.array_equal(C.decode_bf16_tiled(C.encode_bf16_tiled(x), rows, cols), x)


def _block_max_one(r, rows=4, cols=64):
    """rows of 16-blocks whose max is 0.75 (exponent 0, step 2^-5, away from the exponent's boundary), the other values away
    from every rounding boundary (a quarter step off a grid point)"""
    g = r.integers(-23, 24, size=(rows, cols)).astype(np.float64)
    h = (g + np.where(r.integers(2, size=g.shape) == 1, 0.25, -0.25)) / 32.0
    h[:, ::16] = 0.75
    return h


def test_comparator_accepts_a_value_flipped_across_a_rounding_boundary():
    r = np.random.default_rng(1)
    h = _block_max_one(r)
    h[2, 5] = 7.5 / 32.0                                 # a tie: fp32 rounding of h may send it either way
    exact = O.block_fp_quantize(h.astype(np.float32), W, EW, EB, [1, 16], True)
    for v in (7.0 / 32.0, 8.0 / 32.0):
        got = exact.copy()
        got[2, 5] = v
        m = C.match_quantised(got, h, W, EW, EB, 2.0 ** -20)
        assert m.mismatched == 0 and m.ambiguous == 1, m


def test_comparator_rejects_a_one_step_error_away_from_a_boundary():
    r = np.random.default_rng(2)
    h = _block_max_one(r)
    got = O.block_fp_quantize(h.astype(np.float32), W, EW, EB, [1, 16], True)
    assert C.match_quantised(got, h, W, EW, EB, 2.0 ** -20) == (0, 0, h.size, "")
    got[1, 9] += np.float32(1.0 / 32.0)
    m = C.match_quantised(got, h, W, EW, EB, 2.0 ** -20)
    assert m.mismatched == 1 and m.ambiguous == 0, m


def test_comparator_rejects_a_block_whose_exponent_is_off_by_one():
    r = np.random.default_rng(3)
    h = r.normal(size=(8, 64))
    got = O.block_fp_quantize(h.astype(np.float32), W, EW, EB, [1, 16], True)
    code = O.bfp_encode(h.astype(np.float32), W, EW, EB, [1, 16], True)
    e = int(code.exp[4 * 2 + 1]) + 1                     # row 2, block 1, one exponent too high
    x = h[2, 16:32].astype(np.float32)
    m = np.clip(np.rint(np.abs(x) / np.float32(2.0 ** e) * np.float32(32)), 0, 31)
    got[2, 16:32] = np.sign(x) * np.float32(2.0 ** e) * (m / np.float32(32))
    res = C.match_quantised(got, h, W, EW, EB, 2.0 ** -20)
    assert res.mismatched >= 8 and res.ambiguous <= 2, res


def test_comparator_rejects_a_row_missing_one_exception_term():
    r = np.random.default_rng(4)
    M, N, K = 6, 64, 256
    x = r.normal(size=(M, K)).astype(np.float32)
    x[3, 128:144] *= 300.0                               # one exception block
    w = (r.normal(size=(N, K)) * 0.05).astype(np.float32)
    h = x.astype(np.float64) @ w.astype(np.float64).T
    dropped = h.copy()
    dropped[3] -= x[3, 128:144].astype(np.float64) @ w[:, 128:144].astype(np.float64).T
    good = C.match_quantised(O.block_fp_quantize(h.astype(np.float32), W, EW, EB, [1, 16], True), h, W, EW, EB, 2.0 ** -20)
    assert good.mismatched == 0
    bad = C.match_quantised(O.block_fp_quantize(dropped.astype(np.float32), W, EW, EB, [1, 16], True), h, W, EW, EB, 2.0 ** -20)
    assert bad.mismatched > N // 4 and bad.first.startswith("at (3,"), bad


def test_config3_switch_set_is_the_config3_tools():
    """tests/test_gpu_model.py's "config3" switch set == what tools/config3_full_depth.quant_config("resident") turns on"""
    from tests import test_gpu_model as TM
    from tools import config3_full_depth as T
    from tools.config3_full_depth import quant_config
    tool = {k: v for k, v in quant_config("resident")["default"].items() if k.startswith("mi355q_")}
    assert TM.CONFIG3_KNOBS == tool
    assert TM.CONFIG3_LM_HEAD == T.LM_HEAD                   # (set on the model: build() there, the config3 cases here)
    assert "mi355q_weight_storage" not in TM.CONFIG3_KNOBS
    assert quant_config("hybrid")["default"]["mi355q_weight_storage"] == "hybrid"
