"""The row quantiser (bfp_quant_align_rows_kernel, csrc/mi355q_quant.hip) and the kernels that share its row arithmetic, held
bit for bit to the oracle on the reference's edge set: mantissa ties, block maxima a few ulps from a power of two, maxima
that round up into the clamp, the 1e-8 / 1e-9 neighbourhood, both signs -- in every compiled build the launcher picks
among (slabs per lane 1 / 2 / 4 / 8 / 12 / 16, guarded and full, 16-byte stores, segmented rows, relu in front, MX, the
round-5 build, the grid walk).  Inputs and expected values: tests/row_edges_util.py; what the inputs hold is shown on the
CPU by tests/test_row_edges_host.py.  Every comparison is np.array_equal."""
import numpy as np
import pytest

from tests import row_edges_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_operand_reuse(monkeypatch):
    from mi355q import ops
    monkeypatch.setattr(ops, "REUSE_QUANTISED_INPUT", False)


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, dtype=np.float32, order="C")).to("cuda:0")       # (a copy: the layouts are read-only)


def _check_elements(x, width, ew=8, bias=127):
    """no alignment: every block keeps its own exponent -- mantissas and exponents against the oracle, element by element"""
    import torch
    from mi355q import ops
    rows, K = x.shape
    op = ops.block_fp_quantize_aligned_rows(_dev(x), width, ew, bias, bucket_cap=ops.ROW_NO_ALIGN)
    torch.cuda.synchronize()
    assert not bool(op.rowflag.any())
    mant, code = U.operand_codes(op, rows, K)
    emant, eexp, nz = U.oracle_codes(x, width, ew, bias)
    bad = np.argwhere(mant != emant)
    assert np.array_equal(mant, emant), f"{len(bad)} mantissas differ, first (row, block, element) {bad[:4].tolist()}"
    assert np.array_equal((code - bias)[nz], eexp[nz]), "block exponents differ"


# ---- a. element arithmetic alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", U.ELEMENT_WIDTHS)
@pytest.mark.parametrize("K", U.ELEMENT_SHORT_K + U.ELEMENT_LONG_K)
def test_elements_in_every_build(K, width):
    _check_elements(U.element_layout(K), width)


@pytest.mark.parametrize("K,rows", [(64, U.GRID_WALK_ROWS), (4096, U.ELEMENT_LONG_ROWS)])
def test_elements_when_a_workgroup_walks_many_rows(K, rows, monkeypatch):
    monkeypatch.setenv("MI355Q_QROWS_GRID", "7")
    x = U.element_layout(K)[:rows]
    assert x.shape[0] == rows
    for width in (6, 4):
        _check_elements(x, width)


@pytest.mark.parametrize("K", [320, 4096])
def test_elements_in_the_round5_build(K, monkeypatch):
    monkeypatch.setenv("MI355Q_QROWS_VARIANT", "0")
    for width in (6, 4):
        _check_elements(U.element_layout(K), width)


@pytest.mark.parametrize("width", U.DEEP_WIDTHS)
@pytest.mark.parametrize("K", U.DEEP_K)
def test_elements_beside_blocks_below_2_pow_minus_23(K, width):
    """a wave that holds a block below 2^-23 takes the exact per-element rule (mant_f) for all its blocks: ties at ordinary
    magnitudes go through it only here (tests/test_row_edges_host.py counts them)"""
    _check_elements(U.deep_layout(K), width)


def test_elements_at_both_exponent_clamps():
    x = U.clamp_layout()
    _, eexp, nz = U.oracle_codes(x, 6, 4, 7)
    assert (eexp[nz] == -7).sum() > 100 and (eexp[nz] == 8).sum() > 100 and ((eexp[nz] > -7) & (eexp[nz] < 8)).sum() > 100
    _check_elements(x, 6, 4, 7)


# ---- b. with alignment ---------------------------------------------------------------------------------------------------
def _two_step(xt, width, cap=0):
    from mi355q import ops
    _, xm, xe = ops.block_fp_quantize(xt, width, 8, 127, [1, 16], True, want_fake=False, want_packed=True,
                                      fast_zero_blocks=True)
    return ops.bfp_align_rows(xm, xe, width - 1, 127, bucket_cap=cap)


def _entry_set(op, rows):
    from mi355q import ops
    over, ent = ops.row_list_entries(op.sparse, rows, op.list_cap)
    return over, set(map(tuple, ent))


@pytest.mark.parametrize("width", U.ALIGNED_WIDTHS)
@pytest.mark.parametrize("K", sorted(U.ALIGNED_ROWS))
def test_aligned_operand_denotes_the_oracle_values(K, width):
    import torch
    from mi355q import ops
    x = U.aligned_layout(K)
    rows = x.shape[0]
    xt = _dev(x)
    got = ops.block_fp_quantize_aligned_rows(xt, width, 8, 127)
    torch.cuda.synchronize()
    assert np.array_equal(U.decode_operand(got, rows, K), U.expected_values(x, width))
    mant, code = U.operand_codes(got, rows, K)
    fl = got.rowflag.cpu().numpy() == 1
    assert np.all(code[fl] == code[fl][:, :1]), "flagged rows carry one exponent"
    rs = got.gscale.cpu().numpy()[:rows]
    assert np.array_equal(rs[fl], np.exp2((code[fl][:, 0] - (127 + width - 1)).astype(np.float64)).astype(np.float32))
    assert np.all(rs[~fl] == 0)
    over, entries = _entry_set(got, rows)
    assert over == 0 and int(got.sparse[0]) == 0 and fl.all()
    with_exc = {e[0] for e in entries}
    assert len(entries) >= 1 and len(with_exc) < fl.sum(), "rows with and rows without an exception block"
    # the same operand as from the streaming quantiser + bfp_align_rows
    ref = _two_step(xt, width)
    torch.cuda.synchronize()
    over_ref, entries_ref = _entry_set(ref, rows)
    assert over_ref == 0 and entries == entries_ref
    assert np.array_equal(U._untile(got.tiled, rows, K), U._untile(ref.tiled, rows, K))
    full = (rows // 16) * 16 * K
    assert torch.equal(got.tiled[:full], ref.tiled[:full])
    assert torch.equal(got.exp, ref.exp.reshape(-1)) and torch.equal(got.rowflag, ref.rowflag)
    assert torch.equal(got.gscale[:rows], ref.gscale[:rows])


def test_overflowing_rows_keep_their_own_exponents():
    import torch
    from mi355q import ops
    K, width = U.OVERFLOW_K, U.OVERFLOW_WIDTH
    x = U.element_layout(K)
    rows = x.shape[0]
    got = ops.block_fp_quantize_aligned_rows(_dev(x), width, 8, 127)
    torch.cuda.synchronize()
    assert int(got.sparse[0]) > 0
    fl = got.rowflag.cpu().numpy() == 1
    assert (~fl).sum() == int(got.sparse[0])
    dec, exp = U.decode_operand(got, rows, K), U.expected_values(x, width)
    assert np.array_equal(dec[~fl], exp[~fl]), "unflagged rows: own exponents, nothing listed"
    assert np.array_equal(dec[fl], exp[fl])
    mant, code = U.operand_codes(got, rows, K)
    emant, eexp, nz = U.oracle_codes(x, width)
    assert np.array_equal(mant[~fl], emant[~fl]) and np.array_equal((code - 127)[~fl][nz[~fl]], eexp[~fl][nz[~fl]])


# ---- c. the operand as the GEMM reads it --------------------------------------------------------------------------------
def _identity_w6(K):
    """the row-aligned W6 operand of eye(K): mantissa 16 at exponent 1 (16 x 2^(1 - 5) = 1; the quantiser itself cannot
    produce it -- a block whose maximum is a power of two saturates its mantissa, (2^5 - 1) / 2^5)"""
    import torch
    from mi355q import ops
    wm = (torch.eye(K, device="cuda:0") * 16).to(torch.int8)
    we = torch.full((K * (K // 16),), 128, dtype=torch.uint8, device="cuda:0")
    return ops.bfp_align_rows(wm, we, 5, 127)


@pytest.mark.parametrize("tile_rows", [256, 128])
@pytest.mark.parametrize("K", [320, 1024])
def test_product_with_identity_returns_the_oracle_values(K, tile_rows, monkeypatch):
    import torch
    from mi355q import ops
    monkeypatch.setenv("MI355Q_V8_TILE_ROWS", str(tile_rows))
    x = U.element_layout(K)
    wa = _identity_w6(K)
    xa = ops.block_fp_quantize_aligned_rows(_dev(x), 6, 8, 127)
    y = ops.bfp_gemm_aligned(xa, wa)
    torch.cuda.synchronize()
    exp = U.expected_values(x, 6)
    assert np.array_equal(exp.astype(np.float32).astype(np.float64), exp)
    assert np.array_equal(y.cpu().numpy(), exp.astype(np.float32))


# ---- d. siblings that share the row arithmetic ---------------------------------------------------------------------------
def test_segmented_rows():
    import torch
    from mi355q import ops
    K, P = 2048, 4
    x = U.element_layout(K)
    rows = x.shape[0]
    plain = ops.block_fp_quantize_aligned_rows(_dev(x), 6, 8, 127)
    torch.cuda.synchronize()
    assert np.array_equal(U.decode_operand(plain, rows, K), U.expected_values(x, 6))
    p_tiled, p_exp, p_flag, p_scale = (t.clone() for t in (plain.tiled, plain.exp, plain.rowflag, plain.gscale))
    _, p_entries = _entry_set(plain, rows)
    xs = np.ascontiguousarray(x.reshape(rows, P, K // P).transpose(1, 0, 2))
    seg = ops.block_fp_quantize_aligned_rows(_dev(xs), 6, 8, 127, segments=True)
    torch.cuda.synchronize()
    assert torch.equal(seg.tiled, p_tiled) and torch.equal(seg.exp, p_exp) and torch.equal(seg.rowflag, p_flag)
    assert torch.equal(seg.gscale, p_scale) and _entry_set(seg, rows)[1] == p_entries
    assert np.array_equal(U.decode_operand(seg, rows, K), U.expected_values(x, 6))


@pytest.mark.parametrize("K", [1024, 4096])
def test_relu_in_front(K):
    import torch
    from mi355q import ops
    x = U.element_layout(K)
    rows = x.shape[0]
    got = ops.block_fp_quantize_aligned_rows(_dev(x), 6, 8, 127, pre=("relu", None))
    torch.cuda.synchronize()
    assert np.array_equal(U.decode_operand(got, rows, K), U.expected_values(x * (x > 0), 6))


def test_column_classes():
    import torch
    from mi355q import ops
    K = 1024
    x = U.element_layout(K)
    rows = x.shape[0]
    cls = ops.ColumnClasses(K, range(0, K // 16, 8), torch.device("cuda:0"))
    x0, x1 = ops.block_fp_quantize_classes(_dev(x), cls, 6, 8, 127)
    torch.cuda.synchronize()
    exp = U.expected_values(x, 6)
    cols0, cols1 = cls.cols0.cpu().numpy(), cls.cols1.cpu().numpy()
    assert np.array_equal(U.decode_operand(x0, rows, cls.K0), exp[:, cols0])
    eye = ops.bf16_tile(torch.eye(cls.K1, device="cuda:0"))
    y1 = ops.bf16_gemm_tiled(x1, eye, rows, cls.K1, cls.K1)
    torch.cuda.synchronize()
    assert np.array_equal(y1.cpu().numpy(), exp[:, cols1].astype(np.float32))


@pytest.mark.parametrize("width", U.MX_WIDTHS)
@pytest.mark.parametrize("K", sorted(U.MX_ROWS))
def test_mx_operand(K, width):
    """the quantiser cannot produce an identity (a block whose maximum is a power of two saturates its mantissa): the
    weights are 0.75 I, which it represents exactly (mantissa 6 of 8 / 12 of 16), and the product is 0.75 x the expected
    value -- one non-zero term per output, exact in fp32"""
    import torch
    from mi355q import ops
    x = U.mx_layout(K)
    w = torch.eye(K, device="cuda:0") * 0.75
    wq = ops.block_fp_quantize(w, width, 8, 127, [1, 16], False)
    assert torch.equal(wq, w)
    wop = ops.block_fp_quantize_mx(w, width, 8, 127, reuse=False)
    xop = ops.block_fp_quantize_mx(_dev(x), width, 8, 127)
    y = ops.mx_gemm(xop, wop, wq)
    torch.cuda.synchronize()
    assert int(xop.bad[0]) == 0 and int(wop.bad[0]) == 0, "every 32-group of this layout fits one scale"
    exp = 0.75 * U.expected_values(x, width)
    assert np.array_equal(exp.astype(np.float32).astype(np.float64), exp)
    assert np.array_equal(y.cpu().numpy(), exp.astype(np.float32))
