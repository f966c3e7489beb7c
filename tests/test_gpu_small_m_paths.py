"""Every kernel path of the small-batch product on packed weights (ops.bfp_linear_packed_small, csrc/mi355q_gemv.hip:
bfp_gemv_packed_kernel<W, FAST>, gv_chunk<W, FAST, MASKED>) against oracle.np_oracle.bfp_linear_int, at the smallest K that reaches
each: the K lists below are held to the launch geometry by tests/test_small_m_host.py on the CPU.  Helpers, inputs and the 4e-6 bound
are those of tests/test_gpu_small_m.py.  Every comparison prints its figure before it asserts."""
import numpy as np
import pytest

from tests.test_gpu_small_m import DEV, TOL, _cfg, _check, _inputs, _pack, _quantise_w

pytestmark = pytest.mark.gpu

# fast path (K % 128 == 0): one partial chunk and one wave (128, 256, 384); a full chunk + a partial one (640); 16 waves (8192);
# 17 chunks = 2 a wave, 9 waves (8704); 33 chunks = 3 a wave, 11 waves, beyond the row format (16896)
FAST_K = (128, 256, 384, 640, 8192, 8704, 16896)
# halfword path (K % 128 == 64): the smallest K (64); a full chunk taken masked + a 4-block tail (576); a tail with one half-filled
# lane group (832); 9 chunks = 2 a wave, 5 waves (4160)
HALF_K = (64, 576, 832, 4160)
WIDTHS = (6, 4)                          # every K above
WIDTH_K = (384, 640, 832, 8192)          # ... and the other weight widths once at each of these
WIDTHS_ONCE = (2, 3, 5, 7, 8)
REPRODUCIBLE_K = (8192, 4160)
N_EDGE_K = 640
N_EDGES = (1, 15, 17, 200, 280)
N = 48
MS = (1, 3, 16)
MEASURED_ABOVE_K = 4096                  # the project's 4e-6 covers both resident routes up to here; above it the bound is measured


def _operands(K, wx, ww, n=N):
    """fp32 weights and bias, the oracle's outputs with and without bias (16 rows), the flavours that exist at K as PackedWeights"""
    import torch
    from oracle import np_oracle as O
    torch.manual_seed(1000 * ww + K + n)
    w = torch.randn(n, K) * 0.05
    b = torch.randn(n)
    x = _inputs(K, 3 * K + wx)
    cfg = _cfg(wx, ww)
    refs = {False: O.bfp_linear_int(x.numpy(), w.numpy(), None, cfg), True: O.bfp_linear_int(x.numpy(), w.numpy(), b.numpy(), cfg)}
    bq = torch.from_numpy(O.block_fp_quantize(b.numpy(), 6, 8, 127, [16], False)).to(DEV)
    return w, x, bq, refs


def _flavours(w, K, ww):
    from mi355q import ops
    packed = {"block": _pack(w.to(DEV), ww, "block")}
    if ops.row_align_supported(K):
        pw = _pack(w.to(DEV), ww, "row")
        if ww <= 6:
            assert pw is not None, f"K{K} W{ww}: these weights have no row flavour (pick another seed): the flavour may not be dropped"
        if pw is not None:
            packed["row"] = pw
    else:
        assert K > ops.ROW_ALIGN_MAX_K or K % 128, K
    return packed


def _parent_route(x, w, bq, wx, ww):
    """ops.bfp_gemm on the canonical int8 mantissas and exponents of the same operands: the existing route"""
    from mi355q import ops
    wm, we = _quantise_w(w.to(DEV), ww)
    _, xm, xe = ops.block_fp_quantize(x.to(DEV).contiguous(), wx, 8, 127, [1, 16], True, want_fake=False, want_packed=True)
    return ops.bfp_gemm(xm, xe, wm, we, bq, wx - 1, 127, ww - 1, 127).cpu().numpy().astype(np.float64)


def _run(K, wx, ww):
    from mi355q import ops
    w, x, bq, refs = _operands(K, wx, ww)
    packed = _flavours(w, K, ww)
    print(f"K{K} A{wx}W{ww} flavours:", sorted(packed))
    for has_bias in (False, True):
        ref = refs[has_bias]
        scale = float(np.abs(ref).max())
        for M in MS:
            tol = TOL
            if K > MEASURED_ABOVE_K:
                # no project figure at this K: the existing route's own error against the fp64 oracle, measured here; the new route may
                # differ from it by its fp32 summation order only -> twice that, floor 4e-6 of max|ref|
                e_old = float(np.abs(_parent_route(x[:M], w, bq if has_bias else None, wx, ww) - ref[:M]).max())
                tol = max(2 * e_old, TOL * float(np.abs(ref[:M]).max())) / float(np.abs(ref[:M]).max())
                print(f"K{K} A{wx}W{ww} M{M} bias={has_bias}: parent route max|err| {e_old:.3e} ({e_old / scale:.3e} of max|ref|)")
            for f, pw in packed.items():
                y = ops.bfp_linear_packed_small(x[:M].to(DEV), pw, wx, 8, 127, bias=bq if has_bias else None)
                assert y.shape == (M, N)
                _check(y, ref[:M], f"K{K} A{wx}W{ww} M{M} {f} bias={has_bias}", tol=tol)


@pytest.mark.parametrize("ww", WIDTHS)
@pytest.mark.parametrize("K", FAST_K + HALF_K)
def test_every_path_against_the_oracle(K, ww):
    """N = 48, M in {1, 3, 16}, bias on and off, both flavours wherever the row format takes K (16896 > ROW_ALIGN_MAX_K and the
    halfword K: per-block only); for widths <= 6 the row flavour must exist.  K <= 4096: 4e-6 of max|ref|.  K > 4096: twice the error
    of ops.bfp_gemm on the same operands against the oracle, measured in the test, floor 4e-6 of max|ref|.
    Both figures are printed for every case.  Measured on an MI355X: parent route 0.0 and new route 0.0 at K = 4160, 8192, 8704 and
    16896, every width -- both return the oracle's fp32 result bit for bit on these inputs, so the bound is its floor
    (profiles/small_m_packed.jsonl, the "accuracy" records)."""
    _run(K, 6, ww)


@pytest.mark.parametrize("ww", WIDTHS_ONCE)
@pytest.mark.parametrize("K", WIDTH_K)
def test_every_weight_width_on_every_path(K, ww):
    """gv_field<W> takes fields across dword boundaries differently for every W: widths 2, 3, 5, 7, 8 (4 and 6 run above) on a
    partial fast chunk (384), full + partial (640), the halfword path (832) and 16 waves (8192).  Widths 7 and 8 leave too little
    room to shift onto a row exponent, so their row flavour exists only where the packer says so."""
    _run(K, 6, ww)


def test_eight_bit_activations():
    _run(640, 8, 6)


def _plant(w, rows, K):
    """blocks far above and far below their row's window in the given rows (tests/test_gpu_small_m.py's exception test)"""
    wv = w.view(w.shape[0], K // 16, 16)
    for i, r in enumerate(rows):
        wv[r, (3 + 5 * i) % (K // 16)] *= 2.0 ** 10
        wv[r, (17 + 3 * i) % (K // 16)] *= 2.0 ** 11
        wv[r, (30 + i) % (K // 16)] *= 2.0 ** -12
    return w


@pytest.mark.parametrize("n", N_EDGES)
def test_n_edges(n):
    """K = 640 (fast path), N in {1, 15, 17, 200, 280}: fewer rows than a tile, a partial last tile (n = min(n0 + r, N - 1), the
    col >= N skip), and at 280 a second 256-row bucket of 24 rows whose last tile is partial.  The row flavour carries exception blocks
    (code 0xFF, added back from the bucketed list) in rows of the partial last tile and -- at 280 -- of the second bucket.  The
    output is a column slice of a wider 16-row buffer filled with a sentinel: the columns beside it and the rows behind M stay."""
    import torch
    from mi355q import ops
    from oracle import np_oracle as O
    K, wx, ww, S = N_EDGE_K, 6, 6, 12345.0
    torch.manual_seed(77 + n)
    last_tile = list(range((n - 1) // 16 * 16, n))
    rows = sorted(set([0, n // 2] + last_tile[-3:] + ([256, 259] if n > 256 else [])))
    w = _plant(torch.randn(n, K) * 0.05, rows, K)
    b = torch.randn(n)
    x = _inputs(K, 5 * n)
    cfg = _cfg(wx, ww)
    refs = {False: O.bfp_linear_int(x.numpy(), w.numpy(), None, cfg), True: O.bfp_linear_int(x.numpy(), w.numpy(), b.numpy(), cfg)}
    bq = torch.from_numpy(O.block_fp_quantize(b.numpy(), 6, 8, 127, [16], False)).to(DEV)
    packed = {f: _pack(w.to(DEV), ww, f) for f in ("block", "row")}
    pw = packed["row"]
    assert pw is not None and pw.row_scale_flavour, "the row flavour must exist here"
    exc = (pw.codes.view(n, K // 16) == 255).any(1).cpu()
    print(f"N{n}: exception blocks {int((pw.codes == 255).sum())} in rows {exc.nonzero().flatten().tolist()}")
    assert bool((pw.codes == 255).any()), "no exception block: the test would pass vacuously"
    assert bool(exc[last_tile].any()), "no exception block in the partial last tile"
    if n > 256:
        assert bool(exc[256:].any()) and bool(exc[:256].any()), "both buckets must hold entries"
    for f, p in packed.items():
        for has_bias in (False, True):
            for M in MS:
                wide = torch.full((16, n + 112), S, device=DEV)
                got = ops.bfp_linear_packed_small(x[:M].to(DEV), p, wx, 8, 127, bias=bq if has_bias else None, out=wide[:M, 48:48 + n])
                assert got.shape == (M, n) and got.data_ptr() == wide[:, 48:].data_ptr()
                _check(wide[:M, 48:48 + n], refs[has_bias][:M], f"N{n} K{K} M{M} {f} bias={has_bias}")
                assert bool((wide[:, :48] == S).all()) and bool((wide[:, 48 + n:] == S).all()), "neighbouring columns were written"
                assert bool((wide[M:] == S).all()), "rows behind M were written"
    # without the add-back the row flavour misses the bound by orders of magnitude (the checks above are not vacuous)
    lame = ops.PackedWeights(pw.packed, pw.codes, n, K, ww, 127, rowflag=pw.rowflag, rowscale=pw.rowscale, rowexp=pw.rowexp,
                             sparse=torch.zeros_like(pw.sparse))
    y0 = ops.bfp_linear_packed_small(x.to(DEV), lame, wx, 8, 127)
    assert float(np.abs(y0.cpu().numpy() - refs[False]).max()) > 100 * TOL * float(np.abs(refs[False]).max())


@pytest.mark.parametrize("K", REPRODUCIBLE_K)
def test_wave_reductions_are_reproducible(K):
    """two calls on the same inputs give the same bits where 16 fast-path waves (K = 8192) and 5 halfword-path waves (K = 4160)
    meet in LDS"""
    import torch
    from mi355q import ops
    torch.manual_seed(K)
    w = (torch.randn(N, K) * 0.05).to(DEV)
    x = _inputs(K, 1).to(DEV)
    for f, pw in _flavours(w.cpu(), K, 6).items():
        y1 = ops.bfp_linear_packed_small(x, pw, 6, 8, 127).clone()
        junk = torch.randn(2048, 2048, device=DEV) @ torch.randn(2048, 64, device=DEV)        # other work in between
        y2 = ops.bfp_linear_packed_small(x, pw, 6, 8, 127)
        assert torch.equal(y1, y2) and junk is not None, f"K{K} {f}: two runs differ"
        assert float(y1.abs().max()) > 0
