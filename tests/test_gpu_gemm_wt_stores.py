"""The 256 x 256 tile GEMM that ships stores y write-through (sc1) in its one-pass epilogue; the residual unit of the same
kernel keeps plain stores.  With a zero residual the two must give the same bytes: the store flavour changes when a line
leaves the L2, never what is written.  Shapes: the smallest the 256-row tile takes with exception entries on both sides, a
ragged last tile column (the scalar tail stores beside the 16-byte ones), and an output whose row stride is no multiple of
16 bytes (every store scalar).  Bound against the oracle: 1e-5 of the output scale, as smoke() holds the same product to."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG6 = dict(name="block_fp", data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
            data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127,
            weight_block_size=[1, 16], bias_width=6, bias_exponent_width=8, bias_exponent_bias=127,
            bias_block_size=[16])


def _operands(M, N, K, seed):
    import torch
    from mi355q import ops
    r = np.random.default_rng(seed)
    x = (r.normal(size=(M, K)) * np.exp(r.normal(size=(M, 1)))).astype(np.float32)
    w = (r.normal(size=(N, K)) * 0.02).astype(np.float32)
    b = (r.normal(size=(N,)) * 0.02).astype(np.float32)
    # exception blocks on both sides (single 16-value blocks scaled by 2^+-6), two of them meeting at one K position;
    # one w row with three entries, one entry in the last valid w row
    x[3, 32:48] *= 64.0
    x[M - 1, 256:272] *= 64.0
    x[130, 256:272] /= 64.0
    for blk in (20, 3, 11):
        w[N - 200, 16 * blk:16 * blk + 16] *= 64.0
    w[N - 1, 256:272] *= 64.0
    w[N - 77, 48:64] /= 64.0
    dev = torch.device("cuda:0")
    xa = ops.block_fp_quantize_aligned_rows(torch.from_numpy(x).to(dev), 6, 8, 127)
    _, wm, we = ops.block_fp_quantize(torch.from_numpy(w).to(dev), 6, 8, 127, [1, 16], False, want_fake=False, want_packed=True)
    wa = ops.bfp_align_rows(wm, we, 5, 127)
    bq = ops.block_fp_quantize(torch.from_numpy(b).to(dev), 6, 8, 127, [16], False)
    assert int(xa.sparse[0]) == 0 and int(wa.sparse[0]) == 0            # no bucket overflowed: the tile serves the lists itself
    return x, w, b, xa, wa, bq


@pytest.mark.parametrize("M,N,K", [(256, 512, 512), (512, 500, 1024)])
def test_write_through_stores_equal_plain_stores_and_the_oracle(M, N, K, monkeypatch):
    import torch
    from mi355q import ops
    from oracle import np_oracle as O
    monkeypatch.setenv("MI355Q_V8_TILE_ROWS", "256")                   # the 256 x 256 tile at these small shapes
    x, w, b, xa, wa, bq = _operands(M, N, K, 71 + N)
    dev = xa.tiled.device
    y = ops.bfp_gemm_aligned(xa, wa, bq)
    y_plain = ops.bfp_gemm_aligned(xa, wa, bq, residual=torch.zeros(M, N, device=dev))
    # a row stride of N + 1 floats: no 16-byte store applies, every value leaves by the scalar tail stores
    wide = torch.full((M, N + 1), float("nan"), device=dev)
    y_scalar = ops.bfp_gemm_aligned(xa, wa, bq, out=wide[:, :N])
    torch.cuda.synchronize()
    assert torch.equal(y, y_plain), "write-through and plain stores wrote different bytes"
    assert torch.equal(y, y_scalar), "16-byte and scalar stores wrote different bytes"
    assert torch.isnan(wide[:, N]).all(), "a store went past its row"
    ref = O.bfp_linear_int(x, w, b, CFG6)
    err = np.abs(y.cpu().numpy() - ref).max() / np.abs(ref).max()
    print(f"M {M} N {N} K {K}: rel err {err:.3e}")
    assert err < 1e-5
