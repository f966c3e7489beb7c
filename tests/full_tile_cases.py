"""The cases of tests/test_gpu_gemm_full_tile.py and the child interpreter that runs them: the switch MI355Q_V9_FULL is read
once per process, so each setting of it gets a fresh interpreter.

    python tests/full_tile_cases.py <out.npz>        (MI355Q_V9_FULL and MI355Q_V8_TILE_ROWS=256 set by the caller)

Every case is one product y = x . w^T (+ bias) on row-aligned W6A6 operands; the exception entries all lie in the LAST tile
(bottom right) so that the other tiles of the larger shapes have none.  Written out per case: y without and with bias, the
overflow words, the numbers of x / w entries in the last tile's buckets, and how many launches took the full-tile unit."""
import sys
from pathlib import Path

import numpy as np

SHAPES = [(256, 256), (512, 256), (256, 512), (512, 512)]
KS = [128, 256, 384, 768]                # 128: two K-steps (the planner keeps it off the 256 x 256 kernel); 256: the loop ends inside the ring's fill
VARIANTS = ["none", "x_only", "w_only", "several_per_row", "slow_vectors", "overflow"]
V9_FAST_MAX = 33                         # vectors beside the rings (csrc/mi355q_gemm_v9.hip); the slow ones lie in the ring area
ROW_BUCKET_CAP = 120


def case_id(M, N, K, variant):
    return f"{M}x{N}x{K}-{variant}"


def operands(M, N, K, variant):
    """fp32 x [M, K], w [N, K], bias [N]; exception blocks = single 16-value blocks scaled by 2^6 against their row"""
    r = np.random.default_rng(1000 * M + 10 * N + K + len(variant))
    # (magnitudes within a factor of two along a row: every block's exponent lies in its row's window, so the only entries are
    #  the ones made below -- normal values now and then give a block of 16 small ones, an entry nobody asked for)
    def values(rows):
        return r.uniform(0.5, 1.0, size=(rows, K)) * r.choice([-1.0, 1.0], size=(rows, K))
    x = (values(M) * np.exp(0.5 * r.normal(size=(M, 1)))).astype(np.float32)
    w = (values(N) * 0.02 * np.exp(0.25 * r.normal(size=(N, 1)))).astype(np.float32)
    b = (r.normal(size=(N,)) * 0.02).astype(np.float32)
    nblk, m0, n0 = K // 16, M - 256, N - 256

    def up(t, row, blk):
        t[row, 16 * blk:16 * blk + 16] *= 64.0

    if variant == "x_only":
        for i, row in enumerate((m0 + 3, m0 + 130, M - 1)):
            up(x, row, (2 + 3 * i) % nblk)
    elif variant == "w_only":
        for i, row in enumerate((n0, n0 + 77, N - 1)):
            up(w, row, (1 + 3 * i) % nblk)
    elif variant == "several_per_row":
        for blk in (5, 1, 3):                                   # one x row with three entries, listed in no block order
            up(x, m0 + 40, blk)
        for blk in (6, 3):                                      # one w row with two, one of them at an x entry's K position
            up(w, n0 + 200, blk)
        up(x, M - 1, 7)
        up(w, N - 1, 7)                                         # exception x exception at block 7
    elif variant == "slow_vectors":
        for i in range(20):                                     # 40 entries: more than V9_FAST_MAX vectors, every row its own
            up(x, m0 + 5 + 12 * i, i % nblk)
            up(w, n0 + 9 + 12 * i, (i + 3) % nblk)
    elif variant == "overflow":
        for i in range(ROW_BUCKET_CAP + 5):                     # one bucket of x takes 125 entries: it overflows
            up(x, m0 + 2 * i, i % nblk)
    else:
        assert variant == "none"
    return x, w, b


def main(out_path):
    import ctypes as C
    import torch
    from mi355q import _lib, ops
    dev = torch.device("cuda:0")
    count = C.CDLL(str(_lib.library_path())).mi355q_debug_v9_full_count
    count.restype = C.c_longlong
    out = {}
    for M, N in SHAPES:
        for K in KS:
            for variant in VARIANTS:
                x, w, b = operands(M, N, K, variant)
                xa = ops.block_fp_quantize_aligned_rows(torch.from_numpy(x).to(dev), 6, 8, 127)
                _, wm, we = ops.block_fp_quantize(torch.from_numpy(w).to(dev), 6, 8, 127, [1, 16], False, want_fake=False, want_packed=True)
                wa = ops.bfp_align_rows(wm, we, 5, 127)
                bq = ops.block_fp_quantize(torch.from_numpy(b).to(dev), 6, 8, 127, [16], False)
                before = count()
                y0 = ops.bfp_gemm_aligned(xa, wa, None)
                y1 = ops.bfp_gemm_aligned(xa, wa, bq)
                torch.cuda.synchronize()
                ovx, ex = ops.row_list_entries(xa.sparse, M)
                ovw, ew = ops.row_list_entries(wa.sparse, N)
                key = case_id(M, N, K, variant)
                out[key + "/y0"] = y0.cpu().numpy()
                out[key + "/y1"] = y1.cpu().numpy()
                out[key + "/info"] = np.array([ovx, ovw, int((ex[:, 0] >= M - 256).sum()), int((ew[:, 0] >= N - 256).sum()), len(ex), len(ew),
                                               count() - before], dtype=np.int64)
    np.savez(out_path, **out)


if __name__ == "__main__":
    root = Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(root / "llm-mixed-q_amd"), str(root)]
    main(sys.argv[1])
