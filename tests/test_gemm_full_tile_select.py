"""CPU tests of which launches take the full-tile unit of the 256 x 256 tile GEMM (csrc/mi355q_gemm_v9_full.h), through the
diagnostic hook mi355q_debug_v9_full: the planner's plan for the shape, then the launcher's predicate.  The unit's kernel has
no row or column test, no group select, no split-K and no debug bits -- a launch that needs any of them must never reach it.
The table below is written out by hand from that rule; the hook has to agree with every row."""
import ctypes as C

import pytest

from tests.test_gemm_plan import env_words


@pytest.fixture(scope="module")
def hook():
    from mi355q import _lib
    fn = C.CDLL(str(_lib.library_path())).mi355q_debug_v9_full
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int64)]

    def full(M, N, K, *, env=None, ngroup=0, lists=1, flags=1, bf16=0, resid=0, x_post=0, dbg=0, aligned=1, switch=1, ldy=None, workspace_ok=1):
        shape = (C.c_int64 * 8)(M, N, K, ngroup, lists, flags, 1, bf16)
        fl = (C.c_int64 * 6)(resid, x_post, dbg, aligned, switch, N if ldy is None else ldy)
        return fn(shape, (C.c_int32 * 13)(*env_words(env or {})), workspace_ok, fl)
    return full


ROWS256 = {"MI355Q_V8_TILE_ROWS": "256"}          # (small shapes: pins the 256-row tile, as the GPU tests do)
# (expected, M, N, K, keyword arguments)
TABLE = [
    # the headline step and the aligned Linears: full tiles on the 256 x 256 kernel
    (1, 4096, 4096, 4096, {}),
    (1, 4096, 11008, 4096, {}),
    (1, 8192, 4096, 11008 // 128 * 128, {}),
    (1, 256, 256, 256, dict(env=ROWS256)),
    (1, 512, 512, 1024, dict(env=ROWS256)),
    (1, 4096, 4096, 4096, dict(ldy=4100)),
    # a ragged last tile row or column: the general kernel (its descriptors and stores know the edge)
    (0, 384, 256, 512, dict(env=ROWS256)),
    (0, 256, 384, 512, dict(env=ROWS256)),
    (0, 4096 + 128, 4096, 4096, {}),
    (0, 4096, 4096 - 16, 4096, {}),
    (0, 4097, 4096, 4096, {}),
    # grouped operands, a residual, the row post-pass, debug bits, an unaligned y, the switch
    (0, 4096, 4096, 4096, dict(ngroup=2)),
    (0, 4096, 4096, 4096, dict(ngroup=3)),
    (1, 4096, 4096, 4096, dict(ngroup=1)),
    (0, 4096, 4096, 4096, dict(resid=1)),
    (0, 4096, 4096, 4096, dict(x_post=1)),
    (0, 4096, 4096, 4096, dict(dbg=16)),
    (0, 4096, 4096, 4096, dict(env={"MI355Q_V9_DBG": "2"}, dbg=2)),
    (0, 4096, 4096, 4096, dict(aligned=0)),
    (0, 4096, 4096, 4096, dict(switch=0)),
    (0, 4096, 4096, 4096, dict(ldy=2 ** 31)),
    # no lists (the list-less kernel), the bf16 flavour
    (0, 4096, 4096, 4096, dict(lists=0, flags=0)),
    (0, 4096, 4096, 8192, dict(bf16=1, lists=0, flags=0)),
    # split-K: 64 tiles x 2 slices of 32 K-steps on the 256 x 256 kernel -- split; unsplit without a workspace
    (0, 2048, 2048, 4096, dict(env=ROWS256)),
    (1, 2048, 2048, 4096, dict(env=ROWS256, workspace_ok=0)),
    # other kernel families: the small tiles by default at <= 128 tiles, two K-steps, K % 128 == 64, MI355Q_V9=0, the v8 diagnostics
    (0, 2048, 2048, 4096, {}),
    (0, 256, 256, 128, dict(env=ROWS256)),
    (0, 4096, 4096, 4096 + 64, {}),
    (0, 4096, 4096, 4096, dict(env={"MI355Q_V9": "0"})),
    (0, 4096, 4096, 4096, dict(env={"MI355Q_V9_FIX": "0"})),
    (0, 4096, 4096, 4096, dict(env={"MI355Q_V8_STAMPS": "1"})),
    (0, 2048, 2048, 4096, dict(env={"MI355Q_V10_AUTO": "0"})),      # (64 tiles of 256 rows cost more than 128 of 128: the 128-row tile)
]


@pytest.mark.parametrize("row", TABLE, ids=[f"{r[1]}x{r[2]}x{r[3]}-{'-'.join(f'{k}={v}' for k, v in r[4].items()) or 'plain'}" for r in TABLE])
def test_selection_agrees_with_the_table(hook, row):
    want, M, N, K, kw = row
    assert hook(M, N, K, **kw) == want


def test_a_ragged_or_grouped_launch_never_reaches_the_unit(hook):
    """every M, N around the tile size in steps of 16, one to three weight operands: the unit only where both are multiples of 256 and one group"""
    for M in range(16, 1041, 16):
        for N in (256, 496, 512, 528, 768):
            for ngroup in (0, 1, 2, 3):
                got = hook(M, N, 1024, env=ROWS256, ngroup=ngroup)
                assert got == int(M % 256 == 0 and N % 256 == 0 and ngroup <= 1), (M, N, ngroup)
