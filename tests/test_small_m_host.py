"""The small-batch product on width-bit packed weights (mi355q_bfp_gemm_packed_small, ABI 25): what can be checked
without a GPU -- the symbol, its binding and its argument checks (every call below is rejected, or empty, before it
reaches the device)."""
import ctypes as C
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
E_BADARG, E_UNSUPPORTED, E_ALIGN = -1, -2, -3


def test_entry_point_is_exported_and_bound():
    from mi355q import _lib
    header = (ROOT / "include" / "mi355q.h").read_text()
    assert re.search(r"\bmi355q_bfp_gemm_packed_small\s*\(", header)
    assert "mi355q_bfp_gemm_packed_small" in _lib.SIGNATURES
    lib = C.CDLL(str(_lib.library_path()))
    assert hasattr(lib, "mi355q_bfp_gemm_packed_small")
    assert _lib.ABI_VERSION == 25 and _lib.load_library().mi355q_abi_version() == 25
    assert "quantized_modules/linear.py:59-76" in header[header.index("small-batch product on the at-rest form"):][:600]


def _call(lib, *, x=True, packed=True, codes=True, row_exp=False, lst=False, bias=False, y=True, M=4, N=48, K=128, ldy=None,
          x_mbits=5, w_mbits=5, off=0, buf=None):
    p = C.addressof(buf) + off
    return lib.mi355q_bfp_gemm_packed_small(p if x else None, p if packed else None, p if codes else None, p if row_exp else None,
                                            p if lst else None, 0, p if bias else None, p if y else None, M, N, K,
                                            N if ldy is None else ldy, x_mbits, 127, w_mbits, 127, None)


def test_argument_checks_without_a_gpu():
    from mi355q import _lib
    lib = _lib.load_library()
    raw = C.create_string_buffer(256)
    buf = (C.c_char * 64).from_address((C.addressof(raw) + 63) // 64 * 64)       # 64-byte aligned
    call = lambda **kw: _call(lib, buf=buf, **kw)
    assert call(M=17) == E_UNSUPPORTED
    assert call(K=96) == E_UNSUPPORTED
    assert call(K=48) == E_UNSUPPORTED
    assert call(w_mbits=8) == E_BADARG                       # width 9
    assert call(w_mbits=0) == E_BADARG                       # width 1
    assert call(x_mbits=8) == E_BADARG
    assert call(ldy=47) == E_BADARG
    assert call(M=-1) == E_BADARG
    for missing in ("x", "packed", "codes", "y"):
        assert call(**{missing: False}) == E_BADARG
    assert call(row_exp=True, lst=False) == E_BADARG         # the row flavour needs its exception list
    assert call(M=0) == 0 and call(N=0) == 0                 # empty: success, nothing launched
    assert call(M=0, x=False, y=False) == 0
    assert call(off=8) == E_ALIGN                            # x_tiled / packed want 16 bytes
    assert call(off=2) == E_ALIGN


def test_ops_constants_and_module_key_default():
    from mi355q import ops
    assert ops.SMALL_M_MAX == 16
    assert callable(ops.bfp_linear_packed_small) and ops.small_m_calls() >= 0
    import torch
    import mi355q.quantize as Q
    cfg = dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
               data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127,
               weight_block_size=[1, 16], bias_width=6, bias_exponent_width=8, bias_exponent_bias=127, bias_block_size=[16])
    lin = Q.get_quantized_cls("linear", cfg)(64, 32, bias=True, config=cfg)
    assert not lin._small_m_takes(torch.zeros(1, 64))        # key absent: off
    lin2 = Q.get_quantized_cls("linear", dict(cfg, mi355q_small_m="packed"))(64, 32, bias=True, config=dict(cfg, mi355q_small_m="packed"))
    assert not lin2._small_m_takes(torch.zeros(1, 64))       # nothing packed: the old routes


# ---- the launch geometry of launch_bfp_gemm_packed_small (csrc/mi355q_gemv.hip), restated -----------------------------------------
GEMV_MAX_WAVES, GEMV_MAX_WAVES_SLOW, GEMV_CHUNK_BLOCKS = 16, 8, 32


def geometry(K: int):
    """K -> (fast, nchunks, chunks_per_wave, waves, last chunk partial): chunks of 512 values, K % 128 == 0 the fast path with up
    to 16 waves, other K % 64 == 0 the halfword path with up to 8"""
    assert K > 0 and K % 64 == 0
    nkb = K // 16
    nchunks = -(-nkb // GEMV_CHUNK_BLOCKS)
    fast = K % 128 == 0
    max_waves = GEMV_MAX_WAVES if fast else GEMV_MAX_WAVES_SLOW
    cpw = -(-nchunks // max_waves)
    return fast, nchunks, cpw, -(-nchunks // cpw), nkb % GEMV_CHUNK_BLOCKS != 0


def test_restated_geometry_reads_the_sources_constants():
    src = (ROOT / "llm-mixed-q_amd" / "csrc" / "mi355q_gemv.hip").read_text()
    for name, value in (("GEMV_MAX_WAVES", GEMV_MAX_WAVES), ("GEMV_MAX_WAVES_SLOW", GEMV_MAX_WAVES_SLOW), ("GEMV_CHUNK_BLOCKS", GEMV_CHUNK_BLOCKS)):
        assert re.search(rf"constexpr int {name} = {value};", src), name
    assert geometry(4096) == (True, 8, 1, 8, False) and geometry(11008) == (True, 22, 2, 11, True)      # (what the older tests reach)
    assert geometry(320) == (False, 1, 1, 1, True)
    assert geometry(8192) == (True, 16, 1, 16, False) and geometry(8704) == (True, 17, 2, 9, False)
    assert geometry(16896) == (True, 33, 3, 11, False) and geometry(4160) == (False, 9, 2, 5, True)


def test_the_gpu_path_tables_k_list_hits_every_geometry_class():
    """every class of tests/test_gpu_small_m_paths.py's table, from its K lists: an edit of a list that empties a class fails here,
    on the CPU"""
    from tests import test_gpu_small_m_paths as P
    from mi355q import ops
    fast = [geometry(K) for K in P.FAST_K]
    slow = [geometry(K) for K in P.HALF_K]
    assert all(g[0] for g in fast) and not any(g[0] for g in slow), "a K on the wrong path's list"
    classes = {
        "fast: one partial chunk, one wave": any(g[1:] == (1, 1, 1, True) for g in fast),
        "fast: full chunk(s) then a partial one": any(g[1] > 1 and g[4] for g in fast),
        "fast: 16 waves, one chunk each": any(g[2:4] == (1, 16) for g in fast),
        "fast: two chunks a wave": any(g[2] == 2 for g in fast),
        "fast: three or more chunks a wave": any(g[2] >= 3 for g in fast),
        "fast: a last wave with fewer chunks than the others": any(g[1] % g[2] for g in fast),
        "halfword: the smallest K": 64 in P.HALF_K,
        "halfword: a full chunk taken masked": any(g[1] > 1 for g in slow),
        "halfword: a tail with a half-filled lane group": any((K // 16) % 32 % 8 == 4 for K in P.HALF_K),
        "halfword: several waves, more than one chunk each": any(g[2] > 1 and g[3] > 1 for g in slow),
        "a K beyond the row format (per-block flavour only)": any(not ops.row_align_supported(K) for K in P.FAST_K),
    }
    assert all(classes.values()), [k for k, v in classes.items() if not v]
    assert set(P.WIDTH_K) <= set(P.FAST_K) | set(P.HALF_K) and any(geometry(K)[2:4] == (1, 16) for K in P.WIDTH_K)
    assert any(not geometry(K)[0] for K in P.WIDTH_K) and set(P.WIDTHS_ONCE) | set(P.WIDTHS) == set(range(2, 9))
    for K in P.REPRODUCIBLE_K:                               # the two wave reductions: 16 fast waves, several halfword waves
        assert geometry(K)[3] > 1
    assert {geometry(K)[0] for K in P.REPRODUCIBLE_K} == {True, False} and any(geometry(K)[3] == 16 for K in P.REPRODUCIBLE_K)
    assert geometry(P.N_EDGE_K)[0] and P.N_EDGE_K <= 4096 and ops.row_align_supported(P.N_EDGE_K)
    assert any(N < 16 for N in P.N_EDGES) and any(N % 16 and N > 256 for N in P.N_EDGES) and any(N % 16 and 16 < N < 256 for N in P.N_EDGES)
