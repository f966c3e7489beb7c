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
