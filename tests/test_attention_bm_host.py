"""Host side of the one-pass block_minifloat attention (ops.bm_attention): the check function against a table, the registry entry, the
routing of the registry function and of the harness models with the op replaced by a counting stand-in, and the C export's return codes.
Nothing here needs a GPU: block_minifloat has no CPU quantiser, so where the steps run on CPU tensors ops.block_minifloat_quantize is
replaced by the identity (routing is what is tested, not values)."""
import ctypes
import inspect
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import attn_bm_util as U  # noqa: E402
import mi355q.quantize as Q  # noqa: E402
from mi355q import _lib, harness as H, ops  # noqa: E402
from mi355q.quantize import quantized_functions as QF  # noqa: E402

P8 = U.par(U.F848)


# (what is changed from the call of _call -> a word of the reason).  The check touches no device and the device's reason comes last, so
# on CPU tensors "MI355X" is the reason of a call that passes everything else.
Z = lambda *s: torch.zeros(*s)
REFUSED = [
    (dict(q="not a tensor"), "tensors"),
    (dict(q=Z(48, 64)), "leading dims"),
    (dict(k=Z(2, 48, 32), v=Z(2, 48, 32)), "leading dims"),
    (dict(v=Z(2, 32, 64)), "leading dims"),
    (dict(q=Z(3, 48, 64)), "leading dims"),
    (dict(q=Z(2, 48, 64).double()), "fp32"),
    (dict(q=Z(2, 49, 64), causal=True), "causal with T_q = 49 > T_k = 48"),
    (dict(q=Z(0, 48, 64), k=Z(0, 48, 64), v=Z(0, 48, 64)), "rows"),
    (dict(q=Z(2, 0, 64)), "no queries"),
    (dict(k=Z(2, 40, 64), v=Z(2, 40, 64)), "multiple of 16"),
    (dict(k=Z(2, 0, 64), v=Z(2, 0, 64)), "multiple of 16"),
    (dict(q=Z(2, 48, 160), k=Z(2, 48, 160), v=Z(2, 48, 160)), "head_dim 160"),
    (dict(q=Z(2, 48, 16), k=Z(2, 48, 16), v=Z(2, 48, 16)), "head_dim 16"),
    (dict(qk=(8, 4, 8)), "qk_params"),
    (dict(qk=(8, 0, 8, 8, 4, 8)), "exponent width 0"),
    (dict(qk=(8, 9, 8, 8, 4, 8)), "exponent width 9"),
    (dict(pv=(8, 4, 8, 13, 4, 8)), "8 mantissa bits"),
    (dict(pv=(5, 4, 8, 8, 4, 8)), "0 mantissa bits"),
    (dict(pv=(8, 4, 0, 8, 4, 8)), "bias width 0"),
    (dict(qk=(8, 4, 8, 8, 4, 9)), "bias width 9"),
    ({}, "MI355X"),
]
ACCEPTED = [
    dict(q=Z(1, 1, 32), k=Z(1, 16, 32), v=Z(1, 16, 32), causal=True),                       # M = 1, T = 16, D = 32
    dict(q=Z(1, 1, 128), k=Z(1, 16, 128), v=Z(1, 16, 128)),                                 # D = 128
    dict(q=Z(2, 3, 70, 96), k=Z(2, 3, 48, 96), v=Z(2, 3, 48, 96)),                          # more queries than keys, not causal; 4-d
    dict(q=Z(2, 48, 64), k=Z(2, 48, 64), v=Z(2, 48, 64), causal=True),                      # M = T causal
    dict(qk=(3, 1, 1, 3, 1, 1), pv=(3, 1, 1, 3, 1, 1)),                                     # the narrowest: 1 exponent bit, 1 mantissa bit
    dict(qk=(16, 8, 8, 16, 8, 8), pv=(16, 8, 8, 16, 8, 8)),                                 # the widest: 8 exponent bits, 7 mantissa bits
    dict(qk=(9, 1, 8, 3, 1, 1), pv=(10, 8, 1, 9, 1, 8)),                                    # the ends mixed, sides and products differing
]


def _call(kw):
    base = dict(q=Z(2, 48, 64), k=Z(2, 48, 64), v=Z(2, 48, 64), qk=P8, pv=P8, causal=False)
    base.update(kw)
    return (base["q"], base["k"], base["v"], base["qk"], base["pv"]), dict(causal=base["causal"])


@pytest.mark.parametrize("kw,word", REFUSED, ids=[w for _, w in REFUSED])
def test_check_refuses_with_the_reason(kw, word):
    a, k = _call(kw)
    why = ops._bm_attention_check(*a, k["causal"])
    assert why is not None and word in why, why
    assert not ops.bm_attention_supported(*a, **k)
    with pytest.raises(ValueError, match="mi355q.bm_attention: "):
        ops.bm_attention(*a, **k)


@pytest.mark.parametrize("kw", ACCEPTED)
def test_check_accepts_the_corners(kw):
    """every check but the device's passes on CPU tensors; the predicate is the check `is None`"""
    a, k = _call(kw)
    why = ops._bm_attention_check(*a, k["causal"])
    assert why is not None and "MI355X" in why, why

    class OnGpu(torch.Tensor):                                  # (the same tensors, claiming a GPU: nothing in the check touches a device)
        is_cuda = True
    a = tuple(t.as_subclass(OnGpu) if isinstance(t, torch.Tensor) else t for t in a)
    assert ops._bm_attention_check(*a, k["causal"]) is None and ops.bm_attention_supported(*a, **k)


def test_registry_entry():
    assert Q.QUANTIZED_FUNC_MAP["attention"]["block_minifloat"] is QF.attention_block_minifloat
    assert Q.get_quantized_func("attention", {"name": "block_minifloat"}) is QF.attention_block_minifloat
    assert Q.get_quantized_func("attention", {"name": "block_fp"}) is QF.attention_block_fp
    assert set(Q.QUANTIZED_FUNC_MAP["attention"]) == {"block_fp", "block_minifloat"}
    # tests/test_host_logic.py's pins: the top-level key set
    assert set(Q.QUANTIZED_FUNC_MAP) == {"matmul", "bmm", "rotary_positional_encoding", "softmax_matmul", "softmax_bmm", "attention"}
    assert inspect.signature(QF.attention_block_minifloat) == inspect.signature(QF.attention_block_fp)


@pytest.fixture
def op(monkeypatch):
    """ops.bm_attention replaced by a counting stand-in (plain attention in torch), its predicate by the check minus the device's reason,
    and the block_minifloat quantiser by the identity: the routing on CPU tensors"""
    calls = []

    def stand_in(q, k, v, qk_params, pv_params, *, causal=False, scale_div=None, q_scale=None):
        calls.append(dict(shape=tuple(q.shape), causal=causal, scale_div=scale_div, q_scale=q_scale, qk=tuple(qk_params), pv=tuple(pv_params)))
        w = (q * q_scale if q_scale else q) @ k.transpose(-1, -2)
        if scale_div:
            w = w / scale_div
        if causal:
            w = w + torch.full(w.shape[-2:], U.FMIN).triu(1 + w.shape[-1] - w.shape[-2])
        return torch.softmax(w, -1) @ v

    def supported(q, k, v, qk_params, pv_params, *, causal=False):
        why = ops._bm_attention_check(q, k, v, qk_params, pv_params, causal)
        return why is None or "MI355X" in why

    monkeypatch.setattr(ops, "bm_attention", stand_in)
    monkeypatch.setattr(ops, "bm_attention_supported", supported)
    monkeypatch.setattr(ops, "block_minifloat_quantize", lambda x, *a, **kw: x)
    return calls


def test_registry_routing(op):
    f = QF.attention_block_minifloat
    torch.manual_seed(0)
    q, k, v = torch.randn(2, 3, 32, 64), torch.randn(2, 3, 48, 64), torch.randn(2, 3, 48, 64)
    c = lambda **kw: U.cfg(U.F848, **kw)
    a = f(q, k, v, c(), U.cfg(U.F848, U.F634), causal=True, scale_div=8.0, q_scale=0.5)
    assert len(op) == 1 and op[0]["causal"] and op[0]["scale_div"] == 8.0 and op[0]["q_scale"] == 0.5
    assert op[0]["qk"] == U.par(U.F848) and op[0]["pv"] == U.par(U.F848, U.F634)
    # the steps give the stand-in's values here (identity quantiser): every refusal below must still compute the same thing
    for what, args, kw in (
            ("mi355q_fused_matmul off", (c(mi355q_fused_matmul=False), c()), {}),
            ("mi355q_fused_matmul off in the second product", (c(), c(mi355q_fused_matmul=False)), {}),
            ("a blocking that is not [1, 16]", (c(), dict(c(), data_in_block_size=[1, 32])), {}),
            ("a blocking that is not [1, 16]", (dict(c(), weight_block_size=[16, 1]), c()), {}),
            ("head_dim 48", (c(), c()), dict(q=q[..., :48], k=k[..., :48], v=v[..., :48])),
            ("T_k = 40", (c(), c()), dict(k=k[..., :40, :], v=v[..., :40, :]))):
        t = {**dict(q=q, k=k, v=v), **kw}
        n = len(op)
        got = f(t["q"], t["k"], t["v"], *args, causal=True, scale_div=8.0, q_scale=0.5)
        assert len(op) == n, what
        assert got.shape == t["q"].shape
    steps = f(q, k, v, c(mi355q_fused_matmul=False), c(), causal=True, scale_div=8.0, q_scale=0.5)
    assert torch.allclose(a, steps, atol=1e-5)
    # a mask or a key mask sends the call to the steps; the key mask as the dense mask it stands for
    n = len(op)
    km = torch.ones(2, 48, dtype=torch.int64)
    km[1, :5] = 0
    dense = torch.where(km != 0, 0.0, U.FMIN).reshape(2, 1, 1, 48).expand(2, 1, 32, 48).contiguous()
    by_mask = f(q, k, v, c(), c(), causal=True, mask=dense)
    by_key = f(q, k, v, c(), c(), causal=True, key_mask=km)
    assert len(op) == n and torch.equal(by_mask, by_key)
    with pytest.raises(ValueError, match="key_mask together with mask"):
        f(q, k, v, c(), c(), key_mask=km, mask=dense)
    # autograd, a bypassed product, two formats
    qg = q.clone().requires_grad_(True)
    assert f(qg, k, v, c(), c(), causal=True).requires_grad and len(op) == n
    f(q, k, v, dict(c(), bypass=True), c(), causal=True)
    assert len(op) == n
    # `consumer` is ignored: the fp32 tensor either way
    with torch.no_grad():
        o = f(q, k, v, c(), c(), causal=True, consumer=(6, 8, 127))
    assert len(op) == n + 1 and isinstance(o, torch.Tensor) and o.dtype == torch.float32


def test_attention_block_fp_keeps_its_tail(op):
    """attention_block_fp still serves a block_minifloat second product by the shared steps, never by the new op"""
    torch.manual_seed(1)
    q, k, v = torch.randn(2, 32, 64), torch.randn(2, 48, 64), torch.randn(2, 48, 64)
    a = QF.attention_block_fp(q, k, v, U.cfg(U.F848), U.cfg(U.F848), causal=True, scale_div=8.0)
    b = QF._attention_steps(q, k, v, U.cfg(U.F848), U.cfg(U.F848), None, True, 8.0, None, None)
    assert torch.equal(a, b) and not op


_ROPE = dict(name="integer", bypass=True, is_ptq=True, data_in_width=8, data_in_frac_width=4, weight_width=8, weight_frac_width=4,
             bias_width=8, bias_frac_width=4)
_FP = dict(name="block_fp", bypass=True, is_ptq=True, data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
           data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127, weight_block_size=[1, 16])


def _model(family, product, layers=2):
    """a tiny model with every Linear bypassed and `product` as its attention products' config"""
    torch.manual_seed(0)
    full = {"default": dict(product), "linear": dict(product, bypass=True), "model_layer": {"self_attn": {"rotary_positional_encoding": _ROPE}}}
    if family == "llama":
        cfg = H.TinyLlamaConfig(vocab_size=64, hidden_size=64, intermediate_size=128, num_layers=layers, num_heads=2, max_positions=48)
        return H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(full, layers)).eval()
    full.pop("model_layer")
    cfg = H.TinyOPTConfig(vocab_size=64, hidden_size=64, ffn_dim=128, num_layers=layers, num_heads=2, max_positions=48)
    return H.TinyOPTForCausalLM(cfg, H.expand_quant_config(full, layers)).eval()


@pytest.mark.parametrize("family", ["opt", "llama"])
def test_harness_routing(op, family):
    ids = torch.randint(0, 64, (2, 32), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        off = _model(family, U.cfg(U.F848))(ids)[0]
        assert not op, "knob absent: the harness never calls the op"
        off2 = _model(family, U.cfg(U.F848, mi355q_fused_attention=False))(ids)[0]
        assert not op and torch.equal(off, off2), "knob off: the harness never calls the op"
        on = _model(family, U.cfg(U.F848, mi355q_fused_attention=True))(ids)[0]
        assert len(op) == 2, "knob on: once a layer"
        assert all(c["causal"] and c["shape"] == (2, 2, 32, 32) for c in op)
        assert all((c["q_scale"], c["scale_div"]) == ((32 ** -0.5, None) if family == "opt" else (None, 32 ** 0.5)) for c in op)
        assert torch.allclose(on, off, atol=1e-4)
        # a padded batch (attention_mask -> key_mask) goes to the steps
        am = torch.ones(2, 32, dtype=torch.long)
        am[1, 20:] = 0
        _model(family, U.cfg(U.F848, mi355q_fused_attention=True))(ids, attention_mask=am)
        assert len(op) == 2
        # a block_fp model never calls it (bypassed products: no block_fp quantiser on the CPU either)
        _model(family, dict(_FP, mi355q_fused_attention=True))(ids)
        # one block_minifloat product beside a block_fp one: not this function's layer
        mixed = _model(family, U.cfg(U.F848, mi355q_fused_attention=True))
        for layer in mixed.layers:
            qc = layer.self_attn.qc
            qc["bmm_0" if family == "opt" else "matmul_0"] = dict(_FP)
        mixed(ids)
        assert len(op) == 2


def test_c_abi_return_codes():
    """mi355q_bm_attention refuses what it does not take before anything is launched (include/mi355q.h)"""
    lib = _lib.load_library()
    BAD, UNS, ALIGN = _lib.E_BADARG, _lib.E_UNSUPPORTED, _lib.E_ALIGN
    p = 1 << 20
    ok6 = (ctypes.c_int32 * 6)(8, 4, 8, 8, 4, 8)
    six = lambda *a: (ctypes.c_int32 * 6)(*a)
    A = ctypes.addressof

    def call(q=p, k=p, v=p, out=p, ws=p, B=2, M=48, T=48, D=64, qk=ok6, pv=ok6, strides=None, causal=1):
        return lib.mi355q_bm_attention(q, k, v, out, ws, B, M, T, D, A(qk) if qk is not None else None, A(pv) if pv is not None else None,
                                       A(strides) if strides is not None else None, causal, 8.0, 0.0, None)

    assert lib.mi355q_bm_attention_workspace_bytes(2, 48, 64) == 2 * (3 * 2 * 1024 + 2 * 4 * 1024) + 256
    assert lib.mi355q_bm_attention_workspace_bytes(0, 48, 64) == 0
    assert call(B=0) == 0 and call(M=0) == 0 and call(B=0, q=None) == 0               # nothing to do, nothing launched
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(ws=None), dict(qk=None), dict(pv=None), dict(B=-1), dict(M=-1),
               dict(T=-16), dict(D=-64), dict(T=0), dict(B=65536)):
        assert call(**kw) == BAD, kw
    for kw in (dict(T=40), dict(T=8), dict(D=16), dict(D=160), dict(D=48), dict(M=49), dict(qk=six(8, 0, 8, 8, 4, 8)), dict(qk=six(8, 9, 8, 8, 4, 8)),
               dict(pv=six(13, 4, 8, 8, 4, 8)), dict(pv=six(8, 4, 8, 5, 4, 8)), dict(qk=six(8, 4, 0, 8, 4, 8)), dict(pv=six(8, 4, 8, 8, 4, 9))):
        assert call(**kw) == UNS, kw
    assert call(M=49, causal=0, q=p + 4) == ALIGN                                    # (M > T is legal without the causal mask)
    for kw in (dict(q=p + 4), dict(k=p + 8), dict(v=p + 2), dict(out=p + 4), dict(ws=p + 8),
               dict(strides=(ctypes.c_int64 * 8)(48 * 64, 64, 48 * 64, 66, 48 * 64, 64, 48 * 64, 64))):
        assert call(**kw) == ALIGN, kw
    assert lib.mi355q_abi_version() == _lib.ABI_VERSION == 25
