"""Fused attention for padded batches, the parts that need no GPU: the export is declared and bound, ops.bfp_attention_padded's
refusals, the registry's fallback (key_mask = the dense [B, 1, T_q, T_k] mask spelled out, bitwise), and the harness models'
attention_mask keyword."""
import ctypes
import inspect
import re
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))

import mi355q.quantize as Q  # noqa: E402
from mi355q import _lib, harness as H, ops  # noqa: E402

FMIN = torch.finfo(torch.float32).min
PAR = (6, 8, 127, 6, 8, 127)


def _bypassed(**extra):
    return dict(name="block_fp", bypass=True, is_ptq=True, data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
                data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127, weight_block_size=[1, 16],
                bias_width=6, bias_exponent_width=8, bias_exponent_bias=127, bias_block_size=[16], **extra)


def test_export_is_declared_and_bound():
    header = (ROOT / "include" / "mi355q.h").read_text()
    m = re.search(r"int mi355q_bfp_attention_padded\(([^;]*)\);", header)
    assert m, "mi355q_bfp_attention_padded is not declared in include/mi355q.h"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert "const int32_t* key_mask" in args and "int64_t heads" in args and "float q_scale" in args and not any("mask" in a and "key_mask" not in a for a in args)
    assert int(re.search(r"#define MI355Q_ABI_VERSION (\d+)", header).group(1)) == 25
    assert len(_lib.SIGNATURES["mi355q_bfp_attention_padded"][1]) == len(args) == 18
    lib = _lib.load_library()
    assert lib.mi355q_bfp_attention_padded.restype is ctypes.c_int


def test_export_refuses_bad_arguments_before_any_launch():
    """the BADARG paths come first: no pointer is followed and nothing is launched"""
    lib = _lib.load_library()
    pa = (ctypes.c_int32 * 6)(*PAR)
    p = ctypes.addressof(pa)
    buf = ctypes.create_string_buffer(4096 + 16)
    a = (ctypes.addressof(buf) + 15) // 16 * 16

    def call(key_mask=a, heads=2, B=6, M=16, T=16, D=32, causal=1):
        return lib.mi355q_bfp_attention_padded(a, a, a, key_mask, heads, causal, 0.0, 0.0, a, a, B, M, T, D, p, p, None, None)
    codes = {call(key_mask=None), call(heads=0), call(heads=-1), call(heads=4), call(B=-1), call(M=32, T=16), call(T=0)}
    assert codes == {_lib.E_BADARG}, codes
    assert call(B=0, heads=1) == 0                              # (nothing to do)
    assert call(key_mask=a + 4) == _lib.E_ALIGN                 # (the mask is read 16 bytes at a time)


def test_op_refusals_name_the_reason():
    q, k, v = (torch.zeros(3, 2, 32, 32) for _ in range(3))
    km = torch.ones(3, 32, dtype=torch.int32)
    ok = lambda **kw: ops.bfp_attention_padded_supported(kw.get("q", q), kw.get("k", k), kw.get("v", v), kw.get("widths", (6, 6, 6, 6)),
                                                         kw.get("key_mask", km), causal=True, heads=kw.get("heads"))
    assert not ok()                                             # (CPU tensors: the kernels run on the GPU only)
    for kw, word in ((dict(key_mask=torch.ones(3, 31, dtype=torch.int32)), "key_mask"),
                     (dict(key_mask=torch.ones(2, 32, dtype=torch.int32)), "sequences"),
                     (dict(key_mask=torch.zeros(3, 32)), "additive"),
                     (dict(q=torch.zeros(3, 2, 48, 32)), "T_q"),
                     (dict(q=torch.zeros(6, 32, 32), k=torch.zeros(6, 32, 32), v=torch.zeros(6, 32, 32)), "heads="),
                     (dict(q=torch.zeros(6, 32, 32), k=torch.zeros(6, 32, 32), v=torch.zeros(6, 32, 32), heads=4), "sequences"),
                     (dict(heads=0), "heads"),
                     (dict(widths=(6, 6, 12, 6)), "widths"),
                     (dict(q=torch.zeros(3, 2, 32, 40), k=torch.zeros(3, 2, 32, 40), v=torch.zeros(3, 2, 32, 40)), "head_dim"),
                     ({}, "MI355X")):
        assert not ok(**kw)
        with pytest.raises(ValueError, match=word):
            w = kw.get("widths", (6, 6, 6, 6))
            ops.bfp_attention_padded(kw.get("q", q), kw.get("k", k), kw.get("v", v), (w[0], 8, 127, w[1], 8, 127), (w[2], 8, 127, w[3], 8, 127),
                                     kw.get("key_mask", km), causal=True, heads=kw.get("heads"))


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("ndim", [3, 4])
def test_registry_fallback_is_the_dense_mask(ndim, causal):
    """on CPU (and wherever the op does not apply) key_mask = the additive [B, 1, T_q, T_k] mask spelled out, bitwise -- a sequence with
    no real key included: every row uniform"""
    torch.manual_seed(ndim)
    lead = (3, 2) if ndim == 4 else (3,)
    q, k, v = torch.randn(*lead, 24, 32), torch.randn(*lead, 32, 32), torch.randn(*lead, 32, 32)
    km = torch.ones(3, 32, dtype=torch.int64)
    km[1, :7] = 0
    km[2, :] = 0
    f = Q.get_quantized_func("attention", _bypassed())
    dense = torch.where(km != 0, 0.0, FMIN).reshape(3, *([1] * (ndim - 2)), 32).expand(3, *([1] * (ndim - 3)), 24, 32).contiguous()
    a = f(q, k, v, _bypassed(), _bypassed(), causal=causal, key_mask=km)
    b = f(q, k, v, _bypassed(), _bypassed(), causal=causal, mask=dense)
    assert torch.equal(a, b)
    assert torch.allclose(a[2], v[2].mean(-2, keepdim=True).expand_as(a[2]), atol=1e-6)
    with pytest.raises(ValueError, match="key_mask together with mask"):
        f(q, k, v, _bypassed(), _bypassed(), causal=causal, key_mask=km, mask=dense)
    with pytest.raises(ValueError, match="key_mask"):
        f(q, k, v, _bypassed(), _bypassed(), causal=causal, key_mask=km[:2])


def _opt(fused_attention):
    torch.manual_seed(0)
    cfg = H.TinyOPTConfig(vocab_size=64, hidden_size=64, ffn_dim=128, num_layers=2, num_heads=4, max_positions=48)
    return H.TinyOPTForCausalLM(cfg, H.expand_quant_config(_bypassed(mi355q_fused_attention=fused_attention), 2)).eval()


def _llama(fused_attention):
    # (the Llama family's rotary function quantises whatever `bypass` says and block_fp has no CPU quantiser: that node alone is
    #  a bypassed integer one here)
    torch.manual_seed(0)
    rope = dict(name="integer", bypass=True, is_ptq=True, data_in_width=8, data_in_frac_width=4, weight_width=8, weight_frac_width=4,
                bias_width=8, bias_frac_width=4)
    full = {"default": _bypassed(mi355q_fused_attention=fused_attention), "model_layer": {"self_attn": {"rotary_positional_encoding": rope}}}
    cfg = H.TinyLlamaConfig(vocab_size=64, hidden_size=64, intermediate_size=128, num_layers=2, num_heads=4, max_positions=48)
    return H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(full, 2)).eval()


@pytest.mark.parametrize("fused_attention", [False, True])
@pytest.mark.parametrize("build", [_opt, _llama])
def test_model_forward_takes_attention_mask(build, fused_attention):
    model = build(fused_attention)
    sig = inspect.signature(model.forward)
    assert list(sig.parameters)[-1] == "attention_mask" and sig.parameters["attention_mask"].default is None
    ids = torch.randint(0, 64, (3, 40), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        plain = model(ids)[0]
        ones = model(ids, attention_mask=torch.ones(3, 40, dtype=torch.long))[0]
        assert torch.equal(plain, ones)                         # all ones = today's call, bit for bit
        am = torch.ones(3, 40, dtype=torch.long)
        am[1, :11] = 0                                          # left-padded
        am[2, 29:] = 0                                          # right-padded
        got = model(ids, attention_mask=am)[0]
        assert torch.isfinite(got).all() and torch.equal(got[0], plain[0])
        # right padding: the real tokens of a causal model never see a pad key
        assert torch.equal(got[2, :29], plain[2, :29])
        if build is _opt:
            # left padding, unquantised: positions count real tokens, so the real tokens' logits are the unpadded sequence's
            alone = model(ids[1:2, 11:])[0]
            assert torch.allclose(got[1, 11:], alone[0], atol=1e-5)
    with pytest.raises(ValueError, match="attention_mask"):
        model(ids, attention_mask=torch.ones(3, 39, dtype=torch.long))


@pytest.mark.parametrize("build", [_opt, _llama])
def test_cache_with_attention_mask_is_refused_by_name(build):
    model = build(True)
    ids = torch.randint(0, 64, (2, 8))
    with pytest.raises(NotImplementedError, match="DecodeState.*ragged"):
        model(ids, cache=object(), attention_mask=torch.ones(2, 8, dtype=torch.long))


def test_opt_pad_position_row_survives_the_reference_state_dict():
    """a pad position's embedding is row 1 of the reference's table (cumsum * mask - 1 + the offset of 2): kept on load, written back"""
    model = _opt(True)
    sd = model.reference_state_dict()
    assert torch.equal(sd["model.decoder.embed_positions.weight"][:2], torch.zeros(2, 64))
    sd["model.decoder.embed_positions.weight"] = sd["model.decoder.embed_positions.weight"].clone()
    sd["model.decoder.embed_positions.weight"][1] = 0.25
    other = _opt(True).load_reference_state_dict(sd)
    assert torch.equal(other.reference_state_dict()["model.decoder.embed_positions.weight"][1], torch.full((64,), 0.25))
    ids = torch.randint(0, 64, (1, 16))
    am = torch.ones(1, 16, dtype=torch.long)
    am[0, :5] = 0
    with torch.no_grad():
        a, b = model(ids, attention_mask=am)[0], other(ids, attention_mask=am)[0]
    assert not torch.equal(a[0, :5], b[0, :5]) and torch.equal(model(ids)[0], other(ids)[0])
