"""Fused attention for padded batches (ops.bfp_attention_padded behind the registry's attention(key_mask=...) and the harness
models' attention_mask): the per-sequence key mask inside the resident and the streaming kernel against the oracle's restatement of the
reference's steps, called per sequence with mask = broadcast(pad_row) (tests/attn_padded_util.py), at the smallest shapes that can go
wrong -- 3 sequences x 2 heads, 80 / 48 / 16 keys, 32 queries behind 80 keys, pad boundaries inside a 16-key tile, on tile and pair
edges, whole tiles padded, a sequence with no real key -- and the fully masked query: 1 / T_k over ALL keys."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))

from tests import attn_padded_util as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (T_k, T_q, head_dim, width, real lengths, padding side, causal, scale_div, q_scale)
CASES = [
    (80, 80, 64, 6, (80, 37, 1), "left", True, False, False),       # no pad / a boundary inside a tile / whole tiles padded
    (80, 80, 64, 6, (80, 37, 1), "right", True, False, False),
    (80, 80, 128, 6, (16, 33, 64), "left", True, True, False),      # boundaries on tile and pair edges
    (80, 80, 32, 6, (16, 33, 64), "right", False, False, False),
    (80, 80, 96, 6, (80, 37, 1), "left", False, False, False),
    (80, 32, 64, 6, (80, 37, 1), "left", True, False, False),       # 32 queries behind 80 keys
    (80, 32, 128, 6, (16, 33, 64), "right", True, True, False),
    (48, 48, 64, 4, (48, 21, 1), "left", True, False, True),        # width 4, q_scale
    (48, 48, 96, 6, (16, 33, 48), "right", True, True, False),
    (16, 16, 32, 6, (16, 5, 1), "left", True, False, False),        # one tile
    (80, 80, 64, 6, (80, 0, 37), "left", True, False, False),       # a sequence with no real key
    (80, 80, 128, 6, (80, 0, 37), "right", False, False, True),
    (80, 80, 128, 6, (80, 37, 1), "left", True, False, True),
]


def _run(case, kernel, via="op"):
    import torch
    import mi355q.quantize as Q
    from mi355q import ops
    T, M, hd, width = case[:4]
    q, k, v, km, ref, kw = U.case(*case)
    c = U.cfg(width)
    par = (width, 8, 127, width, 8, 127)
    qt, kt, vt = (torch.tensor(t).to(DEV) for t in (q, k, v))
    kmt = torch.tensor(km).to(DEV)
    prev = ops.attention_set_kernel(kernel)
    try:
        if via == "op":
            out = ops.bfp_attention_padded(qt, kt, vt, par, par, kmt, causal=case[6], **kw)
        else:
            out = Q.get_quantized_func("attention", c)(qt, kt, vt, dict(c), dict(c), causal=case[6], key_mask=kmt, **kw)
        torch.cuda.synchronize()
    finally:
        ops.attention_set_kernel(prev)
    return out.cpu().numpy(), ref, km


@pytest.mark.parametrize("kernel", [1, 2, 3])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "T%d_M%d_hd%d_w%d_%s_%s%s%s%s" % (
    c[0], c[1], c[2], c[3], "-".join(map(str, c[4])), c[5], "_causal" if c[6] else "", "_div" if c[7] else "", "_qs" if c[8] else ""))
def test_padded_vs_oracle(case, kernel):
    out, ref, km = _run(case, kernel)
    assert np.isfinite(out).all()
    U.check(out, ref)
    T, M = case[:2]
    for b, n in enumerate(case[4]):
        # fully masked queries: a sequence with no real key (every row), a left-padded sequence's pad queries under the causal rule --
        # 1 / T_k over all keys, so every such row of a head is the same vector, and the oracle's
        if n == 0:
            rows = range(M)
        elif case[6] and case[5] == "left":
            rows = [i for i in range(M) if i + T - M < T - n]
        else:
            rows = []
        for i in rows:
            assert np.array_equal(out[b, :, i], out[b, :, rows[0]]), (b, i)
        if len(rows):
            U.check(out[b][:, list(rows)], ref[b][:, list(rows)])


@pytest.mark.parametrize("kernel", [1, 2, 3])
@pytest.mark.parametrize("hd,q_scaled", [(64, False), (128, False), (64, True), (32, False)])
def test_all_ones_mask_is_the_unmasked_call_bit_for_bit(hd, q_scaled, kernel):
    """a kernel that adds 0 to a score and walks the same tiles keeps the bits of ops.bfp_attention(causal=...) with no mask"""
    import torch
    from mi355q import ops
    T = 80
    q, k, v, _, _, _ = U.case(T, T, hd, 6, (80, 37, 1), "left", True, False, False)
    qt, kt, vt = (torch.tensor(t).to(DEV) for t in (q, k, v))
    par = (6, 8, 127, 6, 8, 127)
    kw = dict(q_scale=hd ** -0.5) if q_scaled else {}
    ones = torch.ones(3, T, dtype=torch.int32, device=DEV)
    prev = ops.attention_set_kernel(kernel)
    try:
        for causal in (True, False):
            a = ops.bfp_attention_padded(qt, kt, vt, par, par, ones, causal=causal, scale_div=2.0, **kw)
            b = ops.bfp_attention(qt, kt, vt, par, par, causal=causal, scale_div=2.0, **kw)
            assert torch.equal(a, b), (causal, (a - b).abs().max().item())
    finally:
        ops.attention_set_kernel(prev)


def test_mask_dtypes_and_flat_heads():
    """bool / int64 masks and the flat [B x heads, T, D] form with heads= give the int32, 4-d call's bits"""
    import torch
    from mi355q import ops
    case = CASES[0]
    q, k, v, km, _, _ = U.case(*case)
    qt, kt, vt = (torch.tensor(t).to(DEV) for t in (q, k, v))
    kmt = torch.tensor(km).to(DEV)
    par = (6, 8, 127, 6, 8, 127)
    base = ops.bfp_attention_padded(qt, kt, vt, par, par, kmt, causal=True)
    assert torch.equal(base, ops.bfp_attention_padded(qt, kt, vt, par, par, kmt.bool(), causal=True))
    assert torch.equal(base, ops.bfp_attention_padded(qt, kt, vt, par, par, kmt.long() * 7, causal=True))
    flat = ops.bfp_attention_padded(qt.reshape(6, 80, 64), kt.reshape(6, 80, 64), vt.reshape(6, 80, 64), par, par, kmt, causal=True, heads=2)
    assert torch.equal(base, flat.view(3, 2, 80, 64))


def _spy(ops):
    calls, real = [], ops.bfp_attention_padded
    ops.bfp_attention_padded = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    return calls, real


def test_registry_takes_the_padded_op():
    from mi355q import ops
    ops.vendor_gemm_calls(reset=True)
    calls, real = _spy(ops)
    try:
        out, ref, _ = _run(CASES[0], 0, via="registry")
    finally:
        ops.bfp_attention_padded = real
    U.check(out, ref)
    assert len(calls) == 1 and not ops.vendor_gemm_calls(), (len(calls), ops.vendor_gemm_calls())


def _models(family, knobs):
    import torch
    from mi355q import harness as H
    d = dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
             data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127, weight_block_size=[1, 16],
             bias_width=6, bias_exponent_width=8, bias_exponent_bias=127, bias_block_size=[16], mi355q_fused_attention=True, **knobs)
    torch.manual_seed(11)
    if family == "opt":
        cfg = H.TinyOPTConfig(vocab_size=128, hidden_size=128, ffn_dim=256, num_layers=2, num_heads=4, max_positions=64)
        m = H.TinyOPTForCausalLM(cfg, H.expand_quant_config(d, cfg.num_layers))
    else:
        cfg = H.TinyLlamaConfig(vocab_size=128, hidden_size=128, intermediate_size=256, num_layers=2, num_heads=4, max_positions=64)
        m = H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(d, cfg.num_layers))
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.ndim == 2 and "embed" not in n:
                p.mul_(4.0)                      # (scores that are not all alike: tests/test_gpu_model.py does the same)
    return m.to(DEV).eval()


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("family", ["opt", "llama"])
def test_model_padded_batch(family, side):
    """tiny OPT / Llama (2 layers, hidden 128, 4 heads, 48 tokens, batch of 3): the fused logits against the same model on
    mi355q_fused_matmul=False -- the generic steps with the dense [B, 1, T, T] mask -- within tests/test_gpu_model.py's bound between
    its forwards (1e-3 of the largest logit), pad rows included; the padded op runs once a layer and no vendor GEMM does"""
    import torch
    from mi355q import ops
    T = 48
    ids = torch.randint(0, 128, (3, T), generator=torch.Generator().manual_seed(2)).to(DEV)
    am = torch.from_numpy(U.key_mask((48, 21, 1), T, side)).to(DEV)
    with torch.no_grad():
        ref = _models(family, dict(mi355q_fused_matmul=False))(ids, attention_mask=am)[0].cpu().numpy()
        model = _models(family, {})
        ops.vendor_gemm_calls(reset=True)
        calls, real = _spy(ops)
        try:
            got = model(ids, attention_mask=am)[0].cpu().numpy()
        finally:
            ops.bfp_attention_padded = real
    err = float(np.abs(got - ref).max())
    print(f"{family} {side}: max|dlogit| {err:.2e} of {np.abs(ref).max():.2e}")
    assert len(calls) == 2 and not ops.vendor_gemm_calls(), (len(calls), ops.vendor_gemm_calls())
    assert np.isfinite(got).all() and err < 1e-3 * max(1.0, float(np.abs(ref).max())), err


@pytest.fixture(scope="module")
def poison():
    import ctypes
    import torch
    so = ROOT / "tools" / "lds_poison" / "liblds_poison.so"
    if not so.exists():
        pytest.fail("tools/lds_poison/liblds_poison.so is not built (__graft_entry__.build())")
    lib = ctypes.CDLL(str(so))

    def fill(pattern):
        rc = lib.lds_poison(ctypes.c_uint(pattern), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
    return fill


@pytest.mark.parametrize("kernel,hd", [(1, 128), (2, 96), (3, 64)])
def test_no_stale_lds(poison, kernel, hd):
    """the same bits behind every pattern left in LDS (tests/test_gpu_stale_lds.py)"""
    import torch
    from mi355q import ops
    patterns = (0x00000000, 0xFFFFFFFF, 0x7FC00000, 0x3F800000, 0x00000001, 0x80000000)
    q, k, v, km, _, _ = U.case(80, 80, hd, 6, (80, 37, 1), "left", True, False, False)
    qt, kt, vt = (torch.tensor(t).to(DEV) for t in (q, k, v))
    kmt = torch.tensor(km).to(DEV)
    par = (6, 8, 127, 6, 8, 127)
    prev = ops.attention_set_kernel(kernel)
    try:
        outs = []
        for p in patterns:
            poison(p)
            outs.append(ops.bfp_attention_padded(qt, kt, vt, par, par, kmt, causal=True, scale_div=float(hd) ** 0.5).clone())
        torch.cuda.synchronize()
    finally:
        ops.attention_set_kernel(prev)
    for p, o in zip(patterns[1:], outs[1:]):
        assert torch.equal(outs[0].view(torch.uint8), o.view(torch.uint8)), f"output depends on stale LDS (pattern {p:#010x})"


@pytest.mark.parametrize("route", ["one_pass", "dense_mask_steps", "steps"])
def test_reference_fixture_left_padded_batch(route):
    """tests/golden/opt_padded.npz (tools/gen_golden_models.py --padded): the REFERENCE's own OPT class on a left-padded batch of 3
    (real lengths 48 / 21 / 1) of the fixture model "opt_w6a6_t48" -- its logits, pad rows included, within the bound the tiny-OPT
    fixture test holds (tests/test_gpu_model.py:_check_fixture).  Pins the fully masked row and the pad positions' embedding to the
    reference, on the padded op, on the registry's dense-mask fallback and on the harness's own stepped attention."""
    import json
    import torch
    from mi355q import harness as H, ops
    from oracle import np_models as NM
    from tests.conftest import GOLDEN
    from tests.test_gpu_model import _with_knob
    meta = json.loads((GOLDEN / "models.json").read_text())
    pad = np.load(GOLDEN / "opt_padded.npz")
    sd, _, _, _, _, m = NM.load_fixture(meta, np.load(GOLDEN / "models.npz"), str(pad["model_tag"]))
    knobs = {"one_pass": dict(mi355q_fused_attention=True), "dense_mask_steps": dict(mi355q_fused_attention=True, mi355q_fused_matmul=False),
             "steps": {}}[route]
    cfg = H.TinyOPTConfig(vocab_size=m["vocab_size"], hidden_size=m["hidden_size"], ffn_dim=m["ffn_dim"], num_layers=m["num_layers"],
                          num_heads=m["num_heads"], max_positions=m["max_positions"])
    model = H.TinyOPTForCausalLM(cfg, H.expand_quant_config(_with_knob(m["quant_config"], **knobs), cfg.num_layers))
    model.load_reference_state_dict(sd).to(DEV).eval()
    calls, real = _spy(ops)
    try:
        with torch.no_grad():
            logits = model(torch.tensor(pad["input_ids"]).to(DEV), attention_mask=torch.tensor(pad["attention_mask"]).to(DEV))[0]
    finally:
        ops.bfp_attention_padded = real
    ref = pad["logits"]
    err = float(np.abs(logits.cpu().numpy() - ref).max())
    print(f"{route}: max|dlogit| {err:.2e} of {np.abs(ref).max():.2e}")
    assert len(calls) == (2 if route == "one_pass" else 0)
    assert err < 1e-3 * max(1.0, float(np.abs(ref).max())), err
