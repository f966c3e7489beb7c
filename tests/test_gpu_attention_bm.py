"""The one-pass attention of block_minifloat layers (ops.bm_attention, csrc/mi355q_attention_bm.hip) against the oracle of
tests/attn_bm_util.py (the reference's steps with an fp64 softmax; its conditions on the inputs and its bounds are stated there), and the
equalities the kernel owes: a query that sees one key returns that key's quantised V row bit for bit, B rows equal B single calls,
strided head views equal their copies, the pack launch leaves the bytes a MinifloatKVCache holds, the last 16 queries agree with the
decode kernels on that cache, the registry's steps and the harness models with the knob off agree with the knob on.
Six tests: each runs its table of cases in a loop (_each) and names every case that fails.  Measured on an MI355X: all 59 oracle cases
within worst 4e-8, mean 2e-9 of max|ref|; the models' logits bit-equal with the knob on and off."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import attn_bm_util as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATTERNS = (0x00000000, 0xFFFFFFFF, 0x7FC00000, 0x3F800000, 0x00000001, 0x80000000)


def _each(cases, fn, name=str):
    """fn(case) for every case, every failing one named: the tables below run inside ONE test each, so the suite's list of test ids grows by
    a handful, not by a hundred; nothing stops at the first failure"""
    failed = []
    for c in cases:
        print("case", name(c))
        try:
            fn(*c) if fn.__code__.co_argcount > 1 else fn(c)
        except AssertionError as e:
            failed.append(f"{name(c)}: {e}")
    assert not failed, f"{len(failed)} of {len(cases)} cases fail:\n" + "\n".join(failed)


def _run(c, q, k, v):
    import torch
    from mi355q import ops
    fmts, causal = c[5], c[4]
    scale_div, q_scale = U.case_scales(c)
    t = [torch.from_numpy(np.array(a)).to(DEV) for a in (q, k, v)]      # (copies: the shared arrays are read-only)
    return ops.bm_attention(*t, U.par(fmts[0], fmts[1]), U.par(fmts[2], fmts[3]), causal=causal, scale_div=scale_div, q_scale=q_scale)


def _quantised_v(v, fmt):
    from oracle import compare, np_oracle as O
    return compare.bf16_rne(O.block_minifloat_quantize(v, fmt[0], fmt[1], fmt[2], block_size=[1, 16], skip_first_dim=True))


def test_vs_oracle():
    """every case of attn_bm_util.CASES (59), each within the bounds of the oracle; bit-identical on a second call; row 0 of a causal M = T call sees one key, P = 1.0, and is that key's
    quantised V row exactly; B > 1 equals the single calls bit for bit"""
    _each(U.CASES, _vs_oracle, U.case_id)


def _vs_oracle(c):
    import torch
    B, M, T, D, causal, fmts = c[:6]
    q, k, v, ref, keep = U.case_reference(c)
    a, b = _run(c, q, k, v), _run(c, q, k, v)
    assert a.shape == (B, M, D) and a.is_contiguous()
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "two runs differ"
    out = a.cpu().numpy()
    assert np.isfinite(out).all()
    U.check(out, ref, keep)
    if causal and M == T:
        # (as values: a -0.0 of the row comes out of the product's accumulator as +0.0)
        assert np.array_equal(out[:, 0], _quantised_v(v, fmts[3])[:, 0]), "a query that sees one key must return that key's quantised V row"
    if B > 1:
        for i in range(B):
            one = _run(c, q[i:i + 1], k[i:i + 1], v[i:i + 1])
            assert torch.equal(one.view(torch.uint8), a[i:i + 1].view(torch.uint8)), f"row {i} of the batch differs from its single call"


def test_strided_head_views():
    """[1, T, H, D] projections viewed as [1, H, T, D] are read in place: the bits of the contiguous copies"""
    _each([(4, 48, 48, 64), (3, 17, 80, 128), (2, 65, 80, 32)], _strided_head_views)


def _strided_head_views(H, M, T, D):
    import torch
    from mi355q import ops
    torch.manual_seed(T + D)
    qp, kp, vp = torch.randn(1, M, H, D, device=DEV) * 3.0, torch.randn(1, T, H, D, device=DEV), torch.randn(1, T, H, D, device=DEV)
    par = U.par(U.F848)
    heads = lambda t: t.transpose(1, 2)
    o_view = ops.bm_attention(heads(qp), heads(kp), heads(vp), par, par, causal=True, scale_div=math.sqrt(D))
    o_copy = ops.bm_attention(*(heads(t).contiguous().view(H, t.shape[1], D) for t in (qp, kp, vp)), par, par, causal=True, scale_div=math.sqrt(D))
    assert o_view.shape == (1, H, M, D) and float(o_copy.abs().max()) > 0
    assert torch.equal(o_view[0].view(torch.uint8), o_copy.view(torch.uint8))


def test_against_the_cache():
    """the pack launch leaves, in the op's workspace, the bytes ops.MinifloatKVCache holds after the same T keys were appended (the last V
    pair's absent half zeros, as the zeroed cache has it); and the op's LAST 16 queries agree with ops.bfp_attention_decode on that cache
    within the oracle's bounds (both are held to the oracle; the sums run in a different order, so not bit for bit)"""
    _each([(2, 48, 64, (U.F848,) * 4), (3, 272, 128, (U.F848, U.F634, U.F735, U.F848)), (2, 16, 96, (U.F634,) * 4), (2, 80, 32, (U.F735,) * 4)],
          _against_the_cache)


def _against_the_cache(B, T, D, fmts):
    import torch
    from mi355q import ops
    q, k, v = U.inputs(B, T, T, D, seed=T + D + 7)
    qk, pv = U.par(fmts[0], fmts[1]), U.par(fmts[2], fmts[3])
    qt, kt, vt = (torch.from_numpy(a).to(DEV) for a in (q, k, v))
    out = ops.bm_attention(qt, kt, vt, qk, pv, causal=True, scale_div=math.sqrt(D))
    ws = ops._BM_ATTN_WS.get((torch.device(DEV).index, ops._stream_ptr(torch.device(DEV)), B, T, D))
    assert ws is not None
    ws = ws.clone()
    cache = ops.MinifloatKVCache(B, T, D, qk, pv, DEV)
    cache.append(kt, vt)
    kq, vq = cache.kq.view(torch.uint8).reshape(-1), cache.vq.view(torch.uint8).reshape(-1)
    assert kq.numel() == B * T * D * 2 and vq.numel() == B * ((T + 31) // 32) * 32 * D * 2
    assert torch.equal(ws[:kq.numel()], kq), "K fragments differ from the cache's"
    assert torch.equal(ws[kq.numel():kq.numel() + vq.numel()], vq), "V fragments differ from the cache's"
    dec = ops.bfp_attention_decode(qt[:, T - 16:].contiguous(), cache, causal=True, scale_div=math.sqrt(D)).cpu().numpy()
    ref, keep = U.reference_of(q, k, v, U.cfg(fmts[0], fmts[1]), U.cfg(fmts[2], fmts[3]), True, math.sqrt(D), count=False)
    last = out[:, T - 16:].cpu().numpy()
    U.check(last, ref[:, T - 16:], keep[:, T - 16:])
    U.check(dec, ref[:, T - 16:], keep[:, T - 16:])
    scale = np.abs(ref).max()
    d = np.abs(last - dec)[keep[:, T - 16:]]
    print("one pass vs decode: worst", d.max() / scale, "mean", d.mean() / scale)
    assert d.max() <= 1e-3 * scale and d.mean() <= 3e-5 * scale


def test_registry_steps():
    """get_quantized_func("attention", cfg) with mi355q_fused_matmul=False (the steps, what the parent commit ran) against the same call
    with the one-pass kernel, within the oracle's bounds; 3-d (bmm) and 4-d (matmul) inputs"""
    _each([((2, 80, 80, 64), True, "div"), ((1, 4, 17, 48, 128), True, "div"), ((3, 70, 48, 32), False, "q")], _registry_steps)


def _registry_steps(shape, causal, scale):
    import torch
    from mi355q import ops
    import mi355q.quantize as Q
    *lead, M, T, D = shape
    B = int(np.prod(lead))
    q, k, v = U.inputs(B, M, T, D, seed=T + D + M)
    scale_div, q_scale = (math.sqrt(D), None) if scale == "div" else (None, float(np.float32(D ** -0.5)))
    qs = q if q_scale is None else (q * np.float32(q_scale)).astype(np.float32)
    ref, keep = U.reference_of(qs, k, v, U.cfg(U.F848), U.cfg(U.F848), causal, scale_div)
    t = [torch.from_numpy(a).to(DEV).view(*lead, a.shape[1], D) for a in (q, k, v)]
    calls = []
    real = ops.bm_attention
    ops.bm_attention = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
    try:
        outs = {}
        for fused in (True, False):
            c0, c1 = U.cfg(U.F848, mi355q_fused_matmul=fused), U.cfg(U.F848, mi355q_fused_matmul=fused)
            f = Q.get_quantized_func("attention", c1)
            assert f.__name__ == "attention_block_minifloat"
            outs[fused] = f(*t, c0, c1, causal=causal, scale_div=scale_div, q_scale=q_scale).reshape(B, M, D).cpu().numpy()
            assert len(calls) == 1, "the one-pass kernel runs with mi355q_fused_matmul on and never with it off"
    finally:
        ops.bm_attention = real
    for fused in (True, False):
        U.check(outs[fused], ref, keep)
    scale_ = np.abs(ref).max()
    d = np.abs(outs[True] - outs[False])[keep]
    assert d.max() <= 1e-3 * scale_ and d.mean() <= 3e-5 * scale_


# ---- models: every Linear bypassed, block_minifloat (8, 4, 8) attention products ----------------------------------------------------
# (The Linears are bypassed on purpose: a coarse quantiser behind the attention turns one ulp into a whole step on a tie, DESIGN 7c-8,
#  and that belongs to no kernel.)
def _model(family, knob, layers=2, seed=0):
    import torch
    from mi355q import harness as H
    torch.manual_seed(seed)
    prod = U.cfg(U.F848, mi355q_values_matmul="fp32", mi355q_fused_attention=knob)
    qc = {"default": dict(prod), "linear": dict(prod, bypass=True)}
    if family == "llama":
        cfg = H.TinyLlamaConfig(vocab_size=97, hidden_size=128, intermediate_size=256, num_layers=layers, num_heads=2, max_positions=48)
        model = H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(qc, layers))
    else:
        cfg = H.TinyOPTConfig(vocab_size=97, hidden_size=128, ffn_dim=256, num_layers=layers, num_heads=2, max_positions=48)
        model = H.TinyOPTForCausalLM(cfg, H.expand_quant_config(qc, layers))
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.ndim == 2 and "embed" not in n:
                p.mul_(40.0)
    return model.to(DEV)


def _ids(T=32, B=2):
    import torch
    return torch.randint(0, 97, (B, T), generator=torch.Generator().manual_seed(5)).to(DEV)


def _counted(fn):
    from mi355q import ops
    calls = []
    real = ops.bm_attention
    ops.bm_attention = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
    try:
        return fn(), len(calls)
    finally:
        ops.bm_attention = real


def test_models_knob_on_against_off():
    """tiny OPT and tiny Llama, full forward and prompt step (_prompt_step): logits with config["mi355q_fused_attention"] on (the one-pass
    kernel, once a layer) against off (the steps), within 1e-3 of the largest logit"""
    _each(["opt", "llama"], _full_forward)
    _each(["opt", "llama"], _prompt_step)


def _full_forward(family):
    import torch
    ids = _ids()
    with torch.no_grad():
        off, n_off = _counted(lambda: _model(family, False)(ids)[0])
        on, n_on = _counted(lambda: _model(family, True)(ids)[0])
    assert n_off == 0 and n_on == 2, (n_off, n_on)
    top = float(off.abs().max())
    e = float((on - off).abs().max())
    print("largest logit", top, "worst difference", e)
    assert top > 0 and e <= 1e-3 * top


def _prompt_step(family):
    """DecodeState(mode="block"): the prompt's first-step logits with the knob on (the one-pass kernel behind the append) within 1e-3 of the
    largest logit of the knob-off state (the steps); the caches hold the same bytes either way"""
    import torch
    from mi355q import harness as H, ops
    ids = _ids()

    def first_step(knob):
        model = _model(family, knob)
        state = H.DecodeState(model, ids.shape[0], 48, "block")
        assert all(type(c) is ops.MinifloatKVCache for c in state.kv)
        with torch.no_grad():
            return model(ids, cache=state)[0][:, -1], state

    (off, s_off), n_off = _counted(lambda: first_step(False))
    (on, s_on), n_on = _counted(lambda: first_step(True))
    assert n_off == 0 and n_on == 2, (n_off, n_on)
    top = float(off.abs().max())
    e = float((on - off).abs().max())
    print("largest logit", top, "worst difference", e)
    assert top > 0 and e <= 1e-3 * top
    assert torch.equal(s_on.kv[0].kq, s_off.kv[0].kq) and torch.equal(s_on.kv[0].vq, s_off.kv[0].vq)


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


def test_stale_lds(poison):
    """as tests/test_gpu_kvbm_decode.py::test_stale_lds, over each DC: every compute unit's LDS is filled with a pattern in front of the call
    and the output must be the same bits under every pattern (the missing second tile of an odd tile count reads a clamped piece and
    discards it; nothing is read from LDS that the step's DMA did not write)"""
    _each([(2, 65, 272, 128), (3, 17, 48, 96), (2, 48, 48, 64), (2, 16, 16, 32)], lambda B, M, T, D: _stale_lds(poison, B, M, T, D))


def _stale_lds(poison, B, M, T, D):
    import torch
    from mi355q import ops
    torch.manual_seed(T + D)
    par = U.par(U.F848)
    q, k, v = torch.randn(B, M, D, device=DEV) * 3.0, torch.randn(B, T, D, device=DEV), torch.randn(B, T, D, device=DEV)
    outs = []
    for p in PATTERNS:
        poison(p)
        outs.append(ops.bm_attention(q, k, v, par, par, causal=True, scale_div=math.sqrt(D)).clone())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    for p, o in zip(PATTERNS[1:], outs[1:]):
        assert torch.equal(o.view(torch.uint8), outs[0].view(torch.uint8)), f"output depends on stale LDS (pattern {p:#010x})"
