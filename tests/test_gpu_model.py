"""Model-level parity (BASELINE configs 0/2/3 in the only form available here: model-shaped random
weights, seeded token ids): a small OPT-style decoder driven through the registry API on the GPU
(HIP quantisers, int8-MFMA Linear) against the same network evaluated on the CPU with the oracle's
quantisers.  Losses must agree so that exp(loss) matches to 3 d.p."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _oracle_forward(model, cfg_default, ids):
    """numpy evaluation of the harness model with the oracle's quantisers (oracle/np_models.py, itself pinned against
    the reference's own model classes by tests/test_oracle_models.py)"""
    from oracle import np_models as NM
    from mi355q.harness import expand_quant_config
    sd = {k: v.cpu().numpy().astype(np.float32) for k, v in model.reference_state_dict().items()}
    return NM.opt_forward(sd, expand_quant_config(cfg_default, model.cfg.num_layers), ids, model.cfg.num_heads)[1]


@pytest.mark.parametrize("toml_default", [
    dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
         data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127,
         weight_block_size=[1, 16], bias_width=6, bias_exponent_width=8, bias_exponent_bias=127, bias_block_size=[16]),
    dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=4, data_in_exponent_width=8, data_in_exponent_bias=127,
         data_in_block_size=[1, 16], weight_width=4, weight_exponent_width=8, weight_exponent_bias=127,
         weight_block_size=[1, 16], bias_width=4, bias_exponent_width=8, bias_exponent_bias=127, bias_block_size=[16]),
    dict(name="block_log", is_ptq=True, bypass=False, data_in_width=8, data_in_exponent_bias_width=8,
         data_in_block_size=[1, 16], weight_width=8, weight_exponent_bias_width=8, weight_block_size=[1, 16],
         bias_width=8, bias_exponent_bias_width=8, bias_block_size=[16]),
    dict(name="block_minifloat", is_ptq=True, bypass=False, data_in_width=8, data_in_exponent_width=4, data_in_exponent_bias_width=8,
         data_in_block_size=[1, 16], weight_width=8, weight_exponent_width=4, weight_exponent_bias_width=8,
         weight_block_size=[1, 16], bias_width=8, bias_exponent_width=4, bias_exponent_bias_width=8, bias_block_size=[16]),
], ids=["bfp_w6a6", "bfp_w4a4", "block_log_w8", "block_minifloat_w8"])
def test_tiny_opt_loss_parity(toml_default):
    import torch
    from mi355q.harness import TinyOPTConfig, TinyOPTForCausalLM, eval_lm_perplexity, expand_quant_config
    torch.manual_seed(0)
    cfg = TinyOPTConfig(vocab_size=384, hidden_size=256, ffn_dim=512, num_layers=2, num_heads=4, max_positions=64)
    qc = expand_quant_config(toml_default, cfg.num_layers)
    model = TinyOPTForCausalLM(cfg, qc)
    with torch.no_grad():                      # make the weights less trivial than N(0, 0.02)
        for n, p in model.named_parameters():
            if p.ndim == 2 and "embed" not in n:
                p.mul_(4.0)
            if n.endswith("bias"):
                p.normal_(0, 0.05)
    ids = torch.randint(0, cfg.vocab_size, (2, 48))
    ref_loss = _oracle_forward(model, toml_default, ids.numpy())      # before the PTQ in-place overwrite
    model = model.to("cuda:0")
    res = eval_lm_perplexity(model, [ids], device="cuda:0")
    assert abs(res["loss"] - ref_loss) < 2e-4, (res["loss"], ref_loss)
    assert round(math.exp(res["loss"]), 3) == round(math.exp(ref_loss), 3) or abs(math.exp(res["loss"]) - math.exp(ref_loss)) < 1e-3
    if toml_default["name"] == "block_fp":
        assert model.layers[0].fc1._packed is not None, "int8-MFMA path not taken by the MLP"
    # second pass: steady state (weights already quantised in place) gives the same loss
    res2 = eval_lm_perplexity(model, [ids], device="cuda:0")
    assert abs(res2["loss"] - res["loss"]) < 1e-6


def _oracle_llama_forward(model, cfg_default, ids):
    from oracle import np_models as NM
    from mi355q.harness import expand_llama_quant_config
    sd = {k: v.cpu().numpy().astype(np.float32) for k, v in model.reference_state_dict().items()}
    return NM.llama_forward(sd, expand_llama_quant_config(cfg_default, model.cfg.num_layers), ids, model.cfg.num_heads,
                            model.cfg.rms_eps)[1]


@pytest.mark.parametrize("width", [6, 4])
def test_tiny_llama_loss_parity(width):
    """Llama-style callers of the path: rotary embedding function, 4-D matmul functions (fused quantise + matmul
    where the blocks tile the operands), bias-free Linear layers with a SiLU-gated input (heavy-tailed: exercises the
    exception add-back of the row-aligned GEMM)"""
    import torch
    from mi355q.harness import TinyLlamaConfig, TinyLlamaForCausalLM, eval_lm_perplexity, expand_llama_quant_config
    d = dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=width, data_in_exponent_width=8,
             data_in_exponent_bias=127, data_in_block_size=[1, 16], weight_width=width, weight_exponent_width=8,
             weight_exponent_bias=127, weight_block_size=[1, 16], bias_width=width, bias_exponent_width=8,
             bias_exponent_bias=127, bias_block_size=[16])
    torch.manual_seed(1)
    cfg = TinyLlamaConfig(vocab_size=384, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=4, max_positions=64)
    model = TinyLlamaForCausalLM(cfg, expand_llama_quant_config(d, cfg.num_layers))
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.ndim == 2 and "embed" not in n:
                p.mul_(4.0)
    ids = torch.randint(0, cfg.vocab_size, (2, 48))
    ref_loss = _oracle_llama_forward(model, d, ids.numpy())
    model = model.to("cuda:0")
    res = eval_lm_perplexity(model, [ids], device="cuda:0")
    assert abs(res["loss"] - ref_loss) < 3e-4, (res["loss"], ref_loss)
    assert model.layers[0].down_proj._packed is not None, "int8-MFMA path not taken by the MLP"
    res2 = eval_lm_perplexity(model, [ids], device="cuda:0")
    assert abs(res2["loss"] - res["loss"]) < 1e-6


# ---- G5: fixtures from the REFERENCE's own model classes (tools/gen_golden_models.py) -------------------------------
import json as _json
from tests.conftest import GOLDEN as _GOLDEN
_G5 = _json.loads((_GOLDEN / "models.json").read_text())


def _with_knob(qc, **knobs):
    """the implementation knobs (mi355q_*) into every node config of a TOML-level quant config (parse_node_config hands
    them through to the modules / functions)"""
    if isinstance(qc, dict):
        out = {k: _with_knob(v, **knobs) for k, v in qc.items()}
        if "name" in qc:
            out.update(knobs)
        return out
    return qc


@pytest.mark.parametrize("attention", ["steps", "folded", "one_pass"])
@pytest.mark.parametrize("tag", sorted(t for t in _G5 if t.endswith("_t48")))
def test_reference_model_fixture_fused_attention(tag, attention):
    """the reference's own logits (48 tokens, head_dim 64, uniform and mixed per-layer widths) against the harness with the
    attention core as the reference steps it, with the softmax folded into P V, and as the one-pass kernel"""
    from mi355q import ops
    knobs = {"steps": {}, "folded": {"mi355q_fused_softmax": True}, "one_pass": {"mi355q_fused_attention": True}}[attention]
    calls, real = [], ops.bfp_attention
    ops.bfp_attention = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        _check_fixture(tag, knobs)
    finally:
        ops.bfp_attention = real
    assert (len(calls) == 2) == (attention == "one_pass"), len(calls)      # (the kernel really ran: once per layer)


@pytest.mark.parametrize("tag", sorted(_G5))
def test_reference_model_fixture(tag):
    _check_fixture(tag, {})


def _check_fixture(tag, knobs, forwards=1, loss_tol=2e-5):
    """weights + token ids + logits + loss of the reference's OPTQuantizedForCausalLM / LlamaQuantizedForCausalLM
    (2 layers; W6A6, W4A4, mixed per-layer widths, K % 128 == 0 variants that take the int8 GEMM): the harness on the
    GPU, driven through the registry API with the reference's per-layer config, must reproduce them."""
    import torch
    from mi355q import harness as H
    from oracle import np_models as NM
    data = np.load(_GOLDEN / "models.npz")
    sd, _, ids, ref_logits, ref_loss, m = NM.load_fixture(_G5, data, tag)
    if m["family"] == "opt":
        cfg = H.TinyOPTConfig(vocab_size=m["vocab_size"], hidden_size=m["hidden_size"], ffn_dim=m["ffn_dim"],
                              num_layers=m["num_layers"], num_heads=m["num_heads"], max_positions=m["max_positions"])
        model = H.TinyOPTForCausalLM(cfg, H.expand_quant_config(_with_knob(m["quant_config"], **knobs), cfg.num_layers))
    else:
        cfg = H.TinyLlamaConfig(vocab_size=m["vocab_size"], hidden_size=m["hidden_size"],
                                intermediate_size=m["intermediate_size"], num_layers=m["num_layers"],
                                num_heads=m["num_heads"], max_positions=m["max_positions"], rms_eps=m["rms_eps"])
        model = H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(_with_knob(m["quant_config"], **knobs), cfg.num_layers))
    model.load_reference_state_dict(sd).to("cuda:0").eval()
    t = torch.from_numpy(ids).to("cuda:0")
    with torch.no_grad():
        for _ in range(forwards):       # (the knobs that need packed weights act from the second forward on)
            logits, loss = model(t, labels=t)
    err = float(np.abs(logits.cpu().numpy() - ref_logits).max())
    dl = abs(float(loss) - ref_loss)
    print(f"{tag}: max|dlogit| {err:.2e}  |dloss| {dl:.2e}  ppl {math.exp(float(loss)):.4f} vs {math.exp(ref_loss):.4f}")
    assert err < 1e-3 * max(1.0, float(np.abs(ref_logits).max())), err          # north_star: fp tolerance <= 1e-3
    assert dl < loss_tol, (float(loss), ref_loss)
    if "k128" in tag:
        lin = model.layers[0].fc2 if m["family"] == "opt" else model.layers[0].down_proj
        assert lin._packed is not None, "K % 128 == 0 layer did not take the int8 path"


# the switches BASELINE config 3 runs with (tools/config3_full_depth.quant_config("resident") and its model.mi355q_lm_head;
# tests/test_oracle_compare.py keeps the two equal): every_knob's five, the residual in the stores, the gated / relu MLP epilogues,
# the mixed contraction, rotary on load in the attention pass, the attention pass writing o_proj's quantised operand, the
# split-bf16 lm_head
CONFIG3_KNOBS = dict(mi355q_fused_attention=True, mi355q_grouped_linear=True, mi355q_fused_activation=True, mi355q_fused_norm=True,
                     mi355q_token_major_output=True, mi355q_fused_residual=True, mi355q_fused_gate_up=True, mi355q_mixed="auto",
                     mi355q_fused_rotary=True, mi355q_fused_attention_output=True)
CONFIG3_LM_HEAD = "split"


def _config3_knobs(knobs):
    return dict(CONFIG3_KNOBS, **({"mi355q_weight_storage": "hybrid"} if knobs == "config3_hybrid" else {}))


def _route_census():
    """wraps the ops entry points of config 3's fused paths; returns (counts, restore).  `residual` is read from the bound
    arguments, so that it counts whether it was passed by keyword or by position"""
    import inspect
    from mi355q import ops
    counts = dict(gated=0, relu=0, attention=0, attention_consumer=0, attention_rope=0, residual=0, mixed=0)
    names = ("bfp_gemm_aligned_gated", "bfp_gemm_aligned_relu", "bfp_attention", "bfp_gemm_aligned", "bf16_gemm_tiled", "bfp_gemm_mixed")
    real = {n: getattr(ops, n) for n in names}
    sig = {n: inspect.signature(f) for n, f in real.items()}

    def wrap(name):
        def f(*a, **k):
            arg = sig[name].bind(*a, **k).arguments
            if name == "bfp_gemm_aligned_gated":
                counts["gated"] += 1
            elif name == "bfp_gemm_aligned_relu":
                counts["relu"] += 1
            elif name == "bfp_attention":
                counts["attention"] += 1
                counts["attention_consumer"] += arg.get("consumer") is not None
                counts["attention_rope"] += arg.get("rope") is not None
            elif name == "bfp_gemm_mixed":
                counts["mixed"] += 1
            counts["residual"] += arg.get("residual") is not None
            return real[name](*a, **k)
        return f

    for n in names:
        setattr(ops, n, wrap(n))

    def restore():
        for n, f in real.items():
            setattr(ops, n, f)
    return counts, restore


def _assert_config3_routes(what, family, counts, io, hooked, reached):
    """prints the route census and the Linears whose hooks fired on the last forward, and asserts both against what the
    first MI355X run of the config-3 cases recorded (hooked / reached: family -> sorted names / paths with a count > 0)"""
    fired = sorted(io)
    print(f"{what} route census, last forward: {counts}; hooks fired: {fired}")
    if hooked.get(family) is not None:
        assert fired == hooked[family], (fired, hooked[family])
    if reached.get(family) is not None:
        assert sorted(k for k, v in counts.items() if v) == reached[family], (counts, reached[family])


_G5W = _json.loads((_GOLDEN / "models_wide.json").read_text())


@pytest.mark.parametrize("knobs", ["plain", "every_knob", "config3"])
@pytest.mark.parametrize("tag", sorted(_G5W))
def test_reference_model_fixture_at_real_widths(tag, knobs):
    _fixture_at_real_widths(tag, knobs)


@pytest.mark.parametrize("tag", sorted(t for t in _G5W if _G5W[t]["family"] == "llama"))
def test_reference_model_fixture_at_real_widths_config3_hybrid(tag):
    """config 3's switches with mi355q_weight_storage = "hybrid" (the layers on the per-block route packed at width + 0.5 bits,
    expanded per forward)"""
    _fixture_at_real_widths(tag, "config3_hybrid")


# which Linears' forward hooks still fire under config 3 at these widths (2 x 128 tokens): the others run inside fused launches
# (grouped q / k / v and gate / up, the residual in o_proj's / down_proj's / fc2's stores) and are held to the oracle by
# tests/test_gpu_fused_oracle.py
# -- none at 2 x 128 tokens, so the teacher-forced per-Linear check has nothing left to hold here
_CONFIG3_HOOKED = {"opt": [], "llama": []}
# which of config 3's fused paths the last forward took (count > 0), per family, as the first MI355X run found them: the gated
# epilogue (Llama) and the relu one (OPT) with down_proj / fc2 on the per-block route, rotary on load, the residual in the stores;
# NOT the attention consumer (2 x 128 tokens: batch 2) and not the mixed contraction (no layer's rows miss every window)
_CONFIG3_REACHED = {"opt": ["attention", "relu", "residual"], "llama": ["attention", "attention_rope", "gated", "residual"]}


def _fixture_at_real_widths(tag, knobs):
    """2 decoder layers at OPT-1.3B width (2048 / 8192, 32 heads of 64) and Llama-7B width (4096 / 11008, 32 heads of 128),
    2 x 128 tokens: the reference's own logits and loss (tools/gen_golden_models.py --wide; the weights are a seeded recipe in
    the fixture).  At these widths every Linear takes the 256 x 256-tile int8 GEMM with its exception lists and the heads
    the one-pass attention kernel -- the kernels the bench lines are quoted on, under the reference's numbers"""
    import torch
    from mi355q import harness as H
    from oracle import np_models as NM
    data = np.load(_GOLDEN / "models_wide.npz")
    sd, _, ids, ref_logits, ref_loss, m = NM.load_wide_fixture(_G5W, data, tag)
    kn = {} if knobs == "plain" else dict(mi355q_grouped_linear=True, mi355q_fused_norm=True, mi355q_fused_activation=True,
                                          mi355q_fused_attention=True, mi355q_token_major_output=True)
    c3 = knobs.startswith("config3")
    if c3:
        kn = _config3_knobs(knobs)
    if m["family"] == "opt":
        cfg = H.TinyOPTConfig(vocab_size=m["vocab_size"], hidden_size=m["hidden_size"], ffn_dim=m["ffn_dim"],
                              num_layers=m["num_layers"], num_heads=m["num_heads"], max_positions=m["max_positions"])
        model = H.TinyOPTForCausalLM(cfg, H.expand_quant_config(_with_knob(m["quant_config"], **kn), cfg.num_layers))
    else:
        cfg = H.TinyLlamaConfig(vocab_size=m["vocab_size"], hidden_size=m["hidden_size"], intermediate_size=m["intermediate_size"],
                                num_layers=m["num_layers"], num_heads=m["num_heads"], max_positions=m["max_positions"],
                                rms_eps=m["rms_eps"])
        model = H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(_with_knob(m["quant_config"], **kn), cfg.num_layers))
    model.load_reference_state_dict(sd).to("cuda:0").eval()
    if c3:
        model.mi355q_lm_head = CONFIG3_LM_HEAD
    taps, io = {}, {}
    if c3:                                                   # (fused residual: the block returns residual + attention)
        model.layers[0].self_attn.register_forward_hook(
            lambda mod, i, k, o: taps.update(attn0=o.detach(), res0=k.get("residual")), with_kwargs=True)
    else:
        model.layers[0].self_attn.register_forward_hook(lambda mod, i, o: taps.__setitem__("attn0", o.detach()))
    if knobs == "plain" or c3:                               # (every Linear's input and output as the forward saw them)
        from mi355q.quantize import get_quantized_cls
        lin_cls = get_quantized_cls("linear", m["quant_config"]["default"])
        for name, mod in model.named_modules():
            if isinstance(mod, lin_cls) and name.startswith("layers."):
                mod.register_forward_hook(lambda mod, i, o, name=name: io.__setitem__(name, (i[0].detach().clone(), o.detach().clone())))
    t = torch.from_numpy(ids).to("cuda:0")
    with torch.no_grad():
        for f in range(2):                                   # (the second forward runs on the packed weights)
            if c3 and f == 1:
                io.clear()
                counts, restore = _route_census()
            try:
                logits, loss = model(t, labels=t)
            finally:
                if c3 and f == 1:
                    restore()
    lin = model.layers[0].fc2 if m["family"] == "opt" else model.layers[0].down_proj
    assert lin._packed is not None and lin._align_mode == "rows", "the row-aligned int8 GEMM was not taken"
    if c3:
        _assert_config3_routes(f"{tag} [{knobs}]", m["family"], counts, io, _CONFIG3_HOOKED, _CONFIG3_REACHED)
    # (1) the first layer's attention output (q / k / v projections at K = hidden, rotary, both products, softmax, the
    #     output projection): tight -- nothing upstream of it amplifies a last-bit difference
    ref_attn = data[tag + "/attn0"]
    a = taps["attn0"].reshape(ids.shape[0], ids.shape[1], -1)[:, :, :128].cpu().numpy()
    ea = float(np.abs(a - ref_attn).max() / np.abs(ref_attn).max())
    if c3:                                                   # out - x: the attn0 bound plus the rounding of the add, 2^-23 max|x|
        x0 = taps["res0"].reshape(ids.shape[0], ids.shape[1], -1)[:, :, :128].cpu().numpy()
        a = a - x0
        ea = max(0.0, float(np.abs(a - ref_attn).max()) - 2.0 ** -23 * float(np.abs(x0).max())) / float(np.abs(ref_attn).max())
    # (2) logits and loss.  Downstream every fp32 value passes W6 quantisers (relative step 2^-5 of its block's maximum): two
    #     implementations whose Linear outputs differ in the last bit (summation order) round a handful of the ~10^6
    #     activations per tensor to different neighbours, and a moved value moves the roundings behind it -- the numpy oracle
    #     against the reference's own logits shows the same (Llama-7B width: max 0.25, mean 0.016 of 5.6;
    #     tests/test_oracle_models.py).  Hence: the tight bound where the run stays on the reference's roundings, a
    #     statistical one (mean error, loss) where it does not.
    d = np.abs(logits.cpu().numpy() - ref_logits)
    scale = float(np.abs(ref_logits).max())
    dl = abs(float(loss) - ref_loss)
    print(f"{tag} [{knobs}]: attn0 rel err {ea:.2e}; logits max {d.max():.2e} mean {d.mean():.2e} of {scale:.2f}; |dloss| {dl:.2e}")
    assert ea < 1e-5, ea
    assert d.mean() < 5e-3 * scale and d.max() < 0.1 * scale, (float(d.max()), float(d.mean()))
    assert dl < 5e-3, (float(loss), ref_loss)
    # (3) every Linear of the run, teacher-forced: the oracle's steady-state PTQ Linear (linear.py:63-71 in float64) on the
    #     very input the module saw and the fixture's un-quantised weights -- the GEMM's usual bound at K = 2048 ... 11008
    from oracle import np_oracle as O
    ref_name = (lambda n: "model.decoder." + n) if m["family"] == "opt" else \
        (lambda n: "model." + n.replace(".gate_proj", ".mlp.gate_proj").replace(".up_proj", ".mlp.up_proj").replace(".down_proj", ".mlp.down_proj"))
    worst = 0.0
    for name, (xin, yout) in io.items():
        w0, b0 = sd[ref_name(name) + ".weight"], sd.get(ref_name(name) + ".bias")
        want = O.linear_ptq(xin.cpu().numpy().reshape(-1, xin.shape[-1]), w0, b0, dict(m["quant_config"]["default"]))[0]
        e = float(np.abs(yout.cpu().numpy().reshape(want.shape) - want).max() / np.abs(want).max())
        worst = max(worst, e)
        assert e < 4e-6, (name, e)
    if io and not c3:
        print(f"{tag}: {len(io)} Linear layers teacher-forced against the oracle, worst relative error {worst:.2e}")
        assert len(io) == (6 if m["family"] == "opt" else 7) * m["num_layers"]
    if c3:
        print(f"{tag} [{knobs}]: {len(io)} Linear layers teacher-forced against the oracle, worst relative error {worst:.2e}")


_G5W2 = _json.loads((_GOLDEN / "models_wide2.json").read_text())


@pytest.mark.parametrize("knobs", ["plain", "every_knob", "config3"])
@pytest.mark.parametrize("tag", sorted(_G5W2))
def test_reference_model_fixture_wide2(tag, knobs):
    _fixture_wide2(tag, knobs)


@pytest.mark.parametrize("tag", sorted(t for t in _G5W2 if _G5W2[t]["family"] == "llama"))
def test_reference_model_fixture_wide2_config3_hybrid(tag):
    """config 3's switches with mi355q_weight_storage = hybrid"""
    _fixture_wide2(tag, "config3_hybrid")


# as _CONFIG3_HOOKED / _CONFIG3_REACHED, for the wide2 fixtures (keyed by tag: the T = 2048 cases run batch 1, so the attention
# pass can write o_proj's / out_proj's operand there)
# (first MI355X run: the Llama T = 2048 case reaches the attention consumer; OPT's out_proj is not on the per-block route in either
#  OPT case, so no OPT fixture reaches it -- held by tests/test_gpu_fused_oracle.py instead; no case reaches the mixed contraction)
_CONFIG3_HOOKED_W2 = {"llama7b_width_w6a6_t2048": [], "opt1p3b_width_w6a6_t2048": [],
                      "opt1p3b_width_w4a4_mixed": ["layers.0.self_attn.k_proj", "layers.0.self_attn.q_proj", "layers.0.self_attn.v_proj"]}
_CONFIG3_REACHED_W2 = {"llama7b_width_w6a6_t2048": ["attention", "attention_consumer", "attention_rope", "gated", "residual"],
                       "opt1p3b_width_w6a6_t2048": ["attention", "relu", "residual"],
                       "opt1p3b_width_w4a4_mixed": ["attention", "relu", "residual"]}


def _fixture_wide2(tag, knobs):
    """tools/gen_golden_models.py --wide2, the reference's own numbers for (1) OPT-1.3B width under W4A4 with MIXED per-layer
    widths (BASELINE config 4's kind: experiments/emnlp/configs/search/opt_1.3b_sst2.toml:24-37) and (2), (3) one T = 2048 case
    per family at OPT-1.3B / Llama-7B width (the one-pass attention kernel at its full length against reference-produced
    numbers; loss, 64 sampled logit rows and the same rows of the first layer's attention output are in the fixture)"""
    import torch
    from mi355q import harness as H
    from oracle import np_models as NM
    data = np.load(_GOLDEN / "models_wide2.npz")
    m = _G5W2[tag]
    sd, ids, ref_loss = NM.weights_from_recipe(m), data[tag + "/input_ids"], m["loss"]
    sampled = "sampled_rows" in m
    kn = {} if knobs == "plain" else dict(mi355q_grouped_linear=True, mi355q_fused_norm=True, mi355q_fused_activation=True,
                                          mi355q_fused_attention=True, mi355q_token_major_output=True)
    if knobs == "plain" and sampled:
        kn = dict(mi355q_fused_attention=True)       # (the stepped attention at T = 2048 needs [32, 2048, 2048] tensors: one-pass only)
    c3 = knobs.startswith("config3")
    if c3:
        kn = _config3_knobs(knobs)
    if m["family"] == "opt":
        cfg = H.TinyOPTConfig(vocab_size=m["vocab_size"], hidden_size=m["hidden_size"], ffn_dim=m["ffn_dim"],
                              num_layers=m["num_layers"], num_heads=m["num_heads"], max_positions=m["max_positions"])
        model = H.TinyOPTForCausalLM(cfg, H.expand_quant_config(_with_knob(m["quant_config"], **kn), cfg.num_layers))
    else:
        cfg = H.TinyLlamaConfig(vocab_size=m["vocab_size"], hidden_size=m["hidden_size"], intermediate_size=m["intermediate_size"],
                                num_layers=m["num_layers"], num_heads=m["num_heads"], max_positions=m["max_positions"],
                                rms_eps=m["rms_eps"])
        model = H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(_with_knob(m["quant_config"], **kn), cfg.num_layers))
    model.load_reference_state_dict(sd).to("cuda:0").eval()
    taps, io = {}, {}
    if c3:
        model.mi355q_lm_head = CONFIG3_LM_HEAD
        model.layers[0].self_attn.register_forward_hook(
            lambda mod, i, k, o: taps.update(attn0=o.detach(), res0=k.get("residual")), with_kwargs=True)
        from mi355q.quantize import get_quantized_cls
        lin_cls = get_quantized_cls("linear", m["quant_config"]["default"])
        for name, mod in model.named_modules():
            if isinstance(mod, lin_cls) and name.startswith("layers."):
                mod.register_forward_hook(lambda mod, i, o, name=name: io.__setitem__(name, True))
    else:
        model.layers[0].self_attn.register_forward_hook(lambda mod, i, o: taps.__setitem__("attn0", o.detach()))
    t = torch.from_numpy(ids).to("cuda:0")
    with torch.no_grad():
        for f in range(2):
            if c3 and f == 1:
                io.clear()
                counts, restore = _route_census()
            try:
                logits, loss = model(t, labels=t)
            finally:
                if c3 and f == 1:
                    restore()
    if c3:
        _assert_config3_routes(f"{tag} [{knobs}]", tag, counts, io, _CONFIG3_HOOKED_W2, _CONFIG3_REACHED_W2)
    a = taps["attn0"].reshape(ids.shape[0], ids.shape[1], -1)[:, :, :128].cpu().numpy()
    x0 = taps["res0"].reshape(ids.shape[0], ids.shape[1], -1)[:, :, :128].cpu().numpy() if c3 else None
    lg = logits.cpu().numpy()
    if sampled:
        rows = data[tag + "/rows"]
        ref_attn, ref_logits = data[tag + "/attn0_rows"], data[tag + "/logits_rows"]
        a, lg = a[0, rows], lg[0, rows]
        x0 = None if x0 is None else x0[0, rows]
    else:
        ref_attn, ref_logits = data[tag + "/attn0"], data[tag + "/logits"]
    ea = float(np.abs(a - ref_attn).max() / np.abs(ref_attn).max())
    if c3:                                                   # out - x: the attn0 bound plus the rounding of the add, 2^-23 max|x|
        a = a - x0
        ea = max(0.0, float(np.abs(a - ref_attn).max()) - 2.0 ** -23 * float(np.abs(x0).max())) / float(np.abs(ref_attn).max())
    d = np.abs(lg - ref_logits)
    scale = float(np.abs(ref_logits).max())
    dl = abs(float(loss) - ref_loss)
    print(f"{tag} [{knobs}]: attn0 rel err {ea:.2e}; logits max {d.max():.2e} mean {d.mean():.2e} of {scale:.2f}; |dloss| {dl:.2e}")
    # the first layer's attention output: tight for the W6A6 cases; under the 3- / 4-bit widths of the mixed case a last-bit
    # difference in a projection moves a mantissa by one of 4 steps -- bounded like the logits there
    assert ea < (1e-5 if "w6a6" in tag and not sampled else 2e-3 if "w6a6" in tag else 0.1), ea
    assert d.mean() < 5e-3 * scale and d.max() < 0.1 * scale, (float(d.max()), float(d.mean()))
    assert dl < 5e-3, (float(loss), ref_loss)


def test_fused_softmax_model_parity():
    """the harness with softmax folded into the P V product (config["mi355q_fused_softmax"], T long enough for the fused
    entry point) against the three-step route and the oracle"""
    import torch
    from mi355q.harness import TinyOPTConfig, TinyOPTForCausalLM, expand_quant_config
    d = dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
             data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127,
             weight_block_size=[1, 16], bias_width=6, bias_exponent_width=8, bias_exponent_bias=127, bias_block_size=[16])
    cfg = TinyOPTConfig(vocab_size=256, hidden_size=128, ffn_dim=256, num_layers=2, num_heads=2, max_positions=256)
    torch.manual_seed(5)
    ids = torch.randint(0, cfg.vocab_size, (1, 256))
    losses = {}
    for fused in (False, True):
        torch.manual_seed(6)
        model = TinyOPTForCausalLM(cfg, expand_quant_config(dict(d, mi355q_fused_softmax=fused), cfg.num_layers))
        with torch.no_grad():
            for n, p in model.named_parameters():
                if p.ndim == 2 and "embed" not in n:
                    p.mul_(4.0)
        if not fused:
            ref_loss = _oracle_forward(model, d, ids.numpy())
        model = model.to("cuda:0")
        with torch.no_grad():
            losses[fused] = float(model(ids.to("cuda:0"), labels=ids.to("cuda:0"))[1])
    assert abs(losses[True] - ref_loss) < 3e-4 and abs(losses[False] - ref_loss) < 3e-4, (losses, ref_loss)


@pytest.mark.parametrize("family", ["opt", "llama"])
def test_grouped_projections_model_bit_identical(family):
    """config["mi355q_grouped_linear"]: q / k / v (and Llama's gate / up) through ONE quantisation + ONE tile-GEMM launch:
    logits bit-identical to the layers called one by one (second forward: the first one packs the weights)"""
    import torch
    from mi355q import harness as H, ops
    base = dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
                data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127,
                weight_block_size=[1, 16], bias_width=6, bias_exponent_width=8, bias_exponent_bias=127, bias_block_size=[16],
                mi355q_fused_attention=True, mi355q_align="rows")
    outs, multi_calls = [], []
    for grouped in (False, True):
        torch.manual_seed(7)
        qc = dict(base, mi355q_grouped_linear=grouped)
        if family == "opt":
            cfg = H.TinyOPTConfig(vocab_size=512, hidden_size=256, ffn_dim=512, num_layers=2, num_heads=4, max_positions=512)
            m = H.TinyOPTForCausalLM(cfg, H.expand_quant_config(qc, cfg.num_layers))
        else:
            cfg = H.TinyLlamaConfig(vocab_size=512, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=4, max_positions=512)
            m = H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(qc, cfg.num_layers))
        m = m.to("cuda:0").eval()
        ids = torch.randint(0, cfg.vocab_size, (1, 320), generator=torch.Generator().manual_seed(1)).to("cuda:0")
        real = ops.bfp_gemm_aligned_multi
        ops.bfp_gemm_aligned_multi = lambda *a, **k: (multi_calls.append(grouped), real(*a, **k))[1]
        try:
            with torch.no_grad():
                m(ids)
                outs.append(m(ids)[0].clone())
        finally:
            ops.bfp_gemm_aligned_multi = real
    assert torch.equal(outs[0], outs[1])
    assert multi_calls and all(multi_calls), multi_calls          # (the grouped launch really ran, and only with the knob)


@pytest.mark.parametrize("family,align", [("opt", "auto"), ("opt", "rows"), ("llama", "auto"), ("llama", "rows")])
def test_fused_activation_model_bit_identical(family, align):
    """config["mi355q_fused_activation"]: relu (OPT fc2) / silu(gate) * up (Llama down_proj) read by the layer's own x
    quantiser (Linear.forward_after) instead of torch kernels in front of it: logits bit-identical (second forward:
    the first one packs the weights and runs the torch ops)"""
    import torch
    from mi355q import harness as H, ops
    base = dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
                data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127,
                weight_block_size=[1, 16], bias_width=6, bias_exponent_width=8, bias_exponent_bias=127, bias_block_size=[16],
                mi355q_fused_attention=True, mi355q_align=align)
    outs, pre_calls = [], []
    for fused in (False, True):
        torch.manual_seed(7)
        qc = dict(base, mi355q_fused_activation=fused)
        if family == "opt":
            cfg = H.TinyOPTConfig(vocab_size=512, hidden_size=256, ffn_dim=512, num_layers=2, num_heads=4, max_positions=512)
            m = H.TinyOPTForCausalLM(cfg, H.expand_quant_config(qc, cfg.num_layers))
        else:
            cfg = H.TinyLlamaConfig(vocab_size=512, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=4, max_positions=512)
            m = H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(qc, cfg.num_layers))
        m = m.to("cuda:0").eval()
        ids = torch.randint(0, cfg.vocab_size, (1, 320), generator=torch.Generator().manual_seed(1)).to("cuda:0")
        real_t, real_r = ops.block_fp_quantize_bf16_tiled, ops.block_fp_quantize_aligned_rows
        ops.block_fp_quantize_bf16_tiled = lambda *a, **k: (pre_calls.append((fused, k.get("pre") is not None)), real_t(*a, **k))[1]
        ops.block_fp_quantize_aligned_rows = lambda *a, **k: (pre_calls.append((fused, k.get("pre") is not None)), real_r(*a, **k))[1]
        try:
            with torch.no_grad():
                m(ids)
                outs.append(m(ids)[0].clone())
        finally:
            ops.block_fp_quantize_bf16_tiled, ops.block_fp_quantize_aligned_rows = real_t, real_r
    assert torch.equal(outs[0], outs[1])
    assert any(f and p for f, p in pre_calls) and not any(p and not f for f, p in pre_calls), pre_calls


@pytest.mark.parametrize("family", ["opt", "llama"])
def test_all_knobs_together_model_bit_identical(family):
    """one-pass attention with token-major output + grouped projections + activation inside the x quantiser, all at once,
    against one-pass attention alone: bit-identical logits, eager and replayed as a HIP graph"""
    import torch
    from mi355q import harness as H
    from mi355q.graphs import GraphedForward
    base = dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
                data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127,
                weight_block_size=[1, 16], bias_width=6, bias_exponent_width=8, bias_exponent_bias=127, bias_block_size=[16],
                mi355q_fused_attention=True)
    outs = []
    for on in (False, True):
        torch.manual_seed(7)
        qc = dict(base, mi355q_grouped_linear=on, mi355q_fused_activation=on, mi355q_token_major_output=on)
        if family == "opt":
            cfg = H.TinyOPTConfig(vocab_size=512, hidden_size=256, ffn_dim=512, num_layers=2, num_heads=4, max_positions=512)
            m = H.TinyOPTForCausalLM(cfg, H.expand_quant_config(qc, cfg.num_layers))
        else:
            cfg = H.TinyLlamaConfig(vocab_size=512, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=4, max_positions=512)
            m = H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(qc, cfg.num_layers))
        m = m.to("cuda:0").eval()
        ids = torch.randint(0, cfg.vocab_size, (1, 320), generator=torch.Generator().manual_seed(1)).to("cuda:0")
        with torch.no_grad():
            m(ids)
            outs.append(m(ids)[0].clone())
            if on:
                g = GraphedForward(lambda t: m(t)[0], (ids,))
                outs.append(g(ids).clone())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])


@pytest.mark.parametrize("tag", sorted(t for t in _G5 if _G5[t]["hidden_size"] == 128))
def test_reference_model_fixture_every_knob(tag):
    """the reference's own logits against the harness with every implementation knob on (one-pass attention with token-major
    output, grouped projections, activation and -- Llama -- RMSNorm inside the x quantisers), second forward (the first one
    packs the weights and decides the routes).  Same tolerances as the plain harness (the fused norm's own summation order
    moves the logits by ~1e-6 here)."""
    from mi355q import ops
    knobs = dict(mi355q_fused_attention=True, mi355q_token_major_output=True, mi355q_grouped_linear=True,
                 mi355q_fused_activation=True, mi355q_fused_norm=True)
    pres, real = [], ops.block_fp_quantize_aligned_rows
    ops.block_fp_quantize_aligned_rows = lambda *a, **k: (pres.append(k.get("pre")), real(*a, **k))[1]
    try:
        _check_fixture(tag, knobs, forwards=2)
    finally:
        ops.block_fp_quantize_aligned_rows = real
    if "mixed" not in tag:
        kind = "rmsnorm" if _G5[tag]["family"] == "llama" else "layernorm"
        assert sum(1 for p in pres if p is not None and p[0] == kind) == 4, pres           # (two norms a layer, two layers)


@pytest.mark.parametrize("tag", sorted(t for t in _G5 if _G5[t]["family"] == "llama" and "mixed" not in t))
def test_fused_norm_knobs_only_in_the_linear_section(tag):
    """the knobs ride per node: set for the Linear layers only (a [linear] section, as search results are saved), the
    decoder layer asks its attention module for the fused norm while that module's own matmul nodes do not group the
    projections -- the norm must then be applied in front of q / k / v, never skipped: the reference's logits"""
    import torch
    from mi355q import harness as H
    from oracle import np_models as NM
    data = np.load(_GOLDEN / "models.npz")
    sd, _, ids, ref_logits, ref_loss, m = NM.load_fixture(_G5, data, tag)
    cfg = H.TinyLlamaConfig(vocab_size=m["vocab_size"], hidden_size=m["hidden_size"], intermediate_size=m["intermediate_size"],
                            num_layers=m["num_layers"], num_heads=m["num_heads"], max_positions=m["max_positions"], rms_eps=m["rms_eps"])
    qc = H.expand_llama_quant_config(m["quant_config"], cfg.num_layers)
    for i in range(cfg.num_layers):             # the Linear nodes only: not rotary / matmul_0 / matmul_1
        layer_qc = qc[f"model_layer_{i}"]
        for node in [layer_qc["mlp"][n] for n in ("gate_proj", "up_proj", "down_proj")] + \
                    [layer_qc["self_attn"][n] for n in ("q_proj", "k_proj", "v_proj", "o_proj")]:
            node.update(mi355q_grouped_linear=True, mi355q_fused_norm=True)
    model = H.TinyLlamaForCausalLM(cfg, qc)
    layer = model.layers[0]
    assert layer.gate_proj.config.get("mi355q_fused_norm") and not layer.self_attn.qc["matmul_1"].get("mi355q_grouped_linear", False)
    model.load_reference_state_dict(sd).to("cuda:0").eval()
    t = torch.from_numpy(ids).to("cuda:0")
    with torch.no_grad():
        for _ in range(2):
            logits, loss = model(t, labels=t)
    err = float(np.abs(logits.cpu().numpy() - ref_logits).max())
    assert err < 1e-3 * max(1.0, float(np.abs(ref_logits).max())), err
    assert abs(float(loss) - ref_loss) < 2e-5


@pytest.mark.parametrize("arith,products", [("block_log", "fp32"), ("block_minifloat", "fp32"), ("block_minifloat", "bf16")])
def test_tiny_llama_loss_parity_other_block_arithmetics(arith, products):
    """BASELINE configs 3 / 5 name Llama with block_minifloat and block_log: the Llama-style harness under those
    arithmetics (HIP fake-quantisers, products of the Linear layers on the bf16 tile GEMM, the registry's matmul / rotary
    functions of that arithmetic) against the oracle's model forward.  `products`: the 4-D attention products through the
    fp32 fake-quantised tensors, or (block_minifloat's default) as bf16 operands on bf16 MFMAs -- every product within 4e-8
    of the other route (summation order), but this model (weights x 40: a loss of 37) turns last-bit differences into
    rounding flips: its loss moves by 0.4 %, so the bf16 route is held to 1 % here and to 2e-6 per product in
    tests/test_gpu_modules.py::test_block_minifloat_and_block_log_products_on_bf16_mfma"""
    import torch
    from mi355q import ops
    from mi355q.harness import TinyLlamaConfig, TinyLlamaForCausalLM, eval_lm_perplexity, expand_llama_quant_config
    if arith == "block_log":
        d = dict(name="block_log", is_ptq=True, bypass=False, data_in_width=8, data_in_exponent_bias_width=8,
                 data_in_block_size=[1, 16], weight_width=8, weight_exponent_bias_width=8, weight_block_size=[1, 16],
                 bias_width=8, bias_exponent_bias_width=8, bias_block_size=[16])
    else:
        d = dict(name="block_minifloat", is_ptq=True, bypass=False, data_in_width=8, data_in_exponent_width=4,
                 data_in_exponent_bias_width=8, data_in_block_size=[1, 16], weight_width=8, weight_exponent_width=4,
                 weight_exponent_bias_width=8, weight_block_size=[1, 16], bias_width=8, bias_exponent_width=4,
                 bias_exponent_bias_width=8, bias_block_size=[16])
    d["mi355q_values_matmul"] = products
    torch.manual_seed(1)
    cfg = TinyLlamaConfig(vocab_size=384, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=4, max_positions=64)
    model = TinyLlamaForCausalLM(cfg, expand_llama_quant_config(d, cfg.num_layers))
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.ndim == 2 and "embed" not in n:
                p.mul_(40.0 if arith == "block_minifloat" else 4.0)      # (quirk 5: minifloat blocks below 2 quantise to zeros)
    ids = torch.randint(0, cfg.vocab_size, (2, 48))
    ref_loss = _oracle_llama_forward(model, d, ids.numpy())
    model = model.to("cuda:0")
    calls, real = [], ops.bf16_gemm_tiled
    ops.bf16_gemm_tiled = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        res = eval_lm_perplexity(model, [ids], device="cuda:0")
        res2 = eval_lm_perplexity(model, [ids], device="cuda:0")
    finally:
        ops.bf16_gemm_tiled = real
    assert len(calls) == 2 * 2 * 7                                     # (every Linear of both forwards took the tile GEMM)
    tol = 5e-4 if products == "fp32" else 1e-2
    assert abs(res["loss"] - ref_loss) < tol * max(1.0, abs(ref_loss)), (res["loss"], ref_loss)
    assert abs(res2["loss"] - res["loss"]) < 1e-6


# ---- trained weights: perplexity as eval/eval_lm.py computes it, on a model that is not noise ------------------------------
_TRAINED = _json.loads((_GOLDEN / "trained.json").read_text()) if (_GOLDEN / "trained.json").exists() else {}

# the fused paths the last config-3 forward took (count > 0), per fixture and widths
# (first MI355X run: Llama W6A6 reaches the attention consumer in 2 of its 4 layers -- the o_proj layers on the per-block route --,
#  Llama W4A4 and OPT in none; hidden 128 has no gated / relu epilogue; no mixed contraction)
_CONFIG3_REACHED_TRAINED = {"llama_trained/w6a6": ["attention", "attention_consumer", "attention_rope", "residual"],
                            "llama_trained/w4a4": ["attention", "attention_rope", "residual"],
                            "opt_trained/w6a6": ["attention", "residual"], "opt_trained/w4a4": ["attention", "residual"]}


@pytest.mark.parametrize("knobs", ["plain", "every_knob", "config3"])
@pytest.mark.parametrize("name", ["w6a6", "w4a4"])
@pytest.mark.parametrize("tag", sorted(_TRAINED))
def test_perplexity_on_trained_weights(tag, name, knobs):
    """BASELINE north_star: "identical Wikitext2 perplexity to 3 d.p." -- on the only trained weights this project can have (no
    checkpoint, no network): a 4-layer byte-level OPT-style and Llama-style LM trained here WITH THE REFERENCE'S OWN CLASSES in
    bypass mode (tools/gen_trained_fixture.py; train loss 1.4 / 0.7 nats per byte), evaluated by the reference's quantised
    classes over 16 chunks of 512 held-out tokens exactly as eval/eval_lm.py:41-63 does.  The harness on the GPU must give the
    reference's perplexity.  How tight "the same" can be is measured, not assumed: the fixture holds the reference against
    ITSELF with every Linear output moved by one fp32 ulp (what any other GEMM summation order does) -- its perplexity moves
    by 1e-3 ... 5e-2 (W6A6) and 6e-3 ... 2e-1 (W4A4): a W6 / W4 rounding flips and the flip propagates, on trained weights as on
    random ones.  So the bound here is the reference's own spread; the measured differences are printed and recorded in
    profiles/r05_trained_perplexity.jsonl (W6A6: inside 3 d.p. for OPT, 2e-3 for Llama)."""
    import torch
    from mi355q import harness as H
    data = np.load(_GOLDEN / "trained.npz")
    m = _TRAINED[tag]
    ev = m["evals"][name]
    pre = tag + "/w/"
    sd = {k[len(pre):]: data[k].astype(np.float32) for k in data.files if k.startswith(pre)}
    kn = {} if knobs == "plain" else dict(mi355q_grouped_linear=True, mi355q_fused_norm=True, mi355q_fused_activation=True,
                                          mi355q_fused_attention=True, mi355q_token_major_output=True)
    if knobs == "config3":
        kn = CONFIG3_KNOBS
    if m["family"] == "opt":
        cfg = H.TinyOPTConfig(vocab_size=m["vocab_size"], hidden_size=m["hidden_size"], ffn_dim=m["ffn_dim"], num_layers=m["num_layers"],
                              num_heads=m["num_heads"], max_positions=m["max_positions"])
        model = H.TinyOPTForCausalLM(cfg, H.expand_quant_config(_with_knob(ev["quant_config"], **kn), cfg.num_layers))
    else:
        cfg = H.TinyLlamaConfig(vocab_size=m["vocab_size"], hidden_size=m["hidden_size"], intermediate_size=m["intermediate_size"],
                                num_layers=m["num_layers"], num_heads=m["num_heads"], max_positions=m["max_positions"], rms_eps=m["rms_eps"])
        model = H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(_with_knob(ev["quant_config"], **kn), cfg.num_layers))
    model.load_reference_state_dict(sd).to("cuda:0").eval()
    if knobs == "config3":
        model.mi355q_lm_head = CONFIG3_LM_HEAD
    chunks = torch.from_numpy(data["input_ids"])
    ref_chunks = data[f"{tag}/{name}/chunk_losses"]
    losses = []
    with torch.no_grad():
        model(chunks[0][None].to("cuda:0"))        # (the first forward quantises and packs the weights; the knobs act from the second on)
        for c in chunks:
            if knobs == "config3" and len(losses) == len(chunks) - 1:
                counts, restore = _route_census()  # (the last forward: which of config 3's fused paths ran)
            try:
                _, loss = model(c[None].to("cuda:0"), labels=c[None].to("cuda:0"))
            finally:
                if knobs == "config3" and len(losses) == len(chunks) - 1:
                    restore()
            losses.append(float(loss))
    if knobs == "config3":
        # route census (hidden 128: no gated / relu MLP epilogue, which needs in_features >= 256)
        assert counts["gated"] == counts["relu"] == 0
        assert counts["attention"] == m["num_layers"] and counts["attention_rope"] == (m["num_layers"] if m["family"] == "llama" else 0)
        _assert_config3_routes(f"{tag} {name} [config3]", f"{tag}/{name}", counts, {}, {}, _CONFIG3_REACHED_TRAINED)
    res = H.eval_lm_perplexity(model, [c[None] for c in chunks], device="cuda:0")       # (the harness's eval_lm loop: same number)
    ppl = math.exp(sum(losses) / len(losses))
    assert abs(res["perplexity"] - ppl) < 1e-9 * ppl and res["num_samples"] == 16 and res["seq_len"] == 512
    d_chunk = float(np.abs(np.asarray(losses) - ref_chunks).max())
    d_ppl = ppl - ev["perplexity"]
    spread = max(abs(r["d_perplexity"]) for r in ev["control"]["runs"])
    spread_chunk = max(r["max_d_chunk_loss"] for r in ev["control"]["runs"])
    print(f"{tag} {name} [{knobs}]: ppl {ppl:.5f} vs reference {ev['perplexity']:.5f} (d {d_ppl:+.2e}; the reference against itself "
          f"under 1-ulp jitter: {spread:.1e}); max |d chunk loss| {d_chunk:.2e} (reference: {spread_chunk:.1e}); "
          f"3 d.p.: {round(ppl, 3)} vs {round(ev['perplexity'], 3)}")
    import os
    if os.path.isdir("gpurun_out"):                                    # (scratch on the GPU box; the committed copy: profiles/)
        with open("gpurun_out/r05_trained_perplexity.jsonl", "a") as f:
            f.write(_json.dumps({"model": tag, "config": name, "knobs": knobs, "perplexity": round(ppl, 6), "reference_perplexity": round(ev["perplexity"], 6),
                                 "d_perplexity": round(d_ppl, 6), "same_to_3dp": round(ppl, 3) == round(ev["perplexity"], 3),
                                 "reference_vs_itself_1ulp_jitter": round(spread, 5), "max_d_chunk_loss": round(d_chunk, 6),
                                 "reference_vs_itself_chunk": round(spread_chunk, 5), "bypass_perplexity": round(m["evals"]["bypass"]["perplexity"], 4)}) + "\n")
    assert abs(d_ppl) <= spread and d_chunk <= spread_chunk, (d_ppl, spread, d_chunk, spread_chunk)
    assert abs(d_ppl) < 1e-3 * ev["perplexity"]                       # (and in any case a per-mille of the perplexity)
    assert ppl < 1.05 * m["evals"]["bypass"]["perplexity"]            # (the quantised model is still the language model it was)


def test_opt125m_shape_twelve_layers_vs_oracle():
    """BASELINE config 0's MODEL SHAPE on the GPU (configuration_opt.py:100-112 -- hidden 768, FFN 3072, 12 heads x 64,
    12 layers) at the perplexity loop's sequence length (T = 2048, eval_wikitext2.sh:51-52), W6A6 block_fp [1,16], random seeded
    weights (no checkpoint offline): (1) EVERY quantised Linear of the run -- the six per layer, 72 in all, at M = 2048 tokens --
    against the oracle's steady-state PTQ Linear on sampled rows of the very input it saw (teacher-forced: summation-order noise
    only, <= 1e-6); the four projections fed by a LayerNorm and fc1 must be on the int8 row-scale route; (2) the end-to-end loss
    against the numpy oracle's forward of the same network.  At this depth fp32 arithmetic itself does not pin the loss more
    tightly than 4e-4 ... 5e-3 (the oracle against itself under 1-ulp jitter, profiles/r02_depth_control.jsonl; measured GPU
    against oracle: 3.1e-3, profiles/r03_teacher_forced_depth.jsonl): the bound here is 8e-3."""
    import torch
    from mi355q.harness import TinyOPTConfig, TinyOPTForCausalLM, expand_quant_config
    from mi355q.quantize.quantized_modules.linear import _LinearBase
    from oracle import np_oracle as O
    W6A6 = dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
                data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127,
                weight_block_size=[1, 16], bias_width=6, bias_exponent_width=8, bias_exponent_bias=127, bias_block_size=[16])
    torch.manual_seed(0)
    T = 2048
    cfg = TinyOPTConfig(vocab_size=2048, hidden_size=768, ffn_dim=3072, num_layers=12, num_heads=12, max_positions=T)
    model = TinyOPTForCausalLM(cfg, expand_quant_config(W6A6, cfg.num_layers))
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.ndim == 2 and "embed" not in n:
                p.mul_(2.0)
    ids = torch.randint(0, cfg.vocab_size, (1, T))
    w0 = {n: (m.weight.detach().clone().numpy(), None if m.bias is None else m.bias.detach().clone().numpy())
          for n, m in model.named_modules() if isinstance(m, _LinearBase) and n.startswith("layers.")}
    assert len(w0) == 72
    ref_loss = _oracle_forward(model, W6A6, ids.numpy())
    dev = torch.device("cuda:0")
    model = model.to(dev)
    rng = np.random.default_rng(3)
    io, routes = {}, {}

    def tap(name):
        def hook(mod, inp, out):
            x2, y2 = inp[0].detach().reshape(-1, inp[0].shape[-1]), out.detach().reshape(-1, out.shape[-1])
            pick = np.sort(rng.choice(x2.shape[0], size=24, replace=False))
            pt = torch.from_numpy(pick).to(x2.device)
            io[name] = (x2[pt].cpu().numpy(), y2[pt].cpu().numpy())
            routes[name] = "bf16" if mod._uses_bf16_route() else ("int8" if mod._packed is not None and mod._packed[0] is not None else "other")
        return hook
    for n, m in model.named_modules():
        if n in w0:
            m.register_forward_hook(tap(n))
    with torch.no_grad():
        loss = float(model(ids.to(dev), labels=ids.to(dev))[1])
    assert len(io) == 72
    worst = 0.0
    for n, (xin, yout) in io.items():
        w, b = w0[n]
        want = O.linear_ptq(xin, w, b, W6A6)[0]
        worst = max(worst, float(np.abs(yout - want).max() / np.abs(want).max()))
        if not n.endswith(("fc2", "out_proj")):              # q / k / v / fc1: fed by a LayerNorm -- rows fit one exponent window
            assert routes[n] == "int8", (n, routes[n])
    assert worst <= 1e-6, worst
    assert abs(loss - ref_loss) <= 8e-3, (loss, ref_loss)
