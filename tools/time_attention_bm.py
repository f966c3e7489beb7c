"""One layer's attention core with two block_minifloat (8, 4, 8) products at [8 x 12, 2048, 64] (OPT-125m, 8 sequences; causal, q_scale) and
[32, 2048, 128] causal with scale_div (Llama-7B), three calls:
  (a) one_pass   the registry's "attention" function: ops.bm_attention (pack launch + streaming kernel)
  (b) steps      the same call with mi355q_fused_matmul=False: the first product, [heads, T, T] scores, the mask add, the softmax, a second
                 [heads, T, T] tensor, the second product -- what a block_minifloat layer ran before the one-pass kernel
  (c) block_fp   ops.bfp_attention at width 8 on the same shapes: what the structure can do (packed Q fragments, the resident-score
                 kernel at T <= 2048)
HIP events over `--calls` calls, `--repeats` times each, after warm-up calls of each; one JSON line a shape with the medians, the spread
(min .. max of the repeats), (a)/(b), (a)/(c), and whether (a) lies below (b) by more than (b)'s own min .. max spread.
Run on the GPU from the repository root:  python tools/time_attention_bm.py --out profiles/attention_bm.jsonl"""
import argparse
import json
import math
import statistics
import sys

sys.path.insert(0, "llm-mixed-q_amd")
sys.path.insert(0, ".")
import torch  # noqa: E402

import mi355q.quantize as Q  # noqa: E402
from mi355q import ops  # noqa: E402


def bm_cfg(**knobs):
    return dict(name="block_minifloat", is_ptq=True, bypass=False, data_in_width=8, data_in_exponent_width=4, data_in_exponent_bias_width=8,
                data_in_block_size=[1, 16], weight_width=8, weight_exponent_width=4, weight_exponent_bias_width=8, weight_block_size=[1, 16],
                **knobs)


def timed(fn, calls, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(e) / calls * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    on, off = bm_cfg(), bm_cfg(mi355q_fused_matmul=False)
    att = Q.get_quantized_func("attention", on)
    par8 = (8, 8, 127, 8, 8, 127)
    lines = []
    for name, B, T, hd, causal, scale, q_scale in (("OPT-125m x 8", 96, 2048, 64, True, None, 64 ** -0.5),
                                                   ("Llama-7B", 32, 2048, 128, True, math.sqrt(128), None)):
        g = torch.Generator().manual_seed(0)
        q, k, v = (torch.randn(B, T, hd, generator=g).to(dev) for _ in range(3))
        q = q * 3.0
        kw = dict(causal=causal, scale_div=scale, q_scale=q_scale)
        calls = {"one_pass": lambda: att(q, k, v, on, on, **kw),
                 "steps": lambda: att(q, k, v, off, off, **kw),
                 "block_fp": lambda: ops.bfp_attention(q, k, v, par8, par8, **kw)}
        spy, real = [], ops.bm_attention
        ops.bm_attention = lambda *a, **k_: (spy.append(1), real(*a, **k_))[1]
        try:
            got, ref = calls["one_pass"](), calls["steps"]()
        finally:
            ops.bm_attention = real
        assert len(spy) == 1, "the one-pass call did not take ops.bm_attention, or the stepped call did"
        err = float((got - ref).abs().max() / ref.abs().max())
        del got, ref
        r = {"shape": f"{name}: q, k, v [{B}, {T}, {hd}], causal, {'scale_div' if scale else 'q_scale'}, block_minifloat (8, 4, 8)",
             "one_pass_vs_steps_max_rel": round(err, 7)}
        med, spread = {}, {}
        for label, fn in calls.items():
            t = timed(fn, args.calls if label != "steps" else max(2, args.calls // 4), args.repeats)
            med[label], spread[label] = statistics.median(t), max(t) - min(t)
            r[f"{label}_us"] = round(med[label], 1)
            r[f"{label}_us_min_max"] = [round(min(t), 1), round(max(t), 1)]
        r["one_pass_over_steps"] = round(med["one_pass"] / med["steps"], 4)
        r["one_pass_over_block_fp"] = round(med["one_pass"] / med["block_fp"], 3)
        r["below_steps_by_more_than_its_spread"] = bool(med["steps"] - med["one_pass"] > spread["steps"])
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
