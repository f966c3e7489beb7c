"""One layer's attention core on a PADDED batch (right-padded, causal, real lengths spread over 0.5 .. 1.0 of T) at the OPT-125m shape
(8 sequences x 12 heads, T = 2048, head_dim 64) and the Llama-7B shape (4 x 32, T = 2048, head_dim 128), three calls of the registry's
"attention" function:
  (a) padded   key_mask=[B, T]: ops.bfp_attention_padded, the mask inside the one-pass kernel
  (b) dense    mask=[B, 1, T, T] additive: what a padded batch took before the key mask -- the generic steps (bmm_0, mask + softmax in
               torch, bmm_1) with scores and probabilities [B x heads, T, T] through memory
  (c) causal   no mask at all, the same shape: the floor
HIP events over `--calls` calls, `--repeats` times each; one JSON line a shape with the medians, the spread (min .. max of the repeats)
and the ratios (a)/(b), (a)/(c).  Run on the GPU from the repository root:  python tools/time_attention_padded.py > profiles/attention_padded.jsonl"""
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

cfg = dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
           data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127, weight_block_size=[1, 16])


def timed(fn, calls, repeats):
    for _ in range(3):
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
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    att = Q.get_quantized_func("attention", cfg)
    for name, B, H, T, hd, scale, q_scale in (("OPT-125m", 8, 12, 2048, 64, None, 64 ** -0.5), ("Llama-7B", 4, 32, 2048, 128, math.sqrt(128), None)):
        g = torch.Generator().manual_seed(0)
        q, k, v = (torch.randn(B, H, T, hd, generator=g).to(dev) for _ in range(3))
        lengths = [int(round(T * (0.5 + 0.5 * i / (B - 1)))) for i in range(B)]
        km = (torch.arange(T)[None] < torch.tensor(lengths)[:, None]).to(torch.int32).to(dev)
        dense = torch.where(km != 0, 0.0, torch.finfo(torch.float32).min)[:, None, None, :].expand(B, 1, T, T).contiguous()
        kw = dict(causal=True, scale_div=scale, q_scale=q_scale)
        calls = {"padded": lambda: att(q, k, v, cfg, cfg, key_mask=km, **kw),
                 "dense": lambda: att(q, k, v, cfg, cfg, mask=dense, **kw),
                 "causal": lambda: att(q, k, v, cfg, cfg, **kw)}
        spy, real = [], ops.bfp_attention_padded
        ops.bfp_attention_padded = lambda *a, **k_: (spy.append(1), real(*a, **k_))[1]
        try:
            ref, got = calls["dense"](), calls["padded"]()
        finally:
            ops.bfp_attention_padded = real
        assert len(spy) == 1, "the padded call did not take ops.bfp_attention_padded"
        real_rows = km.bool()[:, None, :, None].expand_as(ref)
        err = float((got - ref)[real_rows].abs().max() / ref.abs().max())
        del ref, got
        r = {"shape": f"{name}: q, k, v [{B}, {H}, {T}, {hd}], causal, right-padded", "real_lengths": lengths,
             "padded_vs_dense_max_rel": round(err, 7)}
        med = {}
        for label, fn in calls.items():
            t = timed(fn, args.calls if label != "dense" else max(2, args.calls // 4), args.repeats)
            med[label] = statistics.median(t)
            r[f"{label}_us"] = round(med[label], 1)
            r[f"{label}_us_min_max"] = [round(min(t), 1), round(max(t), 1)]
        r["padded_over_dense"] = round(med["padded"] / med["dense"], 4)
        r["padded_over_causal"] = round(med["padded"] / med["causal"], 3)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
