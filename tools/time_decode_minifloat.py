#!/usr/bin/env python
"""One decode step of a block_minifloat attention layer -- append of one key a row + attention of M = 1 query -- on three routes, in the
method of tools/time_decode_paged.py: D = 128, 8 KV heads, batch 1 / 8 / 32 (rows = batch x 8), L = 512 / 2048 / 8192 keys.

    minifloat   ops.MinifloatKVCache + ops.bfp_attention_decode (csrc/mi355q_kvbm.hip)
    block_fp    ops.KVCache at the same shapes: the parent's kernels and the floor the new ones should approach -- the same bytes are
                read, only VALU work (the quantisers) and phase B's second accumulator differ
    fp32        what DecodeState(mode="fp32") runs for such a layer, the route the cache replaces: torch.cat of the fp32 K / V with
                the new key, then the registry's matmul -> scale -> softmax -> matmul on all L keys

The outputs of `minifloat` and `fp32` are compared first (peaked queries; worst difference over max|ref| is recorded).  Per case the
step runs over distinct caches -- as many as make one timed window read more than the 256-MiB memory-side cache, capped at `--sets`
(the record says what a window reads) -- recorded `--calls` steps into one HIP graph per route; the graphs are replayed interleaved
`--repeats` times between HIP events behind one warm-up replay each; median and spread (max - min) per route.

    python tools/time_decode_minifloat.py --out profiles/decode_minifloat.jsonl
"""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
CACHE_BYTES = 256 << 20
BM, FP = (8, 4, 8, 8, 4, 8), (6, 8, 127, 6, 8, 127)
CFG = dict(name="block_minifloat", is_ptq=True, bypass=False, data_in_width=8, data_in_exponent_width=4, data_in_exponent_bias_width=8,
           data_in_block_size=[1, 16], weight_width=8, weight_exponent_width=4, weight_exponent_bias_width=8, weight_block_size=[1, 16])


def main():
    import torch
    from mi355q import ops
    from mi355q.quantize import get_quantized_func
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sets", type=int, default=24)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, D, H = "cuda:0", 128, 8
    stream = torch.cuda.Stream()
    mm = get_quantized_func("matmul", CFG)
    lines = []
    for batch in (1, 8, 32):
        for L in (512, 2048, 8192):
            R = batch * H
            n_sets = max(1, min(args.sets, -(-CACHE_BYTES // (R * L * D * 4)) + 1))
            torch.manual_seed(L + batch)
            i32 = lambda x: torch.full((R,), x, dtype=torch.int32, device=dev)
            before, after = i32(L - 1), i32(L)
            sets = []
            for _ in range(n_sets):
                k, v = torch.randn(R, L, D, device=dev), torch.randn(R, L, D, device=dev)
                q = torch.randn(R, 1, D, device=dev) * 3.0
                bm, fp = ops.MinifloatKVCache(R, L, D, BM, BM, dev), ops.KVCache(R, L, D, FP, FP, dev)
                for c in (bm, fp):
                    c.append(k[:, :L - 1], v[:, :L - 1], lengths=i32(0), max_length=0)
                sets.append(dict(q=q, k1=k[:, L - 1:].contiguous(), v1=v[:, L - 1:].contiguous(), kp=k[:, :L - 1].contiguous(),
                                 vp=v[:, :L - 1].contiguous(), minifloat=bm, block_fp=fp))

            def step(route, i):
                s = sets[i % n_sets]
                if route == "fp32":
                    k, v = torch.cat([s["kp"], s["k1"]], dim=1), torch.cat([s["vp"], s["v1"]], dim=1)
                    w = mm(s["q"], k.transpose(-1, -2), config=CFG) / math.sqrt(D)
                    p = torch.nn.functional.softmax(w, dim=-1, dtype=torch.float32)
                    return mm(p, v, config=CFG)
                s[route].append(s["k1"], s["v1"], lengths=before, max_length=L - 1)
                return ops.bfp_attention_decode(s["q"], s[route], scale_div=math.sqrt(D), lengths=after, max_length=L)

            a, b = step("minifloat", 0), step("fp32", 0)
            worst = float((a - b).abs().max() / b.abs().max())
            graphs = {}
            for route in ("minifloat", "block_fp", "fp32"):
                stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(stream):
                    for i in range(n_sets):
                        step(route, i)
                torch.cuda.current_stream().wait_stream(stream)
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=stream):
                    for i in range(args.calls):
                        step(route, i)
                graphs[route] = gr
            times = {r: [] for r in graphs}
            for rep in range(args.repeats + 1):
                for route, gr in graphs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    gr.replay()
                    e1.record()
                    e1.synchronize()
                    if rep:
                        times[route].append(e0.elapsed_time(e1) * 1e3 / args.calls)
            line = dict(batch=batch, kv_heads=H, L=L, D=D, M=1, caches=n_sets, calls=args.calls, repeats=args.repeats,
                        window_cache_MiB=round(n_sets * R * L * D * 4 / 2 ** 20, 1), minifloat_vs_fp32_worst=worst)
            for route, t in times.items():
                line[route + "_us"] = round(statistics.median(t), 2)
                line[route + "_spread_us"] = round(max(t) - min(t), 2)
            line["minifloat_over_block_fp"] = round(line["minifloat_us"] / line["block_fp_us"], 3)
            line["fp32_over_minifloat"] = round(line["fp32_us"] / line["minifloat_us"], 2)
            print(json.dumps(line), flush=True)
            lines.append(line)
            del sets, graphs
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).write_text("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
