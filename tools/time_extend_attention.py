#!/usr/bin/env python
"""Chunked prefill: M new tokens behind a block_fp KV cache that then holds L keys, three routes at the same shapes (B = 32 rows =
batch x heads, as tools/time_decode_attention.py has them):

    extend   ops.KVCache.append of the M rows + ONE ops.bfp_attention_extend call
    decode   the same tokens as ceil(M / 16) steps of the route there was before it: append of 16 rows + ops.bfp_attention_decode
             with 16 queries, at growing lengths L - M + 16, .., L
    prefill  ops.bfp_attention on fp32 K / V of length L with the M queries (it packs all of K and V again: pack + kernel)

The method of tools/time_decode_attention.py: per case enough DISTINCT key / value sets that one timed window reads more than the
256-MiB memory-side cache (counted for the cache routes, the smaller readers), at least `--calls` calls rotating over them recorded
into one HIP graph per route, the graphs replayed alternately `--repeats` times between HIP events behind one warm-up replay each.
One JSON line per case: median microseconds per call of every route and the spread over the repeats.

    python tools/time_extend_attention.py --out profiles/extend_attention.jsonl
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
PAR = (6, 8, 127, 6, 8, 127)
SHAPES = ((64, 512), (256, 2048), (512, 4096))


def main():
    import torch
    from mi355q import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, B = "cuda:0", 32
    lines = []
    stream = torch.cuda.Stream()
    for D in (64, 128):
        for M, L in SHAPES:
            n_sets = int(CACHE_BYTES // (B * L * D * 4)) + 2
            calls = max(args.calls, n_sets)
            g = torch.Generator(device=dev).manual_seed(L + D)
            sets = []
            for _ in range(n_sets):
                k, v = (torch.randn(B, L, D, device=dev, generator=g) for _ in range(2))
                cache = ops.KVCache(B, L, D, PAR, PAR, dev)
                cache.append(k, v)
                sets.append((k, v, cache))
            q = torch.randn(B, M, D, device=dev, generator=g)
            qs = [q[:, j:j + 16].contiguous() for j in range(0, M, 16)]

            def call(route, i):
                k, v, cache = sets[i % n_sets]
                if route == "prefill":
                    return ops.bfp_attention(q, k, v, PAR, PAR, causal=True, scale_div=math.sqrt(D))
                cache.length = L - M                          # (the call's own M rows go in again: the append is part of the call)
                if route == "extend":
                    cache.append(k[:, L - M:], v[:, L - M:])
                    return ops.bfp_attention_extend(q, cache, causal=True, scale_div=math.sqrt(D))
                for j, qj in enumerate(qs):
                    at = L - M + 16 * j
                    cache.append(k[:, at:at + 16], v[:, at:at + 16])
                    out = ops.bfp_attention_decode(qj, cache, causal=True, scale_div=math.sqrt(D))
                return out

            graphs = {}
            for route in ("extend", "decode", "prefill"):
                stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(stream):
                    for i in range(n_sets):
                        call(route, i)
                torch.cuda.current_stream().wait_stream(stream)
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=stream):
                    for i in range(calls):
                        call(route, i)
                graphs[route] = gr
            times = {r: [] for r in graphs}
            for rep in range(args.repeats + 1):
                for route, gr in graphs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    gr.replay()
                    e1.record()
                    e1.synchronize()
                    if rep:                                  # (the first replay of each is a warm-up)
                        times[route].append(e0.elapsed_time(e1) * 1e3 / calls)
            line = dict(B=B, D=D, M=M, L=L, decode_steps=len(qs), sets=n_sets, calls=calls, repeats=args.repeats)
            for route, t in times.items():
                line[route + "_us"] = round(statistics.median(t), 2)
                line[route + "_spread_us"] = round(max(t) - min(t), 2)
            line["decode_over_extend"] = round(line["decode_us"] / line["extend_us"], 2)
            line["prefill_over_extend"] = round(line["prefill_us"] / line["extend_us"], 2)
            print(json.dumps(line), flush=True)
            lines.append(line)
            del graphs, sets
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
