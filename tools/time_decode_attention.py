#!/usr/bin/env python
"""Decode attention: the block_fp KV cache route (ops.KVCache.append of the step's M rows + ops.bfp_attention_decode) against the
only route there was before it at the same shapes -- ops.bfp_attention on fp32 K / V with M queries (L % 16 == 0), which packs all
of K and V again on every call.

The method of tools/time_small_m.py: per case enough DISTINCT key / value sets that one timed window reads more than the 256-MiB
memory-side cache (counted for the cache route, the smaller reader), at least `--calls` steps rotating over them recorded into one HIP graph per route, the two graphs replayed alternately
`--repeats` times between HIP events.  One JSON line per case: median time per step of both routes and the spread over the repeats.

    python tools/time_decode_attention.py --out profiles/decode_attention.jsonl
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


def main():
    import torch
    from mi355q import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, B = "cuda:0", 32
    lines = []
    stream = torch.cuda.Stream()
    for D in (64, 128):
        for L in (512, 2048, 4096):
            # sized by the SMALLER route: a set's bf16 K + V in the cache is B L D 4 bytes (the other route reads twice that as fp32),
            # and every set is visited once a window, so a window of either route reads more than the memory-side cache
            n_sets = int(CACHE_BYTES // (B * L * D * 4)) + 2
            calls = max(args.calls, n_sets)
            g = torch.Generator(device=dev).manual_seed(L + D)
            sets = []
            for _ in range(n_sets):
                k, v = (torch.randn(B, L, D, device=dev, generator=g) for _ in range(2))
                cache = ops.KVCache(B, L, D, PAR, PAR, dev)
                cache.append(k, v)
                sets.append((k, v, cache))
            for M in (1, 16):
                q = torch.randn(B, M, D, device=dev, generator=g)

                def step(route, i):
                    k, v, cache = sets[i % n_sets]
                    if route == "parent":
                        return ops.bfp_attention(q, k, v, PAR, PAR, causal=True, scale_div=math.sqrt(D))
                    cache.length = L - M                      # (the step's own M rows go in again: the append is part of the step)
                    cache.append(k[:, L - M:], v[:, L - M:])
                    return ops.bfp_attention_decode(q, cache, causal=True, scale_div=math.sqrt(D))

                graphs = {}
                for route in ("parent", "cache"):
                    stream.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(stream):
                        for i in range(n_sets):
                            step(route, i)
                    torch.cuda.current_stream().wait_stream(stream)
                    torch.cuda.synchronize()
                    gr = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gr, stream=stream):
                        for i in range(calls):
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
                        if rep:                                  # (the first replay of each is a warm-up)
                            times[route].append(e0.elapsed_time(e1) * 1e3 / calls)
                line = dict(B=B, D=D, M=M, L=L, splits=ops.decode_splits(B, L, D), sets=n_sets, calls=calls, repeats=args.repeats,
                            parent_us=round(statistics.median(times["parent"]), 2), cache_us=round(statistics.median(times["cache"]), 2),
                            parent_spread_us=round(max(times["parent"]) - min(times["parent"]), 2),
                            cache_spread_us=round(max(times["cache"]) - min(times["cache"]), 2))
                line["speedup"] = round(line["parent_us"] / line["cache_us"], 2)
                print(json.dumps(line), flush=True)
                lines.append(line)
                del graphs
            del sets
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
