#!/usr/bin/env python
"""One decode step of a W4 attention layer -- append of one key a row + attention of M = 1 query -- on the three storages of the
block_fp KV cache, in the method of tools/time_decode_minifloat.py: D = 128, 8 KV heads, width 4, batch 1 / 8 / 32 (rows = batch x 8),
L = 512 / 2048 / 8192 keys.

    nibble      ops.NibbleKVCache (csrc/mi355q_kvp.hip, NibblePieces): 9/32 of the bf16 cache's K / V bytes
    int8        ops.PackedKVCache (csrc/mi355q_kvp.hip, Int8Pieces): 17/32
    bf16        ops.KVCache (csrc/mi355q_decode.hip)

The three outputs of the first step are compared as bits first.  Per case the step runs over distinct caches -- as many as make one
timed window of the NIBBLE route, the smallest, read more than the 256-MiB memory-side cache, capped at `--sets` (the record says what
a window reads on each route) -- recorded `--calls` steps into one HIP graph per route; the graphs are replayed interleaved `--repeats`
times between HIP events behind one warm-up replay each; median and spread (max - min) per route.

    python tools/time_decode_kv4.py --out profiles/decode_kv4.jsonl
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
W4 = (4, 8, 127, 4, 8, 127)
ROUTES = ("nibble", "int8", "bf16")
BITS = dict(nibble=4.5, int8=8.5, bf16=16.0)       # K / V bits a value


def main():
    import torch
    from mi355q import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sets", type=int, default=24)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, D, H = "cuda:0", 128, 8
    classes = dict(nibble=ops.NibbleKVCache, int8=ops.PackedKVCache, bf16=ops.KVCache)
    stream = torch.cuda.Stream()
    lines = []
    for batch in (1, 8, 32):
        for L in (512, 2048, 8192):
            R = batch * H
            values = 2 * R * L * D                                     # K and V values a step reads
            n_sets = max(1, min(args.sets, -(-CACHE_BYTES // int(values * BITS["nibble"] / 8)) + 1))
            torch.manual_seed(L + batch)
            i32 = lambda x: torch.full((R,), x, dtype=torch.int32, device=dev)
            before, after = i32(L - 1), i32(L)
            sets = []
            for _ in range(n_sets):
                k, v = torch.randn(R, L, D, device=dev), torch.randn(R, L, D, device=dev)
                s = dict(q=torch.randn(R, 1, D, device=dev) * 3.0, k1=k[:, L - 1:].contiguous(), v1=v[:, L - 1:].contiguous())
                for route, cls in classes.items():
                    s[route] = cls(R, L, D, W4, W4, dev)
                    s[route].append(k[:, :L - 1], v[:, :L - 1], lengths=i32(0), max_length=0)
                sets.append(s)
                del k, v

            def step(route, i):
                s = sets[i % n_sets]
                s[route].append(s["k1"], s["v1"], lengths=before, max_length=L - 1)
                return ops.bfp_attention_decode(s["q"], s[route], scale_div=math.sqrt(D), lengths=after, max_length=L)

            first = {route: step(route, 0) for route in ROUTES}
            same = all(torch.equal(first["nibble"].view(torch.uint8), first[r].view(torch.uint8)) for r in ("int8", "bf16"))
            graphs = {}
            for route in ROUTES:
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
            line = dict(batch=batch, kv_heads=H, L=L, D=D, M=1, width=4, caches=n_sets, calls=args.calls, repeats=args.repeats,
                        same_bits=same)
            for route, t in times.items():
                line[route + "_window_MiB"] = round(n_sets * values * BITS[route] / 8 / 2 ** 20, 1)
                line[route + "_us"] = round(statistics.median(t), 2)
                line[route + "_spread_us"] = round(max(t) - min(t), 2)
            line["nibble_over_int8"] = round(line["nibble_us"] / line["int8_us"], 3)
            line["nibble_over_bf16"] = round(line["nibble_us"] / line["bf16_us"], 3)
            print(json.dumps(line), flush=True)
            lines.append(line)
            del sets, graphs, first
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).write_text("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
