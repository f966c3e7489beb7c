#!/usr/bin/env python
"""Grouped-query decode on the block_fp KV cache against what a caller had to do before it, at the same query heads (D = 128):

    grouped    the cache holds batch x Hkv rows: ops.KVCache.append of one token + ONE ops.bfp_attention_decode(group=Hq // Hkv), M = 1
    repeated   the cache holds batch x Hq rows, every K / V head stored Hq // Hkv times: append of the repeated token + the ungrouped
               ops.bfp_attention_decode -- the only way to serve such a model without `group`

and one chunked-prefill row (M = 256 new tokens behind 2048 keys) for ops.bfp_attention_extend(group=...) against the same on the
repeated cache.

The method of tools/time_extend_attention.py: per case enough DISTINCT caches that one timed window reads more than the 256-MiB
memory-side cache (counted for the grouped route, the smaller reader), at least `--calls` calls rotating over them recorded into one HIP
graph per route, the graphs replayed alternately `--repeats` times between HIP events behind one warm-up replay each.  One JSON line per
case: median microseconds per call of both routes and the spread over the repeats.

    python tools/time_decode_gqa.py --out profiles/decode_gqa.jsonl
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
D = 128
# (Hq, Hkv, batch, M, L): L keys in the cache once the call's own M tokens are appended
DECODE = [(32, 8, b, 1, L) for b in (1, 8, 32) for L in (512, 2048, 8192)] + [(64, 8, 8, 1, L) for L in (512, 2048, 8192)]
EXTEND = [(32, 8, 8, 256, 2048 + 256)]


def main():
    import torch
    from mi355q import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--max-seconds", type=float, default=None, help="start no further case once this much time has passed")
    args = ap.parse_args()
    import time
    t_start = time.monotonic()
    dev = "cuda:0"
    stream = torch.cuda.Stream()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    out = open(args.out, "w") if args.out else None
    for Hq, Hkv, batch, M, L in EXTEND + DECODE:
        if args.max_seconds is not None and time.monotonic() - t_start > args.max_seconds:
            print(json.dumps(dict(skipped=dict(Hq=Hq, Hkv=Hkv, batch=batch, M=M, L=L), reason="--max-seconds")), flush=True)
            continue
        G, R = Hq // Hkv, batch * Hkv
        n_sets = int(CACHE_BYTES // (R * L * D * 4)) + 2
        calls = max(args.calls, n_sets)
        g = torch.Generator(device=dev).manual_seed(L + Hq + batch)
        C = (L + 15) // 16 * 16
        sets = []
        for _ in range(n_sets):
            k, v = (torch.randn(R, L, D, device=dev, generator=g) for _ in range(2))
            small, big = ops.KVCache(R, C, D, PAR, PAR, dev), ops.KVCache(R * G, C, D, PAR, PAR, dev)
            for at in range(0, L, 1024):                        # (in pieces: the repeated fp32 rows of a large case are gigabytes)
                small.append(k[:, at:at + 1024], v[:, at:at + 1024])
                big.append(k[:, at:at + 1024].repeat_interleave(G, 0), v[:, at:at + 1024].repeat_interleave(G, 0))
            kn, vn = k[:, L - M:].contiguous(), v[:, L - M:].contiguous()
            sets.append((small, big, kn, vn, kn.repeat_interleave(G, 0), vn.repeat_interleave(G, 0)))
            del k, v
        q = torch.randn(R * G, M, D, device=dev, generator=g)
        attend = ops.bfp_attention_decode if M <= ops.DECODE_MAX_QUERIES else ops.bfp_attention_extend

        def call(route, i):
            small, big, kn, vn, knr, vnr = sets[i % n_sets]
            if route == "grouped":
                small.length = L - M                          # (the call's own tokens go in again: the append is part of the call)
                small.append(kn, vn)
                return attend(q, small, causal=True, scale_div=math.sqrt(D), group=G)
            big.length = L - M
            big.append(knr, vnr)
            return attend(q, big, causal=True, scale_div=math.sqrt(D))

        same = bool(torch.equal(call("grouped", 0), call("repeated", 0))) if M > ops.DECODE_MAX_QUERIES else None   # (decode: other default splits)
        graphs = {}
        for route in ("grouped", "repeated"):
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
                if rep:                                      # (the first replay of each is a warm-up)
                    times[route].append(e0.elapsed_time(e1) * 1e3 / calls)
        gw = ops.decode_group_width(G, M) if M <= ops.DECODE_MAX_QUERIES else None
        line = dict(kernel="decode" if gw else "extend", Hq=Hq, Hkv=Hkv, batch=batch, D=D, M=M, L=L, G=G, group_width=gw,
                    cache_MiB_grouped=round(R * L * D * 4 / 2 ** 20, 1), cache_MiB_repeated=round(R * G * L * D * 4 / 2 ** 20, 1),
                    sets=n_sets, calls=calls, repeats=args.repeats)
        if gw:
            line["splits_grouped"], line["splits_repeated"] = ops.decode_splits(R * G // gw, L, D), ops.decode_splits(R * G, L, D)
        else:
            line["same_bits"] = same
        for route, t in times.items():
            line[route + "_us"] = round(statistics.median(t), 2)
            line[route + "_spread_us"] = round(max(t) - min(t), 2)
        line["repeated_over_grouped"] = round(line["repeated_us"] / line["grouped_us"], 2)
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")
            out.flush()
        del graphs, sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
