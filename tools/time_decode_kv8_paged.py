#!/usr/bin/env python
"""The paged int8-mantissa KV cache (ops.PagedPackedKVCache) against the two caches it combines -- ops.PagedKVCache (bf16 pages) and
ops.PackedKVCache (int8 mantissas, contiguous) -- in the method of tools/time_decode_paged.py: the step = append of one key a row +
ops.bfp_attention_decode (M = 1) with per-row lengths; per case enough DISTINCT caches that one timed window reads more than the 256-MiB
memory-side cache, at least `--calls` steps rotating over them recorded into one HIP graph per route, the three graphs replayed
interleaved `--repeats` times between HIP events behind one warm-up replay each; median and spread (max - min) per route.

    shapes   those of profiles/decode_kv8.jsonl (D = 128, 8 KV heads: batch 1, 8, 32, and 4 query heads a KV head at batch 8; every row at
             512, 2048 or 8192 keys), and the beam step of profiles/kv_fork.jsonl ("beam": 8 KV heads x 4 beams = 32 rows)
    pages    P = 64, every row's pages shuffled over a pool that is just large enough
    routes   paged_int8, paged_bf16, packed -- each cache filled by its own append of the same rows; the three outputs must be the same bits
    bytes    K + V bytes a cache row (a beam's KV head) holds in each cache

The expectation to confirm or refute: the contiguous packed cache's time plus the table lookups, no shape slower than the bf16 paged cache.

    python tools/time_decode_kv8_paged.py --out profiles/decode_kv8_paged.jsonl
"""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from time_decode_paged import CACHE_BYTES, PAR, capture, replay  # noqa: E402

D, P, HKV = 128, 64, 8
CASES = [("decode", 1, 1), ("decode", 8, 1), ("decode", 32, 1), ("decode", 8, 4), ("beam", 4, 1)]       # (kind, batch or beams, G)
ROUTES = ("paged_int8", "paged_bf16", "packed")


def main():
    import torch
    from mi355q import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    i32 = lambda xs: torch.tensor(list(xs), dtype=torch.int32, device=dev)
    lines, stream = [], torch.cuda.Stream()
    for kind, batch, G in CASES:
        for L in (512, 2048, 8192):
            B, pages = HKV * batch, L // P
            n_sets = int(CACHE_BYTES // (B * L * D * 4)) + 2
            calls = max(args.calls, n_sets)
            g = torch.Generator(device=dev).manual_seed(L + B + G)
            before, after, zeros = i32([L - 1] * B), i32([L] * B), i32([0] * B)
            sets = []
            for s in range(n_sets):
                k, v = (torch.randn(B, L, D, device=dev, generator=g) for _ in range(2))
                order = torch.randperm(B * pages, generator=torch.Generator().manual_seed(s)).tolist()
                caches = {"paged_int8": ops.PagedPackedKVCache(B, D, PAR, PAR, dev, page_size=P, num_pages=B * pages, max_pages=pages),
                          "paged_bf16": ops.PagedKVCache(B, D, PAR, PAR, dev, page_size=P, num_pages=B * pages, max_pages=pages),
                          "packed": ops.PackedKVCache(B, L, D, PAR, PAR, dev)}
                for name, c in caches.items():
                    if name != "packed":
                        for b in range(B):
                            c.assign(b, order[b * pages:(b + 1) * pages], upload=False)
                        c._upload()
                    c.append(k, v, lengths=zeros, max_length=0)
                sets.append((caches, k[:, L - 1:].contiguous(), v[:, L - 1:].contiguous()))
                del k, v
            q = torch.randn(B * G, 1, D, device=dev, generator=g)

            def step(route, i):
                caches, kn, vn = sets[i % n_sets]
                caches[route].append(kn, vn, lengths=before, max_length=L - 1)
                return ops.bfp_attention_decode(q, caches[route], causal=True, scale_div=math.sqrt(D), lengths=after, max_length=L, group=G)

            same = [step(r, 0) for r in ROUTES]
            assert bool(torch.isfinite(same[0]).all()) and all(torch.equal(same[0], o) for o in same[1:]), "the three caches differ"
            times = replay(capture(step, ROUTES, n_sets, calls, stream), args.repeats, calls)
            c = sets[0][0]
            line = dict(kind=kind, Hkv=HKV, batch=batch, rows=B, G=G, D=D, M=1, P=P, L=L, splits=ops.decode_splits(B * G // ops.decode_group_width(G, 1), L, D),
                        sets=n_sets, calls=calls, repeats=args.repeats, same_bits=True,
                        kv_bytes_a_row=dict(paged_int8=(c["paged_int8"].k8.numel() + c["paged_int8"].v8.numel()) // B,
                                            paged_bf16=(c["paged_bf16"].kq.numel() + c["paged_bf16"].vq.numel()) // B,
                                            packed=(c["packed"].k8.numel() + c["packed"].v8.numel()) // B))
            for route, t in times.items():
                line[route + "_us"] = round(statistics.median(t), 2)
                line[route + "_spread_us"] = round(max(t) - min(t), 2)
            line["paged_int8_over_paged_bf16"] = round(line["paged_int8_us"] / line["paged_bf16_us"], 3)
            line["paged_int8_over_packed"] = round(line["paged_int8_us"] / line["packed_us"], 3)
            print(json.dumps(line), flush=True)
            lines.append(line)
            del sets
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
