#!/usr/bin/env python
"""The paged block_fp KV cache (ops.PagedKVCache) against the contiguous ragged route of the same build, at the shapes and in the method
of tools/time_decode_attention.py --ragged: B = 32 rows, M = 1, the step = append of one key a row + ops.bfp_attention_decode with
per-row lengths.  Per case enough DISTINCT caches that one timed window reads more than the 256-MiB memory-side cache, at least
`--calls` steps rotating over them recorded into one HIP graph per route, all graphs of a case replayed interleaved `--repeats` times
between HIP events behind one warm-up replay each; median and spread (max - min) per route.

    decode   D in {64, 128}; all rows at 512, 2048 or 4096 keys, and 1 x 4096 + 31 x 512 ("mixed"); routes: contiguous, and paged at
             P in {32, 64, 256} with the rows' pages in order ("ord") and shuffled over the pool ("shuf")
    extend   D = 128, M = 256 new tokens behind a cache that then holds 2048 keys: append of the 256 rows + ops.bfp_attention_extend

The paged caches are filled from the contiguous one, page by page (a page of P keys is a run of whole 1-KiB pieces of the contiguous
layout, csrc/mi355q_decode.h), so every route reads the same values.  The mixed case also records the memory: the pool's K + V bytes
(what the rows' pages need) against the contiguous cache's.

    python tools/time_decode_paged.py --out profiles/decode_paged.jsonl
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
PAGES = (32, 64, 256)


def paged_copy(contig, lens, P, shuffled, seed):
    """a PagedKVCache holding what `contig` holds (rows of lens[b] keys), its pool just large enough; shuffled: the rows' pages are a
    random permutation of the pool"""
    import torch
    from mi355q import ops
    B, C, D = contig.B, contig.capacity, contig.D
    need = [-(-n // P) for n in lens]
    cache = ops.PagedKVCache(B, D, PAR, PAR, contig.device, page_size=P, num_pages=sum(need), max_pages=C // P)
    order = torch.randperm(sum(need), generator=torch.Generator().manual_seed(seed)).tolist() if shuffled else list(range(sum(need)))
    at = 0
    for b, n in enumerate(need):
        cache.assign(b, order[at:at + n], upload=False)
        at += n
    cache._upload()
    rows = torch.tensor([b for b, n in enumerate(need) for _ in range(n)], device=contig.device)
    logical = torch.tensor([i for n in need for i in range(n)], device=contig.device)
    pages = torch.tensor([p for h in cache.held for p in h], device=contig.device)
    for pool, src in ((cache.kq, contig.kq), (cache.vq, contig.vq)):
        pool.view(cache.num_pages, -1)[pages] = src.view(B, C // P, -1)[rows, logical]
    cache.stage.copy_(contig.stage)
    return cache


def replay(graphs, repeats, calls):
    import torch
    times = {r: [] for r in graphs}
    for rep in range(repeats + 1):
        for route, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            e1.synchronize()
            if rep:
                times[route].append(e0.elapsed_time(e1) * 1e3 / calls)
    return times


def capture(step, routes, n_sets, calls, stream):
    import torch
    graphs = {}
    for route in routes:
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
    return graphs


def record(line, times):
    for route, t in times.items():
        line[route + "_us"] = round(statistics.median(t), 2)
        line[route + "_spread_us"] = round(max(t) - min(t), 2)
    for route in times:
        if route != "contiguous":
            line[route + "_over_contiguous"] = round(line[route + "_us"] / line["contiguous_us"], 3)
    print(json.dumps(line), flush=True)
    return line


def main():
    import torch
    from mi355q import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("decode", "extend"), default=None)
    args = ap.parse_args()
    dev, B = "cuda:0", 32
    i32 = lambda xs: torch.tensor(list(xs), dtype=torch.int32, device=dev)
    routes = ["contiguous"] + [f"p{P}_{o}" for P in PAGES for o in ("ord", "shuf")]
    lines, stream = [], torch.cuda.Stream()
    for D in (64, 128) if args.only != "extend" else ():
        for case, L in (("equal", 512), ("equal", 2048), ("equal", 4096), ("mixed", 4096)):
            lens = [L] * B if case == "equal" else [L] + [512] * (B - 1)
            n_sets = int(CACHE_BYTES // (sum(lens) * D * 4)) + 2
            calls = max(args.calls, n_sets)
            g = torch.Generator(device=dev).manual_seed(L + D)
            before, after, zeros = i32([n - 1 for n in lens]), i32(lens), i32([0] * B)
            sets = []
            for s in range(n_sets):
                k, v = (torch.randn(B, L, D, device=dev, generator=g) for _ in range(2))
                own = ops.KVCache(B, L, D, PAR, PAR, dev)
                own.append(k, v, lengths=zeros, counts=after, max_length=0)
                last = torch.tensor([n - 1 for n in lens], device=dev)[:, None, None].expand(B, 1, D)
                caches = {"contiguous": own}
                for P in PAGES:
                    for o in ("ord", "shuf"):
                        caches[f"p{P}_{o}"] = paged_copy(own, lens, P, o == "shuf", s)
                sets.append((caches, k.gather(1, last).contiguous(), v.gather(1, last).contiguous()))
                del k, v
            q = torch.randn(B, 1, D, device=dev, generator=g)

            def step(route, i):
                caches, kn, vn = sets[i % n_sets]
                caches[route].append(kn, vn, lengths=before, max_length=L - 1)
                return ops.bfp_attention_decode(q, caches[route], causal=True, scale_div=math.sqrt(D), lengths=after, max_length=L)

            same = [step(r, 0) for r in routes]
            assert all(torch.equal(same[0], o) for o in same[1:]), "a paged route differs from the contiguous one"
            times = replay(capture(step, routes, n_sets, calls, stream), args.repeats, calls)
            line = dict(kind="decode", case=case, B=B, D=D, M=1, L=L, keys=sum(lens), splits=ops.decode_splits(B, L, D), sets=n_sets, calls=calls,
                        repeats=args.repeats)
            if case == "mixed":
                c, p = sets[0][0]["contiguous"], sets[0][0]["p64_ord"]
                line.update(contiguous_kv_bytes=c.kq.numel() + c.vq.numel(), p64_pool_kv_bytes=p.kq.numel() + p.vq.numel(), p64_pages=p.num_pages)
            lines.append(record(line, times))
            del sets
            torch.cuda.empty_cache()
    if args.only != "decode":
        D, M, L = 128, 256, 2048
        n_sets = int(CACHE_BYTES // (B * L * D * 4)) + 2
        calls = max(min(args.calls, 16), n_sets)
        g = torch.Generator(device=dev).manual_seed(L + D)
        before, after = i32([L - M] * B), i32([L] * B)
        sets = []
        for s in range(n_sets):
            k, v = (torch.randn(B, L, D, device=dev, generator=g) for _ in range(2))
            own = ops.KVCache(B, L, D, PAR, PAR, dev)
            own.append(k, v)
            caches = {"contiguous": own}
            for P in PAGES:
                for o in ("ord", "shuf"):
                    caches[f"p{P}_{o}"] = paged_copy(own, [L] * B, P, o == "shuf", s)
            sets.append((caches, k[:, L - M:].contiguous(), v[:, L - M:].contiguous()))
            del k, v
        q = torch.randn(B, M, D, device=dev, generator=g)

        def call(route, i):
            caches, kn, vn = sets[i % n_sets]
            caches[route].append(kn, vn, lengths=before, max_length=L - M)
            return ops.bfp_attention_extend(q, caches[route], causal=True, scale_div=math.sqrt(D), lengths=after, max_length=L)

        same = [call(r, 0) for r in routes]
        assert all(torch.equal(same[0], o) for o in same[1:]), "a paged route differs from the contiguous one"
        times = replay(capture(call, routes, n_sets, calls, stream), args.repeats, calls)
        lines.append(record(dict(kind="extend", B=B, D=D, M=M, L=L, sets=n_sets, calls=calls, repeats=args.repeats), times))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
