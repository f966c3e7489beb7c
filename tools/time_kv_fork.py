#!/usr/bin/env python
"""What a beam-search step pays for its cache reorder: ops.PagedKVCache.reorder (full pages by reference, one partial page and the open
tile's stage rows a row copied by one launch) against the reference's literal `_reorder_cache` -- index_select over the batch dimension
of every row's K and V -- on a contiguous ops.KVCache, and against no reorder at all.

    setup    8 KV heads x 4 beams = 32 cache rows, D = 128, P = 64, every row at L keys, L in {512, 2048, 8192} (L - 1 keys before the
             step: a partial page and an open tile)
    step     reorder by a random beam_idx (each group of 4 beams permuted / duplicated within its group, all 8 heads of a beam alike),
             then the append of one key a row, then one ops.bfp_attention_decode (M = 1)
    routes   floor     append + decode alone on the paged cache
             paged     PagedKVCache.reorder + append + decode; the row lengths are equal, so the caches are simply reordered again
                       and again; the host planning and the two small uploads are part of the figure
             literal   kq, vq, stage = index_select(0, beam_idx) of the contiguous cache, then append + decode
    apart    copy_launch: the copy kernel alone with the last reorder's 32 jobs, back to back, no plan and no upload

Eager calls, interleaved route by route, timed between HIP events over `--calls` steps behind one warm-up round; median of `--repeats`
rounds and their spread (max - min), as the sibling tools report.  reorder is a host-planned eager call (the stage pointer alternates):
no graphs here, for any route, so the floor includes the launch overhead of two eager calls.

    python tools/time_kv_fork.py --out profiles/kv_fork.jsonl
"""
import argparse
import json
import math
import random
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
PAR = (6, 8, 127, 6, 8, 127)
HEADS, BEAMS, D, P = 8, 4, 128, 64


def beam_rows(rng):
    """cache rows [beam][head] -> source rows: every beam takes a random beam, with all its heads"""
    beam_idx = [rng.randrange(BEAMS) for _ in range(BEAMS)]
    return [s * HEADS + h for s in beam_idx for h in range(HEADS)]


def main():
    import torch
    from mi355q import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, B = "cuda:0", HEADS * BEAMS
    i32 = lambda xs: torch.tensor(list(xs), dtype=torch.int32, device=dev)
    lines = []
    for L in (512, 2048, 8192):
        g = torch.Generator(device=dev).manual_seed(L)
        k, v = (torch.randn(B, L - 1, D, device=dev, generator=g) for _ in range(2))
        kn, vn, q = (torch.randn(B, 1, D, device=dev, generator=g) for _ in range(3))
        before, after, zeros = i32([L - 1] * B), i32([L] * B), i32([0] * B)
        pages = L // P
        contig = ops.KVCache(B, L, D, PAR, PAR, dev)
        contig.append(k, v, lengths=zeros, max_length=0)
        paged = ops.PagedKVCache(B, D, PAR, PAR, dev, page_size=P, max_pages=pages, num_pages=B * (pages + 1))
        paged.ensure([L] * B)
        paged.append(k, v, lengths=zeros, max_length=0)
        del k, v
        rng = random.Random(L)
        plans = [beam_rows(rng) for _ in range(args.calls)]
        index = [torch.tensor(p, device=dev) for p in plans]
        shape = {t: getattr(contig, t).shape for t in ("kq", "vq", "stage")}

        def tail(cache):
            cache.append(kn, vn, lengths=before, max_length=L - 1)
            return ops.bfp_attention_decode(q, cache, causal=True, scale_div=math.sqrt(D), lengths=after, max_length=L)

        def floor(i):
            return tail(paged)

        def paged_route(i):
            paged.reorder(plans[i], [L - 1] * B)
            return tail(paged)

        def literal(i):
            for t in ("kq", "vq", "stage"):
                setattr(contig, t, getattr(contig, t).view(B, -1).index_select(0, index[i]).view(shape[t]))
            return tail(contig)

        routes = dict(floor=floor, paged=paged_route, literal=literal)
        same = {r: fn(0) for r, fn in routes.items()}
        assert bool(torch.isfinite(same["paged"]).all()) and torch.equal(same["paged"], same["literal"]), "the paged reorder differs from index_select"
        times = {r: [] for r in routes}
        for rep in range(args.repeats + 1):
            for r, fn in routes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for i in range(args.calls):
                    fn(i)
                e1.record()
                e1.synchronize()
                if rep:
                    times[r].append(e0.elapsed_time(e1) * 1e3 / args.calls)
        # the launch alone: the last reorder's jobs again, back to back (no plan, no upload): an upper bound on the device's share
        n_jobs, launches = B, []
        for rep in range(args.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.calls):
                ops._kv_call(paged.device, "mi355q_bfp_kv_paged_copy", (ops._ptr(paged.kq), ops._ptr(paged.vq), ops._ptr(paged.stage), ops._ptr(paged.stage_alt),
                                                                        ops._ptr(paged._jobs), n_jobs, B, paged.num_pages, P, D, ops._stream_ptr(paged.device)))
            e1.record()
            e1.synchronize()
            if rep:
                launches.append(e0.elapsed_time(e1) * 1e3 / args.calls)
        times["copy_launch"] = launches
        line = dict(kind="reorder", rows=B, heads=HEADS, beams=BEAMS, D=D, P=P, L=L, calls=args.calls, repeats=args.repeats,
                    literal_bytes_moved=2 * (contig.kq.numel() + contig.vq.numel() + contig.stage.numel()),
                    paged_bytes_moved_max=2 * B * (2 * P * D * 2 + 16 * D * 4))
        for r, t in times.items():
            line[r + "_us"] = round(statistics.median(t), 2)
            line[r + "_spread_us"] = round(max(t) - min(t), 2)
        line["paged_over_floor_us"] = round(line["paged_us"] - line["floor_us"], 2)
        line["literal_over_floor_us"] = round(line["literal_us"] - line["floor_us"], 2)
        print(json.dumps(line), flush=True)
        lines.append(line)
        del contig, paged
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
