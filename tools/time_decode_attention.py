#!/usr/bin/env python
"""Decode attention: the block_fp KV cache route (ops.KVCache.append of the step's M rows + ops.bfp_attention_decode) against the
only route there was before it at the same shapes -- ops.bfp_attention on fp32 K / V with M queries (L % 16 == 0), which packs all
of K and V again on every call.

The method of tools/time_small_m.py: per case enough DISTINCT key / value sets that one timed window reads more than the 256-MiB
memory-side cache (counted for the cache route, the smaller reader), at least `--calls` steps rotating over them recorded into one HIP graph per route, the two graphs replayed alternately
`--repeats` times between HIP events.  One JSON line per case: median time per step of both routes and the spread over the repeats.

    python tools/time_decode_attention.py --out profiles/decode_attention.jsonl

--ragged: the per-row-length forms (lengths on the device) of the same step at M = 1 against the uniform route, four cases a head_dim:
all 32 lengths equal at L = 512 / 2048 / 4096 (the ragged kernels' only extra work is one 4-byte load a workgroup), and a mixed
batch -- one row of 4096 keys, 31 of 512 -- against the uniform step at L = 4096, which is what a padded batch costs.  The sets are
sized for the SMALLEST reader of a case, so every route's window reads more than the memory-side cache.  --baseline-lib names a
second build of libmi355q.so (an earlier commit's) whose uniform route is replayed in the same interleaving, through the C ABI.

    python tools/time_decode_attention.py --ragged [--baseline-lib PATH] --out profiles/decode_ragged.jsonl

--packed: the same step (append of one key a row + decode, D = 128, M = 1) on ops.PackedKVCache -- int8 mantissas, 17/32 of the K / V
bytes -- against ops.KVCache holding the same keys, at the shapes of profiles/decode_gqa.jsonl: 8 KV heads, batch 1 / 8 / 32 at
L = 512 / 2048 / 8192, and 4 query heads a KV head at batch 8.  Both routes run their ragged form on the same device lengths (the
packed kernels have no other); the sets are sized for the packed cache, the smaller reader.

    python tools/time_decode_attention.py --packed --out profiles/decode_kv8.jsonl
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


def _replay(graphs, repeats, calls):
    """the graphs replayed alternately, `repeats` times each behind one warm-up replay -> {route: [us per step]}"""
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


def _baseline_step(path):
    """the uniform append + decode step of ANOTHER build of the library, through its C ABI (the signatures are this build's: the
    uniform entry points have not changed)"""
    import ctypes
    import torch
    from mi355q import _lib, ops
    lib = ctypes.CDLL(str(path))
    for name in ("mi355q_bfp_kv_append", "mi355q_bfp_attention_decode"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]

    def step(cache, kn, vn, q, out, ws, L, scale_div):
        B, D = cache.B, cache.D
        sp = torch.cuda.current_stream().cuda_stream
        rc = lib.mi355q_bfp_kv_append(cache.kq.data_ptr(), cache.vq.data_ptr(), cache.stage.data_ptr(), kn.data_ptr(), vn.data_ptr(), B,
                                      cache.capacity, D, L - 1, 1, ctypes.addressof(cache._pa), ctypes.addressof(cache._pb), None, sp)
        rc = rc or lib.mi355q_bfp_attention_decode(q.data_ptr(), cache.kq.data_ptr(), cache.vq.data_ptr(), 1, 0.0, scale_div, out.data_ptr(),
                                                   ws.data_ptr(), B, 1, L, cache.capacity, D, ctypes.addressof(cache._pa),
                                                   ctypes.addressof(cache._pb), None, 0, sp)
        assert rc == 0, rc
    return step


def ragged(args):
    import torch
    from mi355q import ops
    dev, B, M = "cuda:0", 32, 1
    i32 = lambda xs: torch.tensor(list(xs), dtype=torch.int32, device=dev)
    base = _baseline_step(args.baseline_lib) if args.baseline_lib else None
    lines = []
    stream = torch.cuda.Stream()
    for D in (64, 128):
        for case, L in (("equal", 512), ("equal", 2048), ("equal", 4096), ("mixed", 4096)):
            lens = [L] * B if case == "equal" else [L] + [512] * (B - 1)
            n_sets = int(CACHE_BYTES // (sum(lens) * D * 4)) + 2
            calls = max(args.calls, n_sets)
            g = torch.Generator(device=dev).manual_seed(L + D)
            before, after, zeros = i32([n - 1 for n in lens]), i32(lens), i32([0] * B)
            sets = []
            for _ in range(n_sets):
                k, v = (torch.randn(B, L, D, device=dev, generator=g) for _ in range(2))
                own = ops.KVCache(B, L, D, PAR, PAR, dev)                    # every row at its own length
                own.append(k, v, lengths=zeros, counts=after, max_length=0)
                if case == "mixed":                                            # the padded batch: every row at L
                    full = ops.KVCache(B, L, D, PAR, PAR, dev)
                    full.append(k, v)
                else:
                    full = own
                last = torch.tensor([n - 1 for n in lens], device=dev)[:, None, None].expand(B, 1, D)
                sets.append((own, full, k.gather(1, last).contiguous(), v.gather(1, last).contiguous(), k[:, L - 1:].clone(), v[:, L - 1:].clone()))
                del k, v
            q = torch.randn(B, M, D, device=dev, generator=g)
            # (the baseline's output and workspace: score tiles + 64 splits' statistics and partial outputs, as ops sizes its own)
            out = torch.empty(B, M, D, device=dev)
            ws = torch.empty(B * (L // 16) * 1024 + B * 64 * (128 + (D // 16) * 1024), dtype=torch.uint8, device=dev)

            def step(route, i):
                own, full, kn, vn, kf, vf = sets[i % n_sets]
                if route == "ragged":
                    own.append(kn, vn, lengths=before, max_length=L - 1)
                    return ops.bfp_attention_decode(q, own, causal=True, scale_div=math.sqrt(D), lengths=after, max_length=L)
                if route == "baseline_uniform":
                    return base(full, kf, vf, q, out, ws, L, math.sqrt(D))
                full.length = L - M
                full.append(kf, vf)
                return ops.bfp_attention_decode(q, full, causal=True, scale_div=math.sqrt(D))

            graphs = {}
            for route in ("uniform", "ragged") + (("baseline_uniform",) if base else ()):
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
            times = _replay(graphs, args.repeats, calls)
            line = dict(case=case, B=B, D=D, M=M, L=L, keys=sum(lens), splits=ops.decode_splits(B, L, D), sets=n_sets, calls=calls, repeats=args.repeats)
            for route, t in times.items():
                line[route + "_us"] = round(statistics.median(t), 2)
                line[route + "_spread_us"] = round(max(t) - min(t), 2)
            line["ragged_over_uniform"] = round(line["ragged_us"] / line["uniform_us"], 3)
            print(json.dumps(line), flush=True)
            lines.append(line)
            del graphs, sets
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(l) + "\n" for l in lines))


def packed(args):
    import torch
    from mi355q import ops
    dev, D, HKV = "cuda:0", 128, 8
    lines = []
    stream = torch.cuda.Stream()
    for batch, G in ((1, 1), (8, 1), (32, 1), (8, 4)):
        B = batch * HKV
        for L in (512, 2048, 8192):
            made = {"packed": ops.PackedKVCache(B, L, D, PAR, PAR, dev), "bf16": ops.KVCache(B, L, D, PAR, PAR, dev)}
            nbytes = {r: c.kq.numel() + c.vq.numel() if r == "bf16" else c.k8.numel() + c.v8.numel() for r, c in made.items()}
            n_sets = int(CACHE_BYTES // nbytes["packed"]) + 2
            calls = max(args.calls, n_sets)
            g = torch.Generator(device=dev).manual_seed(L + B + G)
            before, after = (torch.full((B,), n, dtype=torch.int32, device=dev) for n in (L - 1, L))
            zero = torch.zeros(B, dtype=torch.int32, device=dev)
            sets = []
            for i in range(n_sets):
                k, v = (torch.randn(B, L, D, device=dev, generator=g) for _ in range(2))
                caches = made if i == 0 else {"packed": ops.PackedKVCache(B, L, D, PAR, PAR, dev), "bf16": ops.KVCache(B, L, D, PAR, PAR, dev)}
                for c in caches.values():
                    c.append(k, v, lengths=zero, max_length=0)
                sets.append((k[:, L - 1:].clone(), v[:, L - 1:].clone(), caches))     # (the step's own row goes in again on every step)
                del k, v
            q = torch.randn(B * G, 1, D, device=dev, generator=g)
            gq = dict(group=G) if G > 1 else {}

            def step(route, i):
                kn, vn, caches = sets[i % n_sets]
                caches[route].append(kn, vn, lengths=before, max_length=L - 1)
                return ops.bfp_attention_decode(q, caches[route], causal=True, scale_div=math.sqrt(D), lengths=after, max_length=L, **gq)

            same = all(torch.equal(step("packed", i), step("bf16", i)) for i in range(min(n_sets, 2)))
            graphs = {}
            for route in ("bf16", "packed"):
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
            times = _replay(graphs, args.repeats, calls)
            R = B if G == 1 else B * G // ops.decode_group_width(G, 1)
            line = dict(kernel="decode", form="ragged", Hkv=HKV, batch=batch, G=G, D=D, M=1, L=L, splits=ops.decode_splits(R, L, D),
                        cache_MiB_bf16=round(nbytes["bf16"] / 2 ** 20, 2), cache_MiB_packed=round(nbytes["packed"] / 2 ** 20, 2),
                        sets=n_sets, calls=calls, repeats=args.repeats, same_bits=bool(same),
                        bf16_us=round(statistics.median(times["bf16"]), 2), bf16_spread_us=round(max(times["bf16"]) - min(times["bf16"]), 2),
                        packed_us=round(statistics.median(times["packed"]), 2),
                        packed_spread_us=round(max(times["packed"]) - min(times["packed"]), 2))
            line["bf16_over_packed"] = round(line["bf16_us"] / line["packed_us"], 2)
            print(json.dumps(line), flush=True)
            lines.append(line)
            del graphs, sets, made
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(l) + "\n" for l in lines))


def main():
    import torch
    from mi355q import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ragged", action="store_true", help="per-row lengths against the uniform route (module docstring)")
    ap.add_argument("--baseline-lib", default=None, help="--ragged: another build of libmi355q.so whose uniform route is timed alongside")
    ap.add_argument("--packed", action="store_true", help="ops.PackedKVCache against ops.KVCache at the grouped-query shapes (module docstring)")
    args = ap.parse_args()
    if args.ragged:
        return ragged(args)
    if args.packed:
        return packed(args)
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
