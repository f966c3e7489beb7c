#!/usr/bin/env python
"""Small-batch Linear on packed weights: the expand + tile GEMM route (config["mi355q_small_m"] off, what every packed layer ran
before) against the product that reads the packed form in place (mi355q_small_m = "packed"), same layers, one process.

Per case (M, widths, shape) the script builds enough DISTINCT layers that the weights read in one timed window exceed the 256-MiB
memory-side cache, records `--calls` forwards rotating over them into one HIP graph per route (so that the host's launch cost
is not what is measured), and replays the two graphs alternately, `--repeats` times each, between HIP events.  One JSON line per
case: both times (median per call), the spread (max - min) of each over the repeats, the algorithmic bytes
N * K * (width + 0.5) / 8 + x + y, and bytes / time of the new route (a device-to-device copy reaches about 6.3 TB/s here).

    python tools/time_small_m.py --out profiles/small_m_packed.jsonl
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "llm-mixed-q_amd"))
CACHE_BYTES = 256 << 20


def cfg_for(width, **extra):
    return dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=width, data_in_exponent_width=8, data_in_exponent_bias=127,
                data_in_block_size=[1, 16], weight_width=width, weight_exponent_width=8, weight_exponent_bias=127,
                weight_block_size=[1, 16], bias_width=width, bias_exponent_width=8, bias_exponent_bias=127, bias_block_size=[16],
                mi355q_weight_storage="packed", mi355q_small_m="off", mi355q_mixed=False, **extra)


def main():
    import torch
    import mi355q.quantize as Q
    from mi355q import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    ops.REUSE_QUANTISED_INPUT = False
    lines = []
    for width in (6, 4):
        for N, K, per_block in ((4096, 4096, False), (11008, 4096, False), (4096, 11008, True)):
            packed_bytes = N * K * (width + 0.5) / 8
            n_layers = int(CACHE_BYTES // packed_bytes) + 2
            # down_proj runs the per-block flavour (post-SiLU inputs fit no row window): every block keeps its exponent
            cfg = cfg_for(width, mi355q_align="blocks" if per_block else "auto")
            g = torch.Generator(device=dev).manual_seed(N + K + width)
            sample = torch.randn(16, K, device=dev, generator=g)
            if per_block:
                sample = torch.nn.functional.silu(sample) * torch.randn(16, K, device=dev, generator=g)
            layers = []
            with torch.no_grad():
                for _ in range(n_layers):
                    lin = Q.get_quantized_cls("linear", cfg)(K, N, bias=True, device=dev, config=dict(cfg))
                    lin(sample)
                    assert lin._w_packed is not None, "the layer did not pack its weights"
                    lin.release_fp32_weight()
                    layers.append(lin)
            flavour = "row" if layers[0]._w_packed.row_scale_flavour else "block"
            assert (flavour == "block") == per_block or not per_block, flavour
            stream = torch.cuda.Stream()
            for M in (1, 4, 16):
                x = sample[:M].contiguous()
                graphs = {}
                with torch.no_grad():
                    for route in ("off", "packed"):
                        for lin in layers:
                            lin.config["mi355q_small_m"] = route
                        stream.wait_stream(torch.cuda.current_stream())
                        with torch.cuda.stream(stream):
                            for lin in layers:
                                lin(x)                                                   # warm-up: buffers of this stream
                        torch.cuda.current_stream().wait_stream(stream)
                        before = ops.small_m_calls()
                        gr = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(gr, stream=stream):
                            for i in range(args.calls):
                                layers[i % n_layers](x)
                        assert (ops.small_m_calls() - before) == (args.calls if route == "packed" else 0)
                        graphs[route] = gr
                times = {"off": [], "packed": []}
                for route in graphs:
                    graphs[route].replay()                                               # warm-up
                torch.cuda.synchronize()
                for _ in range(args.repeats):
                    for route in ("off", "packed"):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        graphs[route].replay()
                        e1.record()
                        torch.cuda.synchronize()
                        times[route].append(e0.elapsed_time(e1) * 1e3 / args.calls)
                t_old, t_new = statistics.median(times["off"]), statistics.median(times["packed"])
                s_old, s_new = max(times["off"]) - min(times["off"]), max(times["packed"]) - min(times["packed"])
                nbytes = packed_bytes + M * K * 4 + M * N * 4
                rec = dict(case=f"M{M}_W{width}A{width}_N{N}_K{K}", M=M, N=N, K=K, width=width, flavour=flavour, layers=n_layers,
                           calls=args.calls, repeats=args.repeats, weights_in_window_MiB=round(min(args.calls, n_layers) * packed_bytes / 2 ** 20, 1),
                           parent_us=round(t_old, 2), parent_spread_us=round(s_old, 2), new_us=round(t_new, 2), new_spread_us=round(s_new, 2),
                           speedup=round(t_old / t_new, 2), algorithmic_bytes=int(nbytes), new_TBps=round(nbytes / t_new * 1e-6, 3),
                           includes="x quantiser + product (+ expand on the parent route), replayed from a HIP graph",
                           new_faster_by_more_than_spread=bool(t_old - t_new > max(s_old, s_new)))
                print(json.dumps(rec), flush=True)
                lines.append(rec)
                del graphs
            del layers
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in lines))
    return 0 if all(r["new_faster_by_more_than_spread"] for r in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
