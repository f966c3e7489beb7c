"""Host overhead of one decode step: the median eager wall time (us, no synchronisation inside the timed span) of KVCache.append of one key +
ops.bfp_attention_decode at B = 8, D = 64, L = 64, M = 1, in the uniform or the ragged form, of the mi355q package under <package dir>.
One process per figure: to compare two trees (profiles/kv_call_host_overhead.jsonl), alternate them, several runs each.

    python tools/prof/kv_step_host_time.py <dir that holds mi355q/> uniform|ragged <steps> <warmup>
"""
import json
import sys
import time

pkg, form, steps, warm = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
sys.path.insert(0, pkg)
import torch
from mi355q import ops
B, D, L, M = 8, 64, 64, 1
dev = "cuda:0"
par = (6, 8, 127, 6, 8, 127)
cache = ops.KVCache(B, L, D, par, par, dev)
g = torch.Generator().manual_seed(0)
k0, v0 = (torch.randn(B, L - 1, D, generator=g).to(dev) for _ in range(2))
k1, v1, q = (torch.randn(B, M, D, generator=g).to(dev) for _ in range(3))
cache.append(k0, v0)
before = torch.full((B,), L - 1, dtype=torch.int32, device=dev)
after = torch.full((B,), L, dtype=torch.int32, device=dev)
def step():
    if form == "uniform":
        cache.length = L - 1
        cache.append(k1, v1)
        return ops.bfp_attention_decode(q, cache, scale_div=8.0)
    cache.append(k1, v1, lengths=before, max_length=L - 1)
    return ops.bfp_attention_decode(q, cache, scale_div=8.0, lengths=after, max_length=L)
for _ in range(warm):
    step()
torch.cuda.synchronize()
times = []
for i in range(steps):
    t = time.perf_counter_ns()
    step()
    times.append(time.perf_counter_ns() - t)
    if i % 64 == 63:
        torch.cuda.synchronize()
torch.cuda.synchronize()
times.sort()
print(json.dumps({"form": form, "steps": steps, "warmup": warm, "median_us": times[len(times) // 2] / 1e3, "p10_us": times[len(times) // 10] / 1e3,
                  "p90_us": times[len(times) * 9 // 10] / 1e3, "module": ops.__file__}))
