// kv_paged_copy_kernel: the private copies a fork or a reorder of the paged block_fp KV cache needs -- a row's last, partially filled
// page and its open tile's fp32 stage rows -- for every row of one layer in ONE launch (layout of a job and the rules: mi355q_kv_copy.h).
// One instantiation, generic in bytes: a page of either pool is P * D * 2 bytes (int8 mantissas: P * D * 17 / 16) whatever D / 32 is,
// and nothing here looks inside a piece, so a template on D / 32 would only multiply code objects.  A fork moves at most 2 x 16 KiB + 8 KiB a row (P = 64, D = 128):
// latency, not bandwidth, so the work is spread one 16-byte unit a thread over as many waves as there are units.
#include <hip/hip_runtime.h>

#include "mi355q_kv_copy.h"

namespace mi355q {

// grid (kv_copy_blocks, n_jobs); unit u of a job: [0, U) page of K, [U, 2 U) page of V, [2 U, 2 U + S) stage rows
__global__ __launch_bounds__(KV_COPY_THREADS) void kv_paged_copy_kernel(KvCopyArgs g) {
    if ((int)blockIdx.y >= g.n_jobs) return;
    const int4 job = reinterpret_cast<const int4*>(g.jobs)[blockIdx.y];      // (uniform: a scalar load)
    const long long u = (long long)blockIdx.x * KV_COPY_THREADS + threadIdx.x, U = g.page_units;
    if (u < 2 * U) {
        if (job.x < 0 || job.y < 0) return;
        const long long sp = min(job.x, g.num_pages - 1), dp = min(job.y, g.num_pages - 1);
        if (sp == dp) return;                                                // (only a clamped, wrong job: nothing to move)
        const bool v = u >= U;
        uint4* pool = static_cast<uint4*>(v ? g.vq : g.kq);
        const long long o = v ? u - U : u;
        pool[dp * U + o] = pool[sp * U + o];
    } else {
        const long long o = u - 2 * U;
        if (o >= g.stage_units || job.z < 0 || job.w < 0) return;
        const long long sr = min(job.z, g.B - 1), dr = min(job.w, g.B - 1);
        reinterpret_cast<uint4*>(g.stage_dst)[dr * g.stage_units + o] = reinterpret_cast<const uint4*>(g.stage_src)[sr * g.stage_units + o];
    }
}

int launch_kv_paged_copy(const KvCopyArgs& g, void* stream) {
    const dim3 grid((unsigned)kv_copy_blocks(g), (unsigned)g.n_jobs);
    hipLaunchKernelGGL(kv_paged_copy_kernel, grid, dim3(KV_COPY_THREADS), 0, static_cast<hipStream_t>(stream), g);
    return (int)hipGetLastError();
}

}  // namespace mi355q
