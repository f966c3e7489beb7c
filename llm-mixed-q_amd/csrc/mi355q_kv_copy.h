// Copy-on-write for the paged block_fp KV cache (mi355q_kv_copy.hip): the ONE launch behind PagedKVCache.fork / .reorder, and the
// argument check of its export, mi355q_bfp_kv_paged_copy.  The check is host code only -- no kernel, no launch, no HIP call, no HIP
// header -- so that a stand-alone program can include it (tools/kv_call_check/kv_copy_rows.cpp).
//
// A JOB is int32 x 4 on the device, 16 bytes: (src_page, dst_page, src_row, dst_row).
//   pages   src_page, dst_page >= 0: the WHOLE page src_page of both pools becomes page dst_page -- P / 16 tiles x D / 32 KiB of K^T and
//           P / 32 pairs x D / 16 KiB of V (mi355q_decode.h: paged cache), P * D * 2 bytes each; of the int8-mantissa pools
//           (mi355q_kvp.h, mi355q_bfp_kv8_paged_copy) the same pieces at 544 bytes, P * D * 17 / 16 bytes each.  Whole pages: a recycled page may hold
//           anything behind the row's keys, and copying all of it keeps the kernel free of per-row lengths.  Either id negative: no page
//           copy.  Ids are clamped into 0 .. num_pages - 1 like every paged kernel's: a wrong job gives wrong numbers, never an address
//           outside the pools.
//   rows    src_row, dst_row >= 0: the 16 x D fp32 stage rows of src_row in `stage_src` become those of dst_row in `stage_dst`, a SECOND
//           buffer of the same shape: a permutation of rows (a beam swap) done in place would read rows another job of the same launch
//           has already overwritten.  Either negative: no stage copy.  Rows are clamped into 0 .. B - 1.
// The caller keeps the jobs of one launch apart: no page is the destination of one job and the source or destination of another
// (PagedKVCache draws every destination from the free list before any page of the call returns to it), no row is two jobs' dst_row.
// No atomics, no grid-wide wait, no LDS, no workspace; 16-byte vector loads and stores only.
#ifndef MI355Q_KV_COPY_H
#define MI355Q_KV_COPY_H
#include <stdint.h>

#include <initializer_list>

#include "mi355q.h"

namespace mi355q {

constexpr int KV_COPY_THREADS = 256;        // one 16-byte unit a thread
constexpr int64_t KV_COPY_MAX_JOBS = 65535; // the grid's second dimension

struct KvCopyArgs {
    void* kq;                 // the pools
    void* vq;
    const float* stage_src;   // [B][16][D] fp32
    float* stage_dst;
    const int32_t* jobs;      // [n_jobs][4] on the device
    long long page_units;     // 16-byte units of one page of ONE pool: P * D / 8 (bf16), P * D * 17 / 256 (int8 mantissas)
    int stage_units;          // 16-byte units of one row's stage: 4 * D
    int num_pages, B, n_jobs;
};

// true: launch with `g`.  false: return rc (an MI355Q_E_* code, or 0 where there is nothing to do).  The order of the checks is ABI.
// int8: the pools hold the 544-byte pieces of mi355q_kvp.h -- only the size of a page differs (P * D is a multiple of 1024: whole units)
inline bool kv_copy_check(const void* kq, const void* vq, const void* stage_src, const void* stage_dst, const void* jobs, int64_t n_jobs,
                          int64_t B, int64_t num_pages, int64_t P, int64_t D, bool int8, KvCopyArgs& g, int& rc) {
    const auto stop = [&rc](int code) { rc = code; return false; };
    g = KvCopyArgs{};
    if (n_jobs < 0 || B < 1 || B > 65535 || num_pages < 1 || num_pages > 0x7FFFFFFFLL) return stop(MI355Q_E_BADARG);
    if (P < 32 || (P & (P - 1)) != 0 || P > (1LL << 30) || D < 32 || D % 32 != 0 || D > 128) return stop(MI355Q_E_BADARG);
    if (n_jobs == 0) return stop(0);
    if (!kq || !vq || !stage_src || !stage_dst || !jobs || stage_src == stage_dst) return stop(MI355Q_E_BADARG);
    if (n_jobs > KV_COPY_MAX_JOBS) return stop(MI355Q_E_UNSUPPORTED);
    uintptr_t low = 0;
    for (const void* p : {kq, vq, stage_src, stage_dst, jobs}) low |= reinterpret_cast<uintptr_t>(p);
    if (low % 16 != 0) return stop(MI355Q_E_ALIGN);
    g.kq = const_cast<void*>(kq); g.vq = const_cast<void*>(vq);
    g.stage_src = static_cast<const float*>(stage_src); g.stage_dst = static_cast<float*>(const_cast<void*>(stage_dst));
    g.jobs = static_cast<const int32_t*>(jobs);
    g.page_units = int8 ? P * D / 256 * 17 : P * D / 8;
    g.stage_units = (int)(4 * D);
    g.num_pages = (int)num_pages; g.B = (int)B; g.n_jobs = (int)n_jobs;
    rc = 0;
    return true;
}
// blocks a job: both pools' pages and the stage rows, one unit a thread.  The kernel picks a unit's segment per THREAD: a bf16 page and
// the stage rows are multiples of 64 units, an int8-mantissa page (68 units at P = D = 32) is not, and a wave may straddle two segments
inline long long kv_copy_blocks(const KvCopyArgs& g) { return (2 * g.page_units + g.stage_units + KV_COPY_THREADS - 1) / KV_COPY_THREADS; }

// mi355q_kv_copy.hip; `stream` is a hipStream_t
int launch_kv_paged_copy(const KvCopyArgs& g, void* stream);

}  // namespace mi355q
#endif
