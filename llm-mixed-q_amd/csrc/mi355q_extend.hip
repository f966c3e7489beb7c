// mi355q_extend.hip -- chunked prefill: the quantised attention core for any number of new tokens behind a block_fp KV cache.
//
// The reference's `past_key_value` route (models/llama_quantized/modeling_llama.py:301-344, the same in modeling_opt.py) takes n new
// tokens behind a past of L - n: K^T is quantised over all L keys (the append has done that, open block included), the mask has the
// offset of modeling_llama.py:53-79.  The decode kernels (mi355q_decode.hip) serve n <= 16 with a score workspace of 1 KiB per
// (row, key tile, query tile); for a chunk of hundreds of queries that is gigabytes, so this kernel keeps no scores: it is
// bfp_attention_stream_kernel (mi355q_attention.hip) on the cache's fragments.
//   A workgroup is one (row b, block of up to 64 queries), a wave 16 queries (the 16 columns of v_mfma_f32_16x16x32_bf16).  The four
//   waves walk the key tiles together, 32 keys a step; the step's K pieces (and, in pass 2, the V pieces of the key pair) come into
//   LDS by LDS-DMA one step ahead, one barrier a step.  Pass 1 keeps a running maximum and sum of exponentials per lane over the
//   VISIBLE keys; pass 2 forms the scores again from the same operands (the same bits), turns them into probabilities with the final
//   statistics, quantises per block of 16 keys of a query, multiplies with V.  No workspace, no exchange between waves.
// Per-row scalars (L_b, m_b) are read once a workgroup and stay scalar; everything that decides the step count is scalar, so all four
// waves reach every barrier the same number of times.  What the stream kernel leaves open and this one closes:
//   out-of-row reads   a K piece is addressed at tile min(t, need - 1), need <= ceil(L_b / 16) <= C / 16: never a tile of the next row
//                      or behind the allocation (kv_k_bytes has no slack); the clamped piece's scores are discarded (t >= need).
//                      V pairs: st < ceil(need / 2) <= ceil(C / 32).
//   divergent barriers the step count comes from the workgroup's LAST REAL query; a wave whose 16 queries lie behind m_b computes the
//                      last real query again and stores zeros.  A workgroup wholly behind m_b stores zeros and leaves before the
//                      first barrier.
//   paged cache        PG = true (layout and address rules: mi355q_decode.h): a step's pieces -- K tiles 2 st and 2 st + 1, V pair st --
//                      lie in ONE logical page, st / (P / 32), since P >= 32; and so does the clamped tile: min(2 st + 1, need - 1) is
//                      2 st or 2 st + 1 for every st < nsteps.  So a step takes one table entry (scalar, clamped into the pool).  The
//                      place inside the page is formed from the CLAMPED tile, as in the contiguous kernel: the piece read in place of
//                      the missing tile is tile need - 1, one the append has written.  (The clamp acts only for odd need, and a page
//                      holds an even number of tiles, so tile need would lie in the same page: the order decides which piece of the
//                      page is read, not which table entry.)  The step's logical page holds key 32 st <= 16 (need - 1) <= L_b - 1: an
//                      entry below ceil(L_b / P).  Entries are asked for two steps ahead of their DMA.
//   sliding window     WN = true (semantics: mi355q_decode.h): query i at p = L_b - m_b + i sees keys max(0, p - W + 1) .. p.  The walk
//                      begins at step st0 = lo / 32, lo the lower bound of the workgroup's FIRST real query (scalar): the later queries'
//                      bounds are no smaller, so no query of the workgroup sees a key below step st0, and the steps below are not read
//                      (no DMA, paged no table entry).  It ends where it ends today.  The three hazards above stay closed:
//                        out-of-row reads    every step taken is st0 <= st < nsteps, a subset of today's steps; the clamp min(t, need - 1)
//                                            and the V bound do not depend on where the walk starts.  lo <= the first query's horizon
//                                            < 16 need, so st0 <= (need - 1) / 2 < nsteps: at least one step, the look-ahead guards
//                                            (st + 1 < nsteps, pg_entry's st < nsteps) hold as they are.
//                        divergent barriers  st0 is scalar like nsteps: all four waves make nsteps - st0 steps in both passes.  Buffers
//                                            alternate by st & 1 from st0 on; the barrier between the passes still separates the last
//                                            read of pass 1 from the first DMA of pass 2, whichever buffer that is.
//                        paged cache         one entry a step as before, for steps st0 .. nsteps - 1 only: step st0 holds key lo, which
//                                            the first query sees, so every page looked up holds a key some query of the row sees.
//                      A lane's early steps can be wholly below ITS bound (a later wave, a lane group): scores of -inf, which the
//                      running statistics take as "no key yet" -- as they do today above the horizon.  Every query sees its own key.
//   missing V pieces   the last pair's second tile may not exist (t >= need): its probabilities are exact zeros, the stored V there
//                      is finite (zeroed storage or older quantised values).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mi355q.h"
#include "mi355q_internal.h"
#include "mi355q_quant_dev.h"
#include "mi355q_attn_dev.h"
#include "mi355q_extend.h"

namespace mi355q {

// GQ = true (grouped queries): workgroup row b is a QUERY head -- q, out and the grid have B * G of them -- and reads cache row b / G:
// its fragments, lengths[b / G], counts[b / G].  Nothing else differs, so a head's bits are those of GQ = false on a private copy of
// the row.  The G workgroups of a group each read the row's fragments themselves (no sharing inside a workgroup).
template <int DC, bool GQ, bool PG, bool WN = false>
__global__ __launch_bounds__(256) void bfp_attention_extend_kernel(const QuantArgs aq, const QuantArgs ap, const ExtendArgs g) {
    constexpr int DT = DC * 2, KSTEP = 2 * DC * 1024, VSTEP = DT * 1024, STEP = KSTEP + VSTEP;      // bytes per 32 keys
    using gptr_t = const __attribute__((address_space(1))) void*;
    using lptr_t = __attribute__((address_space(3))) void*;
    __shared__ __attribute__((aligned(16))) unsigned char stage[2][STEP];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, lg = lane >> 4;
    // work items (query block, row) in one grid dimension, the heaviest query block of every row first (causal: the last one)
    const int xrank = (int)blockIdx.x / g.nb;
    const long long b = (int)blockIdx.x - xrank * g.nb;
    const long long wg0 = (long long)(g.causal ? g.nxb - 1 - xrank : xrank) * 64;
    const long long m0 = wg0 + 16 * wave;
    long long cb = b;                                       // the cache row
    if constexpr (GQ) cb = (long long)((unsigned)b / (unsigned)g.G);
    // the row's keys and queries: one scalar load each a workgroup
    long long L = g.L, m = g.M;
    if (g.lengths) L = min((long long)max(__builtin_amdgcn_readfirstlane(g.lengths[cb]), 0), g.L);
    if (g.counts) m = min((long long)max(__builtin_amdgcn_readfirstlane(g.counts[cb]), 0), g.M);
    if (m > L) m = 0;                                       // (an empty slot: zeros, no fragment read)
    float* __restrict__ op = g.out + b * g.osb + (m0 + c16) * g.osm + 4 * lg;
    if (wg0 >= m) {                                         // wholly behind the row's queries: zeros, before the first barrier
        if (m0 + c16 < g.M) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) *reinterpret_cast<float4*>(op + 16 * dt) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    const long long qrow = min(m0 + c16, m - 1);            // (a lane behind m_b repeats the last real query; it stores zeros)
    bf16x8 qf[DC];                                          // quantised in registers
    at_quant_q_frag(qf, g.q + b * g.qsb + qrow * g.qsm, g.q_scale, lg, aq, at_block_exponent_mem);
    // this lane's horizon, and the tiles the WORKGROUP walks: up to the horizon of its last real query (scalar; 1 <= need <= C / 16)
    const long long kvis = g.causal ? L - m + qrow : L - 1;
    const long long need = (g.causal ? L - m + min(wg0 + 63, m - 1) : L - 1) / 16 + 1;
    const int nsteps = (int)((need + 1) / 2);
    // windowed: this lane's lower bound, and the workgroup's first step (scalar) from that of its first real query
    long long klo = 0;
    int st0 = 0;
    if constexpr (WN) {
        klo = max(kvis - g.W + 1, 0ll);
        st0 = (int)(max(L - m + wg0 - g.W + 1, 0ll) >> 5);
    }
    const unsigned char* __restrict__ kfb = reinterpret_cast<const unsigned char*>(g.kq) + (PG ? 0 : cb * g.NTC * DC * 1024) + lane * 16;
    const unsigned char* __restrict__ vfb = reinterpret_cast<const unsigned char*>(g.vq) + (PG ? 0 : cb * g.NPC * DT * 1024) + lane * 16;
    const float scale_inv = g.scale_div != 0.f ? 1.0f / g.scale_div : 0.f;

    // LDS-DMA of one step: the K pieces of tiles 2 st, 2 st + 1 (DC KiB each) and, when with_v, the V pieces of pair st (DT KiB);
    // piece p by wave p % 4.  An odd tile count: the last step's second tile is tile need - 1 once more, never one behind the row.
    // paged: `page` is the step's table entry as loaded (pg_entry below); the place inside the page comes from the CLAMPED tile
    auto dma = [&](int st, int buf, bool with_v, int page) {
        long long pbase = 0;                                // the page's first pair in vq; twice that its first tile in kq
        if constexpr (PG) pbase = (long long)min(max(__builtin_amdgcn_readfirstlane(page), 0), g.pg.num_pages - 1) << (g.pg.lg_p - 5);
#pragma unroll
        for (int p = 0; p < 2 * DC; ++p)
            if ((p & 3) == wave) {
                long long t = min(2ll * st + p / DC, need - 1);
                if constexpr (PG) t = 2 * pbase + (t & ((2ll << (g.pg.lg_p - 5)) - 1));
                __builtin_amdgcn_global_load_lds((gptr_t)(kfb + (t * DC + p % DC) * 1024), (lptr_t)(&stage[buf][p * 1024]), 16, 0, 0);
            }
        if (with_v) {
#pragma unroll
            for (int p = 0; p < DT; ++p)
                if ((p & 3) == wave) {
                    long long sp = st;
                    if constexpr (PG) sp = pbase + (st & ((1 << (g.pg.lg_p - 5)) - 1));
                    __builtin_amdgcn_global_load_lds((gptr_t)(vfb + (sp * DT + p) * 1024), (lptr_t)(&stage[buf][KSTEP + p * 1024]), 16, 0, 0);
                }
        }
    };
    // the table entry of step st's page (st < nsteps: a page that holds keys of the row), 0 where there is no such step
    auto pg_entry = [&](int st) -> int {
        if constexpr (PG) return st < nsteps ? g.pg.table[cb * g.pg.max_pages + (st >> (g.pg.lg_p - 5))] : 0;
        else return 0;
    };
    // scores of the step's two tiles for this lane's query: sv[h][e] <-> key 32 st + 16 h + 4 lg + e; -inf: not a visible key
    auto scores = [&](int st, int buf, f32x4 (&sv)[2]) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < DC; ++c) {
                const uint4 kv = *reinterpret_cast<const uint4*>(&stage[buf][(h * DC + c) * 1024 + lane * 16]);
                s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kv), qf[c], s, 0, 0, 0);
            }
            const long long t = 2ll * st + h, key0 = t * 16 + 4 * lg;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float x = g.scale_div != 0.f ? at_div(s[e], g.scale_div, scale_inv) : s[e];
                sv[h][e] = (t < need && key0 + e <= kvis && (!WN || key0 + e >= klo)) ? x : -INFINITY;
            }
        }
    };

    // ---- pass 1: running maximum and sum of exponentials per lane
    float m_run = -INFINITY, l_run = 0.f;
    int pg_next = pg_entry(st0 + 1), pg_after = 0;          // entries of steps st + 1, st + 2 (the top-of-step wait covers their loads)
    dma(st0, st0 & 1, false, pg_entry(st0));
    for (int st = st0; st < nsteps; ++st) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if constexpr (PG) pg_after = pg_entry(st + 2);
        if (st + 1 < nsteps) dma(st + 1, (st + 1) & 1, false, pg_next);
        if constexpr (PG) pg_next = pg_after;
        f32x4 sv[2];
        scores(st, st & 1, sv);
        at_softmax_step(sv, m_run, l_run);
    }
    float row_max, row_sum, row_inv;                        // (every query sees its own key: the row maximum is finite)
    at_softmax_finish(m_run, l_run, row_max, row_sum, row_inv);
    __syncthreads();                                        // (every wave is out of the last step's buffer)

    // ---- pass 2: the scores again, probabilities, quantised, times V
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int mbp = (int)__builtin_log2f(ap.shift);
    pg_next = pg_entry(st0 + 1);
    dma(st0, st0 & 1, true, pg_entry(st0));
    for (int st = st0; st < nsteps; ++st) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if constexpr (PG) pg_after = pg_entry(st + 2);
        if (st + 1 < nsteps) dma(st + 1, (st + 1) & 1, true, pg_next);
        if constexpr (PG) pg_next = pg_after;
        f32x4 sv[2];
        scores(st, st & 1, sv);
        float pq[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float pr[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) pr[e] = sv[h][e] == -INFINITY ? 0.f : at_div(at_exp_neg(sv[h][e] - row_max), row_sum, row_inv);
            at_quant_p_block(pr, pq + 4 * h, mbp, ap, at_block_exponent_mem);
        }
        const bf16x8 pf = at_pack_p(pq);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const uint4 vv = *reinterpret_cast<const uint4*>(&stage[st & 1][KSTEP + dt * 1024 + lane * 16]);
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vv), pf, o[dt], 0, 0, 0);
        }
    }
    if (m0 + c16 < g.M) {
        const bool real = m0 + c16 < m;                     // (rows behind m_b: zeros)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
            *reinterpret_cast<float4*>(op + 16 * dt) = real ? make_float4(o[dt][0], o[dt][1], o[dt][2], o[dt][3]) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// G == 0: one query row a cache row (GQ = false).  G >= 1: q / out hold c.B * G rows, query row r on cache row r / G (GQ = true)
int launch_bfp_attention_extend(const QuantArgs& aq, const QuantArgs& ap, const KvCache& c, const float* q, float* out, long long M,
                                long long max_length, int causal, float q_scale, float scale_div, const long long* strides,
                                const int32_t* lengths, const int32_t* counts, hipStream_t st, int G, const KvPages* pages,
                                long long window) {
    if ((pages || window) && !lengths) return MI355Q_E_BADARG;      // (no uniform paged or windowed launch)
    if (window < 0 || (window && !causal)) return MI355Q_E_BADARG;
    ExtendArgs g{};
    g.W = window;
    if (pages) g.pg = *pages;
    g.q = q; g.kq = c.kq; g.vq = c.vq; g.out = out; g.lengths = lengths; g.counts = counts;
    g.M = M; g.L = max_length; g.NTC = c.C / 16; g.NPC = (c.C + 31) / 32;
    fill_qo_strides(g, strides, M, c.D);
    g.causal = causal; g.q_scale = q_scale; g.scale_div = scale_div;
    const long long nxb = (M + 63) / 64, rows = c.B * (G ? G : 1);
    if (rows * nxb > 0x7FFFFFFFLL) return MI355Q_E_UNSUPPORTED;
    g.nb = (int)rows; g.nxb = (int)nxb; g.G = G;
    const dim3 grid((unsigned)(rows * nxb));
#define MI355Q_EXTEND_GO(DC_)                                                                                          \
    if (window && pages && G) hipLaunchKernelGGL((bfp_attention_extend_kernel<DC_, true, true, true>), grid, dim3(256), 0, st, aq, ap, g);   \
    else if (window && pages) hipLaunchKernelGGL((bfp_attention_extend_kernel<DC_, false, true, true>), grid, dim3(256), 0, st, aq, ap, g); \
    else if (window && G) hipLaunchKernelGGL((bfp_attention_extend_kernel<DC_, true, false, true>), grid, dim3(256), 0, st, aq, ap, g);     \
    else if (window) hipLaunchKernelGGL((bfp_attention_extend_kernel<DC_, false, false, true>), grid, dim3(256), 0, st, aq, ap, g);         \
    else if (pages && G) hipLaunchKernelGGL((bfp_attention_extend_kernel<DC_, true, true>), grid, dim3(256), 0, st, aq, ap, g);        \
    else if (pages) hipLaunchKernelGGL((bfp_attention_extend_kernel<DC_, false, true>), grid, dim3(256), 0, st, aq, ap, g);      \
    else if (G) hipLaunchKernelGGL((bfp_attention_extend_kernel<DC_, true, false>), grid, dim3(256), 0, st, aq, ap, g);          \
    else hipLaunchKernelGGL((bfp_attention_extend_kernel<DC_, false, false>), grid, dim3(256), 0, st, aq, ap, g);
    switch (c.D / 32) {
        case 1: MI355Q_EXTEND_GO(1); break;
        case 2: MI355Q_EXTEND_GO(2); break;
        case 3: MI355Q_EXTEND_GO(3); break;
        case 4: MI355Q_EXTEND_GO(4); break;
        default: return MI355Q_E_UNSUPPORTED;
    }
#undef MI355Q_EXTEND_GO
    return (int)hipGetLastError();
}

}  // namespace mi355q
