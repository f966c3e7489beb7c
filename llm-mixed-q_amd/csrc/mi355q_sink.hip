// mi355q_sink.hip -- attention sinks: the sliding-window decode and extend kernels with the first S <= 16 keys visible to every query.
//
// Semantics, the virtual-pair partition of the decode and the host's span: mi355q_sink.h.  The kernels are the WN = true forms of
// mi355q_decode.hip (decode_scores_kernel, decode_pv_kernel) and mi355q_extend.hip (bfp_attention_extend_kernel) with the sink piece in
// front; decode_sum_kernel is reused as it is (launch_decode_sum).  Shared arithmetic comes from mi355q_attn_dev.h and mi355q_decode_dev.h,
// the host arithmetic from decode_args_fill; what those two headers do not hold -- the loops themselves, the lower bound of a window --
// stands here a second time, so this file is a MIRROR SITE of the windowed kernels as mi355q_kvp.hip and mi355q_kvbm.hip are of the
// unwindowed ones: a change to a loop there is made here as well.  Always ragged (per-row lengths), always causal.
//
// Visibility, one rule for every tile of both kernels: key k is visible to a lane whose query has horizon kvis and lower bound klo when
//   klo <= k <= kvis   or   k < smax,   smax = min(S, kvis + 1)
// The second term can hold in key tile 0 only (S <= 16).  In a sink piece -- p0_b >= 1, st0 >= 1 -- every lane's klo is >= 32, so the
// first term is false for every key of pair 0 and the piece's tile 1 holds no visible key.
//
// Decode.  Row b walks VIRTUAL tiles vt = 0 .. NTv - 1: with p0_b >= 1, vt 0 / 1 are tiles 0 / 1 and vt >= 2 is tile vt + 2 p0_b - 2,
// NTv = NT_b - 2 p0_b + 2; with p0_b == 0, vt is the tile.  Not read (no K fragment, no score, probabilities exact zeros): every tile
// below tile lo_b / 16 EXCEPT tile 0 -- that is vt 1 of a sink pair, the first tile of pair p0_b when lo_b lies in its second tile, and
// nothing else.  Tile 0 is read even where the window begins in tile 1 (p0_b == 0, lo_b >= 16): its sinks are visible.
//   bounds      every tile read is < NT_b <= ceil(max_length / 16) <= C / 16: inside the row (and, paged, inside the table's row).  A virtual
//               tile is < NTv <= g.NT, the workspace stride: NT_b - 2 p0_b <= NT(decode_window_span) as in the windowed kernels, and with
//               p0_b >= 1 also <= NT(max_length) - 2; with p0_b == 0, NTv = NT_b <= NT(max_length) and the window's span is max_length or
//               the row is shorter than the span.  The virtual pairs NPv = ceil(NTv / 2) <= g.NP <= pps S: some split takes every pair.
//   paged       the table entry of the NEXT virtual tile is asked for one iteration ahead, read or not: vt 1 lies in logical page 0 with
//               tile 0, and a skipped first tile of pair p0_b in the page of key lo_b.  Logical page 0 must be held (PagedKVCache.trim).
//   empty piece a sink pair in which no lane sees a key -- S = 0 compiled into this form, which the launcher never does -- leaves its
//               lanes at (-inf, 0): alone in a split, the split's statistics are (-inf, 0), which the combination skips, and its P blocks
//               are all zeros, which quantise to zeros (bmax = 0) and meet finite V.  A row with L_b < M counts as empty (dec_length):
//               every split of it takes the empty paths before any K / V read.
//   row maximum every query sees its own key (W >= 1), so some split's maximum is finite, sinks or not.
//   p0_b == 0   the walk, the partition and the workspace index are the windowed kernels'; where no sink lies below a column's klo the
//               extra term changes no predicate and the bits are theirs (given the same splits and pps).
//
// Extend.  A workgroup walks a SEQUENCE of steps j = 0 .. nj - 1: with st0 >= 1, step_of(0) = 0 and step_of(j) = st0 + j - 1,
// nj = 1 + nsteps - st0; with st0 == 0, step_of(j) = j, nj = nsteps -- the windowed walk.  The three hazards of mi355q_extend.hip's comment:
//   out-of-row reads    every step taken is 0 or st0 <= st < nsteps, a subset of the unwindowed kernel's steps; K tiles are clamped to
//                       min(t, need - 1) and V pairs are < ceil(need / 2) as there.  st0 >= 1 means need >= 2 st0 + 1 >= 3: step 0's tiles 0
//                       and 1 both exist, the scores of tile 1 are discarded by the visibility rule (no key of it is a sink, klo >= 32).
//   divergent barriers  st0, nsteps and nj are scalar: all four waves make nj steps in each pass.  The double buffer follows the
//                       SEQUENCE index, buffer j & 1, not the step: the DMA of sequence step j + 1 into buffer (j + 1) & 1 is issued behind
//                       the barrier at the top of step j, which every wave reaches only after its last read of step j - 1 -- the previous
//                       user of that buffer -- whatever key steps j - 1 and j + 1 are.  The barrier between the passes separates the last
//                       read of pass 1 (buffer (nj - 1) & 1) from the first DMA of pass 2 (buffer 0).
//   missing V pieces    step 0 of a sink walk has both tiles (need >= 3); the last pair's missing second tile is handled as there.
//   paged               one table entry a sequence step, asked for two steps ahead: entry 0 for step 0 -- logical page 0 must be held -- and
//                       the entries of steps st0 .. nsteps - 1 as in the windowed kernel.
//   empty piece         a lane that sees no key of a step has scores of -inf there, which the running statistics take as "no key yet".
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mi355q.h"
#include "mi355q_internal.h"
#include "mi355q_quant_dev.h"
#include "mi355q_attn_dev.h"
#include "mi355q_decode.h"
#include "mi355q_decode_dev.h"
#include "mi355q_extend.h"
#include "mi355q_sink.h"

namespace mi355q {

long long decode_sink_span(long long M, long long L, long long window) {
    const long long span = decode_window_span(M, L, window);
    return span + 32 < L ? span + 32 : L;
}

// (mirrors of mi355q_decode.hip's dec_window_lo / dec_window_first)
__device__ __forceinline__ long long sink_window_lo(const DecodeArgs& g, long long kvis) { return max(kvis - g.W + 1, 0ll); }
__device__ __forceinline__ long long sink_window_first(const DecodeArgs& g, long long L) { return max(L - g.M - g.W + 1, 0ll); }

template <int DC, bool GQ, bool PG>
__global__ __launch_bounds__(256) void decode_scores_sink_kernel(const QuantArgs aq, const DecodeArgs g, const int sinks) {
    __shared__ float sm_[4][64], sl_[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, lg = lane >> 4;
    const long long b = blockIdx.y, s = blockIdx.x, cb = dec_cache_row<GQ>(g, b);   // b: launch row (workspace), cb: cache row
    const long long L = dec_length<true>(g, cb), NT = (L + 15) >> 4;
    // virtual tile vt -> tile: vt < 2 itself, else vt + shift (p0 == 0: shift 0, the windowed walk)
    const long long t_first = sink_window_first(g, L) >> 4, p0 = t_first >> 1;
    const long long shift = p0 > 0 ? 2 * p0 - 2 : 0, NTv = NT - shift;
    const long long vt_lo = 2 * g.pps * s, vt_hi = min(NTv, vt_lo + 2 * g.pps);
    if (vt_lo >= NTv) {                 // a split wholly behind the row's last virtual tile: the empty statistics, no kq read
        dec_stats_empty(g, b, s, tid);
        return;
    }
    long long row, qrow;
    dec_column<GQ>(g, b, c16, row, qrow);
    bf16x8 qf[DC];                      // quantised in registers
    at_quant_q_frag(qf, g.q + row * g.qsb + qrow * g.qsm, g.q_scale, lg, aq, at_block_exponent_mem);
    const long long kvis = dec_horizon(g, L, qrow);
    const long long klo = sink_window_lo(g, kvis);
    const int lane_rel = (int)(4 * lg - klo), smax = (int)min((long long)sinks, kvis + 1);
    const unsigned wd = (unsigned)(kvis - klo);
    auto visible = [&](long long t, int e) -> bool {
        return (unsigned)((int)(t << 4) + lane_rel + e) <= wd || (int)(t << 4) + 4 * lg + e < smax;
    };
    auto tile_of = [&](long long vt) -> long long { return vt < 2 ? vt : vt + shift; };
    const float scale_inv = g.scale_div != 0.f ? 1.0f / g.scale_div : 0.f;
    const uint16_t* __restrict__ kfb = g.kq + (PG ? 0 : cb * g.NTC * DC * 512) + lane * 8;
    float* __restrict__ sc = g.scores + b * g.NT * 256 + lane * 4;
    // running (max, sum of exp(x - max)) of this lane's visible scores, re-based when the maximum moves
    float m_run = -INFINITY, l_run = 0.f;
    int raw = 0;                        // paged: the table entry of the next virtual tile of this wave (tile_of(vt) < NT)
    if constexpr (PG) {
        if (vt_lo + wave < vt_hi) raw = pg_raw(g.pg, cb, tile_of(vt_lo + wave) >> (g.pg.lg_p - 4));
    }
    for (long long vt = vt_lo + wave; vt < vt_hi; vt += 4) {
        const long long t = tile_of(vt);
        long long pt = t;                                   // the tile's place in kq; the workspace keeps vt
        if constexpr (PG) {
            pt = pg_place(g.pg, __builtin_amdgcn_readfirstlane(raw), t, g.pg.lg_p - 4);
            if (vt + 4 < vt_hi) raw = pg_raw(g.pg, cb, tile_of(vt + 4) >> (g.pg.lg_p - 4));
        }
        if (vt != 0 && t < t_first) continue;               // (scalar: no query of the row sees a key of this tile)
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < DC; ++c)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(kfb + (pt * DC + c) * 512), qf[c], acc, 0, 0, 0);
        if (g.scale_div != 0.f) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = at_div(acc[e], g.scale_div, scale_inv);
        }
        *reinterpret_cast<float4*>(sc + vt * 256) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        float tm = -INFINITY;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (visible(t, e)) tm = fmaxf(tm, acc[e]);
        if (tm > m_run) {
            l_run = m_run == -INFINITY ? 0.f : l_run * at_exp_neg(m_run - tm);
            m_run = tm;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (visible(t, e)) l_run += at_exp_neg(acc[e] - m_run);
    }
    sm_[wave][lane] = m_run;
    sl_[wave][lane] = l_run;
    __syncthreads();
    if (tid < 16) {
        // the 16 (wave, lane group) pairs of query tid, in a fixed order
        float mx = -INFINITY;
        for (int w = 0; w < 4; ++w)
            for (int q4 = 0; q4 < 4; ++q4) mx = fmaxf(mx, sm_[w][tid + 16 * q4]);
        float sum = 0.f;
        for (int w = 0; w < 4; ++w)
            for (int q4 = 0; q4 < 4; ++q4) {
                const float m = sm_[w][tid + 16 * q4];
                if (m != -INFINITY) sum += sl_[w][tid + 16 * q4] * at_exp_neg(m - mx);
            }
        float* st = g.stats + ((b * g.S + s) * 16 + tid) * 2;
        st[0] = mx;
        st[1] = sum;
    }
}

template <int DC, bool GQ, bool PG>
__global__ __launch_bounds__(256) void decode_pv_sink_kernel(const QuantArgs ap, const DecodeArgs g, const int sinks) {
    constexpr int DT = DC * 2;
    __shared__ f32x4 red[4][DT][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, lg = lane >> 4;
    const long long b = blockIdx.y, s = blockIdx.x, cb = dec_cache_row<GQ>(g, b);
    const long long L = dec_length<true>(g, cb), NT = (L + 15) >> 4;
    // virtual pair v -> pair: v == 0 itself, else v + shift / 2 (decode_scores_sink_kernel's virtual tiles, two a pair)
    const long long t_first = sink_window_first(g, L) >> 4, p0 = t_first >> 1;
    const long long shift = p0 > 0 ? 2 * p0 - 2 : 0, NPv = (NT - shift + 1) >> 1;
    const long long p_lo = g.pps * s, p_hi = min(NPv, p_lo + g.pps);
    if (p_lo >= p_hi) {                 // an empty split (every split of an empty row): a zero partial output, no vq read
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int dt = wave; dt < DT; dt += 4) {
            if (g.S == 1) {
                if (dec_real<GQ>(g, c16)) *reinterpret_cast<float4*>(dec_out<GQ>(g, b, c16) + 16 * dt + 4 * lg) = zero;
            } else {
                *reinterpret_cast<float4*>(g.part + (((b * g.S + s) * DT + dt) * 64 + lane) * 4) = zero;
            }
        }
        return;
    }
    long long row, qrow;
    dec_column<GQ>(g, b, c16, row, qrow);
    const long long kvis = dec_horizon(g, L, qrow);
    const long long klo = sink_window_lo(g, kvis);      // (the visibility test of decode_scores_sink_kernel)
    const int lane_rel = (int)(4 * lg - klo), smax = (int)min((long long)sinks, kvis + 1);
    const unsigned wd = (unsigned)(kvis - klo);
    auto visible = [&](long long t, int e) -> bool {
        return (unsigned)((int)(t << 4) + lane_rel + e) <= wd || (int)(t << 4) + 4 * lg + e < smax;
    };
    auto pair_of = [&](long long v) -> long long { return v < 1 ? v : v + (shift >> 1); };
    // the row's statistics over all its visible keys: the S splits in split order (every query sees its own key: some split's max is
    // finite; a split in which a column sees nothing holds (-inf, 0) for it and is skipped)
    const float* __restrict__ stp = g.stats + (b * g.S * 16 + c16) * 2;
    float row_max = -INFINITY;
    for (int i = 0; i < g.S; ++i) row_max = fmaxf(row_max, stp[i * 32]);
    float row_sum = 0.f;
    for (int i = 0; i < g.S; ++i) {
        const float m = stp[i * 32];
        if (m != -INFINITY) row_sum += stp[i * 32 + 1] * at_exp_neg(m - row_max);
    }
    const float row_inv = 1.0f / row_sum;
    const int mbp = (int)__builtin_log2f(ap.shift);
    const uint16_t* __restrict__ vfb = g.vq + (PG ? 0 : cb * g.NPC * DT * 512) + lane * 8;
    const float* __restrict__ sc = g.scores + b * g.NT * 256 + lane * 4;
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    int raw = 0;                                            // (paged: one pair ahead; pair_of(v) < NP for v < NPv)
    if constexpr (PG) {
        if (p_lo + wave < p_hi) raw = pg_raw(g.pg, cb, pair_of(p_lo + wave) >> (g.pg.lg_p - 5));
    }
    for (long long v = p_lo + wave; v < p_hi; v += 4) {
        const long long pr_i = pair_of(v);
        long long pp = pr_i;                                // the pair's place in vq; the scores keep v, the horizon pr_i
        if constexpr (PG) {
            pp = pg_place(g.pg, __builtin_amdgcn_readfirstlane(raw), pr_i, g.pg.lg_p - 5);
            if (v + 4 < p_hi) raw = pg_raw(g.pg, cb, pair_of(v + 4) >> (g.pg.lg_p - 5));
        }
        uint4 vb[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) vb[dt] = *reinterpret_cast<const uint4*>(vfb + (pp * DT + dt) * 512);
        float pq[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const long long vt = 2 * v + h, t = 2 * pr_i + h;  // (uniform over the wave; the last pair's second tile may not exist)
            const bool has = t < NT && (vt == 0 || t >= t_first);      // (a tile the scores kernel skipped has no scores)
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (has) x = *reinterpret_cast<const float4*>(sc + vt * 256);
            const float xs[4] = {x.x, x.y, x.z, x.w};
            float pr[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) pr[e] = (has && visible(t, e)) ? at_div(at_exp_neg(xs[e] - row_max), row_sum, row_inv) : 0.f;
            at_quant_p_block(pr, pq + 4 * h, mbp, ap, at_block_exponent_mem);
        }
        const bf16x8 pf = at_pack_p(pq);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vb[dt]), pf, o[dt], 0, 0, 0);
    }
    // the four waves' partial outputs, summed in wave order
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) red[wave][dt][lane] = o[dt];
    __syncthreads();
    for (int dt = wave; dt < DT; dt += 4) {
        f32x4 sum = red[0][dt][lane];
#pragma unroll
        for (int w = 1; w < 4; ++w) sum += red[w][dt][lane];
        if (g.S == 1) {
            if (dec_real<GQ>(g, c16))
                *reinterpret_cast<float4*>(dec_out<GQ>(g, b, c16) + 16 * dt + 4 * lg) = make_float4(sum[0], sum[1], sum[2], sum[3]);
        } else {
            *reinterpret_cast<f32x4*>(g.part + (((b * g.S + s) * DT + dt) * 64 + lane) * 4) = sum;
        }
    }
}

// G == 0: one query row a cache row, the GQ = false kernels.  G >= 1: the grouped kernels over c.B * rpc launch rows.
int launch_bfp_attention_decode_sink(const QuantArgs& aq, const QuantArgs& ap, const KvCache& c, const float* q, float* out, void* workspace,
                                     long long M, long long L, float q_scale, float scale_div, const long long* strides, int splits,
                                     hipStream_t st, const int32_t* lengths, int G, const KvPages* pages, long long window, long long sinks) {
    if (!lengths || window < 1 || sinks < 0 || sinks > SINKS_MAX) return MI355Q_E_BADARG;
    if (sinks == 0)                     // today's windowed call: the same kernels, the same bits
        return launch_bfp_attention_decode(aq, ap, c, q, out, workspace, M, L, 1, q_scale, scale_div, strides, splits, st, lengths, G, pages, window);
    DecodeArgs g{};
    long long rows;
    if (const int rc = decode_args_fill(g, c.B, c.C, c.D, M, L, decode_sink_span(M, L, window), G, splits, strides, workspace, pages, rows)) return rc;
    g.W = window;
    g.q = q; g.kq = c.kq; g.vq = c.vq; g.out = out; g.lengths = lengths;
    g.causal = 1; g.q_scale = q_scale; g.scale_div = scale_div;
    const dim3 grid((unsigned)g.S, (unsigned)rows);
    const int S = (int)sinks;
#define MI355Q_SINK_DECODE_GO2(DC_, GQ_, PG_)                                                                       \
    hipLaunchKernelGGL((decode_scores_sink_kernel<DC_, GQ_, PG_>), grid, dim3(256), 0, st, aq, g, S);                \
    hipLaunchKernelGGL((decode_pv_sink_kernel<DC_, GQ_, PG_>), grid, dim3(256), 0, st, ap, g, S);
#define MI355Q_SINK_DECODE_GO(DC_)                                                                                  \
    if (pages) {                                                                                                    \
        if (G) { MI355Q_SINK_DECODE_GO2(DC_, true, true) } else { MI355Q_SINK_DECODE_GO2(DC_, false, true) }         \
    } else {                                                                                                        \
        if (G) { MI355Q_SINK_DECODE_GO2(DC_, true, false) } else { MI355Q_SINK_DECODE_GO2(DC_, false, false) }       \
    }
    switch (c.D / 32) {
        case 1: MI355Q_SINK_DECODE_GO(1); break;
        case 2: MI355Q_SINK_DECODE_GO(2); break;
        case 3: MI355Q_SINK_DECODE_GO(3); break;
        case 4: MI355Q_SINK_DECODE_GO(4); break;
        default: return MI355Q_E_UNSUPPORTED;
    }
#undef MI355Q_SINK_DECODE_GO
#undef MI355Q_SINK_DECODE_GO2
    launch_decode_sum(g, G != 0, rows, st);
    return (int)hipGetLastError();
}

// GQ = true (grouped queries): workgroup row b is a QUERY head and reads cache row b / G, as in bfp_attention_extend_kernel.
template <int DC, bool GQ, bool PG>
__global__ __launch_bounds__(256) void bfp_attention_extend_sink_kernel(const QuantArgs aq, const QuantArgs ap, const ExtendArgs g, const int sinks) {
    constexpr int DT = DC * 2, KSTEP = 2 * DC * 1024, VSTEP = DT * 1024, STEP = KSTEP + VSTEP;      // bytes per 32 keys
    using gptr_t = const __attribute__((address_space(1))) void*;
    using lptr_t = __attribute__((address_space(3))) void*;
    __shared__ __attribute__((aligned(16))) unsigned char stage[2][STEP];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, lg = lane >> 4;
    // work items (query block, row) in one grid dimension, the heaviest query block of every row first (the last one)
    const int xrank = (int)blockIdx.x / g.nb;
    const long long b = (int)blockIdx.x - xrank * g.nb;
    const long long wg0 = (long long)(g.nxb - 1 - xrank) * 64;
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
    const long long kvis = L - m + qrow;
    const long long need = (L - m + min(wg0 + 63, m - 1)) / 16 + 1;
    const int nsteps = (int)((need + 1) / 2);
    // this lane's lower bound and sinks, and the workgroup's first window step (scalar) from the bound of its first real query
    const long long klo = max(kvis - g.W + 1, 0ll), smax = min((long long)sinks, kvis + 1);
    const int st0 = (int)(max(L - m + wg0 - g.W + 1, 0ll) >> 5);
    // the sequence of steps: with st0 >= 1 the sink step 0 in front of steps st0 .. nsteps - 1 (st0 <= (need - 1) / 2 < nsteps: nj >= 1)
    const int jump = st0 > 0 ? st0 - 1 : 0, nj = nsteps - jump;
    auto step_of = [&](int j) -> int { return j < 1 ? j : j + jump; };
    const unsigned char* __restrict__ kfb = reinterpret_cast<const unsigned char*>(g.kq) + (PG ? 0 : cb * g.NTC * DC * 1024) + lane * 16;
    const unsigned char* __restrict__ vfb = reinterpret_cast<const unsigned char*>(g.vq) + (PG ? 0 : cb * g.NPC * DT * 1024) + lane * 16;
    const float scale_inv = g.scale_div != 0.f ? 1.0f / g.scale_div : 0.f;

    // LDS-DMA of key step st into buffer buf (bfp_attention_extend_kernel's): K tiles 2 st, 2 st + 1 clamped to need - 1 and, when
    // with_v, V pair st; paged: `page` is the step's table entry as loaded
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
    // the table entry of sequence step j's page (j < nj: step_of(j) < nsteps, a page that holds keys of the row), 0 where there is none
    auto pg_entry = [&](int j) -> int {
        if constexpr (PG) return j < nj ? g.pg.table[cb * g.pg.max_pages + (step_of(j) >> (g.pg.lg_p - 5))] : 0;
        else return 0;
    };
    // scores of key step st's two tiles for this lane's query: sv[h][e] <-> key 32 st + 16 h + 4 lg + e; -inf: not a visible key
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
                sv[h][e] = (t < need && key0 + e <= kvis && (key0 + e >= klo || key0 + e < smax)) ? x : -INFINITY;
            }
        }
    };

    // ---- pass 1: running maximum and sum of exponentials per lane
    float m_run = -INFINITY, l_run = 0.f;
    int pg_next = pg_entry(1), pg_after = 0;                // entries of sequence steps j + 1, j + 2 (the top-of-step wait covers their loads)
    dma(0, 0, false, pg_entry(0));                          // (step_of(0) = 0)
    for (int j = 0; j < nj; ++j) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if constexpr (PG) pg_after = pg_entry(j + 2);
        if (j + 1 < nj) dma(step_of(j + 1), (j + 1) & 1, false, pg_next);
        if constexpr (PG) pg_next = pg_after;
        f32x4 sv[2];
        scores(step_of(j), j & 1, sv);
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
    pg_next = pg_entry(1);
    dma(0, 0, true, pg_entry(0));
    for (int j = 0; j < nj; ++j) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if constexpr (PG) pg_after = pg_entry(j + 2);
        if (j + 1 < nj) dma(step_of(j + 1), (j + 1) & 1, true, pg_next);
        if constexpr (PG) pg_next = pg_after;
        f32x4 sv[2];
        scores(step_of(j), j & 1, sv);
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
            const uint4 vv = *reinterpret_cast<const uint4*>(&stage[j & 1][KSTEP + dt * 1024 + lane * 16]);
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
int launch_bfp_attention_extend_sink(const QuantArgs& aq, const QuantArgs& ap, const KvCache& c, const float* q, float* out, long long M,
                                     long long max_length, float q_scale, float scale_div, const long long* strides, const int32_t* lengths,
                                     const int32_t* counts, hipStream_t st, int G, const KvPages* pages, long long window, long long sinks) {
    if (!lengths || window < 1 || sinks < 0 || sinks > SINKS_MAX) return MI355Q_E_BADARG;
    if (sinks == 0)                     // today's windowed call: the same kernel, the same bits
        return launch_bfp_attention_extend(aq, ap, c, q, out, M, max_length, 1, q_scale, scale_div, strides, lengths, counts, st, G, pages, window);
    ExtendArgs g{};
    g.W = window;
    if (pages) g.pg = *pages;
    g.q = q; g.kq = c.kq; g.vq = c.vq; g.out = out; g.lengths = lengths; g.counts = counts;
    g.M = M; g.L = max_length; g.NTC = c.C / 16; g.NPC = (c.C + 31) / 32;
    fill_qo_strides(g, strides, M, c.D);
    g.causal = 1; g.q_scale = q_scale; g.scale_div = scale_div;
    const long long nxb = (M + 63) / 64, rows = c.B * (G ? G : 1);
    if (rows * nxb > 0x7FFFFFFFLL) return MI355Q_E_UNSUPPORTED;
    g.nb = (int)rows; g.nxb = (int)nxb; g.G = G;
    const dim3 grid((unsigned)(rows * nxb));
    const int S = (int)sinks;
#define MI355Q_SINK_EXTEND_GO(DC_)                                                                                                     \
    if (pages && G) hipLaunchKernelGGL((bfp_attention_extend_sink_kernel<DC_, true, true>), grid, dim3(256), 0, st, aq, ap, g, S);       \
    else if (pages) hipLaunchKernelGGL((bfp_attention_extend_sink_kernel<DC_, false, true>), grid, dim3(256), 0, st, aq, ap, g, S);     \
    else if (G) hipLaunchKernelGGL((bfp_attention_extend_sink_kernel<DC_, true, false>), grid, dim3(256), 0, st, aq, ap, g, S);         \
    else hipLaunchKernelGGL((bfp_attention_extend_sink_kernel<DC_, false, false>), grid, dim3(256), 0, st, aq, ap, g, S);
    switch (c.D / 32) {
        case 1: MI355Q_SINK_EXTEND_GO(1); break;
        case 2: MI355Q_SINK_EXTEND_GO(2); break;
        case 3: MI355Q_SINK_EXTEND_GO(3); break;
        case 4: MI355Q_SINK_EXTEND_GO(4); break;
        default: return MI355Q_E_UNSUPPORTED;
    }
#undef MI355Q_SINK_EXTEND_GO
    return (int)hipGetLastError();
}

}  // namespace mi355q
