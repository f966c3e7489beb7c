// mi355q_kvbm.hip -- the block_minifloat KV cache and the split-key decode attention on it (layout and scope: mi355q_kvbm.h).
//
// The reference decodes a block_minifloat attention layer as it decodes any other: torch.cat of fp32 K / V (modeling_llama.py:301-306)
// and the four quantisers over all L keys on every step (matmul.py:199-249).  Here the cache holds what the two weight-side quantisers
// make of k^T and v, in the block_fp cache's layout (mi355q_decode.h: bf16 halfwords in MFMA fragment order -- the layout does not care
// which quantiser made them), and a step quantises the new key, the open 16-key tile, Q and P only.
// What this file owns, in the ragged form only (RG = true; not paged, no window), typed like kv_append_kernel<true, false> and
// decode_scores_kernel / decode_pv_kernel<DC, true, GQ, false> of mi355q_decode.hip as mi355q_kvp.hip's kernels are: the append with the
// block_minifloat store (kvbm_store_block) and phases A and B with the block_minifloat Q and P quantisers (mi355q_attn_dev.h:
// at_bm_quant_q_frag, at_bm_quant_p_block).  These bodies are twins of mi355q_decode.hip's ragged kernels: a change there to the K
// walk, the per-tile statistics and their reduction, the zero partial output, the row statistics or the wave reduction is mirrored
// here once (and once in mi355q_kvp.hip, for both mantissa storages): workspace, split partition and the order of every sum are those
// of mi355q_decode.hip.  What it takes from elsewhere: append_row, append_v_block, the column helpers and dec_stats_empty
// (mi355q_decode_dev.h); from mi355q_decode.hip the staging pass (launch_kv_stage_ragged), phase C (launch_decode_sum) and the host
// arithmetic of both launches (append_ragged_grid, decode_args_fill).
// Hazards: the two quantisers call __any (the rare table walks), so every lane that reaches them must do so with its wave's other
// live lanes -- they sit outside per-lane conditions; threads that left the append early are simply not in the vote.  No table is
// staged in LDS: the walks read their threshold from memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mi355q.h"
#include "mi355q_internal.h"
#include "mi355q_quant_dev.h"
#include "mi355q_attn_dev.h"
#include "mi355q_decode.h"
#include "mi355q_decode_dev.h"
#include "mi355q_kvbm.h"

namespace mi355q {

// ---- append ---------------------------------------------------------------------------------------------------------------
struct AppendBmArgs {
    KvCache c;
    const float* k;
    const float* v;
    long long ksb, kst, vsb, vst;
    long long n;
    int kblocks;
    const int32_t* lengths;     // row b's L = lengths[b], its n = counts[b] (NULL: n) <= n
    const int32_t* counts;
};

// (kvbm_store_block, the block_minifloat store of a block of 16 values: mi355q_attn_dev.h, shared with mi355q_attention_bm.hip)
__global__ __launch_bounds__(256) void kvbm_append_kernel(const QuantArgs ak, const QuantArgs av, const AppendBmArgs a) {
    const int tid = threadIdx.x, D = a.c.D;
    const long long b = blockIdx.y, NTC = a.c.C >> 4, NPC = (a.c.C + 31) >> 5;
    long long L, n = a.n;
    if (!append_row(a, b, L, n)) return;
    const long long t0 = L >> 4, t1 = (L + n - 1) >> 4;
    if ((int)blockIdx.x < a.kblocks) {
        // K: thread (tile, d) walks the 16 keys of its block: staged rows in front of L, new rows, zeros behind L + n
        const int per = 256 / D, sub = tid / D, d = tid - sub * D;
        const long long t = t0 + (long long)blockIdx.x * per + sub;
        if (sub >= per || t > t1 || t >= NTC) return;          // (keys behind the capacity are dropped, whatever the host vouched for)
        float* __restrict__ stg = a.c.stage + b * 16 * D + d;
        float x[16];
        float bmax = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const long long key = t * 16 + e;
            float val = 0.f;
            if (key >= L && key < L + n) val = a.k[b * a.ksb + (key - L) * a.kst + d];
            else if (key < L) val = stg[e * D];
            x[e] = val;
            bmax = fmaxf(bmax, fabsf(val));
        }
        // the open tile's rows for the next append, when the tile that reads staged rows is the one that writes them; an append that
        // runs into a later tile leaves them to kv_stage_kernel, behind this launch (mi355q_decode.hip)
        if (t0 == t1) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const long long key = t * 16 + e;
                if (key >= L && key < L + n) stg[e * D] = x[e];
            }
        }
        const int c = d >> 5, g = (d >> 3) & 3, j = d & 7;
        kvbm_store_block(a.c.kq + ((b * NTC + t) * (D >> 5) + c) * 512 + 16 * g * 8 + j, x, bmax, ak);
    } else {
        // V: thread (new key, 16-d block) quantises one block
        const int DT = D >> 4;
        const long long item = ((long long)blockIdx.x - a.kblocks) * 256 + tid;
        if (item >= a.n * DT) return;
        const long long kl = item / DT, key = L + kl;
        const int dt = (int)(item - kl * DT);
        if (kl >= n || key >= a.c.C) return;                   // (input rows behind the row's count are padding: never read)
        float x[16];
        const float bmax = append_v_block(a, b, kl, dt, x);
        const long long s = key >> 5;
        const int h = (int)(key >> 4) & 1, g = (int)(key & 15) >> 2, j = 4 * h + (int)(key & 3);
        kvbm_store_block(a.c.vq + ((b * NPC + s) * DT + dt) * 512 + 16 * g * 8 + j, x, bmax, av);
    }
}

int launch_kvbm_append(const KvCache& c, const QuantArgs& ak, const QuantArgs& av, const float* k, const float* v, long long ksb, long long kst,
                       long long vsb, long long vst, const int32_t* lengths, const int32_t* counts, long long n, hipStream_t st) {
    if (!lengths) return MI355Q_E_BADARG;                   // (no uniform launch)
    AppendBmArgs a{};
    a.c = c; a.k = k; a.v = v;
    a.ksb = ksb; a.kst = kst; a.vsb = vsb; a.vst = vst;
    a.n = n; a.lengths = lengths; a.counts = counts;
    dim3 grid;
    if (const int rc = append_ragged_grid(c.B, c.D, n, a.kblocks, grid)) return rc;
    hipLaunchKernelGGL(kvbm_append_kernel, grid, dim3(256), 0, st, ak, av, a);
    launch_kv_stage_ragged(c, k, ksb, kst, lengths, counts, n, st);
    return (int)hipGetLastError();
}

// ---- decode ---------------------------------------------------------------------------------------------------------------
template <int DC, bool GQ>
__global__ __launch_bounds__(256) void decodebm_scores_kernel(const QuantArgs aq, const DecodeArgs g) {
    __shared__ float sm_[4][64], sl_[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, lg = lane >> 4;
    const long long b = blockIdx.y, s = blockIdx.x, cb = dec_cache_row<GQ>(g, b);   // b: launch row (workspace), cb: cache row
    const long long L = dec_length<true>(g, cb), NT = (L + 15) >> 4;
    if (2 * g.pps * s >= NT) {          // a split wholly behind the row's last tile: the empty statistics, no kq read
        dec_stats_empty(g, b, s, tid);
        return;
    }
    long long row, qrow;
    dec_column<GQ>(g, b, c16, row, qrow);
    bf16x8 qf[DC];                      // quantised in registers (whole waves get here: the quantiser's votes see all 64 lanes)
    at_bm_quant_q_frag(qf, g.q + row * g.qsb + qrow * g.qsm, g.q_scale, lg, aq);
    const long long kvis = dec_horizon(g, L, qrow);
    const float scale_inv = g.scale_div != 0.f ? 1.0f / g.scale_div : 0.f;
    const long long t_lo = 2 * g.pps * s, t_hi = min(NT, t_lo + 2 * g.pps);
    const uint16_t* __restrict__ kfb = g.kq + cb * g.NTC * DC * 512 + lane * 8;      // (t < NT <= NTC)
    float* __restrict__ sc = g.scores + b * g.NT * 256 + lane * 4;
    // running (max, sum of exp(x - max)) of this lane's visible scores, re-based when the maximum moves
    float m_run = -INFINITY, l_run = 0.f;
    for (long long t = t_lo + wave; t < t_hi; t += 4) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < DC; ++c)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(kfb + (t * DC + c) * 512), qf[c], acc, 0, 0, 0);
        if (g.scale_div != 0.f) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = at_div(acc[e], g.scale_div, scale_inv);
        }
        *reinterpret_cast<float4*>(sc + t * 256) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        const long long key0 = t * 16 + 4 * lg;
        float tm = -INFINITY;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (key0 + e <= kvis) tm = fmaxf(tm, acc[e]);
        if (tm > m_run) {
            l_run = m_run == -INFINITY ? 0.f : l_run * at_exp_neg(m_run - tm);
            m_run = tm;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (key0 + e <= kvis) l_run += at_exp_neg(acc[e] - m_run);
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

template <int DC, bool GQ>
__global__ __launch_bounds__(256) void decodebm_pv_kernel(const QuantArgs ap, const DecodeArgs g) {
    constexpr int DT = DC * 2;
    __shared__ f32x4 red[4][DT][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, lg = lane >> 4;
    const long long b = blockIdx.y, s = blockIdx.x, cb = dec_cache_row<GQ>(g, b);
    const long long L = dec_length<true>(g, cb), NT = (L + 15) >> 4, NP = (L + 31) >> 5;
    const long long p_lo = g.pps * s, p_hi = min(NP, p_lo + g.pps);
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
    // the row's statistics over all L keys: the S splits in split order (the first split holds key 0, which every query sees: its
    // maximum is finite; a split behind a ragged row's last tile holds (-inf, 0) and is skipped)
    const float* __restrict__ stp = g.stats + (b * g.S * 16 + c16) * 2;
    float row_max = -INFINITY;
    for (int i = 0; i < g.S; ++i) row_max = fmaxf(row_max, stp[i * 32]);
    float row_sum = 0.f;
    for (int i = 0; i < g.S; ++i) {
        const float m = stp[i * 32];
        if (m != -INFINITY) row_sum += stp[i * 32 + 1] * at_exp_neg(m - row_max);
    }
    const float row_inv = 1.0f / row_sum;
    const float half_up = ap.shift * 0.5f, two_dn = ap.inv_shift * 2.0f;
    const uint16_t* __restrict__ vfb = g.vq + cb * g.NPC * DT * 512 + lane * 8;      // (pair < NP <= NPC)
    const float* __restrict__ sc = g.scores + b * g.NT * 256 + lane * 4;
    // o: the quantised probabilities' products, exact sums; ot: those of the pass-through probabilities (<= 1e-8), kept apart from them
    // until one VALU addition behind the loop (at_bm_quant_p_block says why)
    f32x4 o[DT], ot[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = ot[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long long pr_i = p_lo + wave; pr_i < p_hi; pr_i += 4) {
        uint4 vb[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) vb[dt] = *reinterpret_cast<const uint4*>(vfb + (pr_i * DT + dt) * 512);
        float pq[8], pt[8];
        bool tiny = false;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const long long t = 2 * pr_i + h;                  // (uniform over the wave; the last pair's second tile may not exist)
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < NT) x = *reinterpret_cast<const float4*>(sc + t * 256);
            const float xs[4] = {x.x, x.y, x.z, x.w};
            const long long key0 = t * 16 + 4 * lg;
            float pr[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) pr[e] = (t < NT && key0 + e <= kvis) ? at_div(at_exp_neg(xs[e] - row_max), row_sum, row_inv) : 0.f;
            tiny |= at_bm_quant_p_block(pr, pq + 4 * h, pt + 4 * h, half_up, two_dn, ap);
        }
        const bf16x8 pf = at_pack_p(pq);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vb[dt]), pf, o[dt], 0, 0, 0);
        if (__any(tiny)) {              // (wave-uniform: the pair is walked by whole waves)
            const bf16x8 ptf = at_pack_p(pt);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
                ot[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vb[dt]), ptf, ot[dt], 0, 0, 0);
        }
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] += ot[dt];
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

// launch_bfp_attention_decode's ragged, unwindowed, unpaged forms: decode_args_fill with span = L
int launch_bm_attention_decode(const QuantArgs& aq, const QuantArgs& ap, const KvCache& c, const float* q, float* out, void* workspace,
                               long long M, long long L, int causal, float q_scale, float scale_div, const long long* strides, int splits,
                               hipStream_t st, const int32_t* lengths, int G) {
    if (!lengths) return MI355Q_E_BADARG;                   // (no uniform launch)
    DecodeArgs g{};
    long long rows;
    if (const int rc = decode_args_fill(g, c.B, c.C, c.D, M, L, L, G, splits, strides, workspace, nullptr, rows)) return rc;
    g.q = q; g.kq = c.kq; g.vq = c.vq; g.out = out; g.lengths = lengths;
    g.causal = causal; g.q_scale = q_scale; g.scale_div = scale_div;
    const dim3 grid((unsigned)g.S, (unsigned)rows);
#define MI355Q_DECODEBM_GO2(DC_, GQ_)                                                                           \
    hipLaunchKernelGGL((decodebm_scores_kernel<DC_, GQ_>), grid, dim3(256), 0, st, aq, g);                      \
    hipLaunchKernelGGL((decodebm_pv_kernel<DC_, GQ_>), grid, dim3(256), 0, st, ap, g);
#define MI355Q_DECODEBM_GO(DC_) \
    if (G) { MI355Q_DECODEBM_GO2(DC_, true) } else { MI355Q_DECODEBM_GO2(DC_, false) }
    switch (c.D / 32) {
        case 1: MI355Q_DECODEBM_GO(1); break;
        case 2: MI355Q_DECODEBM_GO(2); break;
        case 3: MI355Q_DECODEBM_GO(3); break;
        case 4: MI355Q_DECODEBM_GO(4); break;
        default: return MI355Q_E_UNSUPPORTED;
    }
#undef MI355Q_DECODEBM_GO
#undef MI355Q_DECODEBM_GO2
    launch_decode_sum(g, G != 0, rows, st);
    return (int)hipGetLastError();
}

}  // namespace mi355q
