// mi355q_attention_padded.hip -- the attention pass of mi355q_attention.hip for PADDED batches: a per-sequence key mask [B / heads, T]
// (non-zero = a real key) in place of the additive [M, T] mask that every batch element shares.
//
//     w(i, j) = max(s(i, j) + causal(i, j) + (key_mask[b / heads][j] ? 0 : finfo.min), finfo.min)      p = softmax(w, -1)
//
// which is modeling_opt.py:262-276 / modeling_llama.py:323-329 with HF's expanded [B, 1, T_q, T_k] mask.  Pad keys stay in every operand
// and in every quantiser block -- K^T, V and P are quantised over ALL keys by the same pack launch (launch_attention_pack_kv) and the
// same P quantiser -- only the softmax masks them.  The two kernels are bfp_attention_kernel / bfp_attention_stream_kernel with the
// key mask's four values of a lane riding where the additive mask's rode (one 16-byte load per 16 x 16 score tile, T int32 a sequence:
// no [T, T] tensor is read), so this file is a MIRROR SITE of those two as mi355q_sink.hip is of the windowed kernels: a change to a loop
// there is made here as well.  Left out of this form: the rotary embedding on load, the consumer's operand as the output, packed Q
// fragments (q_scale is applied where the kernels quantise q: one fp32 multiply, the bits of the pack launch's).
//
// The fully masked query.  A query whose every visible key is masked -- a left-padded sequence's pad queries under the causal rule --
// has w == finfo.min over its WHOLE row, the keys above its causal horizon included (finfo.min + finfo.min clamps to finfo.min), so
// p = 1 / T for every key: the reference's values, and the next layer's pad keys.  The unpadded kernels leave their loops at the causal
// horizon of a workgroup's last query; here they must not for such a query.  first[s] = the index of sequence s's first real key
// (T: none), made on the device by attn_first_key_kernel in front (no host sync).  Causal query i is fully masked  <=>  first > i + off,
// and the fully masked queries of a sequence are a PREFIX of its queries, so a set of consecutive queries holds one  <=>  its first
// query is one:
//   resident   the 16-query group of waves (grp) walks all NT tiles  <=>  first > m0 + off, m0 the group's first query.  first comes
//              through readfirstlane and m0 from the wave index: a scalar per wave.  The kernel's barriers all lie OUTSIDE the tile
//              loops (three for the statistics, one for the output sum), so two groups of a workgroup may walk different numbers of
//              tiles, as they already do under the causal rule (need is per group there).
//   streaming  one barrier a 32-key step, inside both loops: the decision is the WORKGROUP's, first > wg0 + off with wg0 the first of
//              its 64 queries -- nsteps is the same scalar in all four waves, every wave reaches every barrier equally often (the
//              divergent-barrier hazard of mi355q_extend.hip's comment).
// In a group that walks every tile, a query that does see a real key gets finfo.min above its horizon and exp(finfo.min - max) = 0
// there: the exact zeros the skipped tiles stand for.  Non-causal launches walk every tile anyway; a sequence with no real key
// (first = T) gives every row uniform, causal or not.
// Bounds: a mask load is at keys 16 t + 4 lg .. + 3 with t <= need - 1 <= NT - 1, inside row b / heads < B / heads of key_mask;
// K / V fragment reads are the unpadded kernels' with need <= NT.  An all-ones mask adds 0.0f to every score and walks the same
// tiles: the unpadded kernels' bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mi355q.h"
#include "mi355q_internal.h"
#include "mi355q_quant_dev.h"
#include "mi355q_attn_dev.h"

namespace mi355q {

constexpr int PAD_MAX_T = 2048, PAD_MAX_D = 128;       // (AT_MAX_T, AT_MAX_D of mi355q_attention.hip)

struct PadArgs {
    const float* q;
    const uint16_t* kf;
    const uint16_t* vf;
    const int* key_mask;      // [nb / heads, T], non-zero = a real key
    const int* first;         // [nb / heads]: index of the first real key, T when there is none
    float* out;
    long long M, T, NT, NPAIR;
    long long causal_off;     // >= 0: query i sees keys 0 .. i + causal_off; < 0: no causal rule
    float scale_div;          // 0: none
    float q_scale;            // 0: none
    long long qsb, qsm;       // element strides of q's batch (head) and row
    long long osb, osm;       // ... of out's
    int nxb, nb;              // query blocks per head, heads x sequences: the work items of a launch
    int heads;
};

// first[s] = min { j : key_mask[s][j] != 0 }, T if there is none.  One workgroup a sequence.
__global__ __launch_bounds__(256) void attn_first_key_kernel(const int* __restrict__ key_mask, int* __restrict__ first, int T) {
    __shared__ int best;
    const int* __restrict__ row = key_mask + (long long)blockIdx.x * T;
    if (threadIdx.x == 0) best = T;
    __syncthreads();
    int mine = T;
    for (int j = threadIdx.x; j < T; j += 256)
        if (row[j] != 0) { mine = j; break; }
    if (mine < T) atomicMin(&best, mine);
    __syncthreads();
    if (threadIdx.x == 0) first[blockIdx.x] = best;
}

static __device__ __forceinline__ float4 pad_add(const int4 km) {
    constexpr float FMIN = -3.4028234663852886e38f;
    return make_float4(km.x ? 0.f : FMIN, km.y ? 0.f : FMIN, km.z ? 0.f : FMIN, km.w ? 0.f : FMIN);
}

// ---- bfp_attention_kernel<NTW, DC, QG, true, KW> with the key mask ---------------------------------------------------------------
template <int NTW, int DC, int QG, int KW>
__global__ __launch_bounds__(64 * KW * QG) void bfp_attention_padded_kernel(const QuantArgs aq, const QuantArgs ap, const PadArgs g) {
    constexpr int DT = DC * 2;
    constexpr float FMIN = -3.4028234663852886e38f;
    __shared__ float stat_[QG][KW][16];
    __shared__ f32x4 red_[QG][KW][DT][64];
    const int tid = threadIdx.x, lane = tid & 63, wave_all = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave = wave_all % KW, grp = wave_all / KW;
    float (&stat)[KW][16] = stat_[grp];
    f32x4 (&red)[KW][DT][64] = red_[grp];
    const int c16 = lane & 15, lg = lane >> 4;
    // (work items (query block, head) in one grid dimension, the heaviest query block of every head first: mi355q_attention.hip)
    const int item = (int)blockIdx.x, xrank = item / g.nb;
    const long long b = item - xrank * g.nb, m0 = ((long long)(g.causal_off >= 0 ? g.nxb - 1 - xrank : xrank) * QG + grp) * 16;
    const long long qrow = min(m0 + c16, g.M - 1);
    const long long seq = b / g.heads;
    const long long first = __builtin_amdgcn_readfirstlane(g.first[seq]);

    bf16x8 qf[DC];
    at_quant_q_frag(qf, g.q + b * g.qsb + qrow * g.qsm, g.q_scale, lg, aq, at_block_exponent_mem);
    // tiles this query group needs: up to the horizon of its last query -- or all of them, when its first query (and with it a prefix
    // of its queries) sees no real key: see "the fully masked query" at the top
    const long long kvis = g.causal_off >= 0 ? qrow + g.causal_off : g.T - 1;           // this lane's query
    long long need = g.NT;
    if (g.causal_off >= 0 && first <= m0 + g.causal_off) need = min(g.NT, (min(m0 + 15, g.M - 1) + g.causal_off) / 16 + 1);
    const uint16_t* __restrict__ kfb = g.kf + b * g.NT * DC * 512;
    const float scale_inv = g.scale_div != 0.f ? 1.0f / g.scale_div : 0.f;
    const int* __restrict__ mrow = g.key_mask + seq * g.T + 4 * lg;

    constexpr int G = DC == 1 ? 8 : (DC == 2 ? ((KW == 8) ? 2 : 4) : 2), NG = NTW / G;
    f32x4 acc[NTW];
    float mx = -INFINITY;
    const long long tlast = need - 1;
    uint4 kb[2][G][DC];
    int4 mb[2][G];                                         // (the key mask's values ride with the K fragments)
    const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(kfb), 0, (int)(need * DC * 1024), 0x00020000);
    auto load_group = [&](int gi, uint4 (&dst)[G][DC], int4 (&mdst)[G]) {
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const int tu = KW * (gi * G + j) + wave;
            const long long t = min((long long)tu, tlast);
#pragma unroll
            for (int c = 0; c < DC; ++c)
                dst[j][c] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(krs, (tu * DC + c) * 1024 + lane * 16, 0, 0));
            mdst[j] = *reinterpret_cast<const int4*>(mrow + t * 16);
        }
    };
    load_group(0, kb[0], mb[0]);
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) {
        if (gi > 0 && KW * gi * G >= need) break;          // (uniform: every tile from here on lies behind the horizon)
        if (gi + 1 < NG) load_group(gi + 1, kb[(gi + 1) & 1], mb[(gi + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const int i = gi * G + j;
            const long long t = KW * i + wave;
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < DC; ++c)
                s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kb[gi & 1][j][c]), qf[c], s, 0, 0, 0);
            if (t < need) {                                // (uniform over the wave)
                const long long key0 = t * 16 + 4 * lg;
                if (g.scale_div != 0.f) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[e] = at_div(s[e], g.scale_div, scale_inv);
                }
                const float4 mk = pad_add(mb[gi & 1][j]);
                s[0] = fmaxf(s[0] + mk.x, FMIN); s[1] = fmaxf(s[1] + mk.y, FMIN);
                s[2] = fmaxf(s[2] + mk.z, FMIN); s[3] = fmaxf(s[3] + mk.w, FMIN);
                if (t * 16 + 15 > m0 + g.causal_off && g.causal_off >= 0) {      // (uniform: a tile on or above the diagonal)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (key0 + e > kvis) s[e] = FMIN;
                }
                mx = fmaxf(mx, fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3])));
            }
            acc[i] = s;
        }
    }
    mx = at_max4(mx);
    if (lg == 0) stat[wave][c16] = mx;
    __syncthreads();
    float row_max = stat[0][c16];
#pragma unroll
    for (int w = 1; w < KW; ++w) row_max = fmaxf(row_max, stat[w][c16]);
    __syncthreads();
    // ---- exponentials in place, row sum
    float sm = 0.f;
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        if (KW * i + wave < need) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ex = at_exp_neg(acc[i][e] - row_max);
                acc[i][e] = ex;
                sm += ex;
            }
        }
    }
    sm = at_sum4(sm);
    if (lg == 0) stat[wave][c16] = sm;
    __syncthreads();
    float row_sum = (stat[0][c16] + stat[1][c16]) + (stat[2][c16] + stat[3][c16]);
    if (KW == 8) row_sum += (stat[4][c16] + stat[5][c16]) + (stat[6][c16] + stat[7][c16]);
    const float row_inv = 1.0f / row_sum;

    // ---- probabilities, quantised per tile row (one [1,16] block = the 4 lanes c16 + 16 g'), times V
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int mbp = (int)__builtin_log2f(ap.shift);
    const uint16_t* __restrict__ vfb = g.vf + b * DT * g.NPAIR * 512;
    const long long s_full = tlast / (2 * KW), r_last = tlast - 2 * KW * s_full;
    const long long pairs_needed = min((long long)g.NPAIR, KW * s_full + min((long long)KW - 1, r_last) + 1);
    const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(vfb), 0, (int)(pairs_needed * DT * 1024), 0x00020000);
    uint4 vb[2][DT];
    auto load_pair = [&](int sp, uint4 (&dst)[DT]) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
            dst[dt] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(vrs, ((KW * sp + wave) * DT + dt) * 1024 + lane * 16, 0, 0));
    };
    load_pair(0, vb[0]);
#pragma unroll
    for (int s = 0; s < NTW / 2; ++s) {
        if (s > 0 && KW * 2 * s >= need) break;            // (uniform)
        if (s + 1 < NTW / 2) load_pair(s + 1, vb[(s + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        if (KW * (2 * s) + wave < need) {                  // (uniform; tiles are needed in order)
            float pq[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int i = 2 * s + h;
                float pr[4];
                float bmax = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // (a pair's second tile may lie behind the horizon: exact zeros, see mi355q_attention.hip)
                    pr[e] = at_div(acc[i][e], row_sum, row_inv);
                    bmax = fmaxf(bmax, pr[e]);
                }
                bmax = at_max4(bmax);
                const int p = at_block_exponent_mem(bmax, ap);
                const float sc_up = __builtin_ldexpf(1.0f, mbp - p), sc_dn = __builtin_ldexpf(1.0f, p - mbp), eps_up = EPS9 * sc_up;
#pragma unroll
                for (int e = 0; e < 4; ++e) pq[4 * h + e] = at_quant_pos(pr[e], sc_up, eps_up, sc_dn, ap.mant_max);
            }
            const bf16x8 pf = at_pack_p(pq);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vb[s & 1][dt]), pf, o[dt], 0, 0, 0);
        }
    }
    // ---- sum the waves' partial outputs in wave order, store
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) red[wave][dt][lane] = o[dt];
    __syncthreads();
    const long long m = m0 + c16;
    for (int dt = wave; dt < DT; dt += KW) {
        f32x4 sum = red[0][dt][lane];
#pragma unroll
        for (int w = 1; w < KW; ++w) sum += red[w][dt][lane];
        if (m < g.M)
            *reinterpret_cast<float4*>(g.out + b * g.osb + m * g.osm + 16 * dt + 4 * lg) = make_float4(sum[0], sum[1], sum[2], sum[3]);
    }
}

// ---- bfp_attention_stream_kernel<DC, true> with the key mask -----------------------------------------------------------------------
template <int DC>
__global__ __launch_bounds__(256) void bfp_attention_padded_stream_kernel(const QuantArgs aq, const QuantArgs ap, const PadArgs g) {
    constexpr int DT = DC * 2, KSTEP = 2 * DC * 1024, VSTEP = DT * 1024, STEP = KSTEP + VSTEP;      // bytes per 32 keys
    constexpr float FMIN = -3.4028234663852886e38f;
    using gptr_t = const __attribute__((address_space(1))) void*;
    using lptr_t = __attribute__((address_space(3))) void*;
    __shared__ Lut lut;
    __shared__ __attribute__((aligned(16))) unsigned char stage[2][STEP];
    load_lut<FMT_BFP, true>(lut);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, lg = lane >> 4;
    const int xrank = (int)blockIdx.x / g.nb;
    const long long b = (int)blockIdx.x - xrank * g.nb;
    const long long wg0 = (long long)(g.causal_off >= 0 ? g.nxb - 1 - xrank : xrank) * 64;
    const long long m0 = wg0 + 16 * wave;
    const long long qrow = min(m0 + c16, g.M - 1);
    const long long seq = b / g.heads;
    const long long first = __builtin_amdgcn_readfirstlane(g.first[seq]);
    bf16x8 qf[DC];
    at_quant_q_frag(qf, g.q + b * g.qsb + qrow * g.qsm, g.q_scale, lg, aq,
                    [&](float bmax, const QuantArgs& a) { unsigned code; return block_param<FMT_BFP>(bmax != 0.f ? bmax : 1.0f, a, lut, code).p; });
    const long long kvis = g.causal_off >= 0 ? qrow + g.causal_off : g.T - 1;
    // tiles the WORKGROUP walks: up to its last query's horizon, or all of them when its first query sees no real key -- one scalar for
    // the four waves, which meet at a barrier in every step
    long long need = g.NT;
    if (g.causal_off >= 0 && first <= wg0 + g.causal_off) need = min(g.NT, (min(wg0 + 63, g.M - 1) + g.causal_off) / 16 + 1);
    const int nsteps = (int)((need + 1) / 2);
    const unsigned char* __restrict__ kfb = reinterpret_cast<const unsigned char*>(g.kf) + b * g.NT * DC * 1024;
    const unsigned char* __restrict__ vfb = reinterpret_cast<const unsigned char*>(g.vf) + b * g.NPAIR * DT * 1024;
    const int* __restrict__ mrow = g.key_mask + seq * g.T;
    const float scale_inv = g.scale_div != 0.f ? 1.0f / g.scale_div : 0.f;

    // LDS-DMA of one step: K pieces (2 DC KiB, contiguous) and, when with_v, V pieces (DT KiB, contiguous); piece p by wave p % 4
    // (an odd tile count: the last step's second tile reads DC KiB past this batch's K fragments -- the next batch's, or the
    //  V fragments that follow in the workspace; its scores are never used)
    auto dma = [&](int st, int buf, bool with_v) {
#pragma unroll
        for (int p = 0; p < 2 * DC; ++p)
            if ((p & 3) == wave)
                __builtin_amdgcn_global_load_lds((gptr_t)(kfb + (long long)st * KSTEP + p * 1024 + lane * 16),
                                                 (lptr_t)(&stage[buf][p * 1024]), 16, 0, 0);
        if (with_v) {
#pragma unroll
            for (int p = 0; p < DT; ++p)
                if ((p & 3) == wave)
                    __builtin_amdgcn_global_load_lds((gptr_t)(vfb + (long long)st * VSTEP + p * 1024 + lane * 16),
                                                     (lptr_t)(&stage[buf][KSTEP + p * 1024]), 16, 0, 0);
        }
    };
    // scores of the step's two tiles for this lane's query: s[h][e] <-> key 32 st + 16 h + 4 lg + e, masked
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
            if (t < need) {
                if (g.scale_div != 0.f) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[e] = at_div(s[e], g.scale_div, scale_inv);
                }
                const float4 mk = pad_add(*reinterpret_cast<const int4*>(mrow + key0));
                s[0] = fmaxf(s[0] + mk.x, FMIN); s[1] = fmaxf(s[1] + mk.y, FMIN);
                s[2] = fmaxf(s[2] + mk.z, FMIN); s[3] = fmaxf(s[3] + mk.w, FMIN);
                if (g.causal_off >= 0 && t * 16 + 15 > m0 + g.causal_off) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (key0 + e > kvis) s[e] = FMIN;
                }
            } else {
                s = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};       // (not a tile of this product)
            }
            sv[h] = s;
        }
    };

    // ---- pass 1: running maximum and sum of exponentials per lane
    float m_run = -INFINITY, l_run = 0.f;
    dma(0, 0, false);
    for (int st = 0; st < nsteps; ++st) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (st + 1 < nsteps) dma(st + 1, (st + 1) & 1, false);
        f32x4 sv[2];
        scores(st, st & 1, sv);
        at_softmax_step(sv, m_run, l_run);
    }
    float row_max, row_sum, row_inv;
    at_softmax_finish(m_run, l_run, row_max, row_sum, row_inv);
    __syncthreads();                                        // (every wave is out of the last step's buffer)

    // ---- pass 2: the scores again, probabilities, quantised, times V
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int mbp = (int)__builtin_log2f(ap.shift);
    dma(0, 0, true);
    for (int st = 0; st < nsteps; ++st) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (st + 1 < nsteps) dma(st + 1, (st + 1) & 1, true);
        f32x4 sv[2];
        scores(st, st & 1, sv);
        float pq[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float pr[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) pr[e] = sv[h][e] == -INFINITY ? 0.f : at_div(at_exp_neg(sv[h][e] - row_max), row_sum, row_inv);
            at_quant_p_block(pr, pq + 4 * h, mbp, ap, [&](float bmax, const QuantArgs& a) { return at_block_exponent(bmax, a, lut); });
        }
        const bf16x8 pf = at_pack_p(pq);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const uint4 vv = *reinterpret_cast<const uint4*>(&stage[st & 1][KSTEP + dt * 1024 + lane * 16]);
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vv), pf, o[dt], 0, 0, 0);
        }
    }
    const long long m = m0 + c16;
    if (m < g.M) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
            *reinterpret_cast<float4*>(g.out + b * g.osb + m * g.osm + 16 * dt + 4 * lg) = make_float4(o[dt][0], o[dt][1], o[dt][2], o[dt][3]);
    }
}

// The kernel is chosen as launch_bfp_attention chooses it (attention_set_kernel: 0 by size, 1 resident with four key-waves, 2 streaming,
// 3 resident with eight key-waves at head_dim <= 64), so an all-ones mask runs the unpadded launch's twin.
int launch_bfp_attention_padded(const QuantArgs& aq, const QuantArgs& ak, const QuantArgs& ap, const QuantArgs& av, const float* q,
                                const float* k, const float* v, const int* key_mask, long long heads, float* out, void* workspace,
                                long long B, long long M, long long T, long long D, long long causal_off, float q_scale, float scale_div,
                                hipStream_t st, const long long* strides) {
    if (D > PAD_MAX_D || D % 32 != 0 || T % 16 != 0 || M > T || T >= (1ll << 27)) return MI355Q_E_UNSUPPORTED;
    const int which = attention_get_kernel();
    const bool stream = which == 2 || (which == 0 && T > PAD_MAX_T);
    if (!stream && T > PAD_MAX_T) return MI355Q_E_UNSUPPORTED;
    const bool kw8 = !stream && D <= 64 && (which == 3 || (which == 0 && T > 1024));
    const int kw = stream ? 1 : (kw8 ? 8 : 4);
    const long long qsb = strides ? strides[0] : M * D, qsm = strides ? strides[1] : D;
    const long long ksb = strides ? strides[2] : T * D, kst = strides ? strides[3] : D;
    const long long vsb = strides ? strides[4] : T * D, vst = strides ? strides[5] : D;
    const long long osb = strides ? strides[6] : M * D, osm = strides ? strides[7] : D;
    AttnFragments f;
    int rc = launch_attention_pack_kv(ak, av, k, v, workspace, B, T, D, kw, ksb, kst, vsb, vst, st, f);
    if (rc != 0) return rc;
    // (first[B / heads] int32 in the Q fragments' area: B x NT x D / 32 KiB, and no Q fragments are packed here)
    int* first = static_cast<int*>(f.spare);
    hipLaunchKernelGGL(attn_first_key_kernel, dim3((unsigned)(B / heads)), 256, 0, st, key_mask, first, (int)T);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    PadArgs g{q, f.kf, f.vf, key_mask, first, out, M, T, f.NT, f.NPAIR, causal_off, scale_div, q_scale, qsb, qsm, osb, osm, 0, (int)B, (int)heads};
    if (stream) {
        g.nxb = (int)((M + 63) / 64);
        const dim3 sgrid((unsigned)((long long)g.nxb * B));
        switch (D / 32) {
            case 1: hipLaunchKernelGGL(bfp_attention_padded_stream_kernel<1>, sgrid, 256, 0, st, aq, ap, g); break;
            case 2: hipLaunchKernelGGL(bfp_attention_padded_stream_kernel<2>, sgrid, 256, 0, st, aq, ap, g); break;
            case 3: hipLaunchKernelGGL(bfp_attention_padded_stream_kernel<3>, sgrid, 256, 0, st, aq, ap, g); break;
            default: hipLaunchKernelGGL(bfp_attention_padded_stream_kernel<4>, sgrid, 256, 0, st, aq, ap, g); break;
        }
        return (int)hipGetLastError();
    }
#define MI355Q_PAD_GO(QPB_, ...)                                                                                                  \
    {                                                                                                                             \
        g.nxb = (int)((M + (QPB_) - 1) / (QPB_));                                                                                 \
        hipLaunchKernelGGL((bfp_attention_padded_kernel<__VA_ARGS__>), dim3((unsigned)((long long)g.nxb * B)), 512, 0, st, aq, ap, g); \
    }
    if (kw8) {
        if (T <= 1024) { if (D == 32) MI355Q_PAD_GO(16, 8, 1, 1, 8) else MI355Q_PAD_GO(16, 8, 2, 1, 8) }
        else { if (D == 32) MI355Q_PAD_GO(16, 16, 1, 1, 8) else MI355Q_PAD_GO(16, 16, 2, 1, 8) }
        return (int)hipGetLastError();
    }
#define MI355Q_PAD_D(NTW_)                                       \
    switch (D / 32) {                                            \
        case 1: MI355Q_PAD_GO(32, NTW_, 1, 2, 4) break;          \
        case 2: MI355Q_PAD_GO(32, NTW_, 2, 2, 4) break;          \
        case 3: MI355Q_PAD_GO(32, NTW_, 3, 2, 4) break;          \
        default: MI355Q_PAD_GO(32, NTW_, 4, 2, 4) break;         \
    }
    if (T <= 512) { MI355Q_PAD_D(8) }
    else if (T <= 1024) { MI355Q_PAD_D(16) }
    else { MI355Q_PAD_D(32) }
#undef MI355Q_PAD_D
#undef MI355Q_PAD_GO
    return (int)hipGetLastError();
}

}  // namespace mi355q
