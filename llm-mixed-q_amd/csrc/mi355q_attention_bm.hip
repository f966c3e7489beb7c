// mi355q_attention_bm.hip -- the reference's quantised attention core as ONE pass for a layer whose two products are block_minifloat:
//
//     scores = bmm_0(Qa(q), Qb(k^T))            quantized_functions/matmul.py:199-249 (block_minifloat), callers
//     scores = scores / scale                   modeling_llama.py:318-322 (OPT scales q before the product instead: q_scale)
//     scores = max(scores + causal, finfo.min)  modeling_opt.py:262-276, modeling_llama.py:323-329
//     probs  = softmax(scores, -1)              fp32
//     out    = bmm_1(Qc(probs), Qd(v))          modeling_opt.py:312, modeling_llama.py:341
//
// Structure: bfp_attention_stream_kernel<DC, false> of mi355q_attention.hip with the hazards closed as bfp_attention_extend_kernel
// (mi355q_extend.hip) closes them.  A workgroup is 64 queries (4 waves x 16: the 16 columns of v_mfma_f32_16x16x32_bf16) that walk the key
// tiles together, 32 keys a step; the step's K pieces (and, second time round, the V pieces of the key pair) come into LDS by LDS-DMA one
// step ahead, two buffers, ONE barrier a step.  Pass 1 keeps a running (maximum, sum of exponentials) per lane over the visible keys; pass 2
// forms the scores again from the same operands (the same bits), turns them into probabilities with the FINAL statistics -- no probability
// is quantised before they are -- quantises per block of 16 keys of a query, multiplies with V.  No scores, no probabilities in memory, any T.
//   out-of-row reads    a K piece is addressed at tile min(t, need - 1), need <= T / 16: never a tile of the next head or behind the
//                       workspace; the clamped piece's scores are discarded (t >= need -> -inf).  V pairs: st < ceil(need / 2) <= ceil(T / 32).
//   divergent barriers  the step count is ONE scalar from the workgroup's last real query; a wave whose 16 queries lie behind M computes
//                       the last real query again and stores nothing (a launch has no workgroup wholly behind M).
//   missing V pieces    the last pair's second tile may not exist: its probabilities are exact zeros, and the pack launch below wrote
//                       zeros there.
// Arithmetic: that of decodebm_scores_kernel / decodebm_pv_kernel (mi355q_kvbm.hip), not of the block_fp pass -- Q through
// at_bm_quant_q_frag (q_scale in front of the quantiser), P through at_bm_quant_p_block, and the TWO accumulators of phase B there: `o` for
// the quantised probabilities' products (exact sums), `ot` for those of the pass-through probabilities (<= 1e-8; their MFMAs issued only
// when some lane of the wave holds one), added once on the VALU behind the loop (mi355q_attn_dev.h at at_bm_quant_p_block says why: one
// accumulator is how an output ends up one ulp off, which a coarse quantiser behind the attention turns into a whole step).
// The quantisers vote with __any (the rare table walks), so whole waves reach them: they sit outside every per-lane condition.
// Not here: the resident-score form, an additive mask, a key mask, the rotary embedding on load, packed Q fragments, the consumer's operand.
// Token-major output is the out strides of the argument struct, nothing else.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mi355q.h"
#include "mi355q_internal.h"
#include "mi355q_quant_dev.h"
#include "mi355q_attn_dev.h"
#include "mi355q_attention_bm.h"

namespace mi355q {

// ---- k, v [B, T, D] -> the fragments a MinifloatKVCache of capacity T holds after appending them at length 0 ------------------------
// The K and V walks of kvbm_append_kernel (mi355q_kvbm.hip) with L = 0, n = T = the capacity and no open tile (T % 16 == 0), through the
// same store (kvbm_store_block): the same bytes.  Chosen over a launch of the append itself: that one wants a staging area, a zeroed
// lengths array and zeroed V storage in the workspace -- a memset and a staging launch a call -- where this is forty lines.
//   K: thread (tile, d) walks the 16 keys of its [1,16] block of k^T.   V: thread (key, 16-d block) takes one block; keys T .. 32 NP - 1
//   (the absent half of the last pair) are stored as zeros.
struct BmPackArgs {
    const float* k;
    const float* v;
    uint16_t* kf;
    uint16_t* vf;
    long long T, NT, NP;
    long long ksb, kst, vsb, vst;
    int D, kblocks;
};

__global__ __launch_bounds__(256) void bm_attn_pack_kv_kernel(const QuantArgs ak, const QuantArgs av, const BmPackArgs a) {
    const int tid = threadIdx.x, D = a.D;
    const long long b = blockIdx.y;
    if ((int)blockIdx.x < a.kblocks) {
        const int per = 256 / D, sub = tid / D, d = tid - sub * D;
        const long long t = (long long)blockIdx.x * per + sub;
        if (sub >= per || t >= a.NT) return;
        const float* __restrict__ kp = a.k + b * a.ksb + t * 16 * a.kst + d;        // (keys 16 t .. 16 t + 15 < T)
        float x[16];
        float bmax = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            x[e] = kp[e * a.kst];
            bmax = fmaxf(bmax, fabsf(x[e]));
        }
        const int c = d >> 5, g = (d >> 3) & 3, j = d & 7;
        kvbm_store_block(a.kf + ((b * a.NT + t) * (D >> 5) + c) * 512 + 16 * g * 8 + j, x, bmax, ak);
    } else {
        const int DT = D >> 4;
        const long long item = ((long long)blockIdx.x - a.kblocks) * 256 + tid;
        if (item >= 32 * a.NP * DT) return;
        const long long key = item / DT;
        const int dt = (int)(item - key * DT);
        float x[16];
        float bmax = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
            if (key < a.T) f = *reinterpret_cast<const float4*>(a.v + b * a.vsb + key * a.vst + dt * 16 + 4 * i);
            x[4 * i] = f.x; x[4 * i + 1] = f.y; x[4 * i + 2] = f.z; x[4 * i + 3] = f.w;
            bmax = fmaxf(bmax, fmaxf(fmaxf(fabsf(f.x), fabsf(f.y)), fmaxf(fabsf(f.z), fabsf(f.w))));
        }
        const long long s = key >> 5;
        const int h = (int)(key >> 4) & 1, g = (int)(key & 15) >> 2, j = 4 * h + (int)(key & 3);
        kvbm_store_block(a.vf + ((b * a.NP + s) * DT + dt) * 512 + 16 * g * 8 + j, x, bmax, av);
    }
}

// ---- the attention pass -------------------------------------------------------------------------------------------------------------
struct BmAttnArgs {
    const float* q;
    const uint16_t* kf;
    const uint16_t* vf;
    float* out;
    long long M, T, NT, NP;
    long long causal_off;     // >= 0: query i sees keys 0 .. i + causal_off; < 0: no causal rule
    float q_scale, scale_div; // 0: none
    long long qsb, qsm;       // element strides of q's batch (head) and row
    long long osb, osm;       // ... of out's
    int nxb, nb;              // query blocks of 64 per head, heads: the work items of a launch
};

template <int DC>
__global__ __launch_bounds__(256) void bm_attention_stream_kernel(const QuantArgs aq, const QuantArgs ap, const BmAttnArgs g) {
    constexpr int DT = DC * 2, KSTEP = 2 * DC * 1024, VSTEP = DT * 1024, STEP = KSTEP + VSTEP;      // bytes per 32 keys
    using gptr_t = const __attribute__((address_space(1))) void*;
    using lptr_t = __attribute__((address_space(3))) void*;
    __shared__ __attribute__((aligned(16))) unsigned char stage[2][STEP];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, lg = lane >> 4;
    // work items (query block, head) in one grid dimension, the heaviest query block of every head first (causal: the last one)
    const int xrank = (int)blockIdx.x / g.nb;
    const long long b = (int)blockIdx.x - xrank * g.nb;
    const long long wg0 = (long long)(g.causal_off >= 0 ? g.nxb - 1 - xrank : xrank) * 64;        // (< M: nxb = ceil(M / 64))
    const long long m0 = wg0 + 16 * wave;
    const long long qrow = min(m0 + c16, g.M - 1);          // (a lane behind M repeats the last real query; it stores nothing)
    bf16x8 qf[DC];                                          // quantised in registers (whole waves: the quantiser's votes see all 64 lanes)
    at_bm_quant_q_frag(qf, g.q + b * g.qsb + qrow * g.qsm, g.q_scale, lg, aq);
    // this lane's horizon, and the tiles the WORKGROUP walks: up to the horizon of its last real query (scalar; 1 <= need <= NT)
    const long long kvis = g.causal_off >= 0 ? qrow + g.causal_off : g.T - 1;
    const long long need = min(g.NT, (g.causal_off >= 0 ? min(wg0 + 63, g.M - 1) + g.causal_off : g.T - 1) / 16 + 1);
    const int nsteps = (int)((need + 1) / 2);
    const unsigned char* __restrict__ kfb = reinterpret_cast<const unsigned char*>(g.kf) + b * g.NT * DC * 1024 + lane * 16;
    const unsigned char* __restrict__ vfb = reinterpret_cast<const unsigned char*>(g.vf) + b * g.NP * DT * 1024 + lane * 16;
    const float scale_inv = g.scale_div != 0.f ? 1.0f / g.scale_div : 0.f;

    // LDS-DMA of one step: the K pieces of tiles 2 st, 2 st + 1 (DC KiB each) and, when with_v, the V pieces of pair st (DT KiB);
    // piece p by wave p % 4.  An odd tile count: the last step's second tile is tile need - 1 once more, never one behind the head's.
    auto dma = [&](int st, int buf, bool with_v) {
#pragma unroll
        for (int p = 0; p < 2 * DC; ++p)
            if ((p & 3) == wave) {
                const long long t = min(2ll * st + p / DC, need - 1);
                __builtin_amdgcn_global_load_lds((gptr_t)(kfb + (t * DC + p % DC) * 1024), (lptr_t)(&stage[buf][p * 1024]), 16, 0, 0);
            }
        if (with_v) {
#pragma unroll
            for (int p = 0; p < DT; ++p)
                if ((p & 3) == wave)
                    __builtin_amdgcn_global_load_lds((gptr_t)(vfb + ((long long)st * DT + p) * 1024), (lptr_t)(&stage[buf][KSTEP + p * 1024]), 16, 0, 0);
        }
    };
    // scores of the step's two tiles for this lane's query: sv[h][e] <-> key 32 st + 16 h + 4 lg + e; -inf: not a visible key (behind the
    // horizon, or the missing second tile of the last pair)
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
                sv[h][e] = (t < need && key0 + e <= kvis) ? x : -INFINITY;
            }
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
    float row_max, row_sum, row_inv;                        // (every query sees key 0: the row maximum is finite)
    at_softmax_finish(m_run, l_run, row_max, row_sum, row_inv);
    __syncthreads();                                        // (every wave is out of the last step's buffer)

    // ---- pass 2: the scores again, probabilities from the final statistics, quantised, times V
    // o: the quantised probabilities' products, exact sums; ot: those of the pass-through probabilities (<= 1e-8), kept apart from them
    // until one VALU addition behind the loop (at_bm_quant_p_block says why)
    f32x4 o[DT], ot[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = ot[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float half_up = ap.shift * 0.5f, two_dn = ap.inv_shift * 2.0f;
    dma(0, 0, true);
    for (int st = 0; st < nsteps; ++st) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (st + 1 < nsteps) dma(st + 1, (st + 1) & 1, true);
        f32x4 sv[2];
        scores(st, st & 1, sv);
        float pq[8], pt[8];
        bool tiny = false;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float pr[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) pr[e] = sv[h][e] == -INFINITY ? 0.f : at_div(at_exp_neg(sv[h][e] - row_max), row_sum, row_inv);
            tiny |= at_bm_quant_p_block(pr, pq + 4 * h, pt + 4 * h, half_up, two_dn, ap);
        }
        const bf16x8 pf = at_pack_p(pq);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const uint4 vv = *reinterpret_cast<const uint4*>(&stage[st & 1][KSTEP + dt * 1024 + lane * 16]);
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vv), pf, o[dt], 0, 0, 0);
        }
        if (__any(tiny)) {                                  // (wave-uniform: whole waves walk the step)
            const bf16x8 ptf = at_pack_p(pt);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const uint4 vv = *reinterpret_cast<const uint4*>(&stage[st & 1][KSTEP + dt * 1024 + lane * 16]);
                ot[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vv), ptf, ot[dt], 0, 0, 0);
            }
        }
    }
    if (m0 + c16 < g.M) {
        float* __restrict__ op = g.out + b * g.osb + (m0 + c16) * g.osm + 4 * lg;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const f32x4 r = o[dt] + ot[dt];
            *reinterpret_cast<float4*>(op + 16 * dt) = make_float4(r[0], r[1], r[2], r[3]);
        }
    }
}

size_t bm_attention_workspace_bytes(long long B, long long T, long long D) {
    const long long NT = (T + 15) / 16, NP = (T + 31) / 32;
    return (size_t)B * (size_t)(NT * (D / 32) * 1024 + NP * (D / 16) * 1024) + 256;
}

int launch_bm_attention(const QuantArgs& aq, const QuantArgs& ak, const QuantArgs& ap, const QuantArgs& av, const float* q, const float* k,
                        const float* v, float* out, void* workspace, long long B, long long M, long long T, long long D,
                        long long causal_off, float q_scale, float scale_div, const long long* strides, hipStream_t st) {
    if (T % 16 != 0 || T < 16 || (D != 32 && D != 64 && D != 96 && D != 128)) return MI355Q_E_UNSUPPORTED;
    if (B < 1 || M < 1 || B > 65535) return MI355Q_E_BADARG;
    const long long NT = T / 16, NP = (T + 31) / 32, nxb = (M + 63) / 64;
    const int per = 256 / (int)D, DT = (int)D / 16;
    const long long kblocks = (NT + per - 1) / per, vblocks = (32 * NP * DT + 255) / 256;
    if (B * nxb > 0x7FFFFFFFLL || kblocks + vblocks > 0x7FFFFFFFLL) return MI355Q_E_UNSUPPORTED;
    BmPackArgs p{};
    p.k = k; p.v = v;
    p.kf = static_cast<uint16_t*>(workspace);
    p.vf = p.kf + (size_t)B * NT * (D / 32) * 512;
    p.T = T; p.NT = NT; p.NP = NP;
    p.ksb = strides ? strides[2] : T * D; p.kst = strides ? strides[3] : D;
    p.vsb = strides ? strides[4] : T * D; p.vst = strides ? strides[5] : D;
    p.D = (int)D; p.kblocks = (int)kblocks;
    hipLaunchKernelGGL(bm_attn_pack_kv_kernel, dim3((unsigned)(kblocks + vblocks), (unsigned)B), dim3(256), 0, st, ak, av, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    BmAttnArgs g{};
    g.q = q; g.kf = p.kf; g.vf = p.vf; g.out = out;
    g.M = M; g.T = T; g.NT = NT; g.NP = NP;
    g.causal_off = causal_off; g.q_scale = q_scale; g.scale_div = scale_div;
    g.qsb = strides ? strides[0] : M * D; g.qsm = strides ? strides[1] : D;
    g.osb = strides ? strides[6] : M * D; g.osm = strides ? strides[7] : D;
    g.nxb = (int)nxb; g.nb = (int)B;
    const dim3 grid((unsigned)(B * nxb));
    switch (D / 32) {
        case 1: hipLaunchKernelGGL(bm_attention_stream_kernel<1>, grid, dim3(256), 0, st, aq, ap, g); break;
        case 2: hipLaunchKernelGGL(bm_attention_stream_kernel<2>, grid, dim3(256), 0, st, aq, ap, g); break;
        case 3: hipLaunchKernelGGL(bm_attention_stream_kernel<3>, grid, dim3(256), 0, st, aq, ap, g); break;
        default: hipLaunchKernelGGL(bm_attention_stream_kernel<4>, grid, dim3(256), 0, st, aq, ap, g); break;
    }
    return (int)hipGetLastError();
}

}  // namespace mi355q
