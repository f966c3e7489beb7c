// Device helpers shared by the attention kernels (mi355q_attention.hip: prefill; mi355q_decode.hip: KV cache and decode;
// mi355q_extend.hip: chunked prefill behind the cache): the block_fp element / shared-exponent arithmetic of the four quantisers,
// exp and quotient of the softmax, the reductions over the four lanes that hold one query's values of a 16 x 16 MFMA tile -- and,
// built from those, what the decode and extend kernels do with them: the Q fragments (at_quant_q_frag), a block of probabilities
// and the P fragment (at_quant_p_block, at_pack_p) and the running softmax statistics (at_softmax_step, at_softmax_finish).
// The two prefill kernels of mi355q_attention.hip do NOT use these five: they keep the same arithmetic written out (the note at
// "the attention pass" there), so a change to one of the five is made in those two kernels as well.
// ExpFn, where a helper takes one: a callable (float bmax, const QuantArgs&) -> int, the shared exponent of a block with that
// maximum: at_block_exponent_mem in every kernel that uses them today.
#ifndef MI355Q_ATTN_DEV_H
#define MI355Q_ATTN_DEV_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mi355q_internal.h"
#include "mi355q_quant_dev.h"

namespace mi355q {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// element of a block with shared exponent p (mi355q_matmul.hip: quant_elem_fused)
__device__ __forceinline__ float at_quant(float x, int up, int down, float mant_max) {
    const float m = fminf(__builtin_rintf(__builtin_ldexpf(fabsf(x) + EPS9, up)), mant_max);
    const float q = __builtin_copysignf(__builtin_ldexpf(m, down), x);
    return fabsf(x) <= ATOL ? x : q;
}
// the signed integer mantissa at_quant scales back down -- at_quant(x) = ldexp(at_quant_mant(x), down) for |x| > 1e-8 -- and 0 where
// at_quant passes x through (|x| <= 1e-8): what a cache of mantissas and block exponents stores (mi355q_kvp.h)
__device__ __forceinline__ float at_quant_mant(float x, int up, float mant_max) {
    const float m = fminf(__builtin_rintf(__builtin_ldexpf(fabsf(x) + EPS9, up)), mant_max);
    return fabsf(x) <= ATOL ? 0.f : __builtin_copysignf(m, x);
}
__device__ __forceinline__ float at_exp_neg(float x) {
    x = fmaxf(x, -104.0f);
    constexpr float L2E_HI = 1.44269502162933349609375f, L2E_LO = 1.925963033500011e-08f, LN2 = 0.693147182464599609375f;
    const float t = x * L2E_HI;
    float r = __builtin_fmaf(x, L2E_HI, -t);
    r = __builtin_fmaf(x, L2E_LO, r);
    const float p = __builtin_amdgcn_exp2f(t);
    return __builtin_fmaf(p, r * LN2, p);
}
__device__ __forceinline__ float at_div(float e, float l, float inv) {
    const float q = e * inv;
    return __builtin_fmaf(__builtin_fmaf(-q, l, e), inv, q);
}

// max / sum over the four lanes c16, c16 + 16, c16 + 32, c16 + 48 (one query's values of a score tile), on the VALU:
// v_permlane32_swap / v_permlane16_swap of a register with itself leave {own, partner} in the result pair for every lane
// (gfx950; no LDS crossbar round trip as with ds_bpermute, whose latency two waves per SIMD cannot hide)
__device__ __forceinline__ float at_max4(float x) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float at_sum4(float x) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float at_max2_16(float x) {       // lanes l, l ^ 16
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

// shared exponent of a block whose largest magnitude is bmax >= 0 (block_fp.py:72-73): ceil(log2(bmax)) is the fp32
// exponent field, plus one unless bmax is a power of two -- except within 45 ulps above one (fp32 log2 rounds back onto the
// integer there: log2_tables.inc) and for subnormals, where some lane of the wave sends everybody to the table walk.
__device__ __forceinline__ int at_block_exponent(float bmax, const QuantArgs& a, const Lut& lut) {
    const unsigned bits = __float_as_uint(bmax), E = bits >> 23, f = bits & 0x7FFFFFu;
    if (__any((E == 0u && bits != 0u) || (f != 0u && f < MI355Q_LOG2_CEIL_THR_MAX))) {
        unsigned code;
        return block_param<FMT_BFP>(bmax != 0.f ? bmax : 1.0f, a, lut, code).p;
    }
    return clampi((int)E - 127 + (f != 0u ? 1 : 0), a.e_min, a.e_max);
}
// the same with the rare walk reading its threshold from MEMORY (an L2 hit; one block maximum in 2 x 10^5 takes it): a kernel that uses
// only this form need not stage the 277-entry table in LDS in front of its first instruction -- the one-pass attention kernel's
// workgroups live 13-24 us and spent 1 of them on that (tools/dbg/attn_stamps.py)
__device__ __forceinline__ int at_block_exponent_mem(float bmax, const QuantArgs& a) {
    const unsigned bits = __float_as_uint(bmax), E = bits >> 23, f = bits & 0x7FFFFFu;
    if (__any((E == 0u && bits != 0u) || (f != 0u && f < MI355Q_LOG2_CEIL_THR_MAX))) {
        int k; unsigned m;
        split_pos(bmax != 0.f ? bmax : 1.0f, k, m);
        return clampi(k + ((m != 0u && m >= mi355q_log2_ceil_thr[lut_index(k)]) ? 1 : 0), a.e_min, a.e_max);
    }
    return clampi((int)E - 127 + (f != 0u ? 1 : 0), a.e_min, a.e_max);
}
// block_fp element for x >= 0 (probabilities) given the block's scales 2^up, 2^-up (block_fp.py:69-94 with sign = +1)
// (round 6: (x + 1e-9) 2^up as ONE fused multiply-add with eps_up = 1e-9 2^up -- scaling by a power of two commutes with the
//  rounding of the sum, so fma(x, 2^up, 1e-9 2^up) is round(x + 1e-9) 2^up bit for bit; blocks whose scale overflows hold only
//  pass-through values.  One VALU operation of the ~36 per probability.)
__device__ __forceinline__ float at_quant_pos(float x, float sc_up, float eps_up, float sc_dn, float mant_max) {
    const float m = fminf(__builtin_rintf(__builtin_fmaf(x, sc_up, eps_up)), mant_max);
    return x <= ATOL ? x : m * sc_dn;
}

// ---- Q fragments ---------------------------------------------------------------------------------------------------------
// The DC Q fragments of lane (query c16, lg) from its query's fp32 row qp, quantised in registers: chunk c holds d = 32 c + 8 lg .. + 7,
// a [1,16] block is the lanes l, l ^ 16 of a chunk.  q_scale != 0: q is multiplied on the way in.
template <int DC, class ExpFn>
__device__ __forceinline__ void at_quant_q_frag(bf16x8 (&qf)[DC], const float* __restrict__ qp, float q_scale, int lg, const QuantArgs& aq,
                                                ExpFn exponent) {
    const int mb = (int)__builtin_log2f(aq.shift);
#pragma unroll
    for (int c = 0; c < DC; ++c) {
        float4 lo = *reinterpret_cast<const float4*>(qp + 32 * c + 8 * lg);
        float4 hi = *reinterpret_cast<const float4*>(qp + 32 * c + 8 * lg + 4);
        if (q_scale != 0.f) {
            lo.x *= q_scale; lo.y *= q_scale; lo.z *= q_scale; lo.w *= q_scale;
            hi.x *= q_scale; hi.y *= q_scale; hi.z *= q_scale; hi.w *= q_scale;
        }
        float bmax = fmaxf(fmaxf(fmaxf(fabsf(lo.x), fabsf(lo.y)), fmaxf(fabsf(lo.z), fabsf(lo.w))),
                           fmaxf(fmaxf(fabsf(hi.x), fabsf(hi.y)), fmaxf(fabsf(hi.z), fabsf(hi.w))));
        bmax = at_max2_16(bmax);
        const int p = exponent(bmax, aq);
        const int up = mb - p, dn = p - mb;
        uint4 pk;
        pk.x = pack_bf16(at_quant(lo.x, up, dn, aq.mant_max), at_quant(lo.y, up, dn, aq.mant_max));
        pk.y = pack_bf16(at_quant(lo.z, up, dn, aq.mant_max), at_quant(lo.w, up, dn, aq.mant_max));
        pk.z = pack_bf16(at_quant(hi.x, up, dn, aq.mant_max), at_quant(hi.y, up, dn, aq.mant_max));
        pk.w = pack_bf16(at_quant(hi.z, up, dn, aq.mant_max), at_quant(hi.w, up, dn, aq.mant_max));
        qf[c] = __builtin_bit_cast(bf16x8, pk);
    }
}

// ---- probabilities -------------------------------------------------------------------------------------------------------
// One [1,16] block of probabilities = a lane's four values pr of a score tile and those of the three other lanes of its query:
// quantised into pq[0 .. 3].  mbp = log2(ap.shift).
template <class ExpFn>
__device__ __forceinline__ void at_quant_p_block(const float (&pr)[4], float* pq, int mbp, const QuantArgs& ap, ExpFn exponent) {
    float bmax = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) bmax = fmaxf(bmax, pr[e]);
    bmax = at_max4(bmax);
    const int p = exponent(bmax, ap);
    const float sc_up = __builtin_ldexpf(1.0f, mbp - p), sc_dn = __builtin_ldexpf(1.0f, p - mbp), eps_up = EPS9 * sc_up;
#pragma unroll
    for (int e = 0; e < 4; ++e) pq[e] = at_quant_pos(pr[e], sc_up, eps_up, sc_dn, ap.mant_max);
}
// the P fragment of a key pair: the quantised blocks of tiles 2 s (pq[0 .. 3]) and 2 s + 1 (pq[4 .. 7])
__device__ __forceinline__ bf16x8 at_pack_p(const float (&pq)[8]) {
    uint4 pk;
    pk.x = pack_bf16(pq[0], pq[1]); pk.y = pack_bf16(pq[2], pq[3]);
    pk.z = pack_bf16(pq[4], pq[5]); pk.w = pack_bf16(pq[6], pq[7]);
    return __builtin_bit_cast(bf16x8, pk);
}

// ---- block_minifloat (the KV cache of mi355q_kvbm.hip) --------------------------------------------------------------------------
// shared bias of a block whose largest magnitude is bmax >= 0 (block_minifloat.py:57-59): clamp(floor(log2(bmax)), 0, bias_max).
// floor(log2(bmax)) is the fp32 exponent field -- except within a few ulps BELOW a power of two, where torch's fp32 log2 rounds up onto
// the integer (the floor table's band, fraction >= FLOOR_THR_MIN); there, and for subnormals (normalised first; the clamp takes them
// to 0 either way), some lane of the wave sends everybody to the walk, whose threshold comes from MEMORY as in at_block_exponent_mem.
// bmax == 0 gives 0: an all-zero block holds exact zeros under any bias.
__device__ __forceinline__ int at_bm_bias_mem(float bmax, const QuantArgs& a) {
    const unsigned bits = __float_as_uint(bmax), E = bits >> 23, f = bits & 0x7FFFFFu;
    if (__any((E == 0u && bits != 0u) || f >= MI355Q_LOG2_FLOOR_THR_MIN)) {
        int k; unsigned m;
        split_pos(bmax != 0.f ? bmax : 1.0f, k, m);
        return clampi(k + ((k < 128 && m >= mi355q_log2_floor_thr[lut_index(k)]) ? 1 : 0), 0, a.bias_max);
    }
    return clampi((int)E - 127, 0, a.bias_max);
}
// element of a block with shared bias `bias` (minifloat.py:165-194): bm_elem_fused, and -- when ANY lane of the wave holds a value
// whose |x| + 1e-9 lies in the band below a power of two -- the step again as quant_elem<FMT_BM> does it, floor(log2) from the table in
// memory.  Both give the same value outside the band, so the lanes that were not near keep theirs.
__device__ __forceinline__ float at_bm_quant(float x, int bias, int mbits, const QuantArgs& a) {
    bool near = false;
    float q = bm_elem_fused(x, 127 - bias, 127 + a.span - bias, mbits, a.shift, a.mant_max, near);
    if (__any(near)) {
        const float ax = fabsf(x);
        int k; unsigned m;
        split_pos(ax + EPS9, k, m);                                   // (>= 1e-9: normal)
        const int e_min = -bias;
        const int e = clampi(k + ((k < 128 && m >= mi355q_log2_floor_thr[lut_index(k)]) ? 1 : 0), e_min, a.span - bias);
        const float mn = __builtin_ldexpf(ax, -e);
        const bool normal = e != e_min;
        const float sm = normal ? clampf(__builtin_rintf(mn * a.shift - a.shift), 0.f, a.mant_max)
                                : clampf(__builtin_rintf(mn * a.shift * 0.5f), 0.f, a.mant_max);
        const float frac = normal ? (1.0f + sm * a.inv_shift) : (sm * a.inv_shift * 2.0f);
        const float qe = __builtin_copysignf(__builtin_ldexpf(1.0f, e) * frac, x);
        q = ax <= ATOL ? x : qe;
    }
    return q;
}
// kv_store_block of mi355q_decode.hip under block_minifloat: one block of 16 values x with maximum bmax, value e the low halfword of a
// lane's slot, 8 halfwords apart.  An all-zero block (bmax = 0) takes bias 0 and stores zeros: the reference gives it the smallest
// non-zero block maximum of the whole tensor, which no zero can show (|x| <= 1e-8 passes through under any bias).
__device__ __forceinline__ void kvbm_store_block(uint16_t* __restrict__ dst, const float (&x)[16], float bmax, const QuantArgs& a) {
    const int mbits = (int)__builtin_log2f(a.shift);
    const int bias = at_bm_bias_mem(bmax, a);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        // (an input -0.0 becomes +0.0 in the reference's mask arithmetic; a NEGATIVE value whose mantissa rounds to 0 stays -0.0 there --
        //  sign * 2^e * 0 -- unlike block_fp's, so no "+ 0" on the quantised value)
        const float qe = at_bm_quant(x[e], bias, mbits, a);
        const float q = x[e] == 0.f ? 0.f : qe;
        dst[e * 8] = (uint16_t)(pack_bf16(q, 0.f) & 0xFFFFu);
    }
}
// at_quant_q_frag under block_minifloat: the same lanes, loads and block maximum (lanes l, l ^ 16 of a chunk), the block's bias from
// at_bm_bias_mem, the elements through at_bm_quant
template <int DC>
__device__ __forceinline__ void at_bm_quant_q_frag(bf16x8 (&qf)[DC], const float* __restrict__ qp, float q_scale, int lg, const QuantArgs& aq) {
    const int mb = (int)__builtin_log2f(aq.shift);
#pragma unroll
    for (int c = 0; c < DC; ++c) {
        float4 lo = *reinterpret_cast<const float4*>(qp + 32 * c + 8 * lg);
        float4 hi = *reinterpret_cast<const float4*>(qp + 32 * c + 8 * lg + 4);
        if (q_scale != 0.f) {
            lo.x *= q_scale; lo.y *= q_scale; lo.z *= q_scale; lo.w *= q_scale;
            hi.x *= q_scale; hi.y *= q_scale; hi.z *= q_scale; hi.w *= q_scale;
        }
        float bmax = fmaxf(fmaxf(fmaxf(fabsf(lo.x), fabsf(lo.y)), fmaxf(fabsf(lo.z), fabsf(lo.w))),
                           fmaxf(fmaxf(fabsf(hi.x), fabsf(hi.y)), fmaxf(fabsf(hi.z), fabsf(hi.w))));
        bmax = at_max2_16(bmax);
        const int bias = at_bm_bias_mem(bmax, aq);
        uint4 pk;
        pk.x = pack_bf16(at_bm_quant(lo.x, bias, mb, aq), at_bm_quant(lo.y, bias, mb, aq));
        pk.y = pack_bf16(at_bm_quant(lo.z, bias, mb, aq), at_bm_quant(lo.w, bias, mb, aq));
        pk.z = pack_bf16(at_bm_quant(hi.x, bias, mb, aq), at_bm_quant(hi.y, bias, mb, aq));
        pk.w = pack_bf16(at_bm_quant(hi.z, bias, mb, aq), at_bm_quant(hi.w, bias, mb, aq));
        qf[c] = __builtin_bit_cast(bf16x8, pk);
    }
}
// at_quant_p_block under block_minifloat.  A block of probabilities has a maximum <= 1, so its bias is 0 whatever the block holds --
// no maximum, no reduction over the query's four lanes, no table -- and with bias 0 the element exponent clamp(floor(log2(p + 1e-9)),
// 0, span) is 0 = e_min for every 0 <= p < 2: the subnormal branch alone, q = 2 min(rint(p 2^mbits / 2), 2^mbits - 1) / 2^mbits
// (p = 1 stays 1; the band below 1 rounds to exponent 0 as well).  half_up = 2^(mbits - 1), two_dn = 2^(1 - mbits).
// The values come out in TWO parts: pq the quantised probabilities (0 where p passes through), pt the probabilities p <= 1e-8 the
// reference passes through unquantised (0 elsewhere).  pq times a quantised V is a sum of exactly representable terms; the pass-through
// terms lie far below its last bit, and the matrix unit's accumulator does not round such an addend to nearest as the reference's fp32
// product does -- one ulp of the output, which a coarse quantiser behind the attention (the out-projection's) turns into a whole step
// wherever the exact sum sits on one of its ties, as sums of a few 4-bit values often do.  The caller accumulates the two parts apart
// and adds them once, on the VALU.  Returns whether this lane holds a non-zero pass-through value.
__device__ __forceinline__ bool at_bm_quant_p_block(const float (&pr)[4], float* pq, float* pt, float half_up, float two_dn, const QuantArgs& ap) {
    bool tiny = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float m = fminf(__builtin_rintf(pr[e] * half_up), ap.mant_max);
        const bool pass = pr[e] <= ATOL;
        pq[e] = pass ? 0.f : m * two_dn;
        pt[e] = pass ? pr[e] : 0.f;
        tiny |= pass && pr[e] != 0.f;
    }
    return tiny;
}

// ---- softmax statistics of a lane that walks its query's keys 32 a step -------------------------------------------------------
// (m_run, l_run) = (maximum, sum of exp(x - maximum)) over the scores seen so far, from (-inf, 0); a score of -inf is not a key.
// Re-based when the maximum of ANY lane of the wave moves (rare after the first tiles; exp(-inf) = 0 takes care of the first one).
__device__ __forceinline__ void at_softmax_step(const f32x4 (&sv)[2], float& m_run, float& l_run) {
    const float tmax = fmaxf(fmaxf(fmaxf(sv[0][0], sv[0][1]), fmaxf(sv[0][2], sv[0][3])),
                             fmaxf(fmaxf(sv[1][0], sv[1][1]), fmaxf(sv[1][2], sv[1][3])));
    if (__any(tmax > m_run)) {
        const float m_new = fmaxf(m_run, tmax);
        l_run = m_new == -INFINITY ? 0.f : l_run * at_exp_neg(m_run - m_new);
        m_run = m_new;
    }
    float add = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e) add += sv[h][e] == -INFINITY ? 0.f : at_exp_neg(sv[h][e] - m_run);
    l_run += add;
}
// the query's statistics from those of its four lanes (a query that sees a key has a finite maximum)
__device__ __forceinline__ void at_softmax_finish(float m_run, float l_run, float& row_max, float& row_sum, float& row_inv) {
    row_max = at_max4(m_run);
    row_sum = at_sum4(m_run == -INFINITY ? 0.f : l_run * at_exp_neg(m_run - row_max));
    row_inv = 1.0f / row_sum;
}

}  // namespace mi355q
#endif
