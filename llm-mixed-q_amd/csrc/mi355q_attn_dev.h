// Device helpers shared by the attention kernels (mi355q_attention.hip: prefill; mi355q_decode.hip: KV cache and decode):
// the block_fp element / shared-exponent arithmetic of the four quantisers, exp and quotient of the softmax, and the
// reductions over the four lanes that hold one query's values of a 16 x 16 MFMA tile.
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

}  // namespace mi355q
#endif
