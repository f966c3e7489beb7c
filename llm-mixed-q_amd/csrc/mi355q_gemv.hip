// mi355q_gemv.hip -- the block_fp product for a small batch of rows (M <= 16: token-by-token generation, a search trial on a
// few prompts, a classification head) that reads the weights STRAIGHT from their at-rest form (mi355q_pack.hip: width-bit
// mantissas + one code byte per 16-block = width + 0.5 bits per value).  Nothing is expanded to memory: the product is bound by
// the weight stream, so it should read the fewest bytes that define the weights, once.
//
//   y[m, n] = sum_k x[m, k] * wm[n, k] * 2^(e[n, k / 16] - w_off)   (+ bias[n])          (include/mi355q.h, mi355q_bfp_gemm)
//
// with x as the tiled bf16 values the activation quantiser already writes (exact for widths <= 9).
//
// Decomposition.  One workgroup owns 16 weight rows (one column tile of y); its waves split K between them in CHUNKS of 512
// values and each wave keeps one 16 x 16 fp32 accumulator (v_mfma_f32_16x16x32_bf16, x as the 16-row A operand, the unpacked
// weights as B).  Inside a chunk lane (r = lane % 16, g = lane / 16) owns the eight blocks 8 g .. 8 g + 7 of weight row r:
// 16 * width contiguous bytes, `width` 16-byte loads straight into registers (rows are 16-byte aligned when K % 128 == 0), and
// for each of its sixteen half blocks forms the B fragment m * 2^e (exact in bf16) while the x fragment of the SAME eight k --
// 16 bytes of the tiled operand -- comes from the cache.  The order of k inside an MFMA step is therefore a permutation of the
// natural one, the same on both operands.  No LDS on the way in: the weights are used once by the lane that loaded them.
// The waves' accumulators meet in LDS (every word written before the barrier and read after it) and are summed in wave order
// by the first 256 threads, which then add the row flavour's exception blocks from the bucketed list (entries in list order),
// the bias, and store.  No atomics, no scratch: the same inputs give the same bits.  K is never split across workgroups (that
// would need a scratch slab per slice); a 4096-row layer at K = 4096 runs 256 workgroups of 8 waves.
//
// Other K % 64 == 0 (rows only 2-byte aligned, a tail shorter than eight blocks) take the same kernel with halfword loads and
// per-block masks: correct, not fast.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mi355q.h"
#include "mi355q_gemv.h"

namespace mi355q {
namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 gv_bf16x8;
typedef __attribute__((ext_vector_type(4))) float gv_f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned gv_u32x4;

constexpr int GEMV_MAX_WAVES = 16;           // waves of a workgroup on the fast path (128 registers a lane) ...
constexpr int GEMV_MAX_WAVES_SLOW = 8;       // ... and on the halfword path, whose masks and addresses need more of them
constexpr int GEMV_CHUNK_BLOCKS = 32;        // 4 lane groups x 8 blocks = 512 values of K

// value v (0 .. 127) of a lane's 8-block bit string d[]: v, W compile-time after unrolling, so every shift is an immediate
template <int W>
__device__ __forceinline__ int gv_field(const unsigned (&d)[4 * W], int v) {
    const int p = v * W, i = p >> 5, s = p & 31;
    const unsigned u = (s + W <= 32) ? d[i] >> s : __builtin_amdgcn_alignbit(d[i + 1 < 4 * W ? i + 1 : i], d[i], s);
    return ((int)(u << (32 - W))) >> (32 - W);
}

// One chunk of one wave.  xlane: the tiled x operand + (lane % 16) * 16; wrow / crow: this lane's weight row in `packed` /
// `codes`; kb0: the first of the lane's eight blocks (a multiple of 8); rexp: the row's exponent, < 0 on the per-block flavour.
// FAST: K % 128 == 0 (16-byte loads; a lane's eight blocks are all inside the row or all outside).  MASKED: blocks >= nkb exist
// in this chunk: their scale is 0 and their x fragment is replaced by zeros (whatever lies there is not x).
template <int W, bool FAST, bool MASKED>
__device__ __forceinline__ void gv_chunk(gv_f32x4& acc, const uint8_t* __restrict__ xlane, const uint8_t* __restrict__ wrow,
                                         const uint8_t* __restrict__ crow, int kb0, int nkb, int rexp, int w_off) {
    const int nv = MASKED ? min(max(nkb - kb0, 0), 8) : 8;          // valid blocks of this lane
    unsigned d[4 * W];
    unsigned char code[8];
    if (FAST) {
        const long long kbl = (MASKED && nv == 0) ? 0 : kb0;         // (outside the row: any valid address, scale 0)
        const gv_u32x4* wp = reinterpret_cast<const gv_u32x4*>(wrow + kbl * (2 * W));
#pragma unroll
        for (int q = 0; q < W; ++q) {
            const gv_u32x4 v = wp[q];
            d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z; d[4 * q + 3] = v.w;
        }
        const uint2 c2 = *reinterpret_cast<const uint2*>(crow + kbl);
#pragma unroll
        for (int b = 0; b < 8; ++b) code[b] = (unsigned char)((b < 4 ? c2.x >> (8 * b) : c2.y >> (8 * (b - 4))) & 0xFFu);
    } else {
        const uint16_t* wp = reinterpret_cast<const uint16_t*>(wrow);
#pragma unroll
        for (int q = 0; q < 4 * W; ++q) {
            const int b0 = (2 * q) / W, b1 = (2 * q + 1) / W;        // the blocks the two halfwords belong to
            const unsigned lo = wp[b0 < nv ? (long long)kb0 * W + 2 * q : 0];
            const unsigned hi = wp[b1 < nv ? (long long)kb0 * W + 2 * q + 1 : 0];
            d[q] = lo | (hi << 16);
        }
#pragma unroll
        for (int b = 0; b < 8; ++b) code[b] = crow[b < nv ? kb0 + b : 0];
    }
    float sc[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const int c = code[b];
        const bool dead = (MASKED && b >= nv) || (rexp >= 0 && c == 0xFF);       // outside the row / an exception block
        sc[b] = dead ? 0.f : __builtin_ldexpf(1.f, (rexp >= 0 ? rexp + c : c) - w_off);
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const bool live = !MASKED || (t >> 1) < nv;
        gv_u32x4 xa = *reinterpret_cast<const gv_u32x4*>(xlane + (live ? (long long)kb0 * 512 + t * 256 : 0));
        if (MASKED && !live) xa = gv_u32x4{0u, 0u, 0u, 0u};
        gv_u32x4 wb;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float f0 = (float)gv_field<W>(d, 8 * t + 2 * q) * sc[t >> 1];
            const float f1 = (float)gv_field<W>(d, 8 * t + 2 * q + 1) * sc[t >> 1];
            wb[q] = (__float_as_uint(f0) >> 16) | (__float_as_uint(f1) & 0xFFFF0000u);       // exact in bf16: truncation
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(gv_bf16x8, xa), __builtin_bit_cast(gv_bf16x8, wb), acc, 0, 0, 0);
    }
}

__device__ __forceinline__ float gv_x_value(const uint8_t* __restrict__ xt, int m, int k) {      // element (m, k) of the tiled operand
    const uint16_t h = *reinterpret_cast<const uint16_t*>(xt + (long long)(k >> 5) * 1024 + ((((k & 31) >> 3) * 16 + m) * 16) + (k & 7) * 2);
    return __uint_as_float((unsigned)h << 16);
}

template <int W, bool FAST>
__global__ __launch_bounds__(64 * (FAST ? GEMV_MAX_WAVES : GEMV_MAX_WAVES_SLOW)) void bfp_gemv_packed_kernel(PackedSmallArgs a, int chunks_per_wave, int nchunks) {
    __shared__ float part[GEMV_MAX_WAVES][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    const long long n0 = (long long)blockIdx.x * 16;
    const long long n = min(n0 + r, a.N - 1);                        // (rows past N: a valid row, never stored)
    const int nkb = (int)(a.K >> 4);
    const uint8_t* wrow = a.packed + n * (a.K / 8 * W);
    const uint8_t* crow = a.codes + n * nkb;
    const uint8_t* xlane = a.x_tiled + r * 16;
    const int rexp = a.row_exp ? (int)a.row_exp[n] : -1;
    gv_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int c_end = min((wave + 1) * chunks_per_wave, nchunks);
    for (int c = wave * chunks_per_wave; c < c_end; ++c) {
        const int kb0 = c * GEMV_CHUNK_BLOCKS + g * 8;
        if (FAST && (c + 1) * GEMV_CHUNK_BLOCKS <= nkb) gv_chunk<W, true, false>(acc, xlane, wrow, crow, kb0, nkb, rexp, a.w_off);
        else gv_chunk<W, FAST, true>(acc, xlane, wrow, crow, kb0, nkb, rexp, a.w_off);
    }
    // accumulator: column (weight row) lane % 16, x rows 4 g .. 4 g + 3
#pragma unroll
    for (int i = 0; i < 4; ++i) part[wave][(4 * g + i) * 16 + r] = acc[i];
    __syncthreads();
    for (int t = threadIdx.x; t < 256; t += blockDim.x) {
        const int m = t >> 4;
        const long long col = n0 + (t & 15);
        float s = part[0][t];
        for (int w = 1; w < nw; ++w) s += part[w][t];
        if (m >= a.M || col >= a.N) continue;
        if (a.list) {
            // the row flavour's exception blocks (zero in the sweep above): the entries of this tile's bucket, in list order
            const int cap = a.list_cap > 0 ? a.list_cap : 120;
            const int* bucket = a.list + 8 + (n0 >> 8) * (8 + 8 * (long long)cap);
            const int cnt = min(bucket[0], cap);
            for (int i = 0; i < cnt; ++i) {
                const int* e = bucket + 8 + 8 * i;
                if (e[0] != (int)col) continue;
                const int kb = e[1];
                if (kb < 0 || kb >= nkb) continue;
                float dot = 0.f;                                     // exact: 16 products of integers that share x's block exponent
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int mj = (int)(signed char)((e[4 + (j >> 2)] >> (8 * (j & 3))) & 0xFF);
                    dot += gv_x_value(a.x_tiled, m, kb * 16 + j) * (float)mj;
                }
                s += __builtin_ldexpf(dot, e[2] - a.w_off);
            }
        }
        if (a.bias) s += a.bias[col];
        a.y[m * a.ldy + col] = s;
    }
}

}  // namespace

int launch_bfp_gemm_packed_small(const PackedSmallArgs& a, hipStream_t st) {
    const int nkb = (int)(a.K >> 4);
    const int nchunks = (nkb + GEMV_CHUNK_BLOCKS - 1) / GEMV_CHUNK_BLOCKS;
    const bool fast = a.K % 128 == 0;
    const int max_waves = fast ? GEMV_MAX_WAVES : GEMV_MAX_WAVES_SLOW;
    const int cpw = (nchunks + max_waves - 1) / max_waves;
    const int nw = (nchunks + cpw - 1) / cpw;
    const unsigned grid = (unsigned)((a.N + 15) / 16);
#define MI355Q_GEMV(W)                                                                                                        \
    case W:                                                                                                                   \
        if (fast) hipLaunchKernelGGL((bfp_gemv_packed_kernel<W, true>), grid, 64 * nw, 0, st, a, cpw, nchunks);               \
        else hipLaunchKernelGGL((bfp_gemv_packed_kernel<W, false>), grid, 64 * nw, 0, st, a, cpw, nchunks);                   \
        break;
    switch (a.width) {
        MI355Q_GEMV(2) MI355Q_GEMV(3) MI355Q_GEMV(4) MI355Q_GEMV(5) MI355Q_GEMV(6) MI355Q_GEMV(7) MI355Q_GEMV(8)
        default: return MI355Q_E_BADARG;
    }
#undef MI355Q_GEMV
    return (int)hipGetLastError();
}

}  // namespace mi355q
