// mi355q_kvp.hip -- the block_fp KV caches that store a mantissa and a shared exponent instead of bf16, and the split-key decode
// attention on them.  Two storages, one set of kernels:
//   Int8Pieces    int8 mantissas, 544-byte pieces, contiguous or paged pools (PG)       KV_M8 } layout, the one deviation and the pairing
//   NibblePieces  4-bit mantissas, two to a byte, 288-byte pieces, contiguous only      KV_M4 } of nibbles: mi355q_kvp.h
//
// A storage is a trait struct and a template parameter ST of every kernel.  It owns its piece constants (PIECE, CODES), the place of a
// lane's 8 mantissa bytes and of its nibble in them (PAIR, NIB), the append's store of one block (store_block), one value of the
// fp32 read-back (value) and the rebuild of a K or V fragment in registers (rebuild: mantissa -> fp32, ldexp by the block's exponent,
// packed to bf16 pairs).  Everything else is typed once: the K walk and V walk of the append, the read-back, the scores loop with its
// statistics and their reduction, the PV loop with its probability block and wave reduction, the launchers and down().  Where the loads
// sit is part of those bodies: 8 mantissa bytes and 8 exponent bytes a lane, two 8-byte loads issued together in front of the
// arithmetic that needs them, the paged look-ahead (PG: the NEXT tile's or pair's table entry, kept scalar) behind them.
// What it takes from elsewhere: append_row, append_v_block, pg_raw / pg_place, the column helpers and dec_stats_empty
// (mi355q_decode_dev.h), the quantiser and softmax arithmetic (mi355q_attn_dev.h), and from mi355q_decode.hip the staging pass
// (launch_kv_stage_ragged), phase C (launch_decode_sum) and the host arithmetic of both launches (append_ragged_grid, decode_args_fill).
// These bodies are the twins of mi355q_decode.hip's ragged kernels -- decode_scores_kernel / decode_pv_kernel<DC, true, GQ, PG> and
// kv_append_kernel<true, PG>, kept apart from them because a helper shared with the bf16 kernels changed some kernel's instruction text
// (profiles/decode_shared_isa.txt) -- and a change there is mirrored here once: workspace, split partition, statistics and the order of
// every sum must stay those of mi355q_decode.hip, so that a decode gives the bits of the bf16 cache's decode with the same number of
// splits.  What the compiler makes of every instantiation against the two files this one replaces: profiles/decode_kvp_isa.txt.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mi355q.h"
#include "mi355q_internal.h"
#include "mi355q_quant_dev.h"
#include "mi355q_attn_dev.h"
#include "mi355q_decode.h"
#include "mi355q_decode_dev.h"
#include "mi355q_kvp.h"

namespace mi355q {

// ---- the two storages -------------------------------------------------------------------------------------------------------
struct Int8Pieces {
    static constexpr int PIECE = KVP_M8_PIECE, CODES = KVP_M8_CODES;       // a piece's bytes; where its exponent bytes start
    static constexpr bool PAGED = true;                         // PG = true kernels exist
    // lane l's 8 mantissa bytes start at 8 (l >> PAIR), its mantissa at bit NIB (l & 1) of each: the whole byte.  (Constants and no
    // functions: a helper is optimised on its own before it is inlined, and that moved the nibble kernels' text.)
    static constexpr int PAIR = 0;
    static constexpr unsigned NIB = 0u;
    typedef long long lane_t;                                   // the read-back's K lane: the width each storage's kernel formed it in

    // one block of 16 values x with maximum bmax: mantissa e is the byte of a lane's slot, 8 bytes apart in k8 (the 16 keys of a tile
    // at one d) and in v8 (the 16 d of one key) alike; the block's exponent code goes to *code.  Plain byte stores.
    __device__ static __forceinline__ void store_block(uint8_t* __restrict__ dst, uint8_t* __restrict__ code, const float (&x)[16],
                                                       float bmax, const QuantArgs& a) {
        const int mbits = (int)__builtin_log2f(a.shift);
        // (an all-zero block: the lowest exponent's code, whatever its wave's other blocks are -- at_block_exponent_mem gives -bias on its
        //  common path and 0 when ANOTHER lane's maximum sends the wave to the table walk, and the piece's bytes must not depend on that)
        const int pw = at_block_exponent_mem(bmax, a);
        const int p = bmax != 0.f ? pw : a.e_min;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float m = bmax != 0.f ? at_quant_mant(x[e], mbits - p, a.mant_max) : 0.f;      // (|m| <= mant_max <= 127)
            dst[e * 8] = (uint8_t)(int8_t)(int)m;
        }
        *code = (uint8_t)(p + a.code_bias);                                                        // (e_min = -bias: 0 .. 2^exponent width - 1)
    }
    // one value: the fp32 number kv_store_block of mi355q_decode.hip packs to bf16
    __device__ static __forceinline__ float value(unsigned mant_byte, unsigned, unsigned code, int down) {
        return __builtin_ldexpf((float)(int)(int8_t)mant_byte, (int)code + down);
    }
    // a lane's fragment from its 8 mantissa bytes m and their 8 exponent codes e (slot j: byte j of each)
    __device__ static __forceinline__ bf16x8 rebuild(uint2 m, uint2 e, unsigned, int down) {
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const unsigned mw = j < 4 ? m.x : m.y, ew = j < 4 ? e.x : e.y;
            f[j] = value((mw >> (8 * (j & 3))) & 0xFFu, 0u, (ew >> (8 * (j & 3))) & 0xFFu, down);
        }
        uint4 pk;
        pk.x = pack_bf16(f[0], f[1]); pk.y = pack_bf16(f[2], f[3]);
        pk.z = pack_bf16(f[4], f[5]); pk.w = pack_bf16(f[6], f[7]);
        return __builtin_bit_cast(bf16x8, pk);
    }
};

struct NibblePieces {
    static constexpr int PIECE = KVP_M4_PIECE, CODES = KVP_M4_CODES;
    static constexpr bool PAGED = false;                        // contiguous only: the launchers refuse `pages`
    // the two lanes of a pair share 8 mantissa bytes at 8 (l >> 1); lane l's mantissa is the nibble at bit 4 (l & 1) of each
    static constexpr int PAIR = 1;
    static constexpr unsigned NIB = 4u;
    typedef int lane_t;

    // one block of 16 values x with maximum bmax: the mantissas of lanes 2 e and 2 e + 1 of a lane group, at one slot, are the two
    // nibbles of ONE byte, 8 bytes apart in k4 (the 16 keys of a tile at one d) and in v4 (the 16 d of one key) alike; the block's
    // exponent code goes to *code.  Plain byte stores of whole bytes: nothing is read (mi355q_kvp.h).
    __device__ static __forceinline__ void store_block(uint8_t* __restrict__ dst, uint8_t* __restrict__ code, const float (&x)[16],
                                                       float bmax, const QuantArgs& a) {
        const int mbits = (int)__builtin_log2f(a.shift);
        const int pw = at_block_exponent_mem(bmax, a);
        const int p = bmax != 0.f ? pw : a.e_min;                                                        // (as in Int8Pieces::store_block)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float lo = bmax != 0.f ? at_quant_mant(x[2 * e], mbits - p, a.mant_max) : 0.f;        // (|m| <= mant_max <= 7)
            const float hi = bmax != 0.f ? at_quant_mant(x[2 * e + 1], mbits - p, a.mant_max) : 0.f;
            dst[e * 8] = (uint8_t)(((int)lo & 0xF) | (((int)hi & 0xF) << 4));
        }
        *code = (uint8_t)(p + a.code_bias);                                                              // (e_min = -bias: 0 .. 2^exponent width - 1)
    }
    // one value: the fp32 number kv_store_block of mi355q_decode.hip packs to bf16, from the sign-extended nibble at bit `at` of word
    __device__ static __forceinline__ float value(unsigned word, unsigned at, unsigned code, int down) {
        return __builtin_ldexpf((float)(int)__builtin_amdgcn_sbfe(word, at, 4u), (int)code + down);      // (the builtin's result is typed unsigned)
    }
    // a lane's fragment from the 8 mantissa bytes m of its lane pair, nib = 4 (lane & 1) its nibble of each, and its 8 exponent codes e
    // (slot j: byte j of each)
    __device__ static __forceinline__ bf16x8 rebuild(uint2 m, uint2 e, unsigned nib, int down) {
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const unsigned mw = j < 4 ? m.x : m.y, ew = j < 4 ? e.x : e.y;
            f[j] = value(mw, 8u * (j & 3) + nib, (ew >> (8 * (j & 3))) & 0xFFu, down);
        }
        uint4 pk;
        pk.x = pack_bf16(f[0], f[1]); pk.y = pack_bf16(f[2], f[3]);
        pk.z = pack_bf16(f[4], f[5]); pk.w = pack_bf16(f[6], f[7]);
        return __builtin_bit_cast(bf16x8, pk);
    }
};

// exponent code -> the ldexp argument of a mantissa: p - mbits = code - exponent_bias - mbits
static int down(const QuantArgs& a) { return -(a.code_bias + (int)__builtin_log2f(a.shift)); }

// ---- append ---------------------------------------------------------------------------------------------------------------
struct KvpAppendArgs {
    KvpCache c;
    const float* k;
    const float* v;
    long long ksb, kst, vsb, vst;
    long long n;
    int kblocks;
    const int32_t* lengths;     // row b's L = lengths[b], its n = counts[b] (NULL: n) <= n
    const int32_t* counts;
    KvPages pg;                 // paged pools (PG): c.k / c.v are the pools, c.C = max_pages * P; else zeros (behind every other field)
};

template <class ST, bool PG>
__global__ __launch_bounds__(256) void kvp_append_kernel(const QuantArgs ak, const QuantArgs av, const KvpAppendArgs a) {
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
        long long pt = b * NTC + t;
        if constexpr (PG) pt = pg_place(a.pg, pg_raw(a.pg, b, t >> (a.pg.lg_p - 4)), t, a.pg.lg_p - 4);     // (t < NTC: inside the table's row)
        uint8_t* __restrict__ piece = a.c.k + (pt * (D >> 5) + c) * ST::PIECE;
        ST::store_block(piece + (16 >> ST::PAIR) * g * 8 + j, piece + ST::CODES + (d & 31), x, bmax, ak);
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
        long long ps = b * NPC + s;
        if constexpr (PG) ps = pg_place(a.pg, pg_raw(a.pg, b, s >> (a.pg.lg_p - 5)), s, a.pg.lg_p - 5);     // (key < C: inside the table's row)
        uint8_t* __restrict__ piece = a.c.v + (ps * DT + dt) * ST::PIECE;
        ST::store_block(piece + (16 >> ST::PAIR) * g * 8 + j, piece + ST::CODES + 8 * g + j, x, bmax, av);
    }
}

// row b's first counts[b] (NULL: n) input rows behind ITS length lengths[b]: launch_kv_append_ragged on storage ST
template <class ST>
static int kvp_append(const KvpCache& c, const QuantArgs& ak, const QuantArgs& av, const float* k, const float* v, long long ksb,
                      long long kst, long long vsb, long long vst, const int32_t* lengths, const int32_t* counts, long long n,
                      hipStream_t st, const KvPages* pages) {
    if (pages && !ST::PAGED) return MI355Q_E_UNSUPPORTED;
    KvpAppendArgs a{};
    a.c = c; a.k = k; a.v = v;
    a.ksb = ksb; a.kst = kst; a.vsb = vsb; a.vst = vst;
    a.n = n; a.lengths = lengths; a.counts = counts;
    dim3 grid;
    if (const int rc = append_ragged_grid(c.B, c.D, n, a.kblocks, grid)) return rc;
    if (pages) a.pg = *pages;
    if (ST::PAGED && pages) hipLaunchKernelGGL((kvp_append_kernel<ST, ST::PAGED>), grid, dim3(256), 0, st, ak, av, a);
    else hipLaunchKernelGGL((kvp_append_kernel<ST, false>), grid, dim3(256), 0, st, ak, av, a);
    launch_kv_stage_ragged(KvCache{nullptr, nullptr, c.stage, c.B, c.C, c.D}, k, ksb, kst, lengths, counts, n, st);
    return (int)hipGetLastError();
}

// ---- the fp32 read-back -----------------------------------------------------------------------------------------------------
template <class ST, bool PG>
__device__ __forceinline__ void kvp_decode_fp32_body(const KvpCache& c, const int k_down, const int v_down, float* __restrict__ k_out,
                                                     float* __restrict__ v_out, long long L, const int32_t* __restrict__ lengths,
                                                     const KvPages& pg) {
    const int D = c.D;
    const long long b = blockIdx.y, NTC = c.C >> 4, NPC = (c.C + 31) >> 5;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= L * D) return;
    const long long key = idx / D;
    const int d = (int)(idx - key * D);
    if (key >= __builtin_amdgcn_readfirstlane(lengths[b])) {          // (L = max_length <= C: zeros behind the row's own length)
        k_out[(b * L + key) * D + d] = 0.f;
        v_out[(b * L + key) * D + d] = 0.f;
        return;
    }
    const uint8_t* __restrict__ kp = c.k + ((b * NTC + (key >> 4)) * (D >> 5) + (d >> 5)) * ST::PIECE;
    const int h = (int)(key >> 4) & 1, g = (int)(key & 15) >> 2, j = 4 * h + (int)(key & 3);
    const uint8_t* __restrict__ vp = c.v + ((b * NPC + (key >> 5)) * (D >> 4) + (d >> 4)) * ST::PIECE;
    if constexpr (PG) {                                               // (key < lengths[b], key < L <= C: a page of the row's)
        const int raw = pg_raw(pg, b, key >> pg.lg_p);
        kp = c.k + (pg_place(pg, raw, key >> 4, pg.lg_p - 4) * (D >> 5) + (d >> 5)) * ST::PIECE;
        vp = c.v + (pg_place(pg, raw, key >> 5, pg.lg_p - 5) * (D >> 4) + (d >> 4)) * ST::PIECE;
    }
    // K: lane (key & 15) + 16 ((d >> 3) & 3), slot d & 7; V: lane (d & 15) + 16 g, slot j
    const typename ST::lane_t kl = (typename ST::lane_t)(key & 15) + 16 * ((d >> 3) & 3);
    const int vl = (d & 15) + 16 * g;
    const float kf = ST::value(kp[(kl >> ST::PAIR) * 8 + (d & 7)], ST::NIB * (unsigned)(kl & 1), kp[ST::CODES + (d & 31)], k_down);
    const float vf = ST::value(vp[(vl >> ST::PAIR) * 8 + j], ST::NIB * (vl & 1), vp[ST::CODES + 8 * g + j], v_down);
    // through bf16, as the decode kernels' fragments are
    k_out[(b * L + key) * D + d] = __uint_as_float(pack_bf16(kf, 0.f) << 16);
    v_out[(b * L + key) * D + d] = __uint_as_float(pack_bf16(vf, 0.f) << 16);
}

// (two entry points, one body, as kv_decode_fp32_kernel has: the unpaged kernel keeps its argument list and its code)
template <class ST>
__global__ __launch_bounds__(256) void kvp_decode_fp32_kernel(const KvpCache c, const int k_down, const int v_down, float* __restrict__ k_out,
                                                              float* __restrict__ v_out, long long L, const int32_t* __restrict__ lengths) {
    kvp_decode_fp32_body<ST, false>(c, k_down, v_down, k_out, v_out, L, lengths, KvPages{});
}
template <class ST>
__global__ __launch_bounds__(256) void kvp_decode_fp32_paged_kernel(const KvpCache c, const int k_down, const int v_down, float* __restrict__ k_out,
                                                                    float* __restrict__ v_out, long long L, const int32_t* __restrict__ lengths,
                                                                    const KvPages pg) {
    kvp_decode_fp32_body<ST, true>(c, k_down, v_down, k_out, v_out, L, lengths, pg);
}

// the cache's values, as the decode kernels rebuild them, back as fp32 [B, L, D]; zeros behind row b's lengths[b]
template <class ST>
static int kvp_decode_fp32(const KvpCache& c, const QuantArgs& ak, const QuantArgs& av, float* k_out, float* v_out, long long L,
                           const int32_t* lengths, hipStream_t st, const KvPages* pages) {
    if (pages && !ST::PAGED) return MI355Q_E_UNSUPPORTED;
    const long long blocks = (L * c.D + 255) / 256;
    if (blocks > 0x7FFFFFFFLL) return MI355Q_E_UNSUPPORTED;
    if (!lengths) return MI355Q_E_BADARG;
    const dim3 grid((unsigned)blocks, (unsigned)c.B);
    if constexpr (ST::PAGED) {
        if (pages) {
            hipLaunchKernelGGL(kvp_decode_fp32_paged_kernel<ST>, grid, dim3(256), 0, st, c, down(ak), down(av), k_out, v_out, L, lengths, *pages);
            return (int)hipGetLastError();
        }
    }
    hipLaunchKernelGGL(kvp_decode_fp32_kernel<ST>, grid, dim3(256), 0, st, c, down(ak), down(av), k_out, v_out, L, lengths);
    return (int)hipGetLastError();
}

// ---- decode ---------------------------------------------------------------------------------------------------------------
struct KvpDecodeArgs {
    DecodeArgs g;               // as for the ragged launches of mi355q_decode.hip (PG: g.pg the page table); kq / vq stay NULL
    const uint8_t* k;
    const uint8_t* v;
    int k_down, v_down;         // down() of the cached K / V operand's quantiser
};

template <class ST, int DC, bool GQ, bool PG>
__global__ __launch_bounds__(256) void kvp_scores_kernel(const QuantArgs aq, const KvpDecodeArgs a) {
    __shared__ float sm_[4][64], sl_[4][64];
    const DecodeArgs& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, lg = lane >> 4;
    const long long b = blockIdx.y, s = blockIdx.x, cb = dec_cache_row<GQ>(g, b);   // b: launch row (workspace), cb: cache row
    const long long L = dec_length<true>(g, cb), NT = (L + 15) >> 4;
    if (2 * g.pps * s >= NT) {          // a split wholly behind the row's last tile: the empty statistics, no K read
        dec_stats_empty(g, b, s, tid);
        return;
    }
    long long row, qrow;
    dec_column<GQ>(g, b, c16, row, qrow);
    bf16x8 qf[DC];                      // quantised in registers
    at_quant_q_frag(qf, g.q + row * g.qsb + qrow * g.qsm, g.q_scale, lg, aq, at_block_exponent_mem);
    const long long kvis = dec_horizon(g, L, qrow);
    const float scale_inv = g.scale_div != 0.f ? 1.0f / g.scale_div : 0.f;
    const long long t_lo = 2 * g.pps * s, t_hi = min(NT, t_lo + 2 * g.pps);
    // a lane's mantissa bytes at 8 (lane >> PAIR) (its nibble of each: nib), its 8 exponent codes (the d of its group) at CODES + 8 lg of
    // the piece (t < NT <= NTC)
    const uint8_t* __restrict__ kmb = a.k + (PG ? 0 : cb * g.NTC * DC * ST::PIECE) + (lane >> ST::PAIR) * 8;
    const uint8_t* __restrict__ keb = a.k + (PG ? 0 : cb * g.NTC * DC * ST::PIECE) + ST::CODES + lg * 8;
    const unsigned nib = ST::NIB * (lane & 1);
    float* __restrict__ sc = g.scores + b * g.NT * 256 + lane * 4;
    // running (max, sum of exp(x - max)) of this lane's visible scores, re-based when the maximum moves
    float m_run = -INFINITY, l_run = 0.f;
    // paged: the table entry of the NEXT tile this wave takes is asked for while this one's pieces are loaded (t < t_hi <= NT)
    int raw = 0;
    if constexpr (PG) {
        if (t_lo + wave < t_hi) raw = pg_raw(g.pg, cb, (t_lo + wave) >> (g.pg.lg_p - 4));
    }
    for (long long t = t_lo + wave; t < t_hi; t += 4) {
        long long pt = t;                                   // the tile's place in K; the workspace keeps t
        if constexpr (PG) pt = pg_place(g.pg, __builtin_amdgcn_readfirstlane(raw), t, g.pg.lg_p - 4);
        uint2 km[DC], ke[DC];           // both loads of every chunk in front of the first rebuild
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            km[c] = *reinterpret_cast<const uint2*>(kmb + (pt * DC + c) * ST::PIECE);
            ke[c] = *reinterpret_cast<const uint2*>(keb + (pt * DC + c) * ST::PIECE);
        }
        if constexpr (PG) {
            if (t + 4 < t_hi) raw = pg_raw(g.pg, cb, (t + 4) >> (g.pg.lg_p - 4));
        }
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < DC; ++c)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ST::rebuild(km[c], ke[c], nib, a.k_down), qf[c], acc, 0, 0, 0);
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

template <class ST, int DC, bool GQ, bool PG>
__global__ __launch_bounds__(256) void kvp_pv_kernel(const QuantArgs ap, const KvpDecodeArgs a) {
    constexpr int DT = DC * 2;
    __shared__ f32x4 red[4][DT][64];
    const DecodeArgs& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, lg = lane >> 4;
    const long long b = blockIdx.y, s = blockIdx.x, cb = dec_cache_row<GQ>(g, b);
    const long long L = dec_length<true>(g, cb), NT = (L + 15) >> 4, NP = (L + 31) >> 5;
    const long long p_lo = g.pps * s, p_hi = min(NP, p_lo + g.pps);
    if (p_lo >= p_hi) {                 // an empty split (every split of an empty row): a zero partial output, no V read
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
    const int mbp = (int)__builtin_log2f(ap.shift);
    // a lane's mantissa bytes at 8 (lane >> PAIR) (its nibble of each: nib), the 8 exponent codes of its 8 keys at CODES + 8 lg of the
    // piece (pair < NP <= NPC)
    const uint8_t* __restrict__ vmb = a.v + (PG ? 0 : cb * g.NPC * DT * ST::PIECE) + (lane >> ST::PAIR) * 8;
    const uint8_t* __restrict__ veb = a.v + (PG ? 0 : cb * g.NPC * DT * ST::PIECE) + ST::CODES + lg * 8;
    const unsigned nib = ST::NIB * (lane & 1);
    const float* __restrict__ sc = g.scores + b * g.NT * 256 + lane * 4;
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    int raw = 0;                                            // (paged: one pair ahead, as in kvp_scores_kernel; pr_i < p_hi <= NP)
    if constexpr (PG) {
        if (p_lo + wave < p_hi) raw = pg_raw(g.pg, cb, (p_lo + wave) >> (g.pg.lg_p - 5));
    }
    for (long long pr_i = p_lo + wave; pr_i < p_hi; pr_i += 4) {
        long long pp = pr_i;                                // the pair's place in V; scores and horizon keep pr_i
        if constexpr (PG) pp = pg_place(g.pg, __builtin_amdgcn_readfirstlane(raw), pr_i, g.pg.lg_p - 5);
        uint2 vm[DT], ve[DT];           // both loads of every piece in front of the probabilities: in flight while those are made
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            vm[dt] = *reinterpret_cast<const uint2*>(vmb + (pp * DT + dt) * ST::PIECE);
            ve[dt] = *reinterpret_cast<const uint2*>(veb + (pp * DT + dt) * ST::PIECE);
        }
        if constexpr (PG) {
            if (pr_i + 4 < p_hi) raw = pg_raw(g.pg, cb, (pr_i + 4) >> (g.pg.lg_p - 5));
        }
        float pq[8];
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
            at_quant_p_block(pr, pq + 4 * h, mbp, ap, at_block_exponent_mem);
        }
        const bf16x8 pf = at_pack_p(pq);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ST::rebuild(vm[dt], ve[dt], nib, a.v_down), pf, o[dt], 0, 0, 0);
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

// phases A and B of one head-dim chunk count and page form, grouped or not
template <class ST, int DC, bool PG>
static void kvp_decode_go(const dim3 grid, hipStream_t st, const QuantArgs& aq, const QuantArgs& ap, const KvpDecodeArgs& a, int G) {
    if (G) {
        hipLaunchKernelGGL((kvp_scores_kernel<ST, DC, true, PG>), grid, dim3(256), 0, st, aq, a);
        hipLaunchKernelGGL((kvp_pv_kernel<ST, DC, true, PG>), grid, dim3(256), 0, st, ap, a);
    } else {
        hipLaunchKernelGGL((kvp_scores_kernel<ST, DC, false, PG>), grid, dim3(256), 0, st, aq, a);
        hipLaunchKernelGGL((kvp_pv_kernel<ST, DC, false, PG>), grid, dim3(256), 0, st, ap, a);
    }
}

// launch_bfp_attention_decode's ragged, unwindowed forms on storage ST: decode_args_fill with span = L
template <class ST>
static int kvp_decode(const QuantArgs& aq, const QuantArgs& ap, const QuantArgs& ak, const QuantArgs& av, const KvpCache& c, const float* q,
                      float* out, void* workspace, long long M, long long L, int causal, float q_scale, float scale_div,
                      const long long* strides, int splits, hipStream_t st, const int32_t* lengths, int G, const KvPages* pages) {
    if (pages && !ST::PAGED) return MI355Q_E_UNSUPPORTED;
    if (!lengths) return MI355Q_E_BADARG;                   // (no uniform launch)
    KvpDecodeArgs a{};
    DecodeArgs& g = a.g;
    long long rows;
    if (const int rc = decode_args_fill(g, c.B, c.C, c.D, M, L, L, G, splits, strides, workspace, pages, rows)) return rc;
    a.k = c.k; a.v = c.v;
    a.k_down = down(ak); a.v_down = down(av);
    g.q = q; g.out = out; g.lengths = lengths;
    g.causal = causal; g.q_scale = q_scale; g.scale_div = scale_div;
    const dim3 grid((unsigned)g.S, (unsigned)rows);
#define MI355Q_KVP_DECODE_GO(DC_)                                                                                    \
    if (ST::PAGED && pages) kvp_decode_go<ST, DC_, ST::PAGED>(grid, st, aq, ap, a, G);                               \
    else kvp_decode_go<ST, DC_, false>(grid, st, aq, ap, a, G);
    switch (c.D / 32) {
        case 1: MI355Q_KVP_DECODE_GO(1); break;
        case 2: MI355Q_KVP_DECODE_GO(2); break;
        case 3: MI355Q_KVP_DECODE_GO(3); break;
        case 4: MI355Q_KVP_DECODE_GO(4); break;
        default: return MI355Q_E_UNSUPPORTED;
    }
#undef MI355Q_KVP_DECODE_GO
    launch_decode_sum(g, G != 0, rows, st);
    return (int)hipGetLastError();
}

// ---- the launchers mi355q_kvp.h declares: one switch on the storage an operation (a new storage: its trait struct above, a case here) ----
int launch_kvp_append(KvMantissa m, const KvpCache& c, const QuantArgs& ak, const QuantArgs& av, const float* k, const float* v, long long ksb,
                      long long kst, long long vsb, long long vst, const int32_t* lengths, const int32_t* counts, long long n,
                      hipStream_t st, const KvPages* pages) {
    switch (m) {
        case KV_M8: return kvp_append<Int8Pieces>(c, ak, av, k, v, ksb, kst, vsb, vst, lengths, counts, n, st, pages);
        case KV_M4: return kvp_append<NibblePieces>(c, ak, av, k, v, ksb, kst, vsb, vst, lengths, counts, n, st, pages);
    }
    return MI355Q_E_BADARG;
}
int launch_kvp_decode_fp32(KvMantissa m, const KvpCache& c, const QuantArgs& ak, const QuantArgs& av, float* k_out, float* v_out, long long L,
                           const int32_t* lengths, hipStream_t st, const KvPages* pages) {
    switch (m) {
        case KV_M8: return kvp_decode_fp32<Int8Pieces>(c, ak, av, k_out, v_out, L, lengths, st, pages);
        case KV_M4: return kvp_decode_fp32<NibblePieces>(c, ak, av, k_out, v_out, L, lengths, st, pages);
    }
    return MI355Q_E_BADARG;
}
int launch_bfp_attention_decode_kvp(KvMantissa m, const QuantArgs& aq, const QuantArgs& ap, const QuantArgs& ak, const QuantArgs& av,
                                    const KvpCache& c, const float* q, float* out, void* workspace, long long M, long long L, int causal,
                                    float q_scale, float scale_div, const long long* strides, int splits, hipStream_t st,
                                    const int32_t* lengths, int G, const KvPages* pages) {
    switch (m) {
        case KV_M8:
            return kvp_decode<Int8Pieces>(aq, ap, ak, av, c, q, out, workspace, M, L, causal, q_scale, scale_div, strides, splits, st, lengths, G, pages);
        case KV_M4:
            return kvp_decode<NibblePieces>(aq, ap, ak, av, c, q, out, workspace, M, L, causal, q_scale, scale_div, strides, splits, st, lengths, G, pages);
    }
    return MI355Q_E_BADARG;
}

}  // namespace mi355q
