// mi355q_decode.hip -- incremental decoding of the quantised attention core: a block_fp KV cache and a split-key decode kernel.
//
// The reference decodes with `past_key_value`: torch.cat of fp32 K / V (models/llama_quantized/modeling_llama.py:301-306, the
// same in modeling_opt.py) in front of the core (modeling_llama.py:309-344), whose four block_fp quantisers then see the
// concatenated tensors of length L.  Here the cache holds what those quantisers make of K and V (layout: mi355q_decode.h):
//   v [.., L, D]    blocks along D at a fixed key: a key's values are quantised once, when it is appended
//   k^T [.., D, L]  blocks of 16 consecutive KEYS at a fixed d: the last, open block (L % 16 keys) changes its shared exponents
//                   with every key -- its fp32 rows stay in a staging area and the block is quantised again on every append
//                   until it is full (absent keys = the blocking's zero padding: zeros, outside the maximum)
// and the decode kernels read quantised bf16 only: 2 B per cached value instead of 4 B read + a pack launch per step.
// Decode, 1 <= M <= 16 queries (the last M positions) against L keys, keys split over S workgroups per head so that a small batch
// still fills the chip.  The softmax is normalised in fp32 BEFORE the probabilities are quantised (blocks of 16 keys of a query),
// so row maximum and sum over all L keys must be final first: two phases, no grid-wide barrier, no waiting on other workgroups.
//   phase A (decode_scores_kernel, grid S x B): scores of the split's key tiles -> workspace, as their MFMA lanes hold them;
//            the split's per-query (max, sum of exp(x - max)) over VISIBLE keys (key < L and inside the causal horizon)
//   phase B (decode_pv_kernel, grid S x B): the S statistics combined in split order; probabilities per 16-key block, quantised,
//            times the V fragments -> the split's partial output (S == 1: the output itself)
//   phase C (decode_sum_kernel, grid B): partial outputs summed in split order -- the same inputs give the same bits every run.
// Ragged batches (layout note in mi355q_decode.h): the same kernels with RG = true read the row's length from a device array --
// one load a workgroup, kept scalar -- where the uniform instantiations (RG = false) read the host's L; a row's workgroups skip
// the key tiles the row does not have, and a row of length 0 (a finished sequence) costs a few empty workgroups.
// Grouped queries (GQ = true; column map and launch rows: mi355q_decode.h): the G query heads that share a cache row sit in the
// columns one query head leaves unused -- gw heads x M queries a launch row -- and are served by the same K / V fragment loads.
// Everything per query is per column, so a head's bits are those of the GQ = false kernels on a private copy of the row.
// Paged cache (PG = true, with RG = true only; layout and address rules: mi355q_decode.h): a tile's or pair's place goes through the
// row's page table.  In the decode loops the index is wave-uniform, so the entry is one 4-byte load kept scalar like lengths[b], asked
// for one iteration AHEAD of the fragment loads it addresses; the score workspace keeps logical indices.
// Sliding window (WN = true, with RG = true only; semantics and the relative partition: mi355q_decode.h): a query at position p sees keys
// max(0, p - W + 1) .. p.  A lane keeps a lower bound klo next to its horizon; the row's first visible pair p0 -- scalar, from lengths[b] --
// is where the split partition and the score workspace begin, so work, workspace traffic and splits follow W, not the row's length.
// MFMA roles as in mi355q_attention.hip (v_mfma_f32_16x16x32_bf16, the queries are the 16 columns): a lane's own values of the score
// tiles 2 s, 2 s + 1 are the slots of its P fragment, and vq is stored with the same slot order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mi355q.h"
#include "mi355q_internal.h"
#include "mi355q_quant_dev.h"
#include "mi355q_attn_dev.h"
#include "mi355q_decode.h"
#include "mi355q_decode_dev.h"

namespace mi355q {

// ---- append ---------------------------------------------------------------------------------------------------------------
struct AppendArgs {
    KvCache c;
    const float* k;
    const float* v;
    long long ksb, kst, vsb, vst;
    long long L, n, t0, t1;     // key tiles touched: t0 = L / 16 .. t1 = (L + n - 1) / 16
    int kblocks;
    const int32_t* lengths;     // ragged (RG): row b's L = lengths[b], its n = counts[b] (NULL: n) <= n; t0, t1 follow in the kernel
    const int32_t* counts;
    KvPages pg;                 // paged cache (PG): c.kq / c.vq are the pools, c.C = max_pages * P; else zeros
};

// one block of 16 values x with maximum bmax, quantised: value e is the low halfword of a lane's slot, 8 halfwords apart in kq
// (the 16 keys of a tile at one d) and in vq (the 16 d of one key) alike
__device__ __forceinline__ void kv_store_block(uint16_t* __restrict__ dst, const float (&x)[16], float bmax, const QuantArgs& a) {
    const int mbits = (int)__builtin_log2f(a.shift);
    const int p = at_block_exponent_mem(bmax, a);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const float q = bmax != 0.f ? at_quant(x[e], mbits - p, p - mbits, a.mant_max) + 0.0f : 0.f;   // (+ 0: see the layout note)
        dst[e * 8] = (uint16_t)(pack_bf16(q, 0.f) & 0xFFFFu);
    }
}

template <bool RG, bool PG>
__global__ __launch_bounds__(256) void kv_append_kernel(const QuantArgs ak, const QuantArgs av, const AppendArgs a) {
    const int tid = threadIdx.x, D = a.c.D;
    const long long b = blockIdx.y, NTC = a.c.C >> 4, NPC = (a.c.C + 31) >> 5;
    long long L = a.L, n = a.n, t0 = a.t0, t1 = a.t1;
    if constexpr (RG) {
        if (!append_row(a, b, L, n)) return;
        t0 = L >> 4;
        t1 = (L + n - 1) >> 4;
    }
    if ((int)blockIdx.x < a.kblocks) {
        // K: thread (tile, d) walks the 16 keys of its block: staged rows in front of L, new rows, zeros behind L + n
        const int per = 256 / D, sub = tid / D, d = tid - sub * D;
        const long long t = t0 + (long long)blockIdx.x * per + sub;
        if (sub >= per || t > t1) return;
        if constexpr (RG) {
            if (t >= NTC) return;                              // (keys behind the capacity are dropped, whatever the host vouched for)
        }
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
        // the open tile's rows for the next append, when the tile that reads staged rows is the one that writes them (the usual
        // decode step); an append that runs into a later tile leaves them to kv_stage_kernel, behind this launch
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
        kv_store_block(a.c.kq + (pt * (D >> 5) + c) * 512 + 16 * g * 8 + j, x, bmax, ak);
    } else {
        // V: thread (new key, 16-d block) quantises one block
        const int DT = D >> 4;
        const long long item = ((long long)blockIdx.x - a.kblocks) * 256 + tid;
        if (item >= a.n * DT) return;
        const long long kl = item / DT, key = L + kl;
        const int dt = (int)(item - kl * DT);
        if constexpr (RG) {
            if (kl >= n || key >= a.c.C) return;               // (input rows behind the row's count are padding: never read)
        }
        float x[16];
        const float bmax = append_v_block(a, b, kl, dt, x);
        const long long s = key >> 5;
        const int h = (int)(key >> 4) & 1, g = (int)(key & 15) >> 2, j = 4 * h + (int)(key & 3);
        long long ps = b * NPC + s;
        if constexpr (PG) ps = pg_place(a.pg, pg_raw(a.pg, b, s >> (a.pg.lg_p - 5)), s, a.pg.lg_p - 5);     // (key < C: inside the table's row)
        kv_store_block(a.c.vq + (ps * DT + dt) * 512 + 16 * g * 8 + j, x, bmax, av);
    }
}

// the new open tile's fp32 rows -> staging, for an append that crossed a tile boundary: they overlap the rows tile t0 of
// kv_append_kernel reads, so they are written behind it.  grid (rows, B), D threads.
template <bool RG>
__global__ void kv_stage_kernel(const AppendArgs a) {
    const long long b = blockIdx.y;
    long long L = a.L, n = a.n, t1 = a.t1;
    if constexpr (RG) {
        // grid: the most rows any row can have open; this row's own crossing and open rows decide
        if (!append_row(a, b, L, n)) return;
        t1 = (L + n - 1) >> 4;
        if (t1 <= (L >> 4) || (long long)blockIdx.x >= ((L + n) & 15) || t1 >= (a.c.C >> 4)) return;
    }
    const long long key = t1 * 16 + blockIdx.x;                        // (>= L: tile t1 lies behind tile t0 = L / 16)
    a.c.stage[(b * 16 + blockIdx.x) * a.c.D + threadIdx.x] = a.k[b * a.ksb + (key - L) * a.kst + threadIdx.x];
}

int launch_kv_append(const KvCache& c, const QuantArgs& ak, const QuantArgs& av, const float* k, const float* v, long long ksb,
                     long long kst, long long vsb, long long vst, long long L, long long n, hipStream_t st) {
    AppendArgs a{};
    a.c = c; a.k = k; a.v = v;
    a.ksb = ksb; a.kst = kst; a.vsb = vsb; a.vst = vst;
    a.L = L; a.n = n; a.t0 = L / 16; a.t1 = (L + n - 1) / 16;
    const int per = 256 / c.D;
    const long long kblocks = (a.t1 - a.t0 + 1 + per - 1) / per, vblocks = (n * (c.D / 16) + 255) / 256;
    if (kblocks + vblocks > 0x7FFFFFFFLL) return MI355Q_E_UNSUPPORTED;
    a.kblocks = (int)kblocks;
    hipLaunchKernelGGL((kv_append_kernel<false, false>), dim3((unsigned)(kblocks + vblocks), (unsigned)c.B), dim3(256), 0, st, ak, av, a);
    const unsigned open_rows = (unsigned)((L + n) % 16);                // (0: tile t1 is full, nothing to stage)
    if (a.t1 > a.t0 && open_rows) hipLaunchKernelGGL(kv_stage_kernel<false>, dim3(open_rows, (unsigned)c.B), dim3(c.D), 0, st, a);
    return (int)hipGetLastError();
}

// Grids from n alone: n keys touch at most (n + 14) / 16 + 1 tiles wherever they start, and an append that crosses a tile edge
// leaves at most min(n - 1, 15) rows open (one key at least lies in tile t0).  The staging pass stays a second launch: tile t1's
// rows overwrite the staged rows that tile t0's threads of the same row read.  n == 1, the decode step, never crosses.
int append_ragged_grid(long long B, int D, long long n, int& kblocks_out, dim3& grid) {
    const int per = 256 / D;
    const long long kblocks = ((n + 14) / 16 + 1 + per - 1) / per, vblocks = (n * (D / 16) + 255) / 256;
    if (kblocks + vblocks > 0x7FFFFFFFLL) return MI355Q_E_UNSUPPORTED;
    kblocks_out = (int)kblocks;
    grid = dim3((unsigned)(kblocks + vblocks), (unsigned)B);
    return 0;
}

int launch_kv_append_ragged(const KvCache& c, const QuantArgs& ak, const QuantArgs& av, const float* k, const float* v, long long ksb,
                            long long kst, long long vsb, long long vst, const int32_t* lengths, const int32_t* counts, long long n,
                            hipStream_t st, const KvPages* pages) {
    AppendArgs a{};
    a.c = c; a.k = k; a.v = v;
    a.ksb = ksb; a.kst = kst; a.vsb = vsb; a.vst = vst;
    a.n = n; a.lengths = lengths; a.counts = counts;
    dim3 grid;
    if (const int rc = append_ragged_grid(c.B, c.D, n, a.kblocks, grid)) return rc;
    if (pages) {
        a.pg = *pages;
        hipLaunchKernelGGL((kv_append_kernel<true, true>), grid, dim3(256), 0, st, ak, av, a);
    } else {
        hipLaunchKernelGGL((kv_append_kernel<true, false>), grid, dim3(256), 0, st, ak, av, a);
    }
    launch_kv_stage_ragged(c, k, ksb, kst, lengths, counts, n, st);
    return (int)hipGetLastError();
}

// the staging pass alone, for a cache that keeps its quantised values elsewhere (mi355q_kvp.hip): stage, B, C and D are all it reads of c
void launch_kv_stage_ragged(const KvCache& c, const float* k, long long ksb, long long kst, const int32_t* lengths, const int32_t* counts,
                            long long n, hipStream_t st) {
    AppendArgs a{};
    a.c = c; a.k = k; a.ksb = ksb; a.kst = kst;
    a.n = n; a.lengths = lengths; a.counts = counts;
    if (n > 1) hipLaunchKernelGGL(kv_stage_kernel<true>, dim3((unsigned)(n - 1 < 15 ? n - 1 : 15), (unsigned)c.B), dim3(c.D), 0, st, a);
}

template <bool RG, bool PG>
__device__ __forceinline__ void kv_decode_fp32_body(const KvCache& c, float* __restrict__ k_out, float* __restrict__ v_out, long long L,
                                                    const int32_t* __restrict__ lengths, const KvPages& pg) {
    const int D = c.D;
    const long long b = blockIdx.y, NTC = c.C >> 4, NPC = (c.C + 31) >> 5;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= L * D) return;
    const long long key = idx / D;
    const int d = (int)(idx - key * D);
    if constexpr (RG) {
        if (key >= __builtin_amdgcn_readfirstlane(lengths[b])) {      // (L = max_length <= C: zeros behind the row's own length)
            k_out[(b * L + key) * D + d] = 0.f;
            v_out[(b * L + key) * D + d] = 0.f;
            return;
        }
    }
    if constexpr (PG) {                                               // (key < lengths[b], key < L <= C: a page of the row's)
        const int raw = pg_raw(pg, b, key >> pg.lg_p), h = (int)(key >> 4) & 1, g = (int)(key & 15) >> 2, j = 4 * h + (int)(key & 3);
        const long long pt = pg_place(pg, raw, key >> 4, pg.lg_p - 4), ps = pg_place(pg, raw, key >> 5, pg.lg_p - 5);
        const uint16_t kb = c.kq[(pt * (D >> 5) + (d >> 5)) * 512 + ((key & 15) + 16 * ((d >> 3) & 3)) * 8 + (d & 7)];
        const uint16_t vb = c.vq[(ps * (D >> 4) + (d >> 4)) * 512 + ((d & 15) + 16 * g) * 8 + j];
        k_out[(b * L + key) * D + d] = __uint_as_float((unsigned)kb << 16);
        v_out[(b * L + key) * D + d] = __uint_as_float((unsigned)vb << 16);
        return;
    }
    const uint16_t kb = c.kq[((b * NTC + (key >> 4)) * (D >> 5) + (d >> 5)) * 512 + ((key & 15) + 16 * ((d >> 3) & 3)) * 8 + (d & 7)];
    const int h = (int)(key >> 4) & 1, g = (int)(key & 15) >> 2, j = 4 * h + (int)(key & 3);
    const uint16_t vb = c.vq[((b * NPC + (key >> 5)) * (D >> 4) + (d >> 4)) * 512 + ((d & 15) + 16 * g) * 8 + j];
    k_out[(b * L + key) * D + d] = __uint_as_float((unsigned)kb << 16);
    v_out[(b * L + key) * D + d] = __uint_as_float((unsigned)vb << 16);
}

// (two entry points, one body: the unpaged kernels keep their argument list, and with it the code they had before there were pages)
template <bool RG>
__global__ __launch_bounds__(256) void kv_decode_fp32_kernel(const KvCache c, float* __restrict__ k_out, float* __restrict__ v_out,
                                                             long long L, const int32_t* __restrict__ lengths) {
    kv_decode_fp32_body<RG, false>(c, k_out, v_out, L, lengths, KvPages{});
}
__global__ __launch_bounds__(256) void kv_decode_fp32_paged_kernel(const KvCache c, float* __restrict__ k_out, float* __restrict__ v_out,
                                                                   long long L, const int32_t* __restrict__ lengths, const KvPages pg) {
    kv_decode_fp32_body<true, true>(c, k_out, v_out, L, lengths, pg);
}

int launch_kv_decode_fp32(const KvCache& c, float* k_out, float* v_out, long long L, hipStream_t st, const int32_t* lengths,
                          const KvPages* pages) {
    const long long blocks = (L * c.D + 255) / 256;
    if (blocks > 0x7FFFFFFFLL) return MI355Q_E_UNSUPPORTED;
    const dim3 grid((unsigned)blocks, (unsigned)c.B);
    if (pages && !lengths) return MI355Q_E_BADARG;
    if (pages) hipLaunchKernelGGL(kv_decode_fp32_paged_kernel, grid, dim3(256), 0, st, c, k_out, v_out, L, lengths, *pages);
    else if (lengths) hipLaunchKernelGGL(kv_decode_fp32_kernel<true>, grid, dim3(256), 0, st, c, k_out, v_out, L, lengths);
    else hipLaunchKernelGGL(kv_decode_fp32_kernel<false>, grid, dim3(256), 0, st, c, k_out, v_out, L, lengths);
    return (int)hipGetLastError();
}

// ---- decode ---------------------------------------------------------------------------------------------------------------
int decode_splits(long long B, long long L, long long D, int override) {
    (void)D;                            // (part of the exported signature -- ops.decode_splits, the workspace size -- though no rule uses it)
    if (B < 1 || L < 1) return 1;
    const long long NP = (L + 31) / 32;
    // enough workgroups for two a compute unit (256 of them) at at least two key pairs each; never more than 64 statistics to combine
    long long want = override > 0 ? override : (512 + B - 1) / B;
    if (override <= 0 && want > NP / 2) want = NP / 2;
    if (want > 64) want = 64;
    if (want > NP) want = NP;
    if (want < 1) want = 1;
    const long long pps = (NP + want - 1) / want;
    return (int)((NP + pps - 1) / pps);
}

long long decode_window_span(long long M, long long L, long long window) {
    // keys 32 p0 .. L_b - 1 with 32 p0 > L_b - M - W + 1 - 32: fewer than W + M - 1 + 32 of them, and never more than the row has
    return window > 0 && window < L && window + M - 1 + 31 < L ? window + M - 1 + 31 : L;
}

size_t decode_workspace_bytes(long long B, long long L, long long D, int splits) {
    if (B <= 0 || L <= 0 || D <= 0) return 0;
    const long long S = decode_splits(B, L, D, splits), NT = (L + 15) / 16;
    return (size_t)(B * NT * 256 + B * S * 32 + B * S * (D / 16) * 256) * 4;
}

// Sliding window: the first key this lane's query sees (kvis its horizon), and the row's first visible pair and tile -- the first key
// ANY of the row's M queries sees is max(0, L - M - W + 1), that of query 0 (scalar: L is).  An empty row (L = 0) gives 0.
__device__ __forceinline__ long long dec_window_lo(const DecodeArgs& g, long long kvis) { return max(kvis - g.W + 1, 0ll); }
__device__ __forceinline__ long long dec_window_first(const DecodeArgs& g, long long L) { return max(L - g.M - g.W + 1, 0ll); }

template <int DC, bool RG, bool GQ, bool PG, bool WN = false>
__global__ __launch_bounds__(256) void decode_scores_kernel(const QuantArgs aq, const DecodeArgs g) {
    static_assert(RG || !WN, "windowed launches exist in the ragged form only");
    __shared__ float sm_[4][64], sl_[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, lg = lane >> 4;
    const long long b = blockIdx.y, s = blockIdx.x, cb = dec_cache_row<GQ>(g, b);   // b: launch row (workspace), cb: cache row
    const long long L = dec_length<RG>(g, cb), NT = RG ? (L + 15) >> 4 : g.NT;
    // windowed: the partition starts at the row's first visible pair p0 (t0 = 2 p0 its first tile; the workspace holds tile t at t - t0),
    // and the tiles below t_first, the tile of the first visible key -- tile t0 when the lower edge lies in the pair's second tile -- are
    // not read: no query of the row sees a key of theirs
    long long t0 = 0, t_first = 0;
    if constexpr (WN) {
        t_first = dec_window_first(g, L) >> 4;
        t0 = t_first & ~1ll;
    }
    if constexpr (RG) {
        if (t0 + 2 * g.pps * s >= NT) { // a split wholly behind the row's last tile: the empty statistics, no kq read
            dec_stats_empty(g, b, s, tid);
            return;
        }
    }
    long long row, qrow;
    dec_column<GQ>(g, b, c16, row, qrow);
    bf16x8 qf[DC];                      // quantised in registers
    at_quant_q_frag(qf, g.q + row * g.qsb + qrow * g.qsm, g.q_scale, lg, aq, at_block_exponent_mem);
    const long long kvis = dec_horizon(g, L, qrow);
    // windowed: key k is visible when klo <= k <= kvis -- one unsigned compare of k - klo against kvis - klo, in 32 bits (keys < 2^31);
    // a column whose window begins behind this split leaves it with (-inf, 0)
    int lane_rel = 0;
    unsigned wd = 0;
    if constexpr (WN) {
        const long long klo = dec_window_lo(g, kvis);
        lane_rel = (int)(4 * lg - klo);
        wd = (unsigned)(kvis - klo);
    }
    auto visible = [&](long long t, long long key0, int e) -> bool {
        if constexpr (WN) return (unsigned)((int)(t << 4) + lane_rel + e) <= wd;
        else return key0 + e <= kvis;
    };
    const float scale_inv = g.scale_div != 0.f ? 1.0f / g.scale_div : 0.f;
    const long long t_lo = t0 + 2 * g.pps * s, t_hi = min(NT, t_lo + 2 * g.pps);
    const uint16_t* __restrict__ kfb = g.kq + (PG ? 0 : cb * g.NTC * DC * 512) + lane * 8;
    float* __restrict__ sc = g.scores + b * g.NT * 256 + lane * 4 - t0 * 256;
    long long t_begin = t_lo + wave;    // (windowed: the wave that would take a tile below t_first -- only tile t0 can be one -- moves on)
    if constexpr (WN) {
        if (t_begin < t_first) t_begin += 4;
    }
    // running (max, sum of exp(x - max)) of this lane's visible scores, re-based when the maximum moves
    float m_run = -INFINITY, l_run = 0.f;
    // paged: the table entry of the NEXT tile this wave takes is asked for while this one's fragments are loaded (t < t_hi <= NT)
    int raw = 0;
    if constexpr (PG) {
        if (t_begin < t_hi) raw = pg_raw(g.pg, cb, t_begin >> (g.pg.lg_p - 4));
    }
    for (long long t = t_begin; t < t_hi; t += 4) {
        long long pt = t;                                   // the tile's place in kq; the workspace keeps t
        if constexpr (PG) {
            pt = pg_place(g.pg, __builtin_amdgcn_readfirstlane(raw), t, g.pg.lg_p - 4);
            if (t + 4 < t_hi) raw = pg_raw(g.pg, cb, (t + 4) >> (g.pg.lg_p - 4));
        }
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < DC; ++c)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(kfb + (pt * DC + c) * 512), qf[c], acc, 0, 0, 0);
        if (g.scale_div != 0.f) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = at_div(acc[e], g.scale_div, scale_inv);
        }
        *reinterpret_cast<float4*>(sc + t * 256) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        const long long key0 = t * 16 + 4 * lg;
        float tm = -INFINITY;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (visible(t, key0, e)) tm = fmaxf(tm, acc[e]);
        if (tm > m_run) {
            l_run = m_run == -INFINITY ? 0.f : l_run * at_exp_neg(m_run - tm);
            m_run = tm;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (visible(t, key0, e)) l_run += at_exp_neg(acc[e] - m_run);
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

template <int DC, bool RG, bool GQ, bool PG, bool WN = false>
__global__ __launch_bounds__(256) void decode_pv_kernel(const QuantArgs ap, const DecodeArgs g) {
    static_assert(RG || !WN, "windowed launches exist in the ragged form only");
    constexpr int DT = DC * 2;
    __shared__ f32x4 red[4][DT][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, lg = lane >> 4;
    const long long b = blockIdx.y, s = blockIdx.x, cb = dec_cache_row<GQ>(g, b);
    const long long L = dec_length<RG>(g, cb), NT = RG ? (L + 15) >> 4 : g.NT, NP = RG ? (L + 31) >> 5 : g.NP;
    long long t_first = 0;              // windowed: the tile of the row's first visible key, p0 = t_first / 2 its pair (decode_scores_kernel)
    if constexpr (WN) t_first = dec_window_first(g, L) >> 4;
    const long long p0 = t_first >> 1;
    const long long p_lo = p0 + g.pps * s, p_hi = min(NP, p_lo + g.pps);
    if constexpr (RG) {
        if (p_lo >= p_hi) {             // an empty split (every split of an empty row): a zero partial output, no vq read
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
    }
    long long row, qrow;
    dec_column<GQ>(g, b, c16, row, qrow);
    const long long kvis = dec_horizon(g, L, qrow);
    int lane_rel = 0;                   // (windowed: the visibility test of decode_scores_kernel)
    unsigned wd = 0;
    if constexpr (WN) {
        const long long klo = dec_window_lo(g, kvis);
        lane_rel = (int)(4 * lg - klo);
        wd = (unsigned)(kvis - klo);
    }
    auto visible = [&](long long t, long long key0, int e) -> bool {
        if constexpr (WN) return (unsigned)((int)(t << 4) + lane_rel + e) <= wd;
        else return key0 + e <= kvis;
    };
    // the row's statistics over all L keys: the S splits in split order (every query sees its own key: some split's max is finite.
    // Unwindowed that is the first split, which holds key 0; windowed a column's window can begin behind the first split, which then
    // holds (-inf, 0) for it.  Such a split, like those behind a ragged row's last tile, is skipped)
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
    const float* __restrict__ sc = g.scores + b * g.NT * 256 + lane * 4 - 2 * p0 * 256;
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    int raw = 0;                                            // (paged: one pair ahead, as in decode_scores_kernel; pr_i < p_hi <= NP)
    if constexpr (PG) {
        if (p_lo + wave < p_hi) raw = pg_raw(g.pg, cb, (p_lo + wave) >> (g.pg.lg_p - 5));
    }
    for (long long pr_i = p_lo + wave; pr_i < p_hi; pr_i += 4) {
        long long pp = pr_i;                                // the pair's place in vq; scores and horizon keep pr_i
        if constexpr (PG) {
            pp = pg_place(g.pg, __builtin_amdgcn_readfirstlane(raw), pr_i, g.pg.lg_p - 5);
            if (pr_i + 4 < p_hi) raw = pg_raw(g.pg, cb, (pr_i + 4) >> (g.pg.lg_p - 5));
        }
        uint4 vb[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) vb[dt] = *reinterpret_cast<const uint4*>(vfb + (pp * DT + dt) * 512);
        float pq[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const long long t = 2 * pr_i + h;                  // (uniform over the wave; the last pair's second tile may not exist)
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < NT && (!WN || t >= t_first)) x = *reinterpret_cast<const float4*>(sc + t * 256);   // (a tile below t_first has no scores)
            const float xs[4] = {x.x, x.y, x.z, x.w};
            const long long key0 = t * 16 + 4 * lg;
            float pr[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) pr[e] = (t < NT && visible(t, key0, e)) ? at_div(at_exp_neg(xs[e] - row_max), row_sum, row_inv) : 0.f;
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

template <bool GQ>
__global__ __launch_bounds__(256) void decode_sum_kernel(const DecodeArgs g) {
    const int DT = g.D >> 4;
    const long long b = blockIdx.x;
    for (int item = threadIdx.x; item < DT * 64; item += 256) {
        const int dt = item >> 6, lane = item & 63, c16 = lane & 15, lg = lane >> 4;
        const float* __restrict__ pp = g.part + ((b * g.S * DT + dt) * 64 + lane) * 4;
        float4 sum = *reinterpret_cast<const float4*>(pp);
        for (int s = 1; s < g.S; ++s) {
            const float4 x = *reinterpret_cast<const float4*>(pp + (long long)s * DT * 256);
            sum.x += x.x; sum.y += x.y; sum.z += x.z; sum.w += x.w;
        }
        if (dec_real<GQ>(g, c16)) *reinterpret_cast<float4*>(dec_out<GQ>(g, b, c16) + 16 * dt + 4 * lg) = sum;
    }
}

int decode_group_width(long long G, long long M) {
    if (G < 1 || M < 1 || M > 16) return 0;
    for (long long gw = G < 16 / M ? G : 16 / M; gw > 1; --gw)
        if (G % gw == 0) return (int)gw;
    return 1;
}

int decode_args_fill(DecodeArgs& g, long long B, long long C, int D, long long M, long long L, long long span, int G, int splits,
                     const long long* strides, void* workspace, const KvPages* pages, long long& rows) {
    if (pages) g.pg = *pages;
    g.M = M; g.L = L; g.D = D;
    g.NT = (span + 15) / 16; g.NP = (span + 31) / 32; g.NTC = C / 16; g.NPC = (C + 31) / 32;
    g.gw = G ? decode_group_width(G, M) : 1;
    if (g.gw < 1) return MI355Q_E_BADARG;
    g.rpc = G ? G / g.gw : 1;
    rows = B * g.rpc;                                       // launch rows: the workspace's and the grid's
    if (rows > 65535) return MI355Q_E_UNSUPPORTED;
    g.S = decode_splits(rows, span, D, splits);
    g.pps = (int)((g.NP + g.S - 1) / g.S);
    fill_qo_strides(g, strides, M, D);
    g.scores = static_cast<float*>(workspace);
    g.stats = g.scores + rows * g.NT * 256;
    g.part = g.stats + rows * g.S * 32;
    return 0;
}

// G == 0: one query row a cache row, the GQ = false kernels.  G >= 1: the grouped kernels over c.B * rpc launch rows.
int launch_bfp_attention_decode(const QuantArgs& aq, const QuantArgs& ap, const KvCache& c, const float* q, float* out,
                                void* workspace, long long M, long long L, int causal, float q_scale, float scale_div,
                                const long long* strides, int splits, hipStream_t st, const int32_t* lengths, int G, const KvPages* pages,
                                long long window) {
    if ((pages || window) && !lengths) return MI355Q_E_BADARG;      // (no uniform paged or windowed launch)
    if (window < 0 || (window && !causal)) return MI355Q_E_BADARG;
    // windowed: partition, default splits and workspace strides are those of `span` keys, the most a row's queries can touch
    const long long span = window ? decode_window_span(M, L, window) : L;
    DecodeArgs g{};
    long long rows;
    if (const int rc = decode_args_fill(g, c.B, c.C, c.D, M, L, span, G, splits, strides, workspace, pages, rows)) return rc;
    g.W = window;
    g.q = q; g.kq = c.kq; g.vq = c.vq; g.out = out; g.lengths = lengths;
    g.causal = causal; g.q_scale = q_scale; g.scale_div = scale_div;
    const dim3 grid((unsigned)g.S, (unsigned)rows);
#define MI355Q_DECODE_GO2(DC_, RG_, GQ_, PG_, ...)                                                                  \
    hipLaunchKernelGGL((decode_scores_kernel<DC_, RG_, GQ_, PG_, ##__VA_ARGS__>), grid, dim3(256), 0, st, aq, g);    \
    hipLaunchKernelGGL((decode_pv_kernel<DC_, RG_, GQ_, PG_, ##__VA_ARGS__>), grid, dim3(256), 0, st, ap, g);
#define MI355Q_DECODE_GO(DC_)                                                                         \
    if (window) {                                                                                     \
        if (pages) {                                                                                  \
            if (G) { MI355Q_DECODE_GO2(DC_, true, true, true, true) } else { MI355Q_DECODE_GO2(DC_, true, false, true, true) }     \
        } else {                                                                                      \
            if (G) { MI355Q_DECODE_GO2(DC_, true, true, false, true) } else { MI355Q_DECODE_GO2(DC_, true, false, false, true) }   \
        }                                                                                             \
    } else if (pages) {                                                                                      \
        if (G) { MI355Q_DECODE_GO2(DC_, true, true, true) } else { MI355Q_DECODE_GO2(DC_, true, false, true) }             \
    } else if (G) {                                                                                   \
        if (lengths) { MI355Q_DECODE_GO2(DC_, true, true, false) } else { MI355Q_DECODE_GO2(DC_, false, true, false) }     \
    } else {                                                                                          \
        if (lengths) { MI355Q_DECODE_GO2(DC_, true, false, false) } else { MI355Q_DECODE_GO2(DC_, false, false, false) }   \
    }
    switch (c.D / 32) {
        case 1: MI355Q_DECODE_GO(1); break;
        case 2: MI355Q_DECODE_GO(2); break;
        case 3: MI355Q_DECODE_GO(3); break;
        case 4: MI355Q_DECODE_GO(4); break;
        default: return MI355Q_E_UNSUPPORTED;
    }
#undef MI355Q_DECODE_GO
#undef MI355Q_DECODE_GO2
    launch_decode_sum(g, G != 0, rows, st);
    return (int)hipGetLastError();
}

void launch_decode_sum(const DecodeArgs& g, bool grouped, long long rows, hipStream_t st) {
    if (g.S <= 1) return;
    if (grouped) hipLaunchKernelGGL(decode_sum_kernel<true>, dim3((unsigned)rows), dim3(256), 0, st, g);
    else hipLaunchKernelGGL(decode_sum_kernel<false>, dim3((unsigned)rows), dim3(256), 0, st, g);
}

}  // namespace mi355q
