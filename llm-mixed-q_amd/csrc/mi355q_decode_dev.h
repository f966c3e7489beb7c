// Device code the kernels of mi355q_decode.hip (bf16 cache) and mi355q_kvp.hip (mantissa caches) share, one copy of each: a ragged
// row's (length, count) of an append and the V walk that gathers a block, a paged cache's table lookup, what a lane of the split-key
// decode kernels knows of its column -- horizon, length, the grouped column map -- and the empty split's statistics.  All force-inlined,
// and only what leaves every kernel's instruction text as it was with the code in place (profiles/decode_shared_isa.txt, which also
// names the blocks the two files still hold twice because a helper moved the text).  Layout notes: mi355q_decode.h.
#ifndef MI355Q_DECODE_DEV_H
#define MI355Q_DECODE_DEV_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mi355q_decode.h"

namespace mi355q {

// row b's (L, n) of a ragged append, scalar; false: nothing to do (negative values are taken as 0, a count above n as n)
// (Args: lengths, counts -- NULL: n -- and n, the host's number of input rows)
template <class Args>
__device__ __forceinline__ bool append_row(const Args& a, long long b, long long& L, long long& n) {
    L = max(__builtin_amdgcn_readfirstlane(a.lengths[b]), 0);
    if (a.counts) n = min((long long)max(__builtin_amdgcn_readfirstlane(a.counts[b]), 0), a.n);
    return n > 0;
}

// V of an append: thread (new key kl of the row, 16-d block dt) takes one block
template <class Args>
__device__ __forceinline__ float append_v_block(const Args& a, long long b, long long kl, int dt, float (&x)[16]) {
    float bmax = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 f = *reinterpret_cast<const float4*>(a.v + b * a.vsb + kl * a.vst + dt * 16 + 4 * i);
        x[4 * i] = f.x; x[4 * i + 1] = f.y; x[4 * i + 2] = f.z; x[4 * i + 3] = f.w;
        bmax = fmaxf(bmax, fmaxf(fmaxf(fabsf(f.x), fabsf(f.y)), fmaxf(fabsf(f.z), fabsf(f.w))));
    }
    return bmax;
}

// Paged cache: the table entry of row b's logical page i as loaded (pg_raw: i must be a page that holds keys of the row), and the
// physical tile (sh = lg_p - 4) or pair (sh = lg_p - 5) of logical tile / pair t from it -- the page id clamped into the pool first.
__device__ __forceinline__ int pg_raw(const KvPages& p, long long b, long long i) { return p.table[b * p.max_pages + i]; }
__device__ __forceinline__ long long pg_place(const KvPages& p, int raw, long long t, int sh) {
    const long long page = min(max(raw, 0), p.num_pages - 1);
    return (page << sh) + (t & ((1ll << sh) - 1));
}

// this lane's horizon: the last key its query (column c16 of the MFMA tiles) sees
__device__ __forceinline__ long long dec_horizon(const DecodeArgs& g, long long L, long long qrow) {
    return g.causal ? L - g.M + qrow : L - 1;
}

// the keys row b holds.  Ragged: its own length, one scalar load a workgroup, never above max_length (= g.L: the partition and the
// workspace strides are made for that); a row shorter than its M queries -- an empty slot, a finished sequence -- counts as 0
// keys: every split of it is empty and its output is zeros.
template <bool RG>
__device__ __forceinline__ long long dec_length(const DecodeArgs& g, long long b) {
    if constexpr (RG) {
        const long long L = min((long long)max(__builtin_amdgcn_readfirstlane(g.lengths[b]), 0), g.L);
        return L < g.M ? 0 : L;
    } else {
        return g.L;
    }
}

// Column c16 of the MFMA tiles -> (query row of q / out, query).  GQ = false: row y, query min(c16, M - 1).  GQ = true: launch row y
// serves the gw query rows y gw .. y gw + gw - 1, column c16 < gw M is head c16 / M, query c16 % M; the columns behind repeat the
// last real one (and store nothing: dec_real).
template <bool GQ>
__device__ __forceinline__ void dec_column(const DecodeArgs& g, long long y, int c16, long long& row, long long& qrow) {
    if constexpr (GQ) {
        const int M = (int)g.M, col = min(c16, g.gw * M - 1), h = col / M;
        row = y * g.gw + h;
        qrow = col - h * M;
    } else {
        row = y;
        qrow = min((long long)c16, g.M - 1);
    }
}
template <bool GQ>
__device__ __forceinline__ bool dec_real(const DecodeArgs& g, int c16) {
    if constexpr (GQ) return c16 < g.gw * (int)g.M;
    else return c16 < g.M;
}
// where a REAL column c16 of launch row y stores its output row
template <bool GQ>
__device__ __forceinline__ float* dec_out(const DecodeArgs& g, long long y, int c16) {
    if constexpr (GQ) {
        long long row, qrow;
        dec_column<true>(g, y, c16, row, qrow);
        return g.out + row * g.osb + qrow * g.osm;
    } else {
        return g.out + y * g.osb + c16 * g.osm;
    }
}
// the cache row of launch row y (scalar)
template <bool GQ>
__device__ __forceinline__ long long dec_cache_row(const DecodeArgs& g, long long y) {
    if constexpr (GQ) return (long long)((unsigned)y / (unsigned)g.rpc);
    else return y;
}

// phase A, a split wholly behind the row's last tile: the empty statistics
__device__ __forceinline__ void dec_stats_empty(const DecodeArgs& g, long long b, long long s, int tid) {
    if (tid < 16) {
        float* st = g.stats + ((b * g.S + s) * 16 + tid) * 2;
        st[0] = -INFINITY;
        st[1] = 0.f;
    }
}

}  // namespace mi355q
#endif
