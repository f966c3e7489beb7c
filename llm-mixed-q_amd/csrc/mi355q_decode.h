// Incremental decoding (mi355q_decode.hip): the block_fp KV cache and the split-key decode attention, what the C-ABI wrapper
// needs of them.
//
// Cache layout, per b = batch x head, capacity C keys (C % 16 == 0), head_dim D (D % 32 == 0, D <= 128); all quantised values
// are bf16 (exact for widths <= 9) and sit in the order the decode kernels' MFMA operands want them, 16 bytes a lane:
//   kq    [B][C / 16][D / 32][64 lanes][8]   Qb(k^T): piece (b, key tile t, chunk c) = 1 KiB; lane (key 16 t + lane % 16,
//                                            g = lane / 16) holds d = 32 c + 8 g .. + 7.  A [1,16] block of k^T is the 16 keys of
//                                            a tile at one d: keys the cache does not hold yet are the blocking's zero padding
//                                            (stored as zeros, outside the block maximum).
//   vq    [B][ceil(C / 32)][D / 16][64][8]   Qd(v): piece (b, key pair s = 32 keys, dt) = 1 KiB; lane (d = 16 dt + lane % 16,
//                                            g = lane / 16) holds slot j <-> key 32 s + 16 (j / 4) + 4 g + (j & 3).  A block is
//                                            16 d of one key: final once written.  The storage starts out ZEROED (a slot that no
//                                            key has reached meets a probability of exactly 0, and must be finite).
//   stage [B][16][D] fp32                    the rows of the OPEN key tile (L % 16 keys): a block of 16 keys is final only once
//                                            it is full, until then every append re-quantises it from these rows.
// Values are those of attn_pack_k / attn_pack_v (|x| <= 1e-8 passes through, rounded to bf16) with ONE difference: a zero is
// always stored as +0.  A negative value whose mantissa rounds to 0 is -0 in the prefill fragments (copysign) and +0 in the
// oracle's block_fp_quantize (its mantissas are integers); the products cannot tell, the bit-for-bit cache tests can.
// (mi355q_kvp.h: the same cache with each value as a mantissa byte plus one exponent byte a block, 17/32 of these bytes; its one
// further difference -- 0 < |x| <= 1e-8, stored here rounded to bf16, is stored there as 0 -- is noted next to its layout.)
// The length L lives on the host: an append at L writes keys L .. L + n - 1, a decode at L reads keys 0 .. L - 1.
//
// Ragged batches (the *_ragged launches): every cache row b has its own length, lengths[b] in a DEVICE int32 array [B] that the
// kernels read (once a workgroup, kept scalar) in place of the host's L; the host passes only upper bounds, which size grids and
// the workspace and never decide what is addressed:
//   append   row b takes counts[b] (device int32 [B]; NULL: n) of the n input rows as keys lengths[b] .. lengths[b] + counts[b] - 1:
//            lengths holds the lengths BEFORE the append.  The open-tile logic above runs per row (t0, t1 and the open rows come
//            from lengths[b], counts[b]); counts[b] == 0 leaves the row's kq, vq and stage untouched; a key index >= C is dropped.
//   decode   row b sees keys 0 .. lengths[b] - 1, its M queries are its last M positions: lengths holds the lengths INCLUDING
//            the queries' own keys.  lengths[b] is clamped to max_length; a row with lengths[b] < M yields zeros.  The split
//            partition comes from max_length: a split behind a row's last tile writes (-inf, 0) statistics and a zero partial
//            output and reads no kq / vq.  The scores workspace keeps the stride of NT(max_length) tiles a row.
// A row decodes as if it were alone: nothing another row holds (or a pad key would be) enters its blocks' shared exponents.
//
// Grouped queries (GQ = true kernels): a cache row (batch x KV head) is shared by G query heads, q / out hold B * G rows and query
// row r attends to cache row r / G.  The 16 MFMA columns one query head fills with M queries take gw heads, gw = the largest
// divisor of G with gw * M <= 16 (decode_group_width), and a cache row is served by rpc = G / gw LAUNCH ROWS:
//   launch row y = 0 .. B * rpc - 1   reads cache row y / rpc (kq, vq, lengths[y / rpc]) and serves query rows y gw .. y gw + gw - 1
//   column c16 < gw * M               head h = c16 / M, query c16 % M: Q fragment from q + (y gw + h) qsb + (c16 % M) qsm, output to
//                                     out + (y gw + h) osb + (c16 % M) osm, horizon that of query c16 % M
//   columns >= gw * M                 repeat the last real column and store nothing
// The workspace is indexed by launch row with the per-row layout of DecodeArgs (the 16 statistics slots are the 16 columns), sized
// and split (decode_splits without an override) for B * rpc rows.  Per cache row stay: the length, the key tiles, the split
// partition.  Q fragments, horizon, softmax statistics and the [1,16] probability blocks are per column, the MFMA keeps columns
// apart: each head gets the bits the GQ = false kernels give it on a private copy of the row, with the same number of splits.
//
// Paged cache (PG = true kernels, always with RG = true): kq / vq are POOLS of num_pages pages of P keys (P a power of two >= 32, so a
// K tile, a V pair and the two tiles of one extend step never straddle a page), a page holding its pieces in the order above:
//   kq_pool [num_pages][P / 16][D / 32][64][8]     vq_pool [num_pages][P / 32][D / 16][64][8]
// and a device table, int32 [B][max_pages], names the page of row b's logical page i.  Only the piece's place changes:
//   logical K tile t -> tile page * (P / 16) + t % (P / 16), logical V pair s -> pair page * (P / 32) + s % (P / 32),
//   page = clamp(table[b][t / (P / 16)], 0, num_pages - 1): a wrong table gives wrong numbers, never an address outside the pools.
// A kernel looks up only logical pages that hold keys of the row -- below ceil(min(lengths[b], max_length) / P) for the readers, the
// pages of the new keys for the append -- and max_length <= C = max_pages * P keeps those inside the table's row; entries behind are
// never read.  stage stays [B][16][D] (the open tile belongs to a row), the scores workspace stays indexed by LOGICAL tile, and
// every value is the one the contiguous cache holds: the paged kernels give its bits.  Pages start out zeroed; a recycled page holds
// older quantised values, finite, which is all a V slot behind a row's length needs (above).
//
// Sliding window (WN = true kernels, always with RG = true and causal; window = W >= 1): a query at absolute position p sees keys
// max(0, p - W + 1) .. p, W keys with its own -- the reference's call with an additive mask that is finfo.min below the window as well as
// above the horizon.  The cache does not change: K^T's 16-key blocks and the [1,16] P blocks stay aligned to ABSOLUTE key index; a P
// block that straddles the lower edge is quantised with exact zeros, outside the block maximum, for the keys below it.  Decode query i
// is at p = L_b - M + i, so the row's first visible key is lo_b = max(0, L_b - M - W + 1), and the partition is RELATIVE to its pair:
//   p0_b = lo_b / 32 (scalar, from lengths[b])      split s covers pairs p0_b + s pps .., wave w takes p0_b + p_lo + w, + 4, ...
//   span = min(max_length, W + M - 1 + 31)          the keys 32 p0_b .. L_b - 1 a row can touch: the host sizes the partition (pps), the
//                                                   default splits and the workspace stride NT from span, not from max_length
//   scores workspace                                tile t of row b at index t - 2 p0_b
// Tiles below tile lo_b / 16 are not read (no K fragment, paged no table look-up; the V pair of a visible pair is read whole): their
// probabilities are exact zeros.  That is every tile below 2 p0_b, and tile 2 p0_b itself when lo_b lies in the pair's second tile.
// Splits behind the row's last pair keep the (-inf, 0) / zero-partial paths.  With M > 1 the columns' lower bounds differ: a column may
// see no key of the first split(s) -- e.g. lo_b % 32 >= 17 with one pair a split -- and gets (-inf, 0) there, which the combination skips;
// every column sees its own key, so its row maximum is finite.  W < M: the later columns' windows begin behind lo_b, nothing else.
// W = 1: each column sees its own key alone.  With W + M - 1 >= max_length, p0_b = 0 and span = max_length: the unwindowed partition and,
// the lower bound being 0, the unwindowed bits.  A paged windowed kernel looks up only pages that hold a key some query of the row sees
// (P >= 32: the page of pair p0_b is the page of key lo_b), so table entries wholly below the window may be stale (PagedKVCache.trim).
#ifndef MI355Q_DECODE_H
#define MI355Q_DECODE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mi355q_internal.h"

namespace mi355q {

struct KvCache {
    uint16_t* kq;
    uint16_t* vq;
    float* stage;
    long long B, C;
    int D;
};
// the page table of a paged cache: KvCache.kq / .vq are then the pools and KvCache.C = max_pages * P, a row's logical capacity
struct KvPages {
    const int32_t* table;     // [B][max_pages] on the device
    int max_pages, num_pages;
    int lg_p;                 // log2(P), >= 5
};
inline long long kv_k_bytes(long long B, long long C, long long D) { return B * C * D * 2; }
inline long long kv_v_bytes(long long B, long long C, long long D) { return B * ((C + 31) / 32) * 32 * D * 2; }
inline long long kv_stage_bytes(long long B, long long D) { return B * 16 * D * 4; }

// keys L .. L + n - 1 from fp32 rows k / v [B, n, D] (element strides of batch and row; innermost 1)
int launch_kv_append(const KvCache& c, const QuantArgs& ak, const QuantArgs& av, const float* k, const float* v, long long ksb,
                     long long kst, long long vsb, long long vst, long long L, long long n, hipStream_t st);
// ragged: row b's first counts[b] (NULL: n) input rows behind ITS length lengths[b] (device arrays [B])
int launch_kv_append_ragged(const KvCache& c, const QuantArgs& ak, const QuantArgs& av, const float* k, const float* v, long long ksb,
                            long long kst, long long vsb, long long vst, const int32_t* lengths, const int32_t* counts, long long n,
                            hipStream_t st, const KvPages* pages = nullptr);
// the grid of a ragged append of up to n keys a row, from n alone: K blocks (-> kblocks) in front of V blocks, by B rows; more than 2^31
// - 1 blocks: MI355Q_E_UNSUPPORTED.  launch_kv_append_ragged's and, in mi355q_kvp.hip, the mantissa caches' append's
int append_ragged_grid(long long B, int D, long long n, int& kblocks, dim3& grid);
// the staging pass of launch_kv_append_ragged alone (n > 1: the new open tile's fp32 rows, behind the append kernel that read the old
// ones): for the mantissa caches of mi355q_kvp.h, whose stage is this one.  Reads c.stage, c.B, c.C and c.D only
void launch_kv_stage_ragged(const KvCache& c, const float* k, long long ksb, long long kst, const int32_t* lengths, const int32_t* counts,
                            long long n, hipStream_t st);
// the cache's quantised values back as fp32 [B, L, D] (tests, debugging); lengths != NULL: zeros behind row b's lengths[b]
// pages != NULL (with lengths): the paged cache
int launch_kv_decode_fp32(const KvCache& c, float* k_out, float* v_out, long long L, hipStream_t st, const int32_t* lengths = nullptr,
                          const KvPages* pages = nullptr);

// S of a decode over L keys: a pure function of (B, L, D); `override` > 0 asks for that many (clamped, then evened out so
// that no split is empty).  1 <= S <= ceil(L / 32).
int decode_splits(long long B, long long L, long long D, int override);
size_t decode_workspace_bytes(long long B, long long L, long long D, int splits);
// the keys one row of a windowed decode can touch, min(L, window + M - 1 + 31) (window <= 0: L): what sizes partition and workspace
long long decode_window_span(long long M, long long L, long long window);

struct DecodeArgs {
    const float* q;           // [B, M, D] by strides
    const uint16_t* kq;
    const uint16_t* vq;
    float* out;               // [B, M, D] by strides
    float* scores;            // workspace: [B][NT][64][4] the score tiles as their MFMA lanes hold them
    float* stats;             //            [B][S][16][2] a split's (max, sum of exp(x - max)) per query
    float* part;              //            [B][S][D / 16][64][4] a split's partial output
    long long M, L, NT, NP, NTC, NPC;
    long long qsb, qsm, osb, osm;
    int causal;
    float q_scale, scale_div; // 0: none
    int D, S, pps;            // pps = key pairs per split
    const int32_t* lengths;   // ragged: [B] on the device, L / NT / NP above are those of max_length (partition, strides); else NULL
    int gw, rpc;              // grouped queries (GQ): heads a launch row serves, launch rows a cache row; gw * rpc = G.  Else 1, 1
    KvPages pg;               // paged cache (PG): kq / vq are the pools; else zeros (behind every field the other kernels read)
    long long W;              // sliding window (WN): NT / NP / S / pps are those of decode_window_span; else 0 (behind every other field)
};
// q's and out's element strides of batch and row from the wrapper's {q batch, q row, out batch, out row}; NULL: contiguous [B, M, D]
// (DecodeArgs, and ExtendArgs of mi355q_extend.h)
template <class Args>
inline void fill_qo_strides(Args& g, const long long* strides, long long M, long long D) {
    g.qsb = strides ? strides[0] : M * D; g.qsm = strides ? strides[1] : D;
    g.osb = strides ? strides[2] : M * D; g.osm = strides ? strides[3] : D;
}
// heads of a group one launch row serves: the largest divisor gw of G with gw * M <= 16 (0: G < 1 or M outside 1 .. 16)
int decode_group_width(long long G, long long M);
// What a decode launch derives from its shapes, for a cache of B rows, capacity C, head_dim D: tile and pair counts of `span` keys (L,
// or decode_window_span), group width and launch rows (-> rows), splits, pps, q / out strides, the workspace carve-up, the page table.
// The grid is (g.S, rows).  Pointers to q, out, lengths and K / V, the window and the softmax's scalars stay with the caller.  Returns an
// error code (group width, more than 65535 rows).  launch_bfp_attention_decode's and, in mi355q_kvp.hip, the mantissa caches' decode's
int decode_args_fill(DecodeArgs& g, long long B, long long C, int D, long long M, long long L, long long span, int G, int splits,
                     const long long* strides, void* workspace, const KvPages* pages, long long& rows);
// lengths != NULL: the ragged form, L = max_length.  G >= 1: the grouped form (q / out hold c.B * G rows, the workspace is that of
// c.B * G / decode_group_width(G, M) launch rows); G == 0: one query row a cache row.  pages != NULL (with lengths): the paged cache
// window >= 1 (with lengths and causal): the sliding window; the workspace is that of decode_window_span keys
int launch_bfp_attention_decode(const QuantArgs& aq, const QuantArgs& ap, const KvCache& c, const float* q, float* out,
                                void* workspace, long long M, long long L, int causal, float q_scale, float scale_div,
                                const long long* strides, int splits, hipStream_t st, const int32_t* lengths = nullptr, int G = 0,
                                const KvPages* pages = nullptr, long long window = 0);

// phase C alone (nothing to do with one split): the partial outputs of `rows` launch rows summed in split order.  It reads no K / V,
// so the mantissa caches' decode of mi355q_kvp.hip ends in it too
void launch_decode_sum(const DecodeArgs& g, bool grouped, long long rows, hipStream_t st);

}  // namespace mi355q
#endif
