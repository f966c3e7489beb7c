// The mantissa block_fp KV caches (mi355q_kvp.hip): the cache of mi355q_decode.h with every quantised value stored as what it is -- a
// signed mantissa and a power of two that the 16 values of its block share -- instead of as bf16.  Two storages (KvMantissa), one host
// descriptor (KvpCache), one launcher an operation; this header is the specification of the bytes of both.
//   KV_M8   int8 mantissas (storage Int8Pieces), cached operands of width <= 8, contiguous or paged pools      THE INT8 STORAGE below
//   KV_M4   4-bit mantissas, two to a byte (storage NibblePieces), cached operands of width <= 4, contiguous   THE NIBBLE STORAGE below,
//                                                                                                              as the difference from it
//
// ==== THE INT8 STORAGE (KV_M8) ==================================================================================================
// A signed mantissa of at most 8 bits and one exponent byte a block: 1 + 1/16
// bytes a value, 17/32 of the bf16 cache's K and V bytes and decode traffic.  No arithmetic changes: the kernels rebuild the bf16
// fragment the MFMA consumes in registers, and every fragment halfword is the bf16 cache's, bit for bit (one stated deviation below).
//
// Layout, per b = batch x head, capacity C keys (C % 16 == 0), head_dim D (D % 32 == 0, D <= 128).  A PIECE is 544 bytes: the 512
// mantissa bytes of one MFMA operand -- lane l's 8 slots at bytes 8 l .. 8 l + 7, the lane and slot order of mi355q_decode.h -- and
// behind them the 32 shared-exponent bytes of the piece's 32 blocks, as biased codes p + exponent_bias (what QuantArgs.code holds):
//   k8  [B][C / 16][D / 32][544]     piece (b, key tile t, chunk c): lane (key 16 t + lane % 16, g = lane / 16) holds d = 32 c + 8 g + j
//                                    in slot j.  A block is the tile's 16 keys at one d; the exponent of d = 32 c + i is byte 512 + i,
//                                    so the 8 exponents a lane needs (8 different d) are ONE 8-byte load at 512 + 8 g, the same
//                                    address for the 16 lanes of a group.  Keys the cache does not hold yet: mantissa 0.
//   v8  [B][ceil(C / 32)][D / 16][544]   piece (b, key pair s, dt): lane (d = 16 dt + lane % 16, g = lane / 16) holds key
//                                    32 s + 16 (j / 4) + 4 g + (j & 3) in slot j.  A block is 16 d of one key; the exponent of the key
//                                    in slot j of group g is byte 512 + 8 g + j -- slot order, not key order -- so a lane's 8
//                                    exponents (8 keys) are again ONE 8-byte load at 512 + 8 g.  The storage starts out ZEROED: a
//                                    slot no key has reached is mantissa 0 under any exponent byte, a finite 0 for the probability
//                                    of exactly 0 it meets; stale bytes of an earlier sequence rebuild to finite values as well.
//   stage [B][16][D] fp32            the open key tile's rows, exactly as in mi355q_decode.h (shared code: launch_kv_stage_ragged)
// Pieces are 32-byte aligned, a lane's mantissa load 8-byte aligned.  Every address is formed from (b, t < C / 16, c) or
// (b, s < ceil(C / 32), dt): keys at or behind C are dropped by the append as in the bf16 cache.
//
// The rebuild: fragment halfword = pack_bf16(ldexpf((float)m, code - exponent_bias - mbits)), mbits = width - 1.  kv_store_block of
// mi355q_decode.hip packs copysign(ldexp(|m|, p - mbits), x) + 0 of the SAME integer |m| <= 2^mbits - 1 and the same p: the same fp32
// value, hence the same halfword -- also where p sits at a clamp end of the exponent range, and where the product is subnormal or
// rounds in bf16 (both go through the one conversion).  A mantissa that rounds to 0 is +0 on both sides.  Widths: |m| <= 127 needs
// width <= 8 of the CACHED operands (the y side of qk_params and of pv_params); Q and P, which are not stored, keep 2 .. 9.
// ONE DEVIATION: at_quant passes 0 < |x| <= 1e-8 through unquantised (the bf16 cache stores it rounded to bf16); a mantissa and a block
// exponent cannot hold that, and this cache stores 0 there -- a stored value moves by at most 1e-8.  An all-zero block stores zero
// mantissas and the exponent code of the lowest exponent.
//
// Paged pools (PG = true kernels; `pages` of the launchers): the pools of mi355q_decode.h's paged cache in the same page order, of these
// pieces -- num_pages pages of P keys, P a power of two >= 32, so a piece (16 keys of K, 32 keys of V) never straddles a page:
//   k8_pool [num_pages][P / 16][D / 32][544]     v8_pool [num_pages][P / 32][D / 16][544]     table int32 [B][max_pages]
// A page of either pool is P D 17 / 16 bytes, P D 17 / 256 units of 16 bytes (a whole number: P D is a multiple of 1024; 68 at
// P = D = 32), the unit of the copy-on-write launch (mi355q_kv_copy.h).  Only a piece's PLACE changes: logical K tile t sits at tile
// pg_place(pg, pg_raw(pg, b, t >> (lg_p - 4)), t, lg_p - 4), logical V pair s the same with lg_p - 5 (mi355q_decode_dev.h); the page id is
// clamped into the pool, so a wrong table gives wrong numbers and never an address outside the pools.  A kernel looks up only logical
// pages that hold keys of the row (the append: the pages of its new keys, which the host has given the row before); KvpCache.C is
// max_pages * P there.  stage stays per row, the scores workspace stays indexed by LOGICAL tile, and nothing else of a kernel changes:
// split partition, statistics and the order of every sum are the contiguous kernels', so the paged decode gives their bits -- and with
// them those of the bf16 caches -- by construction.  A recycled page pairs stale mantissas with stale exponent bytes: any such pair
// rebuilds to a finite value, which is all a slot behind a row's length needs.  The append stores single BYTES into pieces that
// neighbouring threads of the same launch write too (16 keys of a tile share a piece with the other d): byte stores never read, so no
// thread's store can undo another's -- do not widen them into read-modify-write words.
//
// Kernels (mi355q_kvp.hip, instantiated with Int8Pieces; the same bodies serve the nibble storage): ragged forms only (a
// device lengths array; the Python layer supplies one for the uniform call), no window, no extend.  The decode kernels are the
// RG = true, WN = false kernels of mi355q_decode.hip with another way of getting a K or V fragment into registers; split
// partition, workspace, Q / P quantisers, softmax, (-inf, 0) paths and the grouped column map are theirs, phase C is theirs unchanged.
//
// ==== THE NIBBLE STORAGE (KV_M4) ================================================================================================
// The int8 storage for CACHED operands of width <= 4, whose mantissa
// |m| <= 2^(width - 1) - 1 <= 7 fits a signed nibble: 4 + 1/2 bits a value, 9/32 of the bf16 cache's K and V bytes and decode traffic,
// 9/17 of the int8-mantissa cache's.  No arithmetic changes: the kernels rebuild the bf16 fragment the MFMA consumes in registers, and
// every fragment halfword is the int8-mantissa cache's and the bf16 cache's, bit for bit (the one deviation of the int8 storage carries
// over).
//
// Layout, per b = batch x head, capacity C keys (C % 16 == 0), head_dim D (D % 32 == 0, D <= 128).  A PIECE is 288 bytes: the 256
// mantissa bytes of one MFMA operand, then the 32 shared-exponent bytes of the piece's 32 blocks, as biased codes p + exponent_bias.
// Lane and slot meaning are those of mi355q_decode.h / the int8 storage.  Mantissa byte 8 (l >> 1) + j holds slot j of lane 2 (l >> 1) in
// bits 0 .. 3 and slot j of lane 2 (l >> 1) + 1 in bits 4 .. 7, both two's complement (-8 is never produced).
//   k4  [B][C / 16][D / 32][288]     piece (b, key tile t, chunk c): lane (key 16 t + lane % 16, g = lane / 16) holds d = 32 c + 8 g + j
//                                    in slot j.  A block is the tile's 16 keys at one d; the exponent of d = 32 c + i is byte 256 + i:
//                                    the int8 piece's exponent part, moved from offset 512 to 256.  Keys not held yet: mantissa 0.
//   v4  [B][ceil(C / 32)][D / 16][288]   piece (b, key pair s, dt): lane (d = 16 dt + lane % 16, g = lane / 16) holds key
//                                    32 s + 16 (j / 4) + 4 g + (j & 3) in slot j.  A block is 16 d of one key; the exponent of the key
//                                    in slot j of group g is byte 256 + 8 g + j (slot order).  The storage starts out ZEROED, as v8.
//   stage [B][16][D] fp32            the open key tile's rows, exactly as in mi355q_decode.h (shared code: launch_kv_stage_ragged)
// Pieces are 32-byte aligned (288 = 9 * 32).  A lane's 8 slots are ONE 8-byte load at 8 (l >> 1), the same address for both lanes of a
// pair; its 8 exponents ONE 8-byte load at 256 + 8 g.  Every address is formed from (b, t < C / 16, c) or (b, s < ceil(C / 32), dt):
// keys at or behind C are dropped by the append.
//
// WHY THE TWO NIBBLES OF A BYTE ARE LANES l AND l ^ 1.  In K these are two keys of one tile at one d, in V two d of one key: either way
// two values of ONE block.  One thread of the append quantises that block, holds both values in its x[16], and stores the byte whole.
// A pairing along the slots would put two BLOCKS in one byte -- for K d and d + 1, written by two threads of the same launch; for V
// key k and k + 1, written by two threads of the same launch or by two appends -- and force a read-modify-write that races inside a
// launch.  THE RULE of the int8 storage therefore stays: plain byte stores, and NO STORE EVER READS THE CACHE.  Do not widen them into
// read-modify-write words, and do not re-pair the nibbles.
//
// The rebuild: m = the sign-extended 4-bit field at bit 8 (j & 3) + 4 (l & 1) of the lane's word (v_bfe_i32), then the int8 rebuild's
// pack_bf16(ldexpf((float)m, code - exponent_bias - mbits)): the same fp32 value through the same conversion, hence the int8-mantissa
// cache's halfword.  Widths: |m| <= 7 needs width <= 4 of the CACHED operands (the y side of qk_params and of pv_params); Q and P keep
// 2 .. 9.  THE ONE DEVIATION of the int8 storage: 0 < |x| <= 1e-8 is stored as 0.  A stale piece (after reset(), or storage that was not
// zeroed) pairs stale nibbles with stale or new exponent bytes: any pair of bytes an append wrote rebuilds to a finite value, which is
// all a slot behind a row's length needs.
//
// Kernels: ragged forms only (a device lengths array), contiguous only: no pages, no window, no extend.  They are the kernels of
// mi355q_kvp.hip -- one body for this storage and the int8 one -- instantiated with NibblePieces and PG = false: only the piece
// constants, the place of a lane's bytes and nibble, the store and the rebuild are this storage's own; split partition, workspace, Q / P
// quantisers, softmax, (-inf, 0) paths and the grouped column map are those of mi355q_decode.hip, phase C is its launch_decode_sum
// unchanged.
#ifndef MI355Q_KVP_H
#define MI355Q_KVP_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mi355q_decode.h"
#include "mi355q_internal.h"

namespace mi355q {

// which mantissa storage: the one argument the size functions and the launchers below take in front of what they always took
enum KvMantissa { KV_M8, KV_M4 };

constexpr int KVP_M8_PIECE = 544, KVP_M8_CODES = 512;     // 512 mantissa bytes + 32 exponent bytes; where the exponent bytes start
constexpr int KVP_M4_PIECE = 288, KVP_M4_CODES = 256;     // 256 mantissa bytes (two nibbles each) + 32 exponent bytes

// either storage's cache, as the kernels take it (a kernel argument: field order and types are the kernels')
struct KvpCache {
    uint8_t* k;
    uint8_t* v;
    float* stage;
    long long B, C;
    int D;
};
inline int kvp_piece(KvMantissa m) { return m == KV_M4 ? KVP_M4_PIECE : KVP_M8_PIECE; }
inline int kvp_widest(KvMantissa m) { return m == KV_M4 ? 4 : 8; }       // the widest CACHED operand whose mantissa the storage holds
inline long long kvp_k_bytes(KvMantissa m, long long B, long long C, long long D) { return B * (C / 16) * (D / 32) * kvp_piece(m); }
inline long long kvp_v_bytes(KvMantissa m, long long B, long long C, long long D) { return B * ((C + 31) / 32) * (D / 16) * kvp_piece(m); }

// The launchers: one switch on m into mi355q_kvp.hip's templates.  pages != NULL: c.k / c.v are the paged pools, c.C = max_pages * P;
// on a storage that has no paged kernels (KV_M4) it is MI355Q_E_UNSUPPORTED.
// row b's first counts[b] (NULL: n) input rows behind ITS length lengths[b]: launch_kv_append_ragged on the mantissa storage
// (ak / av: the quantisers of the cached operands, width <= kvp_widest(m))
int launch_kvp_append(KvMantissa m, const KvpCache& c, const QuantArgs& ak, const QuantArgs& av, const float* k, const float* v, long long ksb,
                      long long kst, long long vsb, long long vst, const int32_t* lengths, const int32_t* counts, long long n,
                      hipStream_t st, const KvPages* pages = nullptr);
// the cache's values, as the decode kernels rebuild them, back as fp32 [B, L, D]; zeros behind row b's lengths[b]
int launch_kvp_decode_fp32(KvMantissa m, const KvpCache& c, const QuantArgs& ak, const QuantArgs& av, float* k_out, float* v_out, long long L,
                           const int32_t* lengths, hipStream_t st, const KvPages* pages = nullptr);
// launch_bfp_attention_decode's ragged forms on the mantissa cache: L = max_length, G >= 1 the grouped form, G == 0 one query row a
// cache row; workspace and splits as there
int launch_bfp_attention_decode_kvp(KvMantissa m, const QuantArgs& aq, const QuantArgs& ap, const QuantArgs& ak, const QuantArgs& av,
                                    const KvpCache& c, const float* q, float* out, void* workspace, long long M, long long L, int causal,
                                    float q_scale, float scale_div, const long long* strides, int splits, hipStream_t st,
                                    const int32_t* lengths, int G, const KvPages* pages = nullptr);

}  // namespace mi355q
#endif
