// The 4-bit-mantissa block_fp KV cache (mi355q_kvp.hip, storage NibblePieces): the cache of mi355q_kv8.h for CACHED operands of width <= 4,
// whose mantissa
// |m| <= 2^(width - 1) - 1 <= 7 fits a signed nibble: 4 + 1/2 bits a value, 9/32 of the bf16 cache's K and V bytes and decode traffic,
// 9/17 of the int8-mantissa cache's.  No arithmetic changes: the kernels rebuild the bf16 fragment the MFMA consumes in registers, and
// every fragment halfword is the int8-mantissa cache's and the bf16 cache's, bit for bit (the one deviation of mi355q_kv8.h carries over).
//
// Layout, per b = batch x head, capacity C keys (C % 16 == 0), head_dim D (D % 32 == 0, D <= 128).  A PIECE is 288 bytes: the 256
// mantissa bytes of one MFMA operand, then the 32 shared-exponent bytes of the piece's 32 blocks, as biased codes p + exponent_bias.
// Lane and slot meaning are those of mi355q_decode.h / mi355q_kv8.h.  Mantissa byte 8 (l >> 1) + j holds slot j of lane 2 (l >> 1) in
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
// launch.  THE RULE of mi355q_kv8.h therefore stays: plain byte stores, and NO STORE EVER READS THE CACHE.  Do not widen them into
// read-modify-write words, and do not re-pair the nibbles.
//
// The rebuild: m = the sign-extended 4-bit field at bit 8 (j & 3) + 4 (l & 1) of the lane's word (v_bfe_i32), then the int8 rebuild's
// pack_bf16(ldexpf((float)m, code - exponent_bias - mbits)): the same fp32 value through the same conversion, hence the int8-mantissa
// cache's halfword.  Widths: |m| <= 7 needs width <= 4 of the CACHED operands (the y side of qk_params and of pv_params); Q and P keep
// 2 .. 9.  THE ONE DEVIATION of mi355q_kv8.h: 0 < |x| <= 1e-8 is stored as 0.  A stale piece (after reset(), or storage that was not
// zeroed) pairs stale nibbles with stale or new exponent bytes: any pair of bytes an append wrote rebuilds to a finite value, which is
// all a slot behind a row's length needs.
//
// Kernels: ragged forms only (a device lengths array), contiguous only: no pages, no window, no extend.  They are the kernels of
// mi355q_kvp.hip -- one body for this storage and the int8 one -- instantiated with NibblePieces and PG = false: only the piece
// constants, the place of a lane's bytes and nibble, the store and the rebuild are this storage's own; split partition, workspace, Q / P
// quantisers, softmax, (-inf, 0) paths and the grouped column map are those of mi355q_decode.hip, phase C is its launch_decode_sum
// unchanged.
#ifndef MI355Q_KV4_H
#define MI355Q_KV4_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mi355q_decode.h"
#include "mi355q_internal.h"

namespace mi355q {

constexpr int KV4_PIECE = 288;            // 256 mantissa bytes (two nibbles each) + 32 exponent bytes
constexpr int KV4_CODES = 256;            // where a piece's exponent bytes start

struct Kv4Cache {
    uint8_t* k4;
    uint8_t* v4;
    float* stage;
    long long B, C;
    int D;
};
inline long long kv4_k_bytes(long long B, long long C, long long D) { return B * (C / 16) * (D / 32) * KV4_PIECE; }
inline long long kv4_v_bytes(long long B, long long C, long long D) { return B * ((C + 31) / 32) * (D / 16) * KV4_PIECE; }

// The three launchers are mi355q_kvp.hip's templates on the nibble storage, which has no paged kernels: pages != NULL is
// MI355Q_E_UNSUPPORTED.
// launch_kv8_append on the nibble storage (ak / av: the quantisers of the cached operands, width <= 4)
int launch_kv4_append(const Kv4Cache& c, const QuantArgs& ak, const QuantArgs& av, const float* k, const float* v, long long ksb,
                      long long kst, long long vsb, long long vst, const int32_t* lengths, const int32_t* counts, long long n,
                      hipStream_t st, const KvPages* pages = nullptr);
// the cache's values, as the decode kernels rebuild them, back as fp32 [B, L, D]; zeros behind row b's lengths[b]
int launch_kv4_decode_fp32(const Kv4Cache& c, const QuantArgs& ak, const QuantArgs& av, float* k_out, float* v_out, long long L,
                           const int32_t* lengths, hipStream_t st, const KvPages* pages = nullptr);
// launch_bfp_attention_decode_kv8's contiguous forms on the nibble cache: L = max_length, G >= 1 the grouped form, G == 0 one query
// row a cache row; workspace and splits as there
int launch_bfp_attention_decode_kv4(const QuantArgs& aq, const QuantArgs& ap, const QuantArgs& ak, const QuantArgs& av, const Kv4Cache& c,
                                    const float* q, float* out, void* workspace, long long M, long long L, int causal, float q_scale,
                                    float scale_div, const long long* strides, int splits, hipStream_t st, const int32_t* lengths, int G,
                                    const KvPages* pages = nullptr);

}  // namespace mi355q
#endif
