// The block_minifloat KV cache (mi355q_kvbm.hip): what the C-ABI wrapper needs of it.
//
// The cache IS the KvCache of mi355q_decode.h -- kq / vq / stage, the same pieces, lanes and slots, the same open-tile rule, bf16
// halfwords -- holding what the reference's block_minifloat [1,16] quantisers (block_minifloat.py:44-65, minifloat.py:158-194) make of
// k^T and v in place of block_fp's: values of at most 7 mantissa bits, exact in bf16.  Sizes, workspace, splits and the fp32 read-back
// (mi355q_bfp_kv_cache_bytes, mi355q_bfp_attention_decode_workspace_bytes / _splits, mi355q_bfp_kv_decode_fp32_ragged) are therefore the
// block_fp cache's own.  Ragged form only (lengths on the device), contiguous, no window, no extend.
// QuantArgs of a block_minifloat operand: span = 2^exponent_width - 1, bias_max = 2^exponent_bias_width - 1, shift / inv_shift /
// mant_max of its mantissa bits (kv_call_check fills them).
#ifndef MI355Q_KVBM_H
#define MI355Q_KVBM_H
#include "mi355q_decode.h"

namespace mi355q {

// launch_kv_append_ragged with the block_minifloat quantisers ak (k^T: 16 keys at one d) and av (v: 16 d of one key)
int launch_kvbm_append(const KvCache& c, const QuantArgs& ak, const QuantArgs& av, const float* k, const float* v, long long ksb, long long kst,
                       long long vsb, long long vst, const int32_t* lengths, const int32_t* counts, long long n, hipStream_t st);
// launch_bfp_attention_decode's ragged, unwindowed, unpaged forms with the block_minifloat quantisers aq (Q) and ap (P); G as there
int launch_bm_attention_decode(const QuantArgs& aq, const QuantArgs& ap, const KvCache& c, const float* q, float* out, void* workspace,
                               long long M, long long L, int causal, float q_scale, float scale_div, const long long* strides, int splits,
                               hipStream_t st, const int32_t* lengths, int G);

}  // namespace mi355q
#endif
