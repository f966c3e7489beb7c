// The one-pass attention core of a block_minifloat layer (mi355q_attention_bm.hip): what the C-ABI wrapper needs of it.
//
// Prefill's counterpart of mi355q_kvbm.h: q [B, M, D], k / v [B, T, D] fp32 by strides, both products block_minifloat [1,16].  A pack
// launch leaves K^T and V in the workspace as the fragments a MinifloatKVCache of capacity T holds after the same T keys were appended
// (layout: mi355q_decode.h; T % 16 == 0, so every K tile is closed), one streaming launch reads them.
//   workspace   K pieces [B][T / 16][D / 32][64][8] bf16, then V pieces [B][ceil(T / 32)][D / 16][64][8] -- the absent half of the
//               last V pair (T % 32 == 16) is written as zeros by every pack launch.
// QuantArgs: those of bm_quant_args (mi355q_kv_call.h).
#ifndef MI355Q_ATTENTION_BM_H
#define MI355Q_ATTENTION_BM_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mi355q_internal.h"

namespace mi355q {

size_t bm_attention_workspace_bytes(long long B, long long T, long long D);
// strides: {q batch, q row, k batch, k row, v batch, v row, out batch, out row} in elements (innermost 1); NULL: contiguous.
// causal_off >= 0: query i sees keys 0 .. i + causal_off (T - M of a causal call, M <= T); < 0: every key.
// D in 32 / 64 / 96 / 128 and T % 16 == 0, or MI355Q_E_UNSUPPORTED.
int launch_bm_attention(const QuantArgs& aq, const QuantArgs& ak, const QuantArgs& ap, const QuantArgs& av, const float* q, const float* k,
                        const float* v, float* out, void* workspace, long long B, long long M, long long T, long long D,
                        long long causal_off, float q_scale, float scale_div, const long long* strides, hipStream_t st);

}  // namespace mi355q
#endif
