// Attention sinks (mi355q_sink.hip): sliding-window decode and extend on the block_fp KV cache with the first `sinks` keys visible to
// every query beside its window -- what the C-ABI wrapper needs of them.
//
// Semantics (sinks = S, 0 <= S <= 16, always with window = W >= 1, causal, the ragged form): the query at absolute position p sees keys
//   {0 .. min(S, p + 1) - 1}  u  {max(0, p - W + 1) .. p},      p = L_b - M + i (decode), L_b - m_b + i (extend)
// the reference's `past_key_value` call on the full K / V with an additive mask that is finfo.min between the sinks and the window as
// well as above the horizon.  Positions are the absolute ones baked into the keys: nothing is re-rotated.  The cache and the append
// kernels are those of mi355q_decode.h; K^T's 16-key blocks and the [1,16] P blocks stay aligned to ABSOLUTE key index.  S <= 16 keeps
// every sink inside key tile 0 -- pair 0, extend step 0, logical page 0 -- and the P block of tile 0 is quantised with exact zeros,
// outside the block maximum, for its keys that are neither sink nor inside the window.
//
// Decode: a row whose first visible pair p0_b = lo_b / 32 (mi355q_decode.h) is >= 1 has ONE more leading piece of work, the sink pair:
//   virtual pair 0 = pair 0 (K tile 0 only; tile 1 is never read), virtual pair v >= 1 = pair p0_b + v - 1
// and the split partition, the score workspace (virtual tile 2 v + h) and the statistics are those of the virtual pairs: the sink pair
// is the first pair of split 0 and its statistics are combined in split order like any other split's.  A row with p0_b == 0 keeps the
// windowed kernels' walk (virtual = real); its visibility test alone has the sinks' term.  The host sizes the partition, the default
// number of splits and the workspace from decode_sink_span = min(max_length, decode_window_span + 32) keys.
// Extend: a workgroup whose first step st0 (mi355q_extend.hip) is >= 1 takes step 0 first and then steps st0 .. nsteps - 1, in both passes.
// Paged: the sink pair / step 0 takes table entry 0, so a trimmed row must keep logical page 0 (PagedKVCache.trim(..., sinks=S)).
// sinks == 0 is the windowed launch itself (mi355q_decode.h, mi355q_extend.h): the same kernels, the same bits.
#ifndef MI355Q_SINK_H
#define MI355Q_SINK_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mi355q_internal.h"
#include "mi355q_decode.h"
#include "mi355q_extend.h"

namespace mi355q {

constexpr long long SINKS_MAX = 16;     // every sink lies in key tile 0

// the keys one row of a sink decode can touch: the window's span and the sink pair, never more than the row can hold
long long decode_sink_span(long long M, long long L, long long window);

// the kernels' arguments: those of the windowed launches (DecodeArgs / ExtendArgs with W set) and the number of sinks, a kernel
// parameter of its own so that the structs every other kernel reads keep their layout
int launch_bfp_attention_decode_sink(const QuantArgs& aq, const QuantArgs& ap, const KvCache& c, const float* q, float* out, void* workspace,
                                     long long M, long long L, float q_scale, float scale_div, const long long* strides, int splits,
                                     hipStream_t st, const int32_t* lengths, int G, const KvPages* pages, long long window, long long sinks);
int launch_bfp_attention_extend_sink(const QuantArgs& aq, const QuantArgs& ap, const KvCache& c, const float* q, float* out, long long M,
                                     long long max_length, float q_scale, float scale_div, const long long* strides, const int32_t* lengths,
                                     const int32_t* counts, hipStream_t st, int G, const KvPages* pages, long long window, long long sinks);

}  // namespace mi355q
#endif
