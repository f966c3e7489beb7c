// Chunked prefill (mi355q_extend.hip): cached attention for ANY number of new tokens per row -- what the C-ABI wrapper needs of it.
//
// The cache is the one of mi355q_decode.h (layout, capacity strides, zeroed vq); the queries' own keys are appended first.  Row b
// (batch x head) holds L_b keys and asks m_b queries, q[b, 0 .. m_b - 1]: the row's last m_b positions.
//   lengths   device int32 [B]: L_b, clamped to 0 .. max_length.  NULL: the uniform form, L_b = max_length
//   counts    device int32 [B]: m_b, clamped to 0 .. M.           NULL: m_b = M
// causal: query i sees keys 0 .. L_b - m_b + i (the mask offset of modeling_llama.py:53-79), else all L_b.  Output rows i >= m_b are
// written as zeros; a row with m_b == 0 or m_b > L_b -- an empty slot, the decode kernels' rule -- reads no fragment and returns
// zeros.  The host's M and max_length size the grid only; nothing is addressed from them.  No workspace: the scores are formed twice.
// Grouped queries (G >= 1): q / out hold B * G rows, query row r reads cache row r / G and lengths[r / G], counts[r / G].
// Paged cache (pages != NULL, lengths != NULL): the step's pieces through the row's page table (mi355q_decode.h).
// Sliding window (window >= 1, causal, lengths != NULL): query i sees keys max(0, p - window + 1) .. p, p = L_b - m_b + i; a workgroup's
// walk begins at the 32-key step of its first query's lower bound (mi355q_extend.hip).
#ifndef MI355Q_EXTEND_H
#define MI355Q_EXTEND_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mi355q_internal.h"
#include "mi355q_decode.h"

namespace mi355q {

struct ExtendArgs {
    const float* q;           // [B, M, D] by strides
    const uint16_t* kq;
    const uint16_t* vq;
    float* out;               // [B, M, D] by strides
    long long M, L, NTC, NPC; // L = max_length; NTC / NPC: key tiles / key pairs a cache row is apart
    long long qsb, qsm, osb, osm;
    int causal;
    float q_scale, scale_div; // 0: none
    int nb, nxb;              // rows, query blocks of 64 a row: the grid is nb * nxb work items
    const int32_t* lengths;   // [B] on the device or NULL
    const int32_t* counts;    // [B] on the device or NULL
    int G;                    // grouped queries (GQ): query rows a cache row; nb = B * G, lengths / counts stay [B].  Else 0
    KvPages pg;               // paged cache (PG, mi355q_decode.h): kq / vq are the pools; else zeros
    long long W;              // sliding window (WN, mi355q_decode.h); else 0 (behind every other field)
};

int launch_bfp_attention_extend(const QuantArgs& aq, const QuantArgs& ap, const KvCache& c, const float* q, float* out, long long M,
                                long long max_length, int causal, float q_scale, float scale_div, const long long* strides,
                                const int32_t* lengths, const int32_t* counts, hipStream_t st, int G = 0, const KvPages* pages = nullptr,
                                long long window = 0);

}  // namespace mi355q
#endif
