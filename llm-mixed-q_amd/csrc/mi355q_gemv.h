// The small-M product on width-bit packed weights (mi355q_gemv.hip): what the C-ABI wrapper needs of it.
#ifndef MI355Q_GEMV_H
#define MI355Q_GEMV_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mi355q {

struct PackedSmallArgs {
    const uint8_t* x_tiled;   // tiled bf16 activations (mi355q_block_fp_quantize_bf16_tiled), rows 0 .. 15 are read
    const uint8_t* packed;    // [N, K * width / 8]
    const uint8_t* codes;     // [N, K / 16]
    const uint8_t* row_exp;   // [N] or null (per-block flavour)
    const int* list;          // bucketed exception list of the row flavour (null: per-block flavour)
    int list_cap;             // entries per 256-row bucket
    const float* bias;        // [N] or null
    float* y;                 // [M, ldy]
    long long M, N, K, ldy;
    int width;                // 2 .. 8
    int w_off;                // weight exponent_bias + width - 1
};
int launch_bfp_gemm_packed_small(const PackedSmallArgs& a, hipStream_t st);

}  // namespace mi355q
#endif
