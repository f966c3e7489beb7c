// Host code shared by the Linear-side exports of mi355q_api.hip and the KV-cache calls of mi355q_kv_call.h -- no kernel, no launch, no
// HIP call, no getenv, no statics: the one decoder of a block_fp quantiser's words (block_fp_args / block_fp_fill), the one layout of
// QuantArgs (fill_layout, fill_rows, fill_common) and the pre-op and alignment predicates.  A returned code is ABI, and so is the ORDER
// of the checks: tests/golden/linear_api_codes.json holds both.  What stays written out, because folding it would change a recorded code:
// - the block_minifloat words have three orders (mi355q_block_minifloat_quantize: all malformed; _bf16: too wide in front of the bias
//   width; _bf16_tiled: behind it) and bm_quant_args (mi355q_kv_call.h) a fourth range: they share block_minifloat_fill only;
// - mi355q_bfp_matmul and the attention pass check the words of all their operands before any is too wide: block_fp_fill only.
#ifndef MI355Q_LINEAR_CALL_H
#define MI355Q_LINEAR_CALL_H
#include <stdint.h>

#include <cmath>
#include <initializer_list>

#include "mi355q.h"
#include "mi355q_internal.h"

namespace mi355q {

// ---- the quantisers' words
inline void set_mantissa(QuantArgs& a, int mbits) {
    a.shift = std::ldexp(1.0f, mbits);
    a.inv_shift = std::ldexp(1.0f, -mbits);
    a.mant_max = a.shift - 1.0f;
}
inline int default_bias(int bias, int exponent_width) { return bias == MI355Q_BIAS_DEFAULT ? (1 << (exponent_width - 1)) - 1 : bias; }
// block_fp {width, exponent width, exponent bias}, already checked
inline void block_fp_fill(QuantArgs& a, int width, int exponent_width, int bias) {
    a.code_bias = default_bias(bias, exponent_width);
    a.e_min = -a.code_bias;
    a.e_max = (1 << exponent_width) - 1 - a.code_bias;
    set_mantissa(a, width - 1);
}
// ... checked: exponent width 1 .. 8 and width >= 2 or `malformed`, width <= max_width or `too_wide`
struct WidthLimits { int max_width, malformed, too_wide; };
inline int block_fp_args(QuantArgs& a, int width, int exponent_width, int bias, WidthLimits lim) {
    if (exponent_width < 1 || exponent_width > 8 || width < 2) return lim.malformed;
    if (width > lim.max_width) return lim.too_wide;
    block_fp_fill(a, width, exponent_width, bias);
    return 0;
}
inline void block_minifloat_fill(QuantArgs& a, int mbits, int exponent_width, int exponent_bias_width) {
    a.span = (1 << exponent_width) - 1;
    a.bias_max = (1 << exponent_bias_width) - 1;
    set_mantissa(a, mbits);
}

// ---- the layout of QuantArgs
inline void fill_layout(QuantArgs& a, const float* x, int64_t lead, int64_t rows, int64_t cols, int32_t b0, int32_t b1, uint32_t flags) {
    a.x = x;
    a.lead = lead; a.rows = rows; a.cols = cols;
    a.b0 = b0; a.b1 = b1;
    a.n_elems = lead * rows * cols;
    a.nbr = (rows + b0 - 1) / b0;
    a.nbc = (cols + b1 - 1) / b1;
    a.n_blocks = lead * a.nbr * a.nbc;
    a.flags = flags;
}
// x [rows, K] in [1,16] blocks: what every GEMM-operand quantiser reads
inline void fill_rows(QuantArgs& a, const float* x, int64_t rows, int64_t K) { fill_layout(a, x, 1, rows, K, 1, 16, MI355Q_ZERO_BLOCK_FAST); }
// true: go on with `a`.  false: return rc (MI355Q_E_BADARG, or 0 where there is nothing to do)
inline bool fill_common(QuantArgs& a, const float* x, float* y, void* workspace, int64_t lead, int64_t rows, int64_t cols, int32_t b0, int32_t b1,
                        uint32_t flags, int& rc) {
    rc = MI355Q_E_BADARG;
    if (lead < 0 || rows < 0 || cols < 0 || b0 < 1 || b1 < 1) return false;
    a = QuantArgs{};
    a.y = y;
    a.ws = static_cast<unsigned*>(workspace);
    fill_layout(a, x, lead, rows, cols, b0, b1, flags);
    if (a.n_elems != 0 && (x == nullptr || ((flags & MI355Q_ZERO_BLOCK_FAST) == 0u && workspace == nullptr))) return false;
    rc = 0;
    return a.n_elems != 0;              // (nothing to do: 0)
}

inline bool pre_op_ok(int32_t pre_op, const float* x2, bool rows_kernel = false) {
    const bool norm = pre_op == MI355Q_PRE_RMSNORM || pre_op == MI355Q_PRE_LAYERNORM;
    if (norm && !rows_kernel) return false;                              // (needs the whole row in one workgroup)
    if (pre_op != MI355Q_PRE_NONE && pre_op != MI355Q_PRE_RELU && pre_op != MI355Q_PRE_SILU_MUL && !norm) return false;
    return (pre_op != MI355Q_PRE_SILU_MUL && !norm) || (x2 != nullptr && reinterpret_cast<uintptr_t>(x2) % 16 == 0);
}
inline bool misaligned16(std::initializer_list<const void*> ptrs) {          // (an optional NULL passes)
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
    return bits % 16 != 0;
}

}  // namespace mi355q
#endif
