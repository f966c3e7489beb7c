// C-ABI entry points declared in include/mi355q.h: argument validation and dispatch only.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <utility>
#include <vector>

#include "mi355q.h"
#include <map>
#include <mutex>

#include "mi355q_internal.h"
#include "mi355q_gemv.h"
#include "mi355q_decode.h"
#include "mi355q_kvp.h"
#include "mi355q_extend.h"
#include "mi355q_linear_call.h"
#include "mi355q_kv_call.h"
#include "mi355q_sink.h"
#include "mi355q_kv_copy.h"
#include "mi355q_attention_bm.h"
#include "mi355q_align_row.h"

using namespace mi355q;

namespace {
std::atomic<int> g_gemm_variant{0};

// optional HIP-event bracket around the main GEMM kernel (benchmarks).  Round 6: the events are offered to the launcher
// (g_kernel_events); the 256 x 256 tile kernel's launcher attaches them to its dispatch (hipExtLaunchKernelGGL) -- kernel start to kernel
// end, as the profiler's kernel trace has it -- and every other launcher leaves them: then two marker records bracket the launch as
// before (which also times the command processor's way from marker to dispatch to marker: 5-7 us on round 6's boxes)
struct GemmTiming {
    bool enabled = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    size_t used = 0;
    hipEvent_t begin(hipStream_t st) {
        if (!enabled || used >= 4096) return nullptr;
        if (used == pool.size()) {
            hipEvent_t a, b;
            // (device-scope release: a default event record releases to SYSTEM scope -- the stop marker then waits for the write-back of
            //  the kernel's 64 MiB of output to leave the L2s before it takes its timestamp, 5-7 us that are not the kernel's and that
            //  the step without events never pays; HIP documents this flag for "more precise timings of commands between events")
            if (hipEventCreateWithFlags(&a, hipEventReleaseToDevice) != hipSuccess || hipEventCreateWithFlags(&b, hipEventReleaseToDevice) != hipSuccess)
                return nullptr;
            pool.emplace_back(a, b);
        }
        (void)hipEventRecord(pool[used].first, st);
        mi355q::g_kernel_events = {pool[used].first, pool[used].second};
        return pool[used].second;
    }
    void end(hipEvent_t e, hipStream_t st) {
        if (e) {
            if (mi355q::g_kernel_events.start) (void)hipEventRecord(e, st);      // (no launcher took them: the marker pair)
            mi355q::g_kernel_events = {nullptr, nullptr};
            ++used;
        }
    }
} g_timing;

// the bracket around one launch
template <class Launch>
int timed(hipStream_t st, Launch launch) {
    hipEvent_t te = g_timing.begin(st);
    const int rc = launch();
    g_timing.end(te, st);
    return rc;
}

int bucket_cap_of(int32_t cap) { return cap == 0 ? ROW_BCAP : cap; }
bool bucket_cap_bad(int32_t cap, int32_t least = 0) { return cap < least || cap > ROW_BCAP_MAX; }

// a mi355q_bfp_operand: what a product requires of it -- the fields that must be there, row_aligned (-1: any), list_cap resolving to
// ROW_BCAP -- and what is wrong with it: BADARG, BADARG, UNSUPPORTED, ALIGN.  Each product looks at the faults of its two operands in
// its own recorded order (plain: both operands' pointers, K, both widths, ..., alignment; _multi: each weight whole, then x with its
// width BEHIND the unsupported forms), so the faults are named here and the order stays with the product
enum : unsigned { OP_MANT = 1, OP_EXP = 2, OP_ROWFLAG = 4, OP_GSCALE = 8, OP_LIST = 16, OP_TILED = 7, OP_ALL = 31 };
struct OperandNeeds { unsigned fields; int row_aligned; bool lds_buckets; };
struct OperandFaults { bool missing, mbits, form, misaligned; };
OperandFaults operand_faults(const mi355q_bfp_operand& o, OperandNeeds n) {
    const unsigned has = (o.mant ? OP_MANT : 0u) | (o.exp ? OP_EXP : 0u) | (o.rowflag ? OP_ROWFLAG : 0u) | (o.gscale ? OP_GSCALE : 0u) |
                         (o.list ? OP_LIST : 0u);
    return {(n.fields & ~has) != 0u, o.mbits < 1 || o.mbits > 7,
            (n.row_aligned >= 0 && o.row_aligned != n.row_aligned) || (n.lds_buckets && bucket_cap_of(o.list_cap) != ROW_BCAP),
            misaligned16({o.mant})};
}
constexpr OperandNeeds ANY_ROWS = {OP_TILED, -1, false};    // mi355q_bfp_gemm_aligned: the rest depends on the route
constexpr OperandNeeds ONE_LAUNCH = {OP_ALL, 1, true};      // the tile kernel's own operand: whole rows, lists, 120-entry buckets
// the launch arguments every product of two checked operands starts from
GemmArgs gemm_args(const mi355q_bfp_operand& x, const mi355q_bfp_operand& w, const float* bias, float* y, int64_t M, int64_t N, int64_t K,
                   int64_t ldy) {
    return GemmArgs{x.mant, x.exp, w.mant, w.exp, bias, y, M, N, K, ldy,
                    x.exp_bias + x.mbits + w.exp_bias + w.mbits, x.row_aligned ? 1 : 0,
                    x.exp_bias + x.mbits, w.exp_bias + w.mbits, ROW_BCAP, ROW_BCAP, 0};
}
}  // namespace
namespace mi355q { KernelEvents g_kernel_events = {nullptr, nullptr}; }

extern "C" {

int mi355q_abi_version(void) { return MI355Q_ABI_VERSION; }

const char* mi355q_error_string(int code) {
    switch (code) {
        case 0: return "success";
        case MI355Q_E_BADARG: return "mi355q: bad argument (null pointer, negative size, or width out of range)";
        case MI355Q_E_UNSUPPORTED: return "mi355q: configuration valid for the reference but not built here";
        case MI355Q_E_ALIGN: return "mi355q: pointer or leading-dimension alignment requirement violated";
        default: return code > 0 ? hipGetErrorString(static_cast<hipError_t>(code)) : "mi355q: unknown error";
    }
}

int mi355q_block_fp_quantize(const float* x, float* y, int8_t* mant, uint8_t* exp, int64_t lead, int64_t rows,
                             int64_t cols, int32_t b0, int32_t b1, int32_t width, int32_t exponent_width,
                             int32_t exponent_bias, uint32_t flags, void* workspace, void* stream) {
    QuantArgs a;
    int rc;
    if (!fill_common(a, x, y, workspace, lead, rows, cols, b0, b1, flags, rc)) return rc;
    if ((mant == nullptr) != (exp == nullptr)) return MI355Q_E_BADARG;
    if (y == nullptr && mant == nullptr) return MI355Q_E_BADARG;
    if (block_fp_args(a, width, exponent_width, exponent_bias, {mant ? 8 : 25, MI355Q_E_BADARG, MI355Q_E_BADARG})) return MI355Q_E_BADARG;
    a.mant = mant;
    a.code = exp;
    return launch_quant(a, 0, /*needs_fixup=*/mant != nullptr, static_cast<hipStream_t>(stream));
}

int mi355q_block_fp_quantize_bf16(const float* x, uint16_t* y, int64_t lead, int64_t rows, int64_t cols, int32_t b0,
                                  int32_t b1, int32_t width, int32_t exponent_width, int32_t exponent_bias,
                                  void* workspace, void* stream) {
    QuantArgs a;
    int rc;
    if (!fill_common(a, x, nullptr, workspace, lead, rows, cols, b0, b1, MI355Q_ZERO_BLOCK_FAST, rc)) return rc;
    if (y == nullptr) return MI355Q_E_BADARG;
    // (a quantised value must fit bf16's 8 significant bits)
    if ((rc = block_fp_args(a, width, exponent_width, exponent_bias, {9, MI355Q_E_BADARG, MI355Q_E_UNSUPPORTED})) != 0) return rc;
    a.ybf = y;
    return launch_quant(a, 0, /*needs_fixup=*/false, static_cast<hipStream_t>(stream));
}

int mi355q_block_fp_quantize_bf16_tiled(const float* x, float* y, uint16_t* y_tiled, int64_t rows, int64_t K, int32_t width,
                                        int32_t exponent_width, int32_t exponent_bias, void* workspace, void* stream) {
    return mi355q_block_fp_quantize_bf16_tiled_pre(x, nullptr, MI355Q_PRE_NONE, y, y_tiled, rows, K, width, exponent_width,
                                                   exponent_bias, workspace, stream);
}

int mi355q_block_fp_quantize_bf16_tiled_pre(const float* x, const float* x2, int32_t pre_op, float* y, uint16_t* y_tiled,
                                            int64_t rows, int64_t K, int32_t width, int32_t exponent_width,
                                            int32_t exponent_bias, void* workspace, void* stream) {
    if (pre_op == MI355Q_PRE_RMSNORM) return MI355Q_E_BADARG;            // (mi355q_block_fp_quantize_bf16_tiled_norm)
    return mi355q_block_fp_quantize_bf16_tiled_norm(x, x2, pre_op, 0.f, y, y_tiled, rows, K, width, exponent_width, exponent_bias,
                                                    workspace, stream);
}

int mi355q_block_fp_quantize_bf16_tiled_norm(const float* x, const float* x2, int32_t pre_op, float eps, float* y, uint16_t* y_tiled,
                                             int64_t rows, int64_t K, int32_t width, int32_t exponent_width,
                                             int32_t exponent_bias, void* workspace, void* stream) {
    if (pre_op == MI355Q_PRE_LAYERNORM || !pre_op_ok(pre_op, x2, pre_op == MI355Q_PRE_RMSNORM) || !(eps >= 0.f)) return MI355Q_E_BADARG;
    QuantArgs a;
    int rc;
    if (!fill_common(a, x, y, workspace, 1, rows, K, 1, 16, MI355Q_ZERO_BLOCK_FAST, rc)) return rc;
    a.x2 = x2;
    a.pre_op = pre_op;
    a.pre_eps = eps;
    if (y_tiled == nullptr) return MI355Q_E_BADARG;
    if ((rc = block_fp_args(a, width, exponent_width, exponent_bias, {9, MI355Q_E_BADARG, MI355Q_E_UNSUPPORTED})) != 0) return rc;
    if (K % 32 != 0) return MI355Q_E_UNSUPPORTED;               // (bf16's 8 significant bits: above;) whole 64-byte K-steps
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(y_tiled)) % 16) return MI355Q_E_ALIGN;
    return launch_quant_bf16_tiled(a, y_tiled, static_cast<hipStream_t>(stream));
}

int mi355q_block_minifloat_quantize_bf16_tiled(const float* x, uint16_t* y_tiled, int64_t rows, int64_t K, int32_t width,
                                               int32_t exponent_width, int32_t exponent_bias_width, void* workspace,
                                               void* stream) {
    QuantArgs a;
    int rc;
    if (!fill_common(a, x, nullptr, workspace, 1, rows, K, 1, 16, MI355Q_ZERO_BLOCK_FAST, rc)) return rc;
    if (y_tiled == nullptr) return MI355Q_E_BADARG;
    const int mbits = width - exponent_width - 1;
    if (exponent_width < 1 || exponent_width > 8 || mbits < 0 || mbits > 23) return MI355Q_E_BADARG;
    if (exponent_bias_width < 1 || exponent_bias_width > 8) return MI355Q_E_BADARG;
    if (mbits > 7 || K % 32 != 0) return MI355Q_E_UNSUPPORTED;      // bf16's 8 significant bits; whole 64-byte K-steps
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y_tiled)) % 16) return MI355Q_E_ALIGN;
    block_minifloat_fill(a, mbits, exponent_width, exponent_bias_width);
    return launch_quant_bf16_tiled(a, y_tiled, static_cast<hipStream_t>(stream), false, 1);
}

size_t mi355q_bfp_packed_bytes(int64_t rows, int64_t K, int32_t width) {
    return (rows <= 0 || K <= 0 || width < 2 || width > 8) ? 0 : (size_t)rows * (size_t)(K / 16) * (size_t)width * 2;
}

int mi355q_bfp_pack_bits(const int8_t* mant, uint8_t* packed, int64_t rows, int64_t K, int32_t width, void* stream) {
    if (rows < 0 || K < 0 || width < 2 || width > 8) return MI355Q_E_BADARG;
    if (rows == 0 || K == 0) return 0;
    if (!mant || !packed) return MI355Q_E_BADARG;
    if (K % 16 != 0) return MI355Q_E_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(mant) % 16 || reinterpret_cast<uintptr_t>(packed) % 2) return MI355Q_E_ALIGN;
    return launch_bfp_pack_bits(mant, reinterpret_cast<uint16_t*>(packed), rows, K, width, static_cast<hipStream_t>(stream));
}

int mi355q_bfp_expand(const uint8_t* packed, const uint8_t* codes, void* out_tiled, int64_t rows, int64_t K, int32_t width,
                      int32_t mode, int32_t exp_offset, const uint8_t* row_exp, uint8_t* exp_out, void* stream) {
    if (rows < 0 || K < 0 || width < 2 || width > 8 || (mode != 0 && mode != 1)) return MI355Q_E_BADARG;
    if (rows == 0 || K == 0) return 0;
    if (!packed || !codes || !out_tiled || ((exp_out != nullptr) != (row_exp != nullptr))) return MI355Q_E_BADARG;
    if (K % (mode == 0 ? 64 : 32) != 0) return MI355Q_E_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(packed) % 2 || reinterpret_cast<uintptr_t>(out_tiled) % 16) return MI355Q_E_ALIGN;
    return launch_bfp_expand(mode, reinterpret_cast<const uint16_t*>(packed), codes, out_tiled, rows, K, width, exp_offset,
                             static_cast<hipStream_t>(stream), row_exp, exp_out);
}

int mi355q_bfp_gemm_packed_small(const uint16_t* x_tiled, const uint8_t* packed, const uint8_t* codes, const uint8_t* row_exp,
                                 const int32_t* list, int32_t list_cap, const float* bias, float* y, int64_t M, int64_t N,
                                 int64_t K, int64_t ldy, int32_t x_mbits, int32_t x_exp_bias, int32_t w_mbits,
                                 int32_t w_exp_bias, void* stream) {
    if (M < 0 || N < 0 || K < 0 || x_mbits < 1 || x_mbits > 7 || w_mbits < 1 || w_mbits > 7) return MI355Q_E_BADARG;
    if (x_exp_bias < 0 || w_exp_bias < 0 || list_cap < 0 || list_cap > MI355Q_ROW_BUCKET_CAP_MAX) return MI355Q_E_BADARG;
    if (M == 0 || N == 0) return 0;
    if (!x_tiled || !packed || !codes || !y || (row_exp != nullptr && list == nullptr)) return MI355Q_E_BADARG;
    if (ldy < N) return MI355Q_E_BADARG;
    if (M > 16 || K == 0 || K % 64 != 0) return MI355Q_E_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(x_tiled) % 16 || reinterpret_cast<uintptr_t>(packed) % 16 || reinterpret_cast<uintptr_t>(codes) % 8 ||
        reinterpret_cast<uintptr_t>(y) % 4 || reinterpret_cast<uintptr_t>(bias) % 4 || reinterpret_cast<uintptr_t>(list) % 4)
        return MI355Q_E_ALIGN;
    PackedSmallArgs a;
    a.x_tiled = reinterpret_cast<const uint8_t*>(x_tiled);
    a.packed = packed; a.codes = codes; a.row_exp = row_exp;
    a.list = row_exp ? list : nullptr; a.list_cap = list_cap;
    a.bias = bias; a.y = y; a.M = M; a.N = N; a.K = K; a.ldy = ldy;
    a.width = w_mbits + 1; a.w_off = w_exp_bias + w_mbits;
    return launch_bfp_gemm_packed_small(a, static_cast<hipStream_t>(stream));
}

int mi355q_bf16_tile(const float* x, uint16_t* y_tiled, int64_t rows, int64_t K, void* stream) {
    QuantArgs a;
    int rc;
    if (!fill_common(a, x, nullptr, nullptr, 1, rows, K, 1, 16, MI355Q_ZERO_BLOCK_FAST, rc)) return rc;
    if (y_tiled == nullptr) return MI355Q_E_BADARG;
    if (K % 32 != 0) return MI355Q_E_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y_tiled)) % 16) return MI355Q_E_ALIGN;
    block_fp_fill(a, 8, 8, 127);                                 // bf16 itself
    return launch_quant_bf16_tiled(a, y_tiled, static_cast<hipStream_t>(stream), /*cast_only=*/true);
}

int mi355q_fp32_split_tile(const float* x, uint16_t* y_tiled, int64_t rows, int64_t K, int32_t role, void* stream) {
    if (rows < 0 || K < 0 || (role != 0 && role != 1)) return MI355Q_E_BADARG;
    if (rows == 0 || K == 0) return 0;
    if (!x || !y_tiled) return MI355Q_E_BADARG;
    if (K % 32 != 0) return MI355Q_E_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y_tiled)) % 16) return MI355Q_E_ALIGN;
    return launch_fp32_split_tile(x, y_tiled, rows, K, role, static_cast<hipStream_t>(stream));
}

static int bf16_gemm_tiled_impl(const uint16_t* x_tiled, const uint16_t* w_tiled, const float* bias, float* y, int64_t M, int64_t N,
                                int64_t K, int64_t ldy, int32_t x_segments, int64_t x_segment_stride_bytes, void* stream,
                                const float* residual = nullptr, int64_t ldr = 0) {
    if (M < 0 || N < 0 || K < 0 || ldy < N) return MI355Q_E_BADARG;
    if (M == 0 || N == 0) return 0;
    if (!y || (K > 0 && (!x_tiled || !w_tiled))) return MI355Q_E_BADARG;
    if (K % 32 != 0 || K == 0) return MI355Q_E_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(x_tiled) | reinterpret_cast<uintptr_t>(w_tiled)) % 16) return MI355Q_E_ALIGN;
    GemmArgs a{};
    a.xm = reinterpret_cast<const int8_t*>(x_tiled);
    a.wm = reinterpret_cast<const int8_t*>(w_tiled);
    a.bias = bias;
    a.y = y;
    a.M = M; a.N = N; a.K = 2 * K; a.ldy = ldy;      // (the tile kernel counts the contraction in bytes)
    a.x_segs = x_segments;
    a.x_seg_stride = x_segment_stride_bytes;
    a.resid = residual;
    a.ldr = ldr;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return timed(st, [&] { return launch_bf16_gemm_tiled(a, st); });
}

int mi355q_bf16_gemm_tiled(const uint16_t* x_tiled, const uint16_t* w_tiled, const float* bias, float* y, int64_t M, int64_t N,
                           int64_t K, int64_t ldy, void* stream) {
    return bf16_gemm_tiled_impl(x_tiled, w_tiled, bias, y, M, N, K, ldy, 1, 0, stream);
}

int mi355q_bf16_gemm_tiled_res(const uint16_t* x_tiled, const uint16_t* w_tiled, const float* bias, const float* residual, int64_t ldr,
                               float* y, int64_t M, int64_t N, int64_t K, int64_t ldy, void* stream) {
    if (!residual || ldr < N || ldr % 4 != 0) return MI355Q_E_BADARG;
    if (reinterpret_cast<uintptr_t>(residual) % 16) return MI355Q_E_ALIGN;
    return bf16_gemm_tiled_impl(x_tiled, w_tiled, bias, y, M, N, K, ldy, 1, 0, stream, residual, ldr);
}

int mi355q_bf16_gemm_tiled_seg(const uint16_t* x_tiled, const uint16_t* w_tiled, const float* bias, float* y, int64_t M, int64_t N,
                               int64_t K, int64_t ldy, int32_t x_segments, int64_t x_segment_stride_bytes, void* stream) {
    if (x_segments < 1 || (x_segments > 1 && (x_segment_stride_bytes <= 0 || x_segment_stride_bytes % 16))) return MI355Q_E_BADARG;
    if (x_segments > 1 && K > 0 && (K % (32 * (int64_t)x_segments) != 0)) return MI355Q_E_UNSUPPORTED;   // whole 64-byte K-steps per segment
    // (a stride shorter than one tiled segment would make the kernel read overlapping segments: wrong results with rc 0)
    if (x_segments > 1 && M > 0 && K > 0 && x_segment_stride_bytes < (int64_t)mi355q_bfp_tiled_bytes(M, 2 * K / x_segments)) return MI355Q_E_BADARG;
    return bf16_gemm_tiled_impl(x_tiled, w_tiled, bias, y, M, N, K, ldy, x_segments, x_segment_stride_bytes, stream);
}

int mi355q_block_minifloat_quantize(const float* x, float* y, uint8_t* bias, int64_t lead, int64_t rows, int64_t cols,
                                    int32_t b0, int32_t b1, int32_t width, int32_t exponent_width,
                                    int32_t exponent_bias_width, uint32_t flags, void* workspace, void* stream) {
    QuantArgs a;
    int rc;
    if (!fill_common(a, x, y, workspace, lead, rows, cols, b0, b1, flags, rc)) return rc;
    if (y == nullptr) return MI355Q_E_BADARG;
    const int mbits = width - exponent_width - 1;
    if (exponent_width < 1 || exponent_width > 8 || mbits < 0 || mbits > 23) return MI355Q_E_BADARG;
    if (exponent_bias_width < 1 || exponent_bias_width > 8) return MI355Q_E_BADARG;
    a.code = bias;
    block_minifloat_fill(a, mbits, exponent_width, exponent_bias_width);
    return launch_quant(a, 1, /*needs_fixup=*/bias != nullptr, static_cast<hipStream_t>(stream));
}

int mi355q_block_log_quantize(const float* x, float* y, uint8_t* bias, int64_t lead, int64_t rows, int64_t cols,
                              int32_t b0, int32_t b1, int32_t width, int32_t exponent_bias_width, uint32_t flags,
                              void* workspace, void* stream) {
    QuantArgs a;
    int rc;
    if (!fill_common(a, x, y, workspace, lead, rows, cols, b0, b1, flags, rc)) return rc;
    if (y == nullptr) return MI355Q_E_BADARG;
    if (width < 2 || width > 9) return MI355Q_E_BADARG;       // exponent code of width-1 <= 8 bits
    if (exponent_bias_width < 1 || exponent_bias_width > 8) return MI355Q_E_BADARG;
    a.code = bias;
    block_minifloat_fill(a, 0, width - 1, exponent_bias_width);
    return launch_quant(a, 2, /*needs_fixup=*/true, static_cast<hipStream_t>(stream));
}

// the block_minifloat / block_log fake-quantised values straight to bf16 (exact: <= 7 mantissa bits / signed powers of two;
// elements with |x| <= 1e-8, which the reference passes through, are rounded to bf16): the operands of a bf16-MFMA product
int mi355q_block_minifloat_quantize_bf16(const float* x, uint16_t* y, int64_t lead, int64_t rows, int64_t cols, int32_t b0,
                                         int32_t b1, int32_t width, int32_t exponent_width, int32_t exponent_bias_width,
                                         void* workspace, void* stream) {
    QuantArgs a;
    int rc;
    if (!fill_common(a, x, nullptr, workspace, lead, rows, cols, b0, b1, MI355Q_ZERO_BLOCK_FAST, rc)) return rc;
    if (y == nullptr) return MI355Q_E_BADARG;
    const int mbits = width - exponent_width - 1;
    if (exponent_width < 1 || exponent_width > 8 || mbits < 0) return MI355Q_E_BADARG;
    if (mbits > 7) return MI355Q_E_UNSUPPORTED;              // a quantised value must fit bf16's 8 significant bits
    if (exponent_bias_width < 1 || exponent_bias_width > 8) return MI355Q_E_BADARG;
    a.ybf = y;
    block_minifloat_fill(a, mbits, exponent_width, exponent_bias_width);
    return launch_quant(a, 1, /*needs_fixup=*/false, static_cast<hipStream_t>(stream));     // (an all-zero block stays zero)
}

int mi355q_block_log_quantize_bf16(const float* x, uint16_t* y, int64_t lead, int64_t rows, int64_t cols, int32_t b0,
                                   int32_t b1, int32_t width, int32_t exponent_bias_width, void* workspace, void* stream) {
    QuantArgs a;
    int rc;
    if (!fill_common(a, x, nullptr, workspace, lead, rows, cols, b0, b1, 0u, rc)) return rc;
    if (y == nullptr) return MI355Q_E_BADARG;
    if (width < 2 || width > 9) return MI355Q_E_BADARG;
    if (exponent_bias_width < 1 || exponent_bias_width > 8) return MI355Q_E_BADARG;
    // (all-zero blocks take the tensor-global fill -- a non-zero value here: the fix-up pass writes bf16 in its row-block form only)
    if (b0 != 1 || b1 != 16 || cols % 16 || reinterpret_cast<uintptr_t>(y) % 16) return MI355Q_E_UNSUPPORTED;
    a.ybf = y;
    block_minifloat_fill(a, 0, width - 1, exponent_bias_width);
    return launch_quant(a, 2, /*needs_fixup=*/true, static_cast<hipStream_t>(stream));
}

int mi355q_minifloat_quantize(const float* x, float* y, int64_t n, int32_t width, int32_t exponent_width, int32_t exponent_bias,
                              int32_t denorm, void* stream) {
    if (n < 0) return MI355Q_E_BADARG;
    if (n == 0) return 0;
    if (!x || !y) return MI355Q_E_BADARG;
    const int mbits = width - exponent_width - 1;
    if (exponent_width < 1 || exponent_width > 8 || mbits < 0 || mbits > 23) return MI355Q_E_BADARG;
    exponent_bias = default_bias(exponent_bias, exponent_width);
    if (exponent_bias < -100 || exponent_bias > 140) return MI355Q_E_UNSUPPORTED;      // (exponents must stay inside fp32's)
    QuantArgs a{};
    a.x = x; a.y = y; a.n_elems = n;
    a.span = (1 << exponent_width) - 1;                       // ieee: e in [-bias, span - bias]
    a.e_min = -exponent_bias;                                 // denorm: the same range
    a.e_max = a.span - exponent_bias;
    set_mantissa(a, mbits);
    return launch_quant_flat(a, denorm ? 3 : 1, exponent_bias, static_cast<hipStream_t>(stream));
}

int mi355q_log_quantize(const float* x, float* y, int64_t n, int32_t width, int32_t exponent_bias, void* stream) {
    if (n < 0 || width < 2 || width > 9) return MI355Q_E_BADARG;      // exponent code of width - 1 <= 8 bits
    if (n == 0) return 0;
    if (!x || !y) return MI355Q_E_BADARG;
    exponent_bias = default_bias(exponent_bias, width - 1);
    if (exponent_bias < -100 || exponent_bias > 140) return MI355Q_E_UNSUPPORTED;
    QuantArgs a{};
    a.x = x; a.y = y; a.n_elems = n;
    a.span = (1 << (width - 1)) - 1;
    set_mantissa(a, 0);
    return launch_quant_flat(a, 2, exponent_bias, static_cast<hipStream_t>(stream));
}

int mi355q_integer_quantize(const float* x, float* y, int64_t n, int32_t width, int32_t frac_width,
                            int32_t is_signed, void* stream) {
    if (n < 0 || width < 1 || width > 24) return MI355Q_E_BADARG;
    if (n == 0) return 0;
    if (x == nullptr || y == nullptr) return MI355Q_E_BADARG;
    const float lo = is_signed ? -std::ldexp(1.0f, width - 1) : 0.0f;
    const float hi = is_signed ? std::ldexp(1.0f, width - 1) - 1.0f : std::ldexp(1.0f, width) - 1.0f;
    return launch_integer(x, y, n, std::ldexp(1.0f, frac_width), lo, hi, static_cast<hipStream_t>(stream));
}

int mi355q_bfp_gemm(const int8_t* xm, const uint8_t* xe, const int8_t* wm, const uint8_t* we, const float* bias,
                    float* y, int64_t M, int64_t N, int64_t K, int64_t ldy, int32_t x_mbits, int32_t x_exp_bias,
                    int32_t w_mbits, int32_t w_exp_bias, void* stream) {
    if (M < 0 || N < 0 || K < 0 || ldy < N) return MI355Q_E_BADARG;
    if (M == 0 || N == 0) return 0;
    if (!y || (K > 0 && (!xm || !xe || !wm || !we))) return MI355Q_E_BADARG;
    if (K % 16 != 0) return MI355Q_E_UNSUPPORTED;
    if (x_mbits < 1 || x_mbits > 7 || w_mbits < 1 || w_mbits > 7) return MI355Q_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(xm) | reinterpret_cast<uintptr_t>(wm)) % 16) return MI355Q_E_ALIGN;
    GemmArgs a{xm, xe, wm, we, bias, y, M, N, K, ldy, x_exp_bias + x_mbits + w_exp_bias + w_mbits};
    return launch_bfp_gemm(a, static_cast<hipStream_t>(stream));
}

size_t mi355q_bfp_rowflag_bytes(int64_t rows, int64_t K) {
    if (rows <= 0 || K <= 0) return 0;
    return static_cast<size_t>(rows) * static_cast<size_t>((K + 255) / 256);
}

int64_t mi355q_bfp_rows_pad(int64_t rows) { return rows <= 0 ? 0 : (rows + 255) / 256 * 256 + 256; }

size_t mi355q_bfp_tiled_bytes(int64_t rows, int64_t K) {
    if (rows <= 0 || K <= 0) return 0;
    return static_cast<size_t>((rows + 127) / 128 * 128) * static_cast<size_t>((K + 63) / 64 * 64);
}

size_t mi355q_bfp_row_list_bytes(int64_t rows, int32_t bucket_cap) {
    if (rows < 0 || bucket_cap_bad(bucket_cap)) return 0;
    return (size_t)row_list_words(rows, bucket_cap_of(bucket_cap)) * 4;
}

int mi355q_bfp_align_rows(const int8_t* mant_in, const uint8_t* exp_in, int8_t* mant_tiled, uint8_t* exp_out,
                          uint8_t* rowflag, float* rowscale, int32_t* list, int32_t exp_offset, int64_t rows, int64_t K,
                          int32_t bucket_cap, void* stream) {
    if (rows < 0 || K < 0 || bucket_cap_bad(bucket_cap)) return MI355Q_E_BADARG;
    if (rows == 0 || K == 0) return 0;
    if (!mant_in || !exp_in || !mant_tiled || !exp_out || !rowflag || !rowscale) return MI355Q_E_BADARG;
    if (K % 64 != 0 || K > MI355Q_ROW_ALIGN_MAX_K) return MI355Q_E_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(mant_in) | reinterpret_cast<uintptr_t>(mant_tiled)) % 4) return MI355Q_E_ALIGN;
    return launch_bfp_align_rows(mant_in, exp_in, mant_tiled, exp_out, rowflag, rowscale, exp_offset, list, rows, K,
                                 static_cast<hipStream_t>(stream), bucket_cap_of(bucket_cap));
}

int mi355q_block_fp_quantize_aligned_rows(const float* x, int8_t* mant_tiled, uint8_t* exp_out, uint8_t* rowflag,
                                          float* rowscale, int32_t* list, int32_t* list_to_clear, int64_t rows,
                                          int64_t K, int32_t width, int32_t exponent_width, int32_t exponent_bias,
                                          int32_t bucket_cap, void* stream) {
    return mi355q_block_fp_quantize_aligned_rows_pre(x, nullptr, MI355Q_PRE_NONE, mant_tiled, exp_out, rowflag, rowscale, list,
                                                     list_to_clear, rows, K, width, exponent_width, exponent_bias, bucket_cap,
                                                     stream);
}

int mi355q_block_fp_quantize_aligned_rows_pre(const float* x, const float* x2, int32_t pre_op, int8_t* mant_tiled,
                                              uint8_t* exp_out, uint8_t* rowflag, float* rowscale, int32_t* list,
                                              int32_t* list_to_clear, int64_t rows, int64_t K, int32_t width,
                                              int32_t exponent_width, int32_t exponent_bias, int32_t bucket_cap,
                                              void* stream) {
    if (pre_op == MI355Q_PRE_LAYERNORM) return MI355Q_E_BADARG;          // (mi355q_block_fp_quantize_aligned_rows_norm)
    return mi355q_block_fp_quantize_aligned_rows_norm(x, x2, nullptr, pre_op, 0.f, mant_tiled, exp_out, rowflag, rowscale, list,
                                                      list_to_clear, rows, K, width, exponent_width, exponent_bias, bucket_cap,
                                                      stream);
}

int mi355q_block_fp_quantize_aligned_rows_norm(const float* x, const float* x2, const float* x3, int32_t pre_op, float eps,
                                               int8_t* mant_tiled,
                                               uint8_t* exp_out, uint8_t* rowflag, float* rowscale, int32_t* list,
                                               int32_t* list_to_clear, int64_t rows, int64_t K, int32_t width,
                                               int32_t exponent_width, int32_t exponent_bias, int32_t bucket_cap,
                                               void* stream) {
    return mi355q_block_fp_quantize_aligned_rows_seg(x, x2, x3, pre_op, eps, mant_tiled, exp_out, rowflag, rowscale, list,
                                                     list_to_clear, rows, K, 0, 0, width, exponent_width, exponent_bias,
                                                     bucket_cap, stream);
}

int mi355q_block_fp_quantize_aligned_rows_seg(const float* x, const float* x2, const float* x3, int32_t pre_op, float eps,
                                              int8_t* mant_tiled, uint8_t* exp_out, uint8_t* rowflag, float* rowscale,
                                              int32_t* list, int32_t* list_to_clear, int64_t rows, int64_t K, int64_t seg_len,
                                              int64_t seg_stride, int32_t width, int32_t exponent_width, int32_t exponent_bias,
                                              int32_t bucket_cap, void* stream) {
    if (seg_len < 0 || seg_stride < 0) return MI355Q_E_BADARG;
    if (seg_len > 0 && (seg_len % 4 || seg_stride % 4 || K % seg_len || seg_stride < rows * seg_len)) return MI355Q_E_BADARG;
    if (!pre_op_ok(pre_op, x2, true) || !(eps >= 0.f) || reinterpret_cast<uintptr_t>(x3) % 16) return MI355Q_E_BADARG;
    if (rows < 0 || K < 0 || bucket_cap_bad(bucket_cap, MI355Q_ROW_NO_ALIGN)) return MI355Q_E_BADARG;
    if (rows == 0 || K == 0) return 0;
    if (!x || !mant_tiled || !exp_out || !rowflag || !rowscale || (!list && bucket_cap >= 0) || (list && list_to_clear == list))
        return MI355Q_E_BADARG;
    if (K % 64 != 0 || K > MI355Q_ROW_ALIGN_MAX_K) return MI355Q_E_UNSUPPORTED;
    QuantArgs a{};
    if (block_fp_args(a, width, exponent_width, exponent_bias, {8, MI355Q_E_BADARG, MI355Q_E_BADARG})) return MI355Q_E_BADARG;
    if (reinterpret_cast<uintptr_t>(x) % 16 || reinterpret_cast<uintptr_t>(mant_tiled) % 16) return MI355Q_E_ALIGN;
    if (a.code_bias < 0) return MI355Q_E_UNSUPPORTED;            // biased uint8 exponent codes: non-negative biases only
    fill_rows(a, x, rows, K);
    a.x2 = x2;
    a.pre_op = pre_op;
    a.pre_eps = eps;
    a.x3 = pre_op == MI355Q_PRE_LAYERNORM ? x3 : nullptr;
    a.code = exp_out;
    a.seg_len = seg_len == K ? 0 : seg_len;                 // (one segment: plain rows)
    a.seg_stride = seg_stride;
    return launch_quant_align_rows(a, mant_tiled, rowflag, rowscale, a.code_bias + width - 1, list, list_to_clear,
                                   static_cast<hipStream_t>(stream), bucket_cap < 0 ? -1 : bucket_cap_of(bucket_cap));
}

// the class-aware activation quantiser of the mixed contraction (mi355q.h; mi355q_quant_cls.hip)
int mi355q_block_fp_quantize_classes(const float* x, const uint16_t* colmap, int64_t n0_blocks, int64_t n1_blocks, int8_t* mant_tiled,
                                     uint8_t* exp_out, uint8_t* rowflag, float* rowscale, int32_t* list, int32_t* list_to_clear,
                                     void* x1_bf16_tiled, int64_t rows, int64_t K, int32_t width, int32_t exponent_width,
                                     int32_t exponent_bias, int32_t bucket_cap, void* stream) {
    if (rows < 0 || K < 0 || n0_blocks < 0 || n1_blocks < 0 || bucket_cap_bad(bucket_cap)) return MI355Q_E_BADARG;
    if (rows == 0 || K == 0) return 0;
    if (!x || !colmap || !mant_tiled || !exp_out || !rowflag || !rowscale || !list || !x1_bf16_tiled || list_to_clear == list)
        return MI355Q_E_BADARG;
    // whole 64-byte K-steps in both operands: class 0 a multiple of 4 blocks, class 1 a multiple of 2
    if (K % 64 != 0 || K > MI355Q_ROW_ALIGN_MAX_K || (n0_blocks + n1_blocks) * 16 != K || n0_blocks % 4 || n1_blocks % 2 || n0_blocks >= 32768 ||
        n1_blocks >= 32768)
        return MI355Q_E_UNSUPPORTED;
    QuantArgs a{};
    if (block_fp_args(a, width, exponent_width, exponent_bias, {8, MI355Q_E_BADARG, MI355Q_E_BADARG})) return MI355Q_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(mant_tiled) | reinterpret_cast<uintptr_t>(x1_bf16_tiled)) % 16) return MI355Q_E_ALIGN;
    if (a.code_bias < 0) return MI355Q_E_UNSUPPORTED;
    fill_rows(a, x, rows, K);
    a.code = exp_out;
    return launch_quant_classes(a, colmap, (int)n0_blocks, (int)n1_blocks, mant_tiled, rowflag, rowscale, a.code_bias + width - 1, list,
                                list_to_clear, static_cast<uint16_t*>(x1_bf16_tiled), static_cast<hipStream_t>(stream),
                                bucket_cap_of(bucket_cap));
}

// y = x . w^T + bias on ROW-aligned tiled operands; with `residual` the add rides the store (the one-launch route only).  variant: what
// mi355q_bfp_gemm_set_variant set (0 the planned tile launch, 2 the blockwise kernel, 8 the tile kernel without lists)
static int gemm_aligned_impl(const mi355q_bfp_operand* x, const mi355q_bfp_operand* w, const float* bias, float* y, int64_t M, int64_t N,
                             int64_t K, int64_t ldy, void* stream, int variant, const float* residual = nullptr, int64_t ldr = 0) {
    if (!x || !w || M < 0 || N < 0 || K < 0 || ldy < N) return MI355Q_E_BADARG;
    if (M == 0 || N == 0) return 0;
    const OperandFaults fx = operand_faults(*x, ANY_ROWS), fw = operand_faults(*w, ANY_ROWS);
    if (!y || (K > 0 && (fx.missing || fw.missing))) return MI355Q_E_BADARG;
    if (K % 64 != 0) return MI355Q_E_UNSUPPORTED;   // tiled operands; use mi355q_bfp_gemm otherwise
    if (fx.mbits || fw.mbits) return MI355Q_E_BADARG;
    // both operands in the same alignment flavour; x may also be in row format with NOTHING aligned (row_aligned = 2)
    if (x->row_aligned != w->row_aligned && !(x->row_aligned == 2 && w->row_aligned == 1)) return MI355Q_E_BADARG;
    if (!x->row_aligned && x->list && w->list && x->list_cap != w->list_cap) return MI355Q_E_BADARG;
    if (fx.misaligned || fw.misaligned) return MI355Q_E_ALIGN;
    if (!x->row_aligned) return MI355Q_E_UNSUPPORTED;      // (operands aligned per 256-value group: the format went with its kernel)
    GemmArgs a = gemm_args(*x, *w, bias, y, M, N, K, ldy);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!x->gscale || !w->gscale || bucket_cap_bad(w->list_cap)) return MI355Q_E_BADARG;
    a.w_bcap = bucket_cap_of(w->list_cap);          // (before the early return: the kernel below indexes w's buckets)
    if (residual && x->row_aligned == 2) return MI355Q_E_UNSUPPORTED;
    if (x->row_aligned == 2)            // unaligned activations: the blockwise-exact kernel, w's exception blocks per tile
        return launch_bfp_gemm_aligned(a, x->rowflag, w->rowflag, nullptr, w->list, st);
    if (bucket_cap_bad(x->list_cap)) return MI355Q_E_BADARG;
    a.x_bcap = bucket_cap_of(x->list_cap);
    // x's exception blocks: in-LDS vectors of the GEMM (120-entry buckets) or the row post-pass (larger buckets)
    a.x_post = a.x_bcap != ROW_BCAP ? 1 : 0;
    const bool fast_ok = x->list && w->list && K % 128 == 0 && K <= MI355Q_ROW_ALIGN_MAX_K && a.w_bcap == ROW_BCAP;
    if (residual && (variant == 2 || variant == 8 || !fast_ok || a.x_post)) return MI355Q_E_UNSUPPORTED;
    a.resid = residual;
    a.ldr = ldr;
    if (variant == 2 || !fast_ok) return launch_bfp_gemm_aligned(a, x->rowflag, w->rowflag, x->list, w->list, st);
    if (variant == 8) return launch_bfp_gemm_v8(a, x->gscale, w->gscale, nullptr, nullptr, st);
    // ONE launch: the row-scale GEMM forms the correction vectors of its tile's exception blocks itself and adds them in its epilogue;
    // if an exception bucket overflowed anywhere its workgroups form the whole product blockwise-exact between them instead (decided on
    // the device)
    a.x_mbits = x->mbits;
    a.w_mbits = w->mbits;
    int rc = timed(st, [&] { return launch_bfp_gemm_v8(a, x->gscale, w->gscale, x->list, w->list, st, x->rowflag, w->rowflag); });
    if (rc == 0 && a.x_post) rc = launch_bfp_gemm_rowpost(a, x->list, w->list, x->gscale, w->gscale, st);
    return rc;
}

int mi355q_bfp_gemm_aligned(const mi355q_bfp_operand* x, const mi355q_bfp_operand* w, const float* bias, float* y,
                            int64_t M, int64_t N, int64_t K, int64_t ldy, void* stream) {
    return gemm_aligned_impl(x, w, bias, y, M, N, K, ldy, stream, g_gemm_variant.load());
}

int mi355q_bfp_gemm_aligned_res(const mi355q_bfp_operand* x, const mi355q_bfp_operand* w, const float* bias, const float* residual,
                                int64_t ldr, float* y, int64_t M, int64_t N, int64_t K, int64_t ldy, void* stream) {
    if (!residual || ldr < N || ldr % 4 != 0) return MI355Q_E_BADARG;
    if (misaligned16({residual})) return MI355Q_E_ALIGN;
    return gemm_aligned_impl(x, w, bias, y, M, N, K, ldy, stream, g_gemm_variant.load(), residual, ldr);
}

// ONE launch of the 256 x 256 tile kernel on its own operands (mi355q.h).  epi_op 0, mi355q_bfp_gemm_mixed: the contraction in two
// column classes, class 0 = K values as row-aligned int8 operands with their exception lists, class 1 = K1 values as tiled bf16
// operands x1 / w1, y with ldy.  epi_op 1 / 2, mi355q_bfp_gemm_aligned_gated / _relu: x . [gate; up]^T with the gated MLP's elementwise
// step, or x . w^T with relu, and the consumer's quantiser q_* in the store epilogue: y = scratch, yb = out_bf16_tiled, N = the layer's width
static int gemm_one_launch(int epi_op, const mi355q_bfp_operand* x, const mi355q_bfp_operand* w, const void* x1, const void* w1,
                           const float* bias, float* y, void* yb, int64_t M, int64_t N, int64_t K, int64_t K1, int64_t ldy, int32_t q_width,
                           int32_t q_exponent_width, int32_t q_exponent_bias, void* stream) {
    QuantArgs q{};
    if (!x || !w || M < 0 || N < 0 || K < 0 || (!epi_op && (K1 < 0 || ldy < N))) return MI355Q_E_BADARG;
    if (M == 0 || N == 0) return 0;
    const OperandFaults fx = operand_faults(*x, ONE_LAUNCH), fw = operand_faults(*w, ONE_LAUNCH);
    if (!y || (epi_op ? !yb : (!x1 || !w1)) || fx.missing || fw.missing) return MI355Q_E_BADARG;
    if (fx.mbits || fw.mbits) return MI355Q_E_BADARG;
    // (the consumer's values exact in bf16: <= 8 mantissa bits)
    if (epi_op && block_fp_args(q, q_width, q_exponent_width, q_exponent_bias, {9, MI355Q_E_UNSUPPORTED, MI355Q_E_UNSUPPORTED}))
        return MI355Q_E_UNSUPPORTED;
    if (fx.form || fw.form || K % 128 != 0 || K < 256 || K > MI355Q_ROW_ALIGN_MAX_K ||
        (epi_op ? N % 32 != 0 : (K1 % 64 != 0 || K1 < 128 || K1 > MI355Q_ROW_ALIGN_MAX_K)))
        return MI355Q_E_UNSUPPORTED;
    if (fx.misaligned || fw.misaligned || (epi_op ? misaligned16({yb, y}) : misaligned16({x1, w1}))) return MI355Q_E_ALIGN;
    if (epi_op == 1) N *= 2;
    GemmArgs a = gemm_args(*x, *w, bias, y, M, N, K, epi_op ? N : ldy);
    a.x_mbits = x->mbits;
    a.w_mbits = w->mbits;
    a.xm1 = static_cast<const int8_t*>(x1);
    a.wm1 = static_cast<const int8_t*>(w1);
    a.K1 = K1;
    a.yb = yb;
    a.epi_op = epi_op;
    if (epi_op) {
        a.q_mbits = q_width - 1;
        a.q_emin = q.e_min;
        a.q_emax = q.e_max;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const auto launch = epi_op ? launch_bfp_gemm_v9_gated : launch_bfp_gemm_v9_mixed;
    return timed(st, [&] { return launch(a, x->gscale, w->gscale, x->list, w->list, st, x->rowflag, w->rowflag); });
}

int mi355q_bfp_gemm_mixed(const mi355q_bfp_operand* x0, const mi355q_bfp_operand* w0, const void* x1, const void* w1, const float* bias,
                          float* y, int64_t M, int64_t N, int64_t K0, int64_t K1, int64_t ldy, void* stream) {
    return gemm_one_launch(0, x0, w0, x1, w1, bias, y, nullptr, M, N, K0, K1, ldy, 0, 0, 0, stream);
}

int mi355q_bfp_gemm_aligned_gated(const mi355q_bfp_operand* x, const mi355q_bfp_operand* w, const float* bias, float* scratch,
                                  void* out_bf16_tiled, int64_t M, int64_t I, int64_t K, int32_t q_width, int32_t q_exponent_width,
                                  int32_t q_exponent_bias, void* stream) {
    return gemm_one_launch(1, x, w, nullptr, nullptr, bias, scratch, out_bf16_tiled, M, I, K, 0, 0, q_width, q_exponent_width,
                           q_exponent_bias, stream);
}

int mi355q_bfp_gemm_aligned_relu(const mi355q_bfp_operand* x, const mi355q_bfp_operand* w, const float* bias, float* scratch,
                                 void* out_bf16_tiled, int64_t M, int64_t N, int64_t K, int32_t q_width, int32_t q_exponent_width,
                                 int32_t q_exponent_bias, void* stream) {
    return gemm_one_launch(2, x, w, nullptr, nullptr, bias, scratch, out_bf16_tiled, M, N, K, 0, 0, q_width, q_exponent_width,
                           q_exponent_bias, stream);
}

// `count` weights of one shape against ONE x in one grid: the same flavour, scales and bucket size everywhere
int mi355q_bfp_gemm_aligned_multi(const mi355q_bfp_operand* x, const mi355q_bfp_operand* const* w, const float* const* bias,
                                  float* const* y, int32_t count, int64_t M, int64_t N, int64_t K, int64_t ldy, void* stream) {
    if (!x || !w || !y || count < 1 || count > 3 || M < 0 || N < 0 || K < 0 || ldy < N) return MI355Q_E_BADARG;
    if (M == 0 || N == 0) return 0;
    for (int i = 0; i < count; ++i) {
        if (!w[i] || !y[i]) return MI355Q_E_BADARG;
        const OperandFaults fw = operand_faults(*w[i], ONE_LAUNCH);
        if (fw.missing) return MI355Q_E_BADARG;
        if (fw.form || w[i]->mbits != w[0]->mbits || w[i]->exp_bias != w[0]->exp_bias) return MI355Q_E_UNSUPPORTED;
        if (fw.misaligned) return MI355Q_E_ALIGN;
    }
    const OperandFaults fx = operand_faults(*x, ONE_LAUNCH);
    const int variant = g_gemm_variant.load();
    if (fx.missing) return MI355Q_E_BADARG;
    if (fx.form || K % 128 != 0 || K > MI355Q_ROW_ALIGN_MAX_K || variant != 0) return MI355Q_E_UNSUPPORTED;     // (callers then launch per weight)
    if (fx.mbits || w[0]->mbits < 1 || w[0]->mbits > 7) return MI355Q_E_BADARG;
    if (fx.misaligned) return MI355Q_E_ALIGN;
    if (count == 1) return gemm_aligned_impl(x, w[0], bias ? bias[0] : nullptr, y[0], M, N, K, ldy, stream, variant);
    GemmArgs a = gemm_args(*x, *w[0], bias ? bias[0] : nullptr, y[0], M, N, K, ldy);
    a.ngroup = count;
    for (int i = 0; i < count; ++i) {
        a.g_wm[i] = w[i]->mant; a.g_we[i] = w[i]->exp; a.g_sw[i] = w[i]->gscale; a.g_wlist[i] = w[i]->list;
        a.g_wf[i] = w[i]->rowflag; a.g_bias[i] = bias ? bias[i] : nullptr; a.g_y[i] = y[i];
    }
    a.x_mbits = x->mbits;
    a.w_mbits = w[0]->mbits;
    return launch_bfp_gemm_v8(a, x->gscale, w[0]->gscale, x->list, w[0]->list, static_cast<hipStream_t>(stream), x->rowflag, w[0]->rowflag);
}


// ---- W4A4 / W5A5 on the MX scaled matrix instruction (mi355q_mx.hip)
size_t mi355q_mx_plane_bytes(int64_t rows, int64_t K, int32_t plane) {
    if (rows <= 0 || K <= 0 || plane < 0 || plane > 2) return 0;
    const size_t rp = (size_t)((rows + 255) / 256 * 256), kp = (size_t)((K + 127) / 128 * 128);
    return plane == 0 ? rp * kp / 2 : (plane == 1 ? rp * kp / 4 : rp * kp / 32);
}

static int mx_quant_args(QuantArgs& a, const float* x, int64_t rows, int64_t K, int32_t width, int32_t exponent_width, int32_t exponent_bias) {
    if (rows < 0 || K < 0) return MI355Q_E_BADARG;
    if (K % 128 != 0 || K > MI355Q_ROW_ALIGN_MAX_K) return MI355Q_E_UNSUPPORTED;
    QuantArgs q{};
    // (<= 4 mantissa bits: exact in e2m3)
    if (block_fp_args(q, width, exponent_width, exponent_bias, {5, MI355Q_E_UNSUPPORTED, MI355Q_E_UNSUPPORTED}) || q.code_bias < 0) return MI355Q_E_UNSUPPORTED;
    a = q;
    fill_rows(a, x, rows, K);
    return 0;
}

int mi355q_block_fp_quantize_mx(const float* x, uint8_t* codes16, uint8_t* codes8, uint8_t* scales, int32_t* bad, int32_t* bad_to_clear,
                                int64_t rows, int64_t K, int32_t width, int32_t exponent_width, int32_t exponent_bias, void* stream) {
    QuantArgs a;
    if (const int rc = mx_quant_args(a, x, rows, K, width, exponent_width, exponent_bias)) return rc;
    if (rows == 0 || K == 0) return 0;
    if (!x || !codes16 || !codes8 || !scales || !bad) return MI355Q_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(codes16) | reinterpret_cast<uintptr_t>(codes8) | reinterpret_cast<uintptr_t>(scales)) % 16)
        return MI355Q_E_ALIGN;
    if (bad_to_clear == bad) return MI355Q_E_BADARG;
    // no "next call's word" to clear (a caller recording a HIP graph: the flag words cannot alternate between replays): this
    // call clears its OWN word in front of the kernel -- a memset node in the graph -- so that a replay whose activations fit
    // the format is never sent to the exact route by an earlier replay's flag
    if (!bad_to_clear) {
        if (hipMemsetAsync(bad, 0, sizeof(int32_t), static_cast<hipStream_t>(stream)) != hipSuccess) return (int)hipGetLastError();
    }
    return launch_quant_mx_rows(a, codes16, codes8, scales, bad, bad_to_clear, static_cast<hipStream_t>(stream));
}

int mi355q_mx_gemm(const uint8_t* x16, const uint8_t* x8, const uint8_t* xs, const uint8_t* w16, const uint8_t* w8, const uint8_t* ws,
                   const int32_t* bad2, const float* x_fp32, const float* w_fp32, const float* bias, float* y, int64_t M, int64_t N,
                   int64_t K, int64_t ldy, int32_t x_width, int32_t x_exponent_width, int32_t x_exponent_bias, void* stream) {
    if (M < 0 || N < 0 || ldy < N) return MI355Q_E_BADARG;
    MxGemmArgs a{};
    if (const int rc = mx_quant_args(a.qx, x_fp32, M, K, x_width, x_exponent_width, x_exponent_bias)) return rc;
    if (M == 0 || N == 0) return 0;
    if (K == 0 || !x16 || !x8 || !xs || !w16 || !w8 || !ws || !bad2 || !x_fp32 || !w_fp32 || !y) return MI355Q_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(x16) | reinterpret_cast<uintptr_t>(x8) | reinterpret_cast<uintptr_t>(xs) | reinterpret_cast<uintptr_t>(w16) |
         reinterpret_cast<uintptr_t>(w8) | reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(x_fp32) | reinterpret_cast<uintptr_t>(w_fp32)) % 16)
        return MI355Q_E_ALIGN;
    a.x16 = x16; a.x8 = x8; a.xs = xs; a.w16 = w16; a.w8 = w8; a.ws = ws;
    a.bad = bad2;
    a.xf = x_fp32; a.wf = w_fp32;
    a.bias = bias; a.y = y;
    a.M = M; a.N = N; a.K = K; a.ldy = ldy;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return timed(st, [&] { return launch_mx_gemm(a, st); });
}

size_t mi355q_bfp_matmul_workspace_bytes(int64_t B, int64_t K, int64_t N) {
    if (B <= 0 || K <= 0 || N <= 0) return 0;
    return (size_t)B * (size_t)((K + 63) / 64 * 64) * (size_t)N * 2 + 64;
}

static int bfp_matmul_impl(bool softmax, const float* mask, long long causal_off, const float* x, const float* y, float* out, void* workspace, int64_t B, int64_t M, int64_t K,
                      int64_t N, int32_t x_width, int32_t x_exponent_width, int32_t x_exponent_bias, int32_t y_width,
                      int32_t y_exponent_width, int32_t y_exponent_bias, void* stream) {
    if (B < 0 || M < 0 || K < 0 || N < 0) return MI355Q_E_BADARG;
    if (B == 0 || M == 0 || N == 0) return 0;
    if (!out || B > 65535) return MI355Q_E_BADARG;
    if (K == 0) return (int)hipMemsetAsync(out, 0, (size_t)B * M * N * 4, static_cast<hipStream_t>(stream));
    if (!x || !y || !workspace) return MI355Q_E_BADARG;
    if (x_exponent_width < 1 || x_exponent_width > 8 || y_exponent_width < 1 || y_exponent_width > 8) return MI355Q_E_BADARG;
    if (x_width < 2 || y_width < 2) return MI355Q_E_BADARG;
    // blocks of 16 along K (x) and N (y) must tile the operands; a quantised value must fit bf16's 8 significant bits
    if (K % 16 != 0 || N % 16 != 0 || x_width > 9 || y_width > 9) return MI355Q_E_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(workspace)) % 16)
        return MI355Q_E_ALIGN;
    QuantArgs ax{}, ay{};
    ax.b0 = ay.b0 = 1; ax.b1 = ay.b1 = 16;
    block_fp_fill(ax, x_width, x_exponent_width, x_exponent_bias);
    block_fp_fill(ay, y_width, y_exponent_width, y_exponent_bias);
    return launch_bfp_qmatmul(ax, ay, x, y, out, workspace, B, M, K, N, static_cast<hipStream_t>(stream), softmax, mask, causal_off);
}

unsigned long long mi355q_stream_capture_id(void* stream) {
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    if (hipStreamGetCaptureInfo(static_cast<hipStream_t>(stream), &status, &id) != hipSuccess) return 0;
    return status == hipStreamCaptureStatusActive ? (id ? id : ~0ull) : 0;
}

int mi355q_rope_apply(const float* q, const float* k, const float* cos_q, const float* sin_q, const int64_t* position_ids,
                      float* q_out, float* k_out, int64_t B, int64_t Hq, int64_t Hk, int64_t T, int64_t D, int64_t table_rows,
                      const int64_t* q_strides, const int64_t* k_strides, void* stream) {
    if (B < 0 || Hq < 0 || Hk < 0 || T < 0 || D < 0) return MI355Q_E_BADARG;
    if (B == 0 || T == 0 || D == 0 || (Hq == 0 && Hk == 0)) return 0;
    if (!q || !k || !cos_q || !sin_q || !position_ids || !q_out || !k_out || !q_strides || !k_strides || table_rows <= 0)
        return MI355Q_E_BADARG;
    if (D % 8 != 0) return MI355Q_E_UNSUPPORTED;              // float4 halves
    for (int i = 0; i < 3; ++i)
        if (q_strides[i] % 4 || k_strides[i] % 4) return MI355Q_E_ALIGN;
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(cos_q) |
         reinterpret_cast<uintptr_t>(sin_q) | reinterpret_cast<uintptr_t>(q_out) | reinterpret_cast<uintptr_t>(k_out)) % 16)
        return MI355Q_E_ALIGN;
    RopeArgs a{};
    a.x[0] = q; a.x[1] = k; a.y[0] = q_out; a.y[1] = k_out;
    a.sb[0] = q_strides[0]; a.sh[0] = q_strides[1]; a.st[0] = q_strides[2];
    a.sb[1] = k_strides[0]; a.sh[1] = k_strides[1]; a.st[1] = k_strides[2];
    a.heads[0] = Hq; a.heads[1] = Hk;
    a.cos = cos_q; a.sin = sin_q;
    a.pos = reinterpret_cast<const long long*>(position_ids);
    a.B = B; a.T = T; a.D = D; a.table_rows = table_rows;
    return launch_rope(a, static_cast<hipStream_t>(stream));
}

int mi355q_bfp_attention_set_kernel(int which) { return attention_set_kernel(which); }
int mi355q_bfp_attention_set_qpack(int on) { return attention_set_qpack(on); }

size_t mi355q_bfp_attention_workspace_bytes(int64_t B, int64_t T, int64_t D) {
    if (B <= 0 || T <= 0 || D <= 0) return 0;
    return attention_workspace_bytes(B, T, D);
}

int mi355q_bfp_attention(const float* q, const float* k, const float* v, const float* mask, int32_t causal, float scale_div,
                         float* out, void* workspace, int64_t B, int64_t M, int64_t T, int64_t D, const int32_t* qk_params,
                         const int32_t* pv_params, void* stream) {
    return mi355q_bfp_attention_strided(q, k, v, mask, causal, scale_div, out, workspace, B, M, T, D, qk_params, pv_params,
                                        nullptr, stream);
}

int mi355q_bfp_attention_strided(const float* q, const float* k, const float* v, const float* mask, int32_t causal, float scale_div,
                                 float* out, void* workspace, int64_t B, int64_t M, int64_t T, int64_t D,
                                 const int32_t* qk_params, const int32_t* pv_params, const int64_t* strides, void* stream) {
    return mi355q_bfp_attention_rope(q, k, v, mask, causal, scale_div, out, workspace, B, M, T, D, qk_params, pv_params, strides, nullptr,
                                     nullptr, nullptr, 0, 1, stream);
}

int mi355q_bfp_attention_rope(const float* q, const float* k, const float* v, const float* mask, int32_t causal, float scale_div,
                              float* out, void* workspace, int64_t B, int64_t M, int64_t T, int64_t D, const int32_t* qk_params,
                              const int32_t* pv_params, const int64_t* strides, const float* cos, const float* sin,
                              const int64_t* position_ids, int64_t table_rows, int32_t heads, void* stream) {
    return mi355q_bfp_attention_fused(q, k, v, mask, causal, 0.f, scale_div, out, nullptr, nullptr, workspace, B, M, T, D, qk_params, pv_params,
                                      strides, cos, sin, position_ids, table_rows, heads, stream);
}

int mi355q_bfp_attention_fused(const float* q, const float* k, const float* v, const float* mask, int32_t causal, float q_scale,
                               float scale_div, float* out, void* out_bf16_tiled, const int32_t* consumer_params, void* workspace, int64_t B, int64_t M,
                               int64_t T, int64_t D, const int32_t* qk_params, const int32_t* pv_params, const int64_t* strides,
                               const float* cos, const float* sin, const int64_t* position_ids, int64_t table_rows, int32_t heads,
                               void* stream) {
    QuantArgs ao{};
    if (out_bf16_tiled) {
        // the consumer's data_in quantiser {width, exponent width, exponent bias}; its operand is [M, B x D] in head order: ONE batch element
        if (!consumer_params || consumer_params[0] < 2 || consumer_params[1] < 1 || consumer_params[1] > 8 || (cos && heads != B)) return MI355Q_E_BADARG;
        if (consumer_params[0] > 9) return MI355Q_E_UNSUPPORTED;
        if (reinterpret_cast<uintptr_t>(out_bf16_tiled) % 16) return MI355Q_E_ALIGN;
        ao.b0 = 1; ao.b1 = 16;
        block_fp_fill(ao, consumer_params[0], consumer_params[1], consumer_params[2]);
        if (!out) out = reinterpret_cast<float*>(out_bf16_tiled);       // (never written; keeps the argument checks below uniform)
    }
    if (cos || sin || position_ids) {
        if (!cos || !sin || !position_ids || table_rows < 1 || heads < 1) return MI355Q_E_BADARG;
        if ((reinterpret_cast<uintptr_t>(cos) | reinterpret_cast<uintptr_t>(sin)) % 16 || reinterpret_cast<uintptr_t>(position_ids) % 8) return MI355Q_E_ALIGN;
    }
    if (B < 0 || M < 0 || T < 0 || D < 0) return MI355Q_E_BADARG;
    if (B == 0 || M == 0 || D == 0) return 0;
    if (!q || !k || !v || !out || !workspace || !qk_params || !pv_params || T == 0 || B > 65535) return MI355Q_E_BADARG;
    if (causal && T < M) return MI355Q_E_BADARG;              // (query i sees keys 0 .. i + T - M)
    for (int i = 0; i < 2; ++i) {
        const int32_t* pr = i ? pv_params : qk_params;
        if (pr[0] < 2 || pr[3] < 2 || pr[1] < 1 || pr[1] > 8 || pr[4] < 1 || pr[4] > 8) return MI355Q_E_BADARG;
        if (pr[0] > 9 || pr[3] > 9) return MI355Q_E_UNSUPPORTED;      // a quantised value must fit bf16's 8 significant bits
    }
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
         reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(mask)) % 16)
        return MI355Q_E_ALIGN;
    QuantArgs a[4] = {};
    for (int i = 0; i < 4; ++i) {
        const int32_t* pr = (i < 2 ? qk_params : pv_params) + 3 * (i & 1);
        a[i].b0 = 1; a[i].b1 = 16;
        block_fp_fill(a[i], pr[0], pr[1], pr[2]);
    }
    long long st6[8];
    if (strides)
        for (int i = 0; i < 8; ++i) {
            if (strides[i] % 4) return MI355Q_E_ALIGN;            // (16-byte loads / stores of every row)
            st6[i] = strides[i];
        }
    return launch_bfp_attention(a[0], a[1], a[2], a[3], q, k, v, mask, out, workspace, B, M, T, D, causal ? T - M : -1,
                                scale_div, static_cast<hipStream_t>(stream), strides ? st6 : nullptr, cos, sin,
                                reinterpret_cast<const long long*>(position_ids), table_rows, heads, static_cast<uint16_t*>(out_bf16_tiled),
                                out_bf16_tiled ? &ao : nullptr, q_scale);
}

int mi355q_bfp_attention_padded(const float* q, const float* k, const float* v, const int32_t* key_mask, int64_t heads, int32_t causal,
                                float q_scale, float scale_div, float* out, void* workspace, int64_t B, int64_t M, int64_t T, int64_t D,
                                const int32_t* qk_params, const int32_t* pv_params, const int64_t* strides, void* stream) {
    // (the checks of mi355q_bfp_attention_fused without its rotary / consumer arguments, and the mask's own)
    if (B < 0 || M < 0 || T < 0 || D < 0) return MI355Q_E_BADARG;
    if (!key_mask || heads < 1 || B % heads != 0) return MI355Q_E_BADARG;
    if (B == 0 || M == 0 || D == 0) return 0;
    if (!q || !k || !v || !out || !workspace || !qk_params || !pv_params || T == 0 || B > 65535) return MI355Q_E_BADARG;
    if (causal && T < M) return MI355Q_E_BADARG;
    for (int i = 0; i < 2; ++i) {
        const int32_t* pr = i ? pv_params : qk_params;
        if (pr[0] < 2 || pr[3] < 2 || pr[1] < 1 || pr[1] > 8 || pr[4] < 1 || pr[4] > 8) return MI355Q_E_BADARG;
        if (pr[0] > 9 || pr[3] > 9) return MI355Q_E_UNSUPPORTED;
    }
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
         reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(key_mask)) % 16)
        return MI355Q_E_ALIGN;
    QuantArgs a[4] = {};
    for (int i = 0; i < 4; ++i) {
        const int32_t* pr = (i < 2 ? qk_params : pv_params) + 3 * (i & 1);
        a[i].b0 = 1; a[i].b1 = 16;
        block_fp_fill(a[i], pr[0], pr[1], pr[2]);
    }
    long long st8[8];
    if (strides)
        for (int i = 0; i < 8; ++i) {
            if (strides[i] % 4) return MI355Q_E_ALIGN;
            st8[i] = strides[i];
        }
    return launch_bfp_attention_padded(a[0], a[1], a[2], a[3], q, k, v, key_mask, heads, out, workspace, B, M, T, D, causal ? T - M : -1,
                                       q_scale, scale_div, static_cast<hipStream_t>(stream), strides ? st8 : nullptr);
}

// ---- the KV cache and the attention that reads it (mi355q_decode.h, mi355q_extend.h, mi355q_kvp.h, mi355q_kvbm.h) --------------
// Every export below fills a KvCall, has kv_call_check (mi355q_kv_call.h) refuse it or fill what the launchers take, and launches.
// Uniform, ragged (per-row lengths on the device), grouped (G query rows a cache row), paged (pools of pages and a page table per row),
// int8 mantissas (kv8) and the sliding window differ in the KV_EXPORTS entry they start from and in the arguments they have.
namespace {
hipStream_t hs(void* stream) { return static_cast<hipStream_t>(stream); }
int sizes(const KvCall& d, int64_t* k_bytes, int64_t* v_bytes, int64_t* stage_bytes) {
    KvChecked c;
    int rc;
    if (!kv_call_check(d, c, rc)) return rc;
    const int64_t rows = kv_paged(d.storage) ? d.num_pages : d.B, keys = kv_paged(d.storage) ? d.P : d.C;      // (a page is a cache row of P keys)
    const KvMantissa m = kv_mantissa(d.storage);
    *k_bytes = kv_mantissas(d.storage) ? kvp_k_bytes(m, rows, keys, d.D) : kv_k_bytes(rows, keys, d.D);
    *v_bytes = kv_mantissas(d.storage) ? kvp_v_bytes(m, rows, keys, d.D) : kv_v_bytes(rows, keys, d.D);
    *stage_bytes = kv_stage_bytes(d.B, d.D);
    return 0;
}
int append(const KvCall& d, const float* k, const float* v, void* stream) {
    KvChecked c;
    int rc;
    if (!kv_call_check(d, c, rc)) return rc;
    if (kv_mantissas(d.storage))
        return launch_kvp_append(kv_mantissa(d.storage), c.cp, c.ak, c.av, k, v, c.st[0], c.st[1], c.st[2], c.st[3], d.lengths, d.counts, d.n, hs(stream), c.pages);
    if (d.form & KV_MINIFLOAT)
        return launch_kvbm_append(c.c, c.ak, c.av, k, v, c.st[0], c.st[1], c.st[2], c.st[3], d.lengths, d.counts, d.n, hs(stream));
    if (!(d.form & KV_LENGTHS)) return launch_kv_append(c.c, c.ak, c.av, k, v, c.st[0], c.st[1], c.st[2], c.st[3], d.L, d.n, hs(stream));
    return launch_kv_append_ragged(c.c, c.ak, c.av, k, v, c.st[0], c.st[1], c.st[2], c.st[3], d.lengths, d.counts, d.n, hs(stream), c.pages);
}
int dequantise(const KvCall& d, float* k_out, float* v_out, void* stream) {
    KvChecked c;
    int rc;
    if (!kv_call_check(d, c, rc)) return rc;
    if (kv_mantissas(d.storage))
        return launch_kvp_decode_fp32(kv_mantissa(d.storage), c.cp, c.ak, c.av, k_out, v_out, d.L, d.lengths, hs(stream), c.pages);
    return launch_kv_decode_fp32(c.c, k_out, v_out, d.L, hs(stream), d.lengths, c.pages);
}
int decode(const KvCall& d, const float* q, float* out, void* workspace, float q_scale, float scale_div, void* stream) {
    KvChecked c;
    int rc;
    if (!kv_call_check(d, c, rc)) return rc;
    if (kv_mantissas(d.storage))
        return launch_bfp_attention_decode_kvp(kv_mantissa(d.storage), c.aq, c.ap, c.ak, c.av, c.cp, q, out, workspace, d.M, d.L, c.causal, q_scale,
                                               scale_div, c.strides, d.splits, hs(stream), d.lengths, c.G, c.pages);
    if (d.form & KV_MINIFLOAT)
        return launch_bm_attention_decode(c.aq, c.ap, c.c, q, out, workspace, d.M, d.L, c.causal, q_scale, scale_div, c.strides, d.splits, hs(stream),
                                          d.lengths, c.G);
    if (d.form & KV_SINKS)
        return launch_bfp_attention_decode_sink(c.aq, c.ap, c.c, q, out, workspace, d.M, d.L, q_scale, scale_div, c.strides, d.splits, hs(stream),
                                                d.lengths, c.G, c.pages, c.window, c.sinks);
    return launch_bfp_attention_decode(c.aq, c.ap, c.c, q, out, workspace, d.M, d.L, c.causal, q_scale, scale_div, c.strides, d.splits, hs(stream),
                                       d.lengths, c.G, c.pages, c.window);
}
int extend(const KvCall& d, const float* q, float* out, float q_scale, float scale_div, void* stream) {
    KvChecked c;
    int rc;
    if (!kv_call_check(d, c, rc)) return rc;
    if (d.form & KV_SINKS)
        return launch_bfp_attention_extend_sink(c.aq, c.ap, c.c, q, out, d.M, d.L, q_scale, scale_div, c.strides, d.lengths, d.counts, hs(stream), c.G,
                                                c.pages, c.window, c.sinks);
    return launch_bfp_attention_extend(c.aq, c.ap, c.c, q, out, d.M, d.L, c.causal, q_scale, scale_div, c.strides, d.lengths, d.counts, hs(stream),
                                       c.G, c.pages, c.window);
}
}  // namespace

int mi355q_bfp_kv_cache_bytes(int64_t B, int64_t C, int64_t D, int64_t* k_bytes, int64_t* v_bytes, int64_t* stage_bytes) {
    return sizes(KvCall(KV_EXPORTS[KVX_CACHE_BYTES]).cache(nullptr, nullptr, nullptr, B, C, D).sizes(k_bytes, v_bytes, stage_bytes), k_bytes, v_bytes,
                 stage_bytes);
}

int mi355q_bfp_kv_append(void* kq, void* vq, float* stage, const float* k, const float* v, int64_t B, int64_t C, int64_t D,
                         int64_t L, int64_t n, const int32_t* qk_params, const int32_t* pv_params, const int64_t* strides,
                         void* stream) {
    return append(KvCall(KV_EXPORTS[KVX_APPEND]).cache(kq, vq, stage, B, C, D).rows(k, v, n).lens(nullptr, nullptr, L).quant(qk_params, pv_params, strides),
                  k, v, stream);
}

int mi355q_bfp_kv_decode_fp32(const void* kq, const void* vq, float* k_out, float* v_out, int64_t B, int64_t C, int64_t D, int64_t L,
                              void* stream) {
    return dequantise(KvCall(KV_EXPORTS[KVX_DECODE_FP32]).cache(kq, vq, nullptr, B, C, D).rows(k_out, v_out, 0).lens(nullptr, nullptr, L), k_out, v_out,
                      stream);
}

int mi355q_bfp_attention_decode_splits(int64_t B, int64_t L, int64_t D, int32_t splits) { return decode_splits(B, L, D, splits); }

size_t mi355q_bfp_attention_decode_workspace_bytes(int64_t B, int64_t L, int64_t D, int32_t splits) {
    if (B <= 0 || L <= 0 || D <= 0 || D % 32 != 0 || D > 128) return 0;
    return decode_workspace_bytes(B, L, D, splits);
}

int mi355q_bfp_attention_decode(const float* q, const void* kq, const void* vq, int32_t causal, float q_scale, float scale_div,
                                float* out, void* workspace, int64_t B, int64_t M, int64_t L, int64_t C, int64_t D,
                                const int32_t* qk_params, const int32_t* pv_params, const int64_t* strides, int32_t splits,
                                void* stream) {
    return decode(KvCall(KV_EXPORTS[KVX_DECODE]).cache(kq, vq, nullptr, B, C, D).lens(nullptr, nullptr, L).query(q, out, workspace, M, 0, causal, 0, splits)
                      .quant(qk_params, pv_params, strides), q, out, workspace, q_scale, scale_div, stream);
}

// ragged batches: per-row lengths on the device
int mi355q_bfp_kv_append_ragged(void* kq, void* vq, float* stage, const float* k, const float* v, const int32_t* lengths,
                                const int32_t* counts, int64_t B, int64_t C, int64_t D, int64_t n, int64_t max_length,
                                const int32_t* qk_params, const int32_t* pv_params, const int64_t* strides, void* stream) {
    return append(KvCall(KV_EXPORTS[KVX_APPEND_RAGGED]).cache(kq, vq, stage, B, C, D).rows(k, v, n).lens(lengths, counts, max_length)
                      .quant(qk_params, pv_params, strides), k, v, stream);
}

int mi355q_bfp_kv_decode_fp32_ragged(const void* kq, const void* vq, const int32_t* lengths, float* k_out, float* v_out, int64_t B,
                                     int64_t C, int64_t D, int64_t max_length, void* stream) {
    return dequantise(KvCall(KV_EXPORTS[KVX_DECODE_FP32_RAGGED]).cache(kq, vq, nullptr, B, C, D).rows(k_out, v_out, 0).lens(lengths, nullptr, max_length),
                      k_out, v_out, stream);
}

int mi355q_bfp_attention_decode_ragged(const float* q, const void* kq, const void* vq, const int32_t* lengths, int32_t causal,
                                       float q_scale, float scale_div, float* out, void* workspace, int64_t B, int64_t M,
                                       int64_t max_length, int64_t C, int64_t D, const int32_t* qk_params, const int32_t* pv_params,
                                       const int64_t* strides, int32_t splits, void* stream) {
    return decode(KvCall(KV_EXPORTS[KVX_DECODE_RAGGED]).cache(kq, vq, nullptr, B, C, D).lens(lengths, nullptr, max_length)
                      .query(q, out, workspace, M, 0, causal, 0, splits).quant(qk_params, pv_params, strides), q, out, workspace, q_scale, scale_div, stream);
}

// chunked prefill: any number of queries per row behind the cache; lengths == NULL is the uniform form
int mi355q_bfp_attention_extend(const float* q, const void* kq, const void* vq, const int32_t* lengths, const int32_t* counts,
                                int32_t causal, float q_scale, float scale_div, float* out, int64_t B, int64_t M, int64_t max_length,
                                int64_t C, int64_t D, const int32_t* qk_params, const int32_t* pv_params, const int64_t* strides,
                                void* stream) {
    return extend(KvCall(KV_EXPORTS[KVX_EXTEND]).cache(kq, vq, nullptr, B, C, D).lens(lengths, counts, max_length).query(q, out, nullptr, M, 0, causal, 0, 0)
                      .quant(qk_params, pv_params, strides), q, out, q_scale, scale_div, stream);
}

// grouped queries: G query rows a cache row, query row r on cache row r / G
int mi355q_bfp_attention_decode_group_width(int64_t G, int64_t M) { return decode_group_width(G, M); }

int mi355q_bfp_attention_decode_grouped(const float* q, const void* kq, const void* vq, int32_t G, const int32_t* lengths,
                                        int32_t causal, float q_scale, float scale_div, float* out, void* workspace, int64_t B,
                                        int64_t M, int64_t max_length, int64_t C, int64_t D, const int32_t* qk_params,
                                        const int32_t* pv_params, const int64_t* strides, int32_t splits, void* stream) {
    return decode(KvCall(KV_EXPORTS[KVX_DECODE_GROUPED]).cache(kq, vq, nullptr, B, C, D).lens(lengths, nullptr, max_length)
                      .query(q, out, workspace, M, G, causal, 0, splits).quant(qk_params, pv_params, strides), q, out, workspace, q_scale, scale_div, stream);
}

int mi355q_bfp_attention_extend_grouped(const float* q, const void* kq, const void* vq, int32_t G, const int32_t* lengths,
                                        const int32_t* counts, int32_t causal, float q_scale, float scale_div, float* out, int64_t B,
                                        int64_t M, int64_t max_length, int64_t C, int64_t D, const int32_t* qk_params,
                                        const int32_t* pv_params, const int64_t* strides, void* stream) {
    return extend(KvCall(KV_EXPORTS[KVX_EXTEND_GROUPED]).cache(kq, vq, nullptr, B, C, D).lens(lengths, counts, max_length)
                      .query(q, out, nullptr, M, G, causal, 0, 0).quant(qk_params, pv_params, strides), q, out, q_scale, scale_div, stream);
}

// paged cache: pools of pages and a page table per row; always the ragged form
int mi355q_bfp_kv_paged_bytes(int64_t num_pages, int64_t P, int64_t B, int64_t D, int64_t* k_bytes, int64_t* v_bytes, int64_t* stage_bytes) {
    return sizes(KvCall(KV_EXPORTS[KVX_PAGED_BYTES]).pools(nullptr, nullptr, nullptr, nullptr, B, 0, num_pages, P, D).sizes(k_bytes, v_bytes, stage_bytes),
                 k_bytes, v_bytes, stage_bytes);
}

int mi355q_bfp_kv_append_paged(void* kq_pool, void* vq_pool, float* stage, const float* k, const float* v, const int32_t* lengths,
                               const int32_t* counts, const int32_t* block_table, int64_t B, int64_t max_pages, int64_t num_pages,
                               int64_t P, int64_t D, int64_t n, int64_t max_length, const int32_t* qk_params, const int32_t* pv_params,
                               const int64_t* strides, void* stream) {
    return append(KvCall(KV_EXPORTS[KVX_APPEND_PAGED]).pools(kq_pool, vq_pool, stage, block_table, B, max_pages, num_pages, P, D).rows(k, v, n)
                      .lens(lengths, counts, max_length).quant(qk_params, pv_params, strides), k, v, stream);
}

int mi355q_bfp_kv_decode_fp32_paged(const void* kq_pool, const void* vq_pool, const int32_t* lengths, const int32_t* block_table,
                                    float* k_out, float* v_out, int64_t B, int64_t max_pages, int64_t num_pages, int64_t P, int64_t D,
                                    int64_t max_length, void* stream) {
    return dequantise(KvCall(KV_EXPORTS[KVX_DECODE_FP32_PAGED]).pools(kq_pool, vq_pool, nullptr, block_table, B, max_pages, num_pages, P, D)
                          .rows(k_out, v_out, 0).lens(lengths, nullptr, max_length), k_out, v_out, stream);
}

int mi355q_bfp_attention_decode_paged(const float* q, const void* kq_pool, const void* vq_pool, int32_t G, const int32_t* lengths,
                                      const int32_t* block_table, int32_t causal, float q_scale, float scale_div, float* out,
                                      void* workspace, int64_t B, int64_t M, int64_t max_length, int64_t max_pages, int64_t num_pages,
                                      int64_t P, int64_t D, const int32_t* qk_params, const int32_t* pv_params, const int64_t* strides,
                                      int32_t splits, void* stream) {
    return decode(KvCall(KV_EXPORTS[KVX_DECODE_PAGED]).pools(kq_pool, vq_pool, nullptr, block_table, B, max_pages, num_pages, P, D)
                      .lens(lengths, nullptr, max_length).query(q, out, workspace, M, G, causal, 0, splits).quant(qk_params, pv_params, strides),
                  q, out, workspace, q_scale, scale_div, stream);
}

int mi355q_bfp_attention_extend_paged(const float* q, const void* kq_pool, const void* vq_pool, int32_t G, const int32_t* lengths,
                                      const int32_t* counts, const int32_t* block_table, int32_t causal, float q_scale, float scale_div,
                                      float* out, int64_t B, int64_t M, int64_t max_length, int64_t max_pages, int64_t num_pages,
                                      int64_t P, int64_t D, const int32_t* qk_params, const int32_t* pv_params, const int64_t* strides,
                                      void* stream) {
    return extend(KvCall(KV_EXPORTS[KVX_EXTEND_PAGED]).pools(kq_pool, vq_pool, nullptr, block_table, B, max_pages, num_pages, P, D)
                      .lens(lengths, counts, max_length).query(q, out, nullptr, M, G, causal, 0, 0).quant(qk_params, pv_params, strides),
                  q, out, q_scale, scale_div, stream);
}

// copy-on-write (fork, reorder): whole pages and stage rows by a device list of jobs, one launch; its check is mi355q_kv_copy.h's
int mi355q_bfp_kv_paged_copy(void* kq_pool, void* vq_pool, const float* stage_src, float* stage_dst, const int32_t* jobs, int64_t n_jobs,
                             int64_t B, int64_t num_pages, int64_t P, int64_t D, void* stream) {
    KvCopyArgs g;
    int rc;
    if (!kv_copy_check(kq_pool, vq_pool, stage_src, stage_dst, jobs, n_jobs, B, num_pages, P, D, false, g, rc)) return rc;
    return launch_kv_paged_copy(g, stream);
}

// int8-mantissa cache: mantissa bytes and one exponent byte a block; always the ragged form, contiguous
int mi355q_bfp_kv8_cache_bytes(int64_t B, int64_t C, int64_t D, int64_t* k_bytes, int64_t* v_bytes, int64_t* stage_bytes) {
    return sizes(KvCall(KV_EXPORTS[KVX_KV8_CACHE_BYTES]).cache(nullptr, nullptr, nullptr, B, C, D).sizes(k_bytes, v_bytes, stage_bytes), k_bytes, v_bytes,
                 stage_bytes);
}

int mi355q_bfp_kv8_append(void* k8, void* v8, float* stage, const float* k, const float* v, const int32_t* lengths,
                          const int32_t* counts, int64_t B, int64_t C, int64_t D, int64_t n, int64_t max_length,
                          const int32_t* qk_params, const int32_t* pv_params, const int64_t* strides, void* stream) {
    return append(KvCall(KV_EXPORTS[KVX_KV8_APPEND]).cache(k8, v8, stage, B, C, D).rows(k, v, n).lens(lengths, counts, max_length)
                      .quant(qk_params, pv_params, strides), k, v, stream);
}

int mi355q_bfp_kv8_decode_fp32(const void* k8, const void* v8, const int32_t* lengths, float* k_out, float* v_out, int64_t B, int64_t C,
                               int64_t D, int64_t max_length, const int32_t* qk_params, const int32_t* pv_params, void* stream) {
    return dequantise(KvCall(KV_EXPORTS[KVX_KV8_DECODE_FP32]).cache(k8, v8, nullptr, B, C, D).rows(k_out, v_out, 0).lens(lengths, nullptr, max_length)
                          .quant(qk_params, pv_params, nullptr), k_out, v_out, stream);
}

int mi355q_bfp_attention_decode_kv8(const float* q, const void* k8, const void* v8, int32_t G, const int32_t* lengths, int32_t causal,
                                    float q_scale, float scale_div, float* out, void* workspace, int64_t B, int64_t M,
                                    int64_t max_length, int64_t C, int64_t D, const int32_t* qk_params, const int32_t* pv_params,
                                    const int64_t* strides, int32_t splits, void* stream) {
    return decode(KvCall(KV_EXPORTS[KVX_DECODE_KV8]).cache(k8, v8, nullptr, B, C, D).lens(lengths, nullptr, max_length)
                      .query(q, out, workspace, M, G, causal, 0, splits).quant(qk_params, pv_params, strides), q, out, workspace, q_scale, scale_div, stream);
}

// int8-mantissa cache in pages: the pools of the paged cache holding the 544-byte pieces above; always the ragged form, no extend, no window
int mi355q_bfp_kv8_paged_bytes(int64_t num_pages, int64_t P, int64_t B, int64_t D, int64_t* k_bytes, int64_t* v_bytes, int64_t* stage_bytes) {
    return sizes(KvCall(KV_EXPORTS[KVX_KV8P_BYTES]).pools(nullptr, nullptr, nullptr, nullptr, B, 0, num_pages, P, D).sizes(k_bytes, v_bytes, stage_bytes),
                 k_bytes, v_bytes, stage_bytes);
}

int mi355q_bfp_kv8_append_paged(void* k8_pool, void* v8_pool, float* stage, const float* k, const float* v, const int32_t* lengths,
                                const int32_t* counts, const int32_t* block_table, int64_t B, int64_t max_pages, int64_t num_pages,
                                int64_t P, int64_t D, int64_t n, int64_t max_length, const int32_t* qk_params, const int32_t* pv_params,
                                const int64_t* strides, void* stream) {
    return append(KvCall(KV_EXPORTS[KVX_KV8P_APPEND]).pools(k8_pool, v8_pool, stage, block_table, B, max_pages, num_pages, P, D).rows(k, v, n)
                      .lens(lengths, counts, max_length).quant(qk_params, pv_params, strides), k, v, stream);
}

int mi355q_bfp_kv8_decode_fp32_paged(const void* k8_pool, const void* v8_pool, const int32_t* lengths, const int32_t* block_table,
                                     float* k_out, float* v_out, int64_t B, int64_t max_pages, int64_t num_pages, int64_t P, int64_t D,
                                     int64_t max_length, const int32_t* qk_params, const int32_t* pv_params, void* stream) {
    return dequantise(KvCall(KV_EXPORTS[KVX_KV8P_DECODE_FP32]).pools(k8_pool, v8_pool, nullptr, block_table, B, max_pages, num_pages, P, D)
                          .rows(k_out, v_out, 0).lens(lengths, nullptr, max_length).quant(qk_params, pv_params, nullptr), k_out, v_out, stream);
}

int mi355q_bfp_attention_decode_kv8_paged(const float* q, const void* k8_pool, const void* v8_pool, int32_t G, const int32_t* lengths,
                                          const int32_t* block_table, int32_t causal, float q_scale, float scale_div, float* out,
                                          void* workspace, int64_t B, int64_t M, int64_t max_length, int64_t max_pages, int64_t num_pages,
                                          int64_t P, int64_t D, const int32_t* qk_params, const int32_t* pv_params, const int64_t* strides,
                                          int32_t splits, void* stream) {
    return decode(KvCall(KV_EXPORTS[KVX_KV8P_DECODE]).pools(k8_pool, v8_pool, nullptr, block_table, B, max_pages, num_pages, P, D)
                      .lens(lengths, nullptr, max_length).query(q, out, workspace, M, G, causal, 0, splits).quant(qk_params, pv_params, strides),
                  q, out, workspace, q_scale, scale_div, stream);
}

// its copy-on-write: mi355q_bfp_kv_paged_copy's kernel and check on pages of P * D * 17 / 16 bytes
int mi355q_bfp_kv8_paged_copy(void* k8_pool, void* v8_pool, const float* stage_src, float* stage_dst, const int32_t* jobs, int64_t n_jobs,
                              int64_t B, int64_t num_pages, int64_t P, int64_t D, void* stream) {
    KvCopyArgs g;
    int rc;
    if (!kv_copy_check(k8_pool, v8_pool, stage_src, stage_dst, jobs, n_jobs, B, num_pages, P, D, true, g, rc)) return rc;
    return launch_kv_paged_copy(g, stream);
}

// 4-bit-mantissa cache: two mantissa nibbles a byte and one exponent byte a block (mi355q_kvp.h); always the ragged form, contiguous
int mi355q_bfp_kv4_cache_bytes(int64_t B, int64_t C, int64_t D, int64_t* k_bytes, int64_t* v_bytes, int64_t* stage_bytes) {
    return sizes(KvCall(KV_EXPORTS[KVX_KV4_CACHE_BYTES]).cache(nullptr, nullptr, nullptr, B, C, D).sizes(k_bytes, v_bytes, stage_bytes), k_bytes, v_bytes,
                 stage_bytes);
}

int mi355q_bfp_kv4_append(void* k4, void* v4, float* stage, const float* k, const float* v, const int32_t* lengths,
                          const int32_t* counts, int64_t B, int64_t C, int64_t D, int64_t n, int64_t max_length,
                          const int32_t* qk_params, const int32_t* pv_params, const int64_t* strides, void* stream) {
    return append(KvCall(KV_EXPORTS[KVX_KV4_APPEND]).cache(k4, v4, stage, B, C, D).rows(k, v, n).lens(lengths, counts, max_length)
                      .quant(qk_params, pv_params, strides), k, v, stream);
}

int mi355q_bfp_kv4_decode_fp32(const void* k4, const void* v4, const int32_t* lengths, float* k_out, float* v_out, int64_t B, int64_t C,
                               int64_t D, int64_t max_length, const int32_t* qk_params, const int32_t* pv_params, void* stream) {
    return dequantise(KvCall(KV_EXPORTS[KVX_KV4_DECODE_FP32]).cache(k4, v4, nullptr, B, C, D).rows(k_out, v_out, 0).lens(lengths, nullptr, max_length)
                          .quant(qk_params, pv_params, nullptr), k_out, v_out, stream);
}

int mi355q_bfp_attention_decode_kv4(const float* q, const void* k4, const void* v4, int32_t G, const int32_t* lengths, int32_t causal,
                                    float q_scale, float scale_div, float* out, void* workspace, int64_t B, int64_t M,
                                    int64_t max_length, int64_t C, int64_t D, const int32_t* qk_params, const int32_t* pv_params,
                                    const int64_t* strides, int32_t splits, void* stream) {
    return decode(KvCall(KV_EXPORTS[KVX_DECODE_KV4]).cache(k4, v4, nullptr, B, C, D).lens(lengths, nullptr, max_length)
                      .query(q, out, workspace, M, G, causal, 0, splits).quant(qk_params, pv_params, strides), q, out, workspace, q_scale, scale_div, stream);
}

// block_minifloat cache: KVCache's storage and layout, the block_minifloat quantisers (mi355q_kvbm.h); always the ragged form, contiguous
int mi355q_bm_kv_append(void* kq, void* vq, float* stage, const float* k, const float* v, const int32_t* lengths, const int32_t* counts,
                        int64_t B, int64_t C, int64_t D, int64_t n, int64_t max_length, const int32_t* qk_params, const int32_t* pv_params,
                        const int64_t* strides, void* stream) {
    return append(KvCall(KV_EXPORTS[KVX_BM_APPEND]).cache(kq, vq, stage, B, C, D).rows(k, v, n).lens(lengths, counts, max_length)
                      .quant(qk_params, pv_params, strides), k, v, stream);
}

int mi355q_bm_attention_decode(const float* q, const void* kq, const void* vq, int32_t G, const int32_t* lengths, int32_t causal,
                               float q_scale, float scale_div, float* out, void* workspace, int64_t B, int64_t M, int64_t max_length,
                               int64_t C, int64_t D, const int32_t* qk_params, const int32_t* pv_params, const int64_t* strides,
                               int32_t splits, void* stream) {
    return decode(KvCall(KV_EXPORTS[KVX_BM_DECODE]).cache(kq, vq, nullptr, B, C, D).lens(lengths, nullptr, max_length)
                      .query(q, out, workspace, M, G, causal, 0, splits).quant(qk_params, pv_params, strides), q, out, workspace, q_scale, scale_div, stream);
}

// the one-pass attention core of a block_minifloat layer (mi355q_attention_bm.h): pack launch + streaming launch, no cache involved
size_t mi355q_bm_attention_workspace_bytes(int64_t B, int64_t T, int64_t D) {
    if (B <= 0 || T <= 0 || D <= 0) return 0;
    return bm_attention_workspace_bytes(B, T, D);
}

int mi355q_bm_attention(const float* q, const float* k, const float* v, float* out, void* workspace, int64_t B, int64_t M, int64_t T,
                        int64_t D, const int32_t* qk_params, const int32_t* pv_params, const int64_t* strides, int32_t causal,
                        float scale_div, float q_scale, void* stream) {
    if (B < 0 || M < 0 || T < 0 || D < 0) return MI355Q_E_BADARG;
    if (B == 0 || M == 0) return 0;
    if (!q || !k || !v || !out || !workspace || !qk_params || !pv_params || T == 0 || B > 65535) return MI355Q_E_BADARG;
    if (T % 16 != 0 || (D != 32 && D != 64 && D != 96 && D != 128) || (causal && M > T)) return MI355Q_E_UNSUPPORTED;
    QuantArgs a[4] = {};                                    // Q, K^T, P, V
    int rc;
    if ((rc = bm_quant_pair(qk_params, pv_params, 0, a[0], a[2])) != 0 || (rc = bm_quant_pair(qk_params, pv_params, 3, a[1], a[3])) != 0) return rc;
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(out) |
         reinterpret_cast<uintptr_t>(workspace)) % 16)
        return MI355Q_E_ALIGN;
    long long st8[8];
    if (strides)
        for (int i = 0; i < 8; ++i) {
            if (strides[i] % 4) return MI355Q_E_ALIGN;            // (16-byte loads / stores of every row)
            st8[i] = strides[i];
        }
    return launch_bm_attention(a[0], a[1], a[2], a[3], q, k, v, out, workspace, B, M, T, D, causal ? T - M : -1, q_scale, scale_div,
                               strides ? st8 : nullptr, static_cast<hipStream_t>(stream));
}

// sliding window: a query sees its last `window` keys; always the ragged form, paged or (block_table == NULL) contiguous
int64_t mi355q_bfp_attention_decode_window_span(int64_t M, int64_t max_length, int64_t window) {
    if (M < 1 || max_length < 1 || window < 1) return 0;
    return decode_window_span(M, max_length, window);
}

size_t mi355q_bfp_attention_decode_window_workspace_bytes(int64_t B, int64_t M, int64_t max_length, int64_t window, int64_t D, int32_t splits) {
    if (B <= 0 || M < 1 || M > 16 || max_length < M || window < 1 || D <= 0 || D % 32 != 0 || D > 128) return 0;
    return decode_workspace_bytes(B, decode_window_span(M, max_length, window), D, splits);
}

int mi355q_bfp_attention_decode_window(const float* q, const void* kq, const void* vq, int32_t G, const int32_t* lengths,
                                       const int32_t* block_table, int32_t causal, int64_t window, float q_scale, float scale_div,
                                       float* out, void* workspace, int64_t B, int64_t M, int64_t max_length, int64_t max_pages,
                                       int64_t num_pages, int64_t P, int64_t D, const int32_t* qk_params, const int32_t* pv_params,
                                       const int64_t* strides, int32_t splits, void* stream) {
    return decode(KvCall(KV_EXPORTS[KVX_DECODE_WINDOW]).pools(kq, vq, nullptr, block_table, B, max_pages, num_pages, P, D)
                      .lens(lengths, nullptr, max_length).query(q, out, workspace, M, G, causal, window, splits).quant(qk_params, pv_params, strides),
                  q, out, workspace, q_scale, scale_div, stream);
}

int mi355q_bfp_attention_extend_window(const float* q, const void* kq, const void* vq, int32_t G, const int32_t* lengths,
                                       const int32_t* counts, const int32_t* block_table, int32_t causal, int64_t window, float q_scale,
                                       float scale_div, float* out, int64_t B, int64_t M, int64_t max_length, int64_t max_pages,
                                       int64_t num_pages, int64_t P, int64_t D, const int32_t* qk_params, const int32_t* pv_params,
                                       const int64_t* strides, void* stream) {
    return extend(KvCall(KV_EXPORTS[KVX_EXTEND_WINDOW]).pools(kq, vq, nullptr, block_table, B, max_pages, num_pages, P, D)
                      .lens(lengths, counts, max_length).query(q, out, nullptr, M, G, causal, window, 0).quant(qk_params, pv_params, strides),
                  q, out, q_scale, scale_div, stream);
}

// attention sinks (mi355q_sink.h): the *_window calls with the first `sinks` keys (0 .. 16) visible to every query beside its window
int mi355q_bfp_attention_decode_sink(const float* q, const void* kq, const void* vq, int32_t G, const int32_t* lengths,
                                     const int32_t* block_table, int32_t causal, int64_t window, float q_scale, float scale_div,
                                     float* out, void* workspace, int64_t B, int64_t M, int64_t max_length, int64_t max_pages,
                                     int64_t num_pages, int64_t P, int64_t D, const int32_t* qk_params, const int32_t* pv_params,
                                     const int64_t* strides, int32_t splits, void* stream, int64_t sinks) {
    return decode(KvCall(KV_EXPORTS[KVX_DECODE_SINK]).pools(kq, vq, nullptr, block_table, B, max_pages, num_pages, P, D)
                      .lens(lengths, nullptr, max_length).query(q, out, workspace, M, G, causal, window, splits).sunk(sinks)
                      .quant(qk_params, pv_params, strides),
                  q, out, workspace, q_scale, scale_div, stream);
}

int mi355q_bfp_attention_extend_sink(const float* q, const void* kq, const void* vq, int32_t G, const int32_t* lengths,
                                     const int32_t* counts, const int32_t* block_table, int32_t causal, int64_t window, float q_scale,
                                     float scale_div, float* out, int64_t B, int64_t M, int64_t max_length, int64_t max_pages,
                                     int64_t num_pages, int64_t P, int64_t D, const int32_t* qk_params, const int32_t* pv_params,
                                     const int64_t* strides, void* stream, int64_t sinks) {
    return extend(KvCall(KV_EXPORTS[KVX_EXTEND_SINK]).pools(kq, vq, nullptr, block_table, B, max_pages, num_pages, P, D)
                      .lens(lengths, counts, max_length).query(q, out, nullptr, M, G, causal, window, 0).sunk(sinks)
                      .quant(qk_params, pv_params, strides),
                  q, out, q_scale, scale_div, stream);
}

// diagnostic hook, not part of include/mi355q.h: what kv_call_check -- the function every export above calls -- makes of a call,
// without launching (no HIP call: works without a GPU).  id: a KvExport; a: 14 addresses, never dereferenced (kq, vq, stage, k, v, q,
// out, workspace, lengths, counts, block_table, k_bytes, v_bytes, stage_bytes), then B, C, max_pages, num_pages, P, D, M, L, n, G,
// causal, window, splits; qk_params / pv_params / strides as the exports take them.  out: the code, 1 where the export would go on
// to launch (or to write its sizes), then the normalised call: B, capacity, D, M, L, n, G, window, lg_p, pages set, causal, strides set,
// the four strides.
// mi355q_debug_kv_call knows the 25 ids recorded in tests/golden/kv_api_codes.json, 0 .. KVX_KV8P_DECODE, and refuses every other as it
// always has; mi355q_debug_kv_call_all is the same function over every id of KvExport (the block_minifloat exports behind them, then
// -- behind KVX_NONE_27, an id it has always refused and still does -- the 4-bit-mantissa exports, 28 .. 31, then -- behind KVX_NONE_32,
// refused likewise -- the attention-sink exports, 33 and 34.  For those two ids, and for no other, `a` holds a 28th word, a[27] = sinks,
// and out[9] stays the window: the normalised sinks are returned in place of n, out[7], which no attention export has).
static int debug_kv_call(int32_t id, int32_t ids, const int64_t a[27], const int32_t* qk_params, const int32_t* pv_params, const int64_t* strides,
                         int64_t out[18]) {
    if (id < 0 || id >= ids || kvx_hole(id) || !a || !out) return MI355Q_E_BADARG;
    const auto p = [a](int i) { return reinterpret_cast<const void*>(static_cast<uintptr_t>(a[i])); };
    const auto p32 = [a](int i) { return reinterpret_cast<const int32_t*>(static_cast<uintptr_t>(a[i])); };
    const auto p64 = [a](int i) { return reinterpret_cast<const int64_t*>(static_cast<uintptr_t>(a[i])); };
    KvCall d = KV_EXPORTS[id];
    d.cache(p(0), p(1), p(2), a[14], a[15], a[19]).pools(p(0), p(1), p(2), p32(10), a[14], a[16], a[17], a[18], a[19]).sizes(p64(11), p64(12), p64(13))
        .rows(p(3), p(4), a[22]).lens(p32(8), p32(9), a[21]).query(p(5), p(6), p(7), a[20], (int32_t)a[23], (int32_t)a[24], a[25], (int32_t)a[26])
        .quant(qk_params, pv_params, strides);
    const bool sunk = (d.form & KV_SINKS) != 0;
    if (sunk) d.sunk(a[27]);
    KvChecked c;
    int rc;
    const bool go = kv_call_check(d, c, rc);
    const int64_t cap = kv_mantissas(d.storage) ? c.cp.C : c.c.C;
    const int64_t words[18] = {rc, go, d.B, cap, d.D, d.M, d.L, sunk ? c.sinks : d.n, c.G, c.window, c.pg.lg_p, c.pages != nullptr, c.causal, c.strides != nullptr,
                               c.st[0], c.st[1], c.st[2], c.st[3]};
    for (int i = 0; i < 18; ++i) out[i] = words[i];
    return 0;
}
__attribute__((visibility("default"))) int mi355q_debug_kv_call(int32_t id, const int64_t a[27], const int32_t* qk_params, const int32_t* pv_params,
                                                                 const int64_t* strides, int64_t out[18]) {
    return debug_kv_call(id, KVX_KV8P_DECODE + 1, a, qk_params, pv_params, strides, out);
}
__attribute__((visibility("default"))) int mi355q_debug_kv_call_all(int32_t id, const int64_t a[27], const int32_t* qk_params,
                                                                     const int32_t* pv_params, const int64_t* strides, int64_t out[18]) {
    return debug_kv_call(id, KVX_COUNT, a, qk_params, pv_params, strides, out);
}

// block_minifloat (fmt 1) / block_log (fmt 2) products: the same two kernels with the other quantisers' block parameters
static int values_matmul_impl(int fmt, bool softmax, const float* mask, long long causal_off, const float* x, const float* y,
                              float* out, void* workspace, int64_t B, int64_t M, int64_t K, int64_t N, int32_t x_width,
                              int32_t x_exponent_width, int32_t x_exponent_bias_width, int32_t y_width, int32_t y_exponent_width,
                              int32_t y_exponent_bias_width, void* stream) {
    if (B < 0 || M < 0 || K < 0 || N < 0) return MI355Q_E_BADARG;
    if (B == 0 || M == 0 || N == 0) return 0;
    if (!out || B > 65535) return MI355Q_E_BADARG;
    if (K == 0) return (int)hipMemsetAsync(out, 0, (size_t)B * M * N * 4, static_cast<hipStream_t>(stream));
    if (!x || !y || !workspace) return MI355Q_E_BADARG;
    QuantArgs ax{}, ay{};
    ax.b0 = ay.b0 = 1; ax.b1 = ay.b1 = 16;
    if (fmt == 1) {
        auto fill = [](QuantArgs& a, int width, int ew, int ebw) -> int {
            const int mbits = width - ew - 1;
            if (ew < 1 || ew > 8 || mbits < 0 || mbits > 23 || ebw < 1 || ebw > 8) return MI355Q_E_BADARG;
            if (mbits > 7) return MI355Q_E_UNSUPPORTED;          // a quantised value must fit bf16's 8 significant bits
            block_minifloat_fill(a, mbits, ew, ebw);
            return 0;
        };
        int rc = fill(ax, x_width, x_exponent_width, x_exponent_bias_width);
        if (rc == 0) rc = fill(ay, y_width, y_exponent_width, y_exponent_bias_width);
        if (rc) return rc;
    } else {
        if (x_width < 2 || x_width > 9 || x_exponent_bias_width < 1 || x_exponent_bias_width > 8) return MI355Q_E_BADARG;
        block_minifloat_fill(ax, 0, x_width - 1, x_exponent_bias_width);
        set_mantissa(ay, 0);
    }
    if (K % 16 != 0 || N % 16 != 0) return MI355Q_E_UNSUPPORTED;      // blocks of 16 along K (x) and N (y) tile the operands
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(workspace)) % 16)
        return MI355Q_E_ALIGN;
    return launch_bfp_qmatmul(ax, ay, x, y, out, workspace, B, M, K, N, static_cast<hipStream_t>(stream), softmax, mask, causal_off, fmt);
}

int mi355q_block_minifloat_matmul(const float* x, const float* y, float* out, void* workspace, int64_t B, int64_t M, int64_t K,
                                  int64_t N, int32_t x_width, int32_t x_exponent_width, int32_t x_exponent_bias_width,
                                  int32_t y_width, int32_t y_exponent_width, int32_t y_exponent_bias_width, void* stream) {
    return values_matmul_impl(1, false, nullptr, -1, x, y, out, workspace, B, M, K, N, x_width, x_exponent_width,
                              x_exponent_bias_width, y_width, y_exponent_width, y_exponent_bias_width, stream);
}

int mi355q_block_minifloat_softmax_matmul(const float* scores, const float* mask, int32_t causal, const float* y, float* out,
                                          void* workspace, int64_t B, int64_t M, int64_t K, int64_t N, int32_t x_width,
                                          int32_t x_exponent_width, int32_t x_exponent_bias_width, int32_t y_width,
                                          int32_t y_exponent_width, int32_t y_exponent_bias_width, void* stream) {
    if (K > 0 && (K <= 192 || N > 128)) return MI355Q_E_UNSUPPORTED;
    if (causal && K < M) return MI355Q_E_BADARG;              // (query i sees keys 0 .. i + K - M)
    if (mask && reinterpret_cast<uintptr_t>(mask) % 16) return MI355Q_E_ALIGN;
    return values_matmul_impl(1, true, mask, causal ? (long long)(K - M) : -1, scores, y, out, workspace, B, M, K, N, x_width,
                              x_exponent_width, x_exponent_bias_width, y_width, y_exponent_width, y_exponent_bias_width, stream);
}

size_t mi355q_block_log_matmul_workspace_bytes(int64_t B, int64_t K, int64_t N) {
    if (B <= 0 || K <= 0 || N <= 0) return 0;
    return 3 * (size_t)B * (size_t)((K + 63) / 64 * 64) * (size_t)N * 2 + 4096 + 64;      // three bf16 planes of y + the statistics slots (BL_STATS_SLOTS words)
}

int mi355q_block_log_matmul(const float* x, const float* y, float* out, void* workspace, int64_t B, int64_t M, int64_t K,
                            int64_t N, int32_t x_width, int32_t x_exponent_bias_width, void* stream) {
    return values_matmul_impl(2, false, nullptr, -1, x, y, out, workspace, B, M, K, N, x_width, 0, x_exponent_bias_width, 0, 0, 0, stream);
}

int mi355q_bfp_matmul(const float* x, const float* y, float* out, void* workspace, int64_t B, int64_t M, int64_t K,
                      int64_t N, int32_t x_width, int32_t x_exponent_width, int32_t x_exponent_bias, int32_t y_width,
                      int32_t y_exponent_width, int32_t y_exponent_bias, void* stream) {
    return bfp_matmul_impl(false, nullptr, -1, x, y, out, workspace, B, M, K, N, x_width, x_exponent_width, x_exponent_bias, y_width,
                           y_exponent_width, y_exponent_bias, stream);
}

int mi355q_bfp_softmax_matmul(const float* scores, const float* mask, int32_t causal, const float* y, float* out, void* workspace,
                              int64_t B, int64_t M, int64_t K, int64_t N, int32_t x_width, int32_t x_exponent_width,
                              int32_t x_exponent_bias, int32_t y_width, int32_t y_exponent_width, int32_t y_exponent_bias,
                              void* stream) {
    if (K > 0 && (K <= 192 || N > 128)) return MI355Q_E_UNSUPPORTED;
    if (causal && K < M) return MI355Q_E_BADARG;              // (query i sees keys 0 .. i + K - M)
    if (mask && reinterpret_cast<uintptr_t>(mask) % 16) return MI355Q_E_ALIGN;
    return bfp_matmul_impl(true, mask, causal ? (long long)(K - M) : -1, scores, y, out, workspace, B, M, K, N, x_width, x_exponent_width, x_exponent_bias, y_width,
                           y_exponent_width, y_exponent_bias, stream);
}

int mi355q_gemm_timing_enable(int enable) {
    const int prev = g_timing.enabled ? 1 : 0;
    g_timing.enabled = enable != 0;
    return prev;
}

int mi355q_gemm_timing_read(int32_t* count, float* avg_ms, float* min_ms) {
    if (!count || !avg_ms || !min_ms) return MI355Q_E_BADARG;
    double sum = 0.0;
    float mn = 0.f;
    int n = 0;
    for (size_t i = 0; i < g_timing.used; ++i) {
        float ms = 0.f;
        hipError_t e = hipEventSynchronize(g_timing.pool[i].second);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, g_timing.pool[i].first, g_timing.pool[i].second);
        if (e != hipSuccess) return (int)e;
        sum += ms;
        mn = (n == 0 || ms < mn) ? ms : mn;
        ++n;
    }
    g_timing.used = 0;
    *count = n;
    *avg_ms = n ? (float)(sum / n) : 0.f;
    *min_ms = mn;
    return 0;
}

int mi355q_bfp_gemm_set_variant(int variant) { return g_gemm_variant.exchange(variant); }

}  // extern "C"
