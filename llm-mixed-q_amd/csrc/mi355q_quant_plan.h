// mi355q_quant_plan.h -- which build of the row quantiser a launch takes and on how many workgroups, as a pure function of its
// shape and the environment switches.  Host only, plain C++17: no HIP, no environment read, no static.  mi355q_quant.hip reads the
// switches (read_rows_env) and carries the plan out, as mi355q_quant_cls.hip does for the class-aware kernel;
// mi355q_debug_quant_rows_plan exposes it; tests/test_quant_rows_plan.py holds it to the recorded route table
// (tests/golden/quant_rows_plan.json).  DESIGN.md "How a row quantiser launch is chosen".
#ifndef MI355Q_QUANT_PLAN_H
#define MI355Q_QUANT_PLAN_H

#include "mi355q.h"

namespace mi355q {

// the switches as read_rows_env() found them
struct RowsEnv {
    int grid = 0;               // MI355Q_QROWS_GRID, 0 when unset or <= 0
    bool old_variant = false;   // MI355Q_QROWS_VARIANT set to 0
    int short_rows = 1;         // MI355Q_QROWS_SHORT
};
enum RowsKind { ROWS_INT8 = 0, ROWS_MX = 1, ROWS_CLASSES = 2 };
struct RowsShape {
    int kind;
    long long rows, cols;
    int pre_op;                 // MI355Q_PRE_*
    bool segmented;             // seg_len != 0 as the launcher sees it (the API has turned seg_len == K into 0)
};
struct RowsPlan {
    // template arguments of bfp_quant_align_rows_kernel (ROWS_CLASSES: maxit, full, wps of bfp_quant_classes_kernel, the rest 0)
    int maxit;
    bool full, seg, mx;
    int pre;
    bool st16;
    int wps;
    unsigned grid;
    int rc;                     // != 0: the launcher returns it, nothing is launched, every other word is 0
};

// the same template arguments: how a launcher finds a plan's kernel in its table
inline bool same_build(const RowsPlan& a, const RowsPlan& b) {
    return a.maxit == b.maxit && a.full == b.full && a.seg == b.seg && a.mx == b.mx && a.pre == b.pre && a.st16 == b.st16 && a.wps == b.wps;
}

inline RowsPlan rows_refused() { return RowsPlan{0, false, false, false, 0, false, 0, 0, MI355Q_E_UNSUPPORTED}; }

// MAXIT: slabs of 1024 values a lane holds; 0: the row is too long.  `short_ok`: rows of <= 1024 / <= 2048 values -- OPT-125m / 350m / 1.3B
// widths -- hold one / two slabs instead of four guarded ones (fewer registers, more rows resident on a compute unit); `slab12`: rows of
// <= 12288 hold twelve (Llama-7B's 11008: 11 slabs of 16)
inline int rows_slabs(long long cols, bool short_ok, bool slab12) {
    if (cols > 16384) return 0;
    if (short_ok && cols <= 2048) return cols <= 1024 ? 1 : 2;
    return cols <= 4096 ? 4 : cols <= 8192 ? 8 : slab12 && cols <= 12288 ? 12 : 16;
}
// FULL: every lane holds a block in every slab, no guards (the one-, two- and twelve-slab builds have no such flavour)
inline bool rows_full(long long cols) { return cols == 4096 || cols == 8192 || cols == 16384; }

// a workgroup per row up to `cap` (and the 65536 every launch stops at): the kernels walk the rows beyond
inline unsigned rows_grid(long long rows, long long cap) {
    if (cap > 65536) cap = 65536;
    return (unsigned)(rows < 1 ? 1 : rows > cap ? cap : rows);
}

inline RowsPlan plan_int8_rows(const RowsShape& s, const RowsEnv& env) {
    // segmented rows: round 5's addressing, guarded; MI355Q_QROWS_VARIANT=0: round 5's build (PRE 1: any pre-op, decided at run time);
    // else the lean builds -- only the row's own pre-op compiled in (2 LlamaRMSNorm, 3 LayerNorm, 4 the elementwise ones, 0 none),
    // 16-byte stores where every lane holds a block in every slab (the guarded transpose put its scalars in scratch)
    const bool lean = !s.segmented && !env.old_variant, short_ok = env.short_rows && lean;
    RowsPlan p{rows_slabs(s.cols, short_ok, short_ok), !s.segmented && rows_full(s.cols), s.segmented, false, 1, false, 1, 0, 0};
    if (!p.maxit) return rows_refused();
    if (lean || s.segmented) p.pre = s.pre_op == MI355Q_PRE_RMSNORM ? 2 : s.pre_op == MI355Q_PRE_LAYERNORM ? 3 : s.pre_op ? 4 : 0;
    p.st16 = lean && p.full;
    // plain rows: a fixed grid of SIX workgroups per compute unit (what the build without the pre-op code admits: 77 registers), several
    // rows each with the next row's loads in flight (profiles/r06_qrows_variants.txt, 4096 x 4096: 20.6 us for round 5's build -- 121
    // registers, 4 workgroups a compute unit, dword stores -- 19.2 without the pre-op code and with 16-byte stores, 18.0 on six
    // workgroups a compute unit).  MI355Q_QROWS_GRID caps the rows behind a pre-op too (they take one workgroup each otherwise).
    const bool capped = !s.segmented && (s.pre_op == 0 || env.grid > 0);
    p.grid = rows_grid(s.rows, !capped ? 65536 : env.grid > 0 ? env.grid : env.old_variant ? 1024 : 1536);
    return p;
}

// no pre-op code (this entry never has one); six resident workgroups a compute unit at 77 registers, like the int8 flavour
inline RowsPlan plan_mx_rows(const RowsShape& s) {
    const RowsPlan p{rows_slabs(s.cols, true, false), rows_full(s.cols), false, true, 0, false, 1, rows_grid(s.rows, s.pre_op == 0 ? 1536 : 65536), 0};
    return p.maxit ? p : rows_refused();
}

inline RowsPlan plan_class_rows(const RowsShape& s) {
    if (s.rows * s.cols >= (1ll << 30)) return rows_refused();      // (32-bit byte offsets inside the kernel)
    // (K = 4096: 75 registers, six workgroups a compute unit)
    const RowsPlan p{rows_slabs(s.cols, false, false), s.cols == 4096, false, false, 0, false, 1, rows_grid(s.rows, s.cols == 4096 ? 1536 : 1024), 0};
    return p.maxit ? p : rows_refused();
}

inline RowsPlan plan_quant_rows(const RowsShape& s, const RowsEnv& env) {
    return s.kind == ROWS_MX ? plan_mx_rows(s) : s.kind == ROWS_CLASSES ? plan_class_rows(s) : plan_int8_rows(s, env);
}

}  // namespace mi355q
#endif
