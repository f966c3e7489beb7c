// mi355q_gemm_v9_full.h -- when a launch of the 256 x 256 tile kernel takes its full-tile unit (mi355q_gemm_v9f.hip), as a pure
// function of what the family-9 launcher knows.  Host only, plain C++17: no HIP, no environment read, no static.  The launcher
// (launch_bfp_gemm_v9, mi355q_gemm_v9.hip) asks it on every launch; mi355q_debug_v9_full exposes it behind the planner
// (mi355q_gemm_dispatch.hip); tests/test_gemm_full_tile_select.py holds it to a table written out there.
#ifndef MI355Q_GEMM_V9_FULL_H
#define MI355Q_GEMM_V9_FULL_H

namespace mi355q {

// what the full-tile unit's kernel made compile-time facts: everything here must hold, or the general kernel runs
struct V9FullQuery {
    int family, splits, ngroup;     // of the plan / the launch (ngroup 0 or 1: one weight operand)
    bool lists;                     // both exception lists (and both blockwise operands) given
    bool bf16;
    long long M, N, ldy;
    bool resid;                     // a residual operand is given
    bool x_post;                    // x's entries go to the row post-pass
    int dbg;                        // GemmArgs::dbg (MI355Q_V9_DBG)
    bool y_aligned;                 // y and its rows on 16-byte boundaries
    bool enabled;                   // the latched switch MI355Q_V9_FULL (unset: on)
};

inline bool v9_full_tile_ok(const V9FullQuery& q) {
    if (!q.enabled || q.family != 9 || q.bf16 || !q.lists) return false;
    if (q.splits > 1 || q.ngroup > 1) return false;
    if (q.M <= 0 || q.N <= 0 || q.M % 256 != 0 || q.N % 256 != 0) return false;       // every tile full: no row or column test in the kernel
    if (q.M > 0x7fffffffll || q.N > 0x7fffffffll || q.ldy > 0x7fffffffll) return false;     // (plain 32-bit kernel arguments)
    if (q.resid || q.x_post || q.dbg != 0) return false;
    return q.y_aligned;                                        // (the 16-byte stores are unconditional there)
}

}  // namespace mi355q
#endif
