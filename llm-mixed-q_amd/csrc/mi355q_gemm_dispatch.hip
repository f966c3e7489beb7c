// mi355q_gemm_dispatch.hip -- the host side of every tile GEMM launch: read the environment switches, plan
// (mi355q_gemm_plan.h), fetch the split-K workspace where the plan splits, hand the plan to the kernel family's launcher
// (launch_v8_kernel, launch_bfp_gemm_v9, launch_bfp_gemm_v10).  No kernel lives here.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "mi355q_gemm_tile.h"
#include "mi355q_gemm_v9_full.h"

namespace mi355q {

// The environment switches of the tile GEMM: diagnostics, sweeps and A/B runs only -- the default route needs none.  All of
// them are read on every launch, here and nowhere else.
//   MI355Q_V10=1..6          pin that geometry of the small-tile kernel (mi355q_gemm_v10.hip); with it MI355Q_V8_SPLITS=S splits K
//   MI355Q_V10_NS=n          pin the small-tile kernel's ring depth (<= 4: the shallow ring; 6 on geometry 1, 8 on geometry 3)
//   MI355Q_V10_AUTO=0        keep launches off the small-tile kernel
//   MI355Q_V10_KG=0          keep launches off its two-K-group geometry (5)
//   MI355Q_V8_TILE_ROWS=r    pin the tile height of the v8 / v9 kernels: 128, or 256 (any other non-zero value); set at all, it
//                            keeps launches off the small-tile kernel (=0: the bf16 flavour only)
//   MI355Q_V8_SPLITS=S       cap split-K at S slices (0 / 1: none, 8 K-steps a slice at least); set at all, as TILE_ROWS
//   MI355Q_V9=0              keep the 256 x 256 tile on the v8 kernel
//   MI355Q_V9_FIX=0          ... the launches with exception lists only
//   MI355Q_V9_FULL=0         keep full-tile launches on the general 256 x 256 kernel (read ONCE, by the family-9 launcher: A/B runs)
//   MI355Q_V9_DBG=n          GemmArgs::dbg of the int8 launches of the v8 / v9 kernels
//   MI355Q_V8_CLOCK          (set) the v8 kernel that prints the clock it held over the K loop; no lists
//   MI355Q_V8_STAMPS         (set) the v8 kernel that prints its phases' durations; with lists
static int env_int(const char* name, int unset) {
    const char* e = getenv(name);
    return e ? atoi(e) : unset;
}
static bool env_set(const char* name) { return getenv(name) != nullptr; }
static TileEnv read_tile_env() {
    return TileEnv{env_int("MI355Q_V10", 0), env_int("MI355Q_V10_NS", 0), env_int("MI355Q_V10_AUTO", 1), env_int("MI355Q_V10_KG", 1),
                   env_int("MI355Q_V8_TILE_ROWS", 0), env_int("MI355Q_V8_SPLITS", 0), env_int("MI355Q_V9", 1), env_int("MI355Q_V9_FIX", 1),
                   env_int("MI355Q_V9_DBG", 0), env_set("MI355Q_V8_SPLITS"), env_set("MI355Q_V8_CLOCK"), env_set("MI355Q_V8_STAMPS"),
                   env_set("MI355Q_V8_TILE_ROWS")};
}

// ---- split-K workspace: raw accumulator slabs + one ticket per tile, owned by the library, one per (device, stream),
//      grow-only; tickets are zero whenever no launch is in flight (the reducer of a tile clears its ticket).
//      Under stream capture (a HIP graph being recorded) nothing is allocated or freed: a shape that needs growth then
//      gets no workspace (null: the caller launches unsplit), and a workspace that a capture has been handed is never
//      freed afterwards -- an instantiated graph keeps its pointers -- growth retires the old buffers instead.
struct SplitWorkspace {
    void* slabs = nullptr;
    int* tickets = nullptr;
    size_t slab_bytes = 0;
    int ntickets = 0;
};
static SplitWorkspace* split_workspace(hipStream_t st, size_t slab_bytes, int ntickets) {
    struct Owned { SplitWorkspace w; bool slabs_in_graph = false, tickets_in_graph = false; };      // (per buffer: ADVICE r3)
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, Owned> all;
    static std::vector<void*> retired;                     // (buffers a recorded graph may still use: kept for good)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
    std::lock_guard<std::mutex> lock(mu);
    Owned& o = all[{dev, st}];
    SplitWorkspace& w = o.w;
    const bool grow = w.slab_bytes < slab_bytes || w.ntickets < ntickets;
    if (grow && capturing) return nullptr;
    if (w.slab_bytes < slab_bytes) {
        if (w.slabs) {
            if (o.slabs_in_graph) retired.push_back(w.slabs);
            else (void)hipFree(w.slabs);                  // (synchronises: nothing of this workspace is in flight after)
        }
        w.slabs = nullptr;
        w.slab_bytes = 0;
        o.slabs_in_graph = false;                         // (a fresh buffer: no graph knows it yet)
        if (hipMalloc(&w.slabs, slab_bytes) != hipSuccess) return nullptr;
        w.slab_bytes = slab_bytes;
    }
    if (w.ntickets < ntickets) {
        if (w.tickets) {
            if (o.tickets_in_graph) retired.push_back(w.tickets);
            else (void)hipFree(w.tickets);
        }
        w.tickets = nullptr;
        w.ntickets = 0;
        o.tickets_in_graph = false;
        const int n = (ntickets + 1023) / 1024 * 1024;
        if (hipMalloc(reinterpret_cast<void**>(&w.tickets), (size_t)n * 4) != hipSuccess) return nullptr;
        if (hipMemsetAsync(w.tickets, 0, (size_t)n * 4, st) != hipSuccess) return nullptr;
        w.ntickets = n;
    }
    if (capturing) o.slabs_in_graph = o.tickets_in_graph = true;
    return &w;
}

static int launch_planned(const TileShape& shape, const TileEnv& env, GemmArgs a, const float* sx, const float* sw, const int* xlist,
                          const int* wlist, hipStream_t st, const uint8_t* xf, const uint8_t* wf) {
    TilePlan p = plan_tile_gemm(shape, env, true);
    a.splits = 1;
    if (p.rc == 0 && p.splits > 1) {
        const size_t tiles = p.grid / p.splits;
        SplitWorkspace* w = split_workspace(st, tiles * p.splits * p.bm * p.bn * 4, p.ticket_words_per_tile * (int)tiles);
        if (w) {
            a.splits = p.splits;
            a.slabs = w->slabs;
            a.tickets = w->tickets;
        } else {
            p = plan_tile_gemm(shape, env, false);          // (growth under graph capture, or no memory: unsplit)
        }
    }
    if (p.rc) return p.rc;
    if (p.family == 10) return launch_bfp_gemm_v10(p, a, sx, sw, xlist, wlist, st, xf, wf, shape.bf16);
    if (!shape.bf16) a.dbg = env.v9 ? env.v9_dbg : 0;
    if (p.family == 9) return launch_bfp_gemm_v9(a, sx, sw, xlist, wlist, st, xf, wf, shape.bf16);
    return launch_v8_kernel(p, a, sx, sw, xlist, wlist, st, xf, wf, shape.bf16);
}

// y = x . w^T (+ bias) on row-aligned int8 operands, one scale per row of x and of w; with both lists: + the exception add-back
int launch_bfp_gemm_v8(const GemmArgs& a, const float* sx, const float* sw, const int* xlist, const int* wlist, hipStream_t st,
                       const uint8_t* xf, const uint8_t* wf) {
    const TileShape shape{a.M, a.N, a.K, a.ngroup, xlist && wlist, xf && wf, a.x_segs, false};
    return launch_planned(shape, read_tile_env(), a, sx, sw, xlist, wlist, st, xf, wf);
}

// y = x . w^T (+ bias) on TILED bf16 operands (the same 1-KiB pieces: 16 rows x 32 values): a.xm / a.wm point at the
// bf16 pieces and a.K is the contraction length IN BYTES (2 K).  K % 32 == 0.
int launch_bf16_gemm_tiled(const GemmArgs& a, hipStream_t st) {
    const TileShape shape{a.M, a.N, a.K, 0, false, false, a.x_segs, true};
    return launch_planned(shape, read_tile_env(), a, nullptr, nullptr, nullptr, nullptr, st, nullptr, nullptr);
}

}  // namespace mi355q

// diagnostic hook, not part of include/mi355q.h: the plan of a launch, without launching (no HIP call: works without a GPU).
// shape = M, N, K (bytes of a row), ngroup, lists, flags, x_segs, bf16; env = the 13 words of TileEnv in declaration order, or
// NULL for the process environment; out = the 14 words of TilePlan in declaration order, then two zeros.
extern "C" __attribute__((visibility("default"))) int mi355q_debug_gemm_plan(const int64_t shape[8], const int32_t* e, int32_t workspace_ok,
                                                                             int32_t out[16]) {
    using namespace mi355q;
    if (!shape || !out) return MI355Q_E_BADARG;
    const TileShape s{shape[0], shape[1], shape[2], (int)shape[3], shape[4] != 0, shape[5] != 0, (int)shape[6], shape[7] != 0};
    const TileEnv env = e ? TileEnv{e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7], e[8], e[9] != 0, e[10] != 0, e[11] != 0, e[12] != 0} : read_tile_env();
    const TilePlan p = plan_tile_gemm(s, env, workspace_ok != 0);
    const int32_t words[16] = {p.family, p.geom, p.bm, p.bn, p.ti, p.sched, p.fixmode, p.ns, p.occ, p.kg, p.splits, p.ticket_words_per_tile, (int32_t)p.grid, p.rc};
    for (int i = 0; i < 16; ++i) out[i] = words[i];
    return 0;
}

// diagnostic hook, not part of include/mi355q.h: whether a launch takes the full-tile unit of the 256 x 256 kernel (mi355q_gemm_v9_full.h),
// without launching.  shape / e / workspace_ok as mi355q_debug_gemm_plan; flags = resid given, x_post, dbg, y 16-byte aligned,
// the MI355Q_V9_FULL switch (1: on), ldy.  Returns 1 / 0, or a negative error.
extern "C" __attribute__((visibility("default"))) int mi355q_debug_v9_full(const int64_t shape[8], const int32_t* e, int32_t workspace_ok,
                                                                           const int64_t flags[6]) {
    using namespace mi355q;
    if (!shape || !flags) return MI355Q_E_BADARG;
    int32_t plan[16];
    const int rc = mi355q_debug_gemm_plan(shape, e, workspace_ok, plan);
    if (rc) return rc;
    if (plan[13]) return 0;                                     // (the plan refuses the launch)
    const V9FullQuery q{plan[0], plan[10], (int)shape[3], shape[4] != 0 && shape[5] != 0, shape[7] != 0, shape[0], shape[1], flags[5],
                        flags[0] != 0, flags[1] != 0, (int)flags[2], flags[3] != 0, flags[4] != 0};
    return v9_full_tile_ok(q) ? 1 : 0;
}
