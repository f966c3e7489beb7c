// mi355q_gemm_plan.h -- which kernel a tile GEMM launch takes, as a pure function of its shape and the environment
// switches.  Host only, plain C++17: no HIP, no environment read, no static.  mi355q_gemm_dispatch.hip reads the switches
// and carries the plan out; mi355q_debug_gemm_plan exposes it; tests/test_gemm_plan.py holds it to the recorded route
// table (tests/golden/gemm_plan.json).  DESIGN.md "How a tile GEMM launch is routed" has the measurements in full.
#ifndef MI355Q_GEMM_PLAN_H
#define MI355Q_GEMM_PLAN_H

namespace mi355q {

// the switches as read_tile_env() found them (unset: v10_auto = v10_kg = v9 = v9_fix = 1, everything else 0 / false)
struct TileEnv {
    int v10, v10_ns, v10_auto, v10_kg, tile_rows, splits, v9, v9_fix, v9_dbg;
    bool splits_set, clock, stamps, tile_rows_set;      // (sweeps set MI355Q_V8_TILE_ROWS=0: nothing pinned, but bf16 stays off v10)
};
struct TileShape {
    long long M, N, K;          // K as the launchers see it: bytes of a row (int8: values; bf16: 2 x values)
    int ngroup;                 // grouped launch: weight operands side by side (0 / 1: one)
    bool lists;                 // both exception lists given
    bool flags;                 // both row-flag arrays given
    int x_segs;                 // bf16 flavour: column segments of x
    bool bf16;
};
struct TilePlan {
    int family;                 // 8, 9, 10: mi355q_gemm_v8.hip / _v9.hip / _v10.hip
    int geom;                   // v10 geometry 1..6, else 0
    int bm, bn;                 // workgroup tile
    int ti, sched, fixmode;     // v8 template arguments
    int ns, occ, kg;            // v10 ring depth / workgroups a compute unit / K-groups
    int splits;                 // slices of K per tile (>= 1)
    int ticket_words_per_tile;  // 1, or 2 when a pinned v10 geometry is split
    unsigned grid;
    int rc;                     // != 0: the launcher returns it, nothing is launched
};

inline long long tile_count(long long M, long long N, int bm, int bn) { return ((M + bm - 1) / bm) * ((N + bn - 1) / bn); }

// Slices per tile for an under-filled grid: the largest S <= 16 with tiles * S <= 256 (one workgroup a compute unit), whole and, where
// the schedule needs it, even numbers of K-steps a slice, at least `min_steps` of them.  MI355Q_V8_SPLITS caps S instead, at 8 steps.
inline int choose_splits(const TileEnv& env, long long tiles, int nsteps_all, bool need_even, int min_steps) {
    const int forced = env.splits_set ? env.splits : 0;
    if (forced) min_steps = 8;
    int best = 1;
    for (int S = 2; S <= 16; ++S) {
        if (nsteps_all % S) continue;
        const int steps = nsteps_all / S;
        if (steps < min_steps) break;
        if (need_even && (steps & 1)) continue;
        if (forced ? S > forced : tiles * S > 256) break;
        best = S;
    }
    return best;
}

// a v10 launch.  Geometries: 1 = 128 x 256, 2 = 256 x 128, 3 = 128 x 128, 4 = 128 x 64; 5 / 6 = 3 / 1 as two K-groups in an 8-wave workgroup
inline TilePlan plan_v10(const TileShape& s, const TileEnv& env, int geom, int splits) {
    TilePlan p{};
    p.family = 10;
    p.geom = geom;
    p.bm = geom == 2 ? 256 : 128;
    p.bn = (geom == 1 || geom == 6) ? 256 : (geom == 4 ? 64 : 128);
    p.splits = splits;
    p.ticket_words_per_tile = splits > 1 ? 2 : 1;
    p.grid = (unsigned)tile_count(s.M, s.N, p.bm, p.bn) * (s.ngroup > 1 ? s.ngroup : 1) * splits;
    // ring depth: a workgroup alone on its compute unit (<= 256 of them) needs an L2 round trip under load in flight, two side by
    // side cover each other's waits (profiles/r05_small_tiles.txt).  MI355Q_V10_NS pins it: 6 on geometry 1, 8 on geometry 3.
    const bool deep = env.v10_ns ? env.v10_ns > 4 : p.grid <= 256;
    constexpr int ring[7][2] = {{0, 0}, {4, 3}, {4, 3}, {6, 4}, {6, 4}, {4, 4}, {3, 3}};     // [geometry][deep, shallow]
    p.ns = (geom == 1 && env.v10_ns == 6) || (geom == 3 && env.v10_ns == 8) ? env.v10_ns : ring[geom][deep ? 0 : 1];
    p.kg = geom >= 5 ? 2 : 1;
    p.occ = deep || geom >= 5 ? 1 : 2;
    return p;
}

// MI355Q_V10 = 1..6 (sweeps and tests): that geometry, split as MI355Q_V8_SPLITS says (>= 2 K-steps a slice) or not at all
inline TilePlan plan_pinned_v10(const TileShape& s, const TileEnv& env, bool workspace_ok) {
    const int nsteps_all = (int)(s.K >> 6);
    int geom = env.v10, S = env.splits_set && env.splits > 1 ? env.splits : 1;
    while (S > 1 && (nsteps_all % S || nsteps_all / S < 2)) --S;
    if (geom >= 5) {            // the K-group geometries: never split across workgroups; whole pairs of K-steps
        S = 1;
        if (s.K % 128) geom = geom == 5 ? 3 : 1;
    }
    return plan_v10(s, env, geom, workspace_ok ? S : 1);
}

// a launch of `tiles` 128- or 256-row tiles in S slices on the v9 kernel (where `v9_ok`) or the v8 kernel
inline TilePlan plan_v8_v9(const TileShape& s, const TileEnv& env, long long tiles, bool small, int S, bool v9_ok) {
    TilePlan p{};
    p.bm = small ? 128 : 256;
    p.bn = 256;
    p.splits = S;
    p.ticket_words_per_tile = 1;
    p.grid = (unsigned)tiles * S;
    const int steps = (int)(s.K >> 6) / S;
    // the 256 x 256 tile has its own kernel from four K-steps a slice on (profiles/r04_v9_tail_prefetch.txt); MI355Q_V9=0 keeps it on v8
    p.family = v9_ok && env.v9 && !small && s.K % 128 == 0 && steps >= 4 ? 9 : 8;
    if (p.family == 9) return p;
    p.ti = small ? 4 : 8;
    const bool diag = !small && !s.bf16;         // MI355Q_V8_STAMPS / MI355Q_V8_CLOCK: flavours of the int8 256-row tile
    p.fixmode = s.lists ? (diag && env.stamps ? 3 : 1) : (diag && env.clock ? 2 : 0);
    // 128 rows: pipelined on whole pairs of K-steps a slice, one-phase otherwise; 256 rows: K % 128 == 64 takes the unpipelined schedule
    if (small) p.sched = s.K % 128 == 0 && (steps & 1) == 0 ? 2 : 1;
    else p.sched = p.fixmode || s.K % 128 == 0 ? 2 : 0;
    return p;
}

inline TilePlan plan_int8(const TileShape& s, const TileEnv& env, bool workspace_ok) {
    const int ngroup = s.ngroup > 1 ? s.ngroup : 1;
    const bool v10_ok = s.K % 64 == 0 && (!s.lists || s.flags), rows_pinned = env.tile_rows_set && env.tile_rows;
    if (env.v10 >= 1 && env.v10 <= 6 && v10_ok) return plan_pinned_v10(s, env, workspace_ok);
    const long long t256 = tile_count(s.M, s.N, 256, 256) * ngroup, t128 = tile_count(s.M, s.N, 128, 256) * ngroup;
    // at most 128 tiles of 256 x 256 -- half the compute units -- go to the small tiles, unsplit (profiles/r05_small_tiles.txt)
    if (env.v10_auto && t256 <= 128 && v10_ok && !rows_pinned && !env.splits_set && !env.clock && !env.stamps) {
        const long long g3 = tile_count(s.M, s.N, 128, 128) * ngroup;
        // <= 128 tiles of 128 x 128: 128 x 64 ones (r05_small_tiles.txt); 129 .. 256: two K-groups a workgroup (r06_shard_shapes.txt)
        return plan_v10(s, env, g3 <= 128 ? 4 : (env.v10_kg && g3 <= 256 && s.K % 128 == 0 && s.ngroup <= 1 ? 5 : 3), 1);
    }
    if (s.lists && !s.flags) {
        TilePlan bad{};
        bad.rc = -1;            // MI355Q_E_BADARG
        return bad;
    }
    // a 128 x 256 tile does half the work in 0.82 of the time (48 vs 58 us at 2048 x 4096 x 4096): fewer rounds of 256 win
    const double cost256 = (double)((t256 + 255) / 256) * 1.0, cost128 = (double)((t128 + 255) / 256) * 0.82;
    const bool small = rows_pinned ? env.tile_rows == 128 : cost128 < cost256;
    const long long tiles = (unsigned)(small ? t128 : t256);
    // splitting costs 16-22 us at 128 tiles x 2: with lists only while a slice keeps 32 K-steps, without them 8
    const int S = workspace_ok ? choose_splits(env, tiles, (int)(s.K >> 6), true, s.lists ? 32 : 8) : 1;
    // (MI355Q_V9_FIX=0 and the v8 diagnostics keep launches off v9)
    return plan_v8_v9(s, env, tiles, small, S, (env.v9_fix || !s.lists) && !env.clock && !env.stamps);
}

inline TilePlan plan_bf16(const TileShape& s, const TileEnv& env, bool workspace_ok) {
    if (env.v10 >= 1 && env.v10 <= 6 && s.K % 64 == 0) return plan_pinned_v10(s, env, workspace_ok);
    const long long t256 = tile_count(s.M, s.N, 256, 256), t128 = tile_count(s.M, s.N, 128, 256);
    const bool rows_pinned = env.tile_rows_set && env.tile_rows;
    // Tile height and split together, by a cost model fitted to tools/timing/sweep_bf16_tile_split.py (us): rounds of 256 x K-steps
    // a slice x 0.70 (256 rows) or 0.56 (128 rows), plus, when split, 12 + 0.7 per MiB of slab traffic
    const int nsteps_all = (int)(s.K >> 6);
    const double out_mib = (double)s.M * (double)s.N * 4.0 / 1048576.0;
    bool small = false;
    int S = 1;
    double best_t = 1e30;
    for (int kind = 0; kind < 2; ++kind) {                      // 0: 256 rows, 1: 128 rows
        if (rows_pinned && (env.tile_rows == 128) != (kind == 1)) continue;
        const long long t = kind ? t128 : t256;
        const bool need_even = kind == 0 && s.K % 128 == 0;
        const int smax = choose_splits(env, t, nsteps_all, need_even, 8);
        for (int sp = 1; sp <= smax; ++sp) {
            if (env.splits_set && sp != smax) continue;         // (sweeps pin the split too)
            if (nsteps_all % sp || (need_even && ((nsteps_all / sp) & 1))) continue;
            const double rounds = (double)((t * sp + 255) / 256);
            const double est = rounds * (nsteps_all / sp) * (kind ? 0.56 : 0.70) + (sp > 1 ? 12.0 + 0.7 * out_mib * sp : 0.0);
            if (est < best_t) { best_t = est; small = kind == 1; S = sp; }
        }
    }
    // the small tiles, unsplit, where their estimate is lower by a 1.12 margin (beyond ~1000 tiles the line flatters them:
    // profiles/r05_shard_shapes.txt).  us a K-step: 128 x 64 tiles 0.12 (r05_small_tiles.txt); 128 x 128 alone on a compute unit 0.23,
    // rounds of 512 side by side 0.43 (r05_column_offsets.txt); 128 x 256 0.39; two K-groups 0.20 (r06_shard_shapes.txt); + 8 us a launch
    if (env.v10_auto && !env.tile_rows_set && !env.splits_set && s.K % 64 == 0) {
        const long long g3 = tile_count(s.M, s.N, 128, 128), g1 = tile_count(s.M, s.N, 128, 256);
        const double est3 = (g3 <= 128 ? nsteps_all * 0.12 : g3 <= 256 ? nsteps_all * 0.23 : nsteps_all * 0.43 * (double)((g3 + 511) / 512)) + 8.0;
        const double est1 = g1 <= 256 ? nsteps_all * 0.39 + 8.0 : 1e30;
        const double est5 = env.v10_kg && g3 > 128 && g3 <= 256 && s.K % 128 == 0 && s.x_segs <= 1 ? nsteps_all * 0.20 + 8.0 : 1e30;
        if (est3 * 1.12 < best_t || est1 * 1.12 < best_t || est5 * 1.12 < best_t)
            return plan_v10(s, env, est5 < est3 && est5 < est1 ? 5 : (est1 < est3 ? 1 : (g3 <= 128 ? 4 : 3)), 1);
    }
    return plan_v8_v9(s, env, (unsigned)(small ? t128 : t256), small, workspace_ok ? S : 1, s.x_segs <= 1);
}

// workspace_ok = false: the launch when the split-K workspace cannot be had (growth under graph capture, no memory): unsplit
inline TilePlan plan_tile_gemm(const TileShape& s, const TileEnv& env, bool workspace_ok) {
    return s.bf16 ? plan_bf16(s, env, workspace_ok) : plan_int8(s, env, workspace_ok);
}

}  // namespace mi355q
#endif
