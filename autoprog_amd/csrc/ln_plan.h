// Host-side planning of the LayerNorm launches (layernorm.hip): lane-group width, chunks per lane, the kernel instantiation, the grid with
// its caps and the number of dgamma / dbeta partial rows.  Plain C++17, no HIP; tests/host/attn_ln_plan_check.cpp plans on a CPU.
#pragma once
#include <stdint.h>
#include "../../include/autoprog_hip.h"
#include "switches.h"

enum { LN_FWD = 0, LN_FWD_LP = 1, LN_BWD = 2, LN_BWD_PF = 3 };
#define LN_MAX_PARTIAL 1024             // rows of dgamma / dbeta partials that ap_layernorm_bwd_workspace holds
// V, U, OCC, pool: the template arguments of k_ln_fwd<V, U>, k_ln_fwd_lp<V>, k_ln_bwd<V, U> and k_ln_bwd_pf<V, U, OCC, POOL>.  G: lanes per
// row.  grid 0 with status AP_OK: no rows, nothing to launch.  n_partial (backward): partial rows the launch writes, one per workgroup.
struct LnPlan { int status, family, V, U, OCC, pool, G, grid, block, lds_bytes, n_partial; };

// lane-group width G (8..64) and chunks per lane V (1..4) with G*V >= C/8 and the fewest idle lanes; ties go to the
// narrower group (more rows per wave in flight).  C = 384 -> (16,3), 192 -> (8,3), 768 -> (32,3), 256 -> (8,4), 1000 -> (32,4)
static inline int ln_pick_group(int C, int* V) {
    const int nch = C / 8;
    int bestG = 64, bestV = 4, best_waste = 1 << 30;
    for (int G = 8; G <= 64; G <<= 1)
        for (int v = 1; v <= 4; ++v) {
            if (G * v < nch) continue;
            const int waste = G * v - nch;
            if (waste < best_waste) { best_waste = waste; bestG = G; bestV = v; }
        }
    *V = bestV;
    return bestG;
}
// backward keeps 3 operand rows per row in registers next to the dgamma/dbeta accumulators: one chunk per lane and a
// wide group (G >= C/8) with 4 rows unrolled measured faster there (22.7 vs 27.4 us at 25088 x 384) than the
// no-idle-lane mapping above, whose register footprint halves the occupancy
static inline int ln_pick_group_wide(int C, int* V) {
    const int nch = C / 8;
    int G = 16;
    while (G < 64 && G < nch) G <<= 1;
    const int v = (nch + G - 1) / G;
    *V = v <= 1 ? 1 : (v <= 2 ? 2 : 4);
    return G;
}
static inline int ln_status(int C) { return (C <= 0 || (C & 7)) ? AP_ERR_SHAPE : C > 2048 ? AP_ERR_UNSUPPORTED : AP_OK; }
static inline int ln_grid(int64_t rows, int64_t per_block, int cap) { const int64_t g = (rows + per_block - 1) / per_block; return g > cap ? cap : (int)g; }

// fp8: the e4m3 side output rides in every forward instantiation, so the plan does not depend on it
static inline LnPlan ln_fwd_plan(int64_t rows, int C, const ApSwitches& sw, bool fp8) {
    (void)fp8;
    LnPlan p = {};
    if ((p.status = ln_status(C)) != AP_OK || rows <= 0) return p;
    p.G = sw.ln_fwd_wide ? ln_pick_group_wide(C, &p.V) : ln_pick_group(C, &p.V);
    // one row per lane group and workgroup (AP_LN_FWD_RPG): 10.3 vs 10.7 us at 25088 x 384 (4: 11.4, 8: 15.3)
    p.grid = ln_grid(rows, (int64_t)(256 / p.G) * sw.ln_fwd_rpg, 256 * 8);
    p.block = 256; p.lds_bytes = 2 * C * (int)sizeof(float);
    // the low-register forward (the widths it was measured on: 192, 384, 768)
    if (sw.ln_fwd_lp && p.V <= 3) p.family = LN_FWD_LP;
    else { p.family = LN_FWD; p.U = p.V <= 2 ? 4 : 2; }
    return p;
}

// pool: the average pool's gradient rides in (ap_layernorm_bwd_partial_pool)
static inline LnPlan ln_bwd_plan(int64_t rows, int C, const ApSwitches& sw, bool pool) {
    LnPlan p = {};
    if ((p.status = ln_status(C)) != AP_OK || rows <= 0) return p;
    p.G = ln_pick_group_wide(C, &p.V);
    // the grid bounds the dgamma / dbeta partial rows (the workspace holds LN_MAX_PARTIAL).  AP_LN_BWD_GRID, default 768: 3 blocks per CU
    // measured best (20.7 vs 23.5 us at 1024)
    p.grid = ln_grid(rows, 256 / p.G, sw.ln_bwd_grid);
    // 768-wide rows (DeiT-Base, VOLO-D5): 19.6 us at two workgroups per CU, 24.3 at three
    if (p.V >= 2 && p.grid > 512 && !sw.ln_bwd_grid_set) p.grid = 512;
    p.n_partial = p.grid; p.block = 256; p.lds_bytes = 2 * 4 * C * (int)sizeof(float);
    // (5 rows per trip instead of 4 -- every lane group of the VOLO-D1 launch then finishes its 8 or 9 rows in two trips instead of three for
    // a sixth of them -- measured equal, 17.5 vs 17.7 us: the trips are not what the launch waits for)
    // AP_LN_BWD_PF: 0 = the trip-by-trip kernel; 1 = pipelined, half the rows per trip (the same registers in flight); 2 = pipelined with the
    // old rows per trip (twice the registers); 3 = 1 with four workgroups per SIMD asked for (one chunk per lane only)
    const int pf = sw.ln_bwd_pf;
    p.OCC = 1;
    if (pool) {                         // pipelined kernel, one chunk per lane: C <= 512
        if (!pf || p.V != 1) { p.status = AP_ERR_UNSUPPORTED; return p; }
        p.family = LN_BWD_PF; p.U = 2; p.pool = 1;
    } else if (pf && p.V <= 2) {        // (four chunks per lane: two register sets do not fit 256 registers)
        p.family = LN_BWD_PF;
        if (p.V == 1) { p.U = pf == 2 ? 4 : 2; if (pf == 3) p.OCC = 4; }
        else p.U = pf == 2 ? 2 : 1;
    } else { p.family = LN_BWD; p.U = p.V == 1 ? 4 : p.V == 4 ? 1 : 2; }
    return p;
}
