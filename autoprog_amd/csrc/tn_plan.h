// Host-side planning of the weight-gradient launches (gemm.hip: ap_gemm_tn_acc*, ap_gemm_tn8_acc*): how a launch is cut along the
// tokens, where its work items are placed, and which kernel takes which problems.  Plain C++17, no HIP: the CU count, the resident
// capacity and the run-time switches come in as arguments (gemm.hip reads them), so tests/host/tn_plan_check.cpp plans on a CPU.
// The kernel-argument tables that are plain data (TnMap, T8Map, TnLn) live here too.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/autoprog_hip.h"

#define TN_STEP 64                  // tokens per reduction step of the 128 x 128-tile kernels
#define TN_MAX_GROUP 8              // problems per launch of the 128 x 128-tile kernels
// Placement of a grouped launch: entry b = (problem << 12 | split * tiles + tile) of workgroup b, TN_MAP_IDLE = none.  Workgroup
// b runs on XCD b % 8, so the host puts ALL output tiles of one (problem, token split) on one XCD: that split's operand slab is
// then fetched through ONE L2 instead of the 1.5-2 that a contiguous id range per XCD gives when 5 splits meet 8 XCDs
// (transformer block: 486 MB of beyond-L2 traffic per launch for 270 MB of operands before).
#define TN_MAP_MAX 1024
#define TN_MAP_SHIFT 12
#define TN_MAP_IDLE 0xFFFFu
struct TnMap { unsigned short e[TN_MAP_MAX]; };
// the 192 x 192-tile kernels (up to AP_TN_MAX_GROUP = 32 problems, one work item per CU): their own, smaller table,
// entry = problem << 11 | split * tiles + tile, so that the kernel arguments stay under 4 KB
#define T8_MAP_MAX 320
#define T8_MAP_SHIFT 11
struct T8Map { unsigned short e[T8_MAP_MAX]; };
// LayerNorm dgamma / dbeta reductions riding in a grouped launch, on the workgroups behind the placement table
struct TnLnItem { const float* partial; float* dgamma; float* dbeta; int nblocks; int C; };
struct TnLn { TnLnItem it[AP_LN_MAX_BATCH]; int count; int first; };            // first: blockIdx.x of the first reduction workgroup

struct TnTiles { int tiles, splits; };                  // what the placement needs of a problem
struct TnItemPlan { int t1, t2, steps, sps, splits, start, shared_out; };      // steps: reduction steps of the problem, sps: per token range
struct TnGroupPlan {                // a launch of the contiguous-range kernels (k_gemm_tn_grouped, k_gemm_tn_fp8) and its deterministic slabs
    TnItemPlan p[AP_TN_MAX_GROUP];
    int count, blocks;
    size_t range_floats[AP_TN_MAX_GROUP];               // what one token range of the problem stores in the deterministic mode
    size_t slab_floats, slab_off[AP_TN_MAX_GROUP];
};
struct T8Plan { int ksps; TnTiles pl[AP_TN_MAX_GROUP]; int shared_out[AP_TN_MAX_GROUP]; T8Map map; int blocks; };

// ---- one rule each
static inline float tn_alpha(float alpha) { return alpha != 0.0f ? alpha : 1.0f; }                      // 0 is read as 1
static inline float tn_cs_scale(const void* colsum_weight, float colsum_scale) { return colsum_weight ? colsum_scale : 1.0f; }
static inline int tn_ceil(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// token cut: `want` ranges at most, of equal length, none of them empty
static inline void tn_split(TnItemPlan& p, int want) {
    p.sps = tn_ceil(p.steps, want > 1 ? want : 1);
    p.splits = tn_ceil(p.steps, p.sps);
}

// a launch of the contiguous-range kernels: its workgroups when every problem is cut into ranges of `sps` steps ...
static inline int64_t tn_group_blocks(const TnGroupPlan& grp, int count, int sps) {
    int64_t nb = 0;
    for (int i = 0; i < count; ++i) nb += (int64_t)grp.p[i].t1 * grp.p[i].t2 * tn_ceil(grp.p[i].steps, sps);
    return nb;
}
// ... and that cut: every problem's workgroups and deterministic slab follow those of the problems before it
static inline void tn_group_cut(TnGroupPlan& grp, int count, int sps) {
    grp.count = count; grp.blocks = 0; grp.slab_floats = 0;
    for (int i = 0; i < count; ++i) {
        TnItemPlan& p = grp.p[i];
        tn_split(p, tn_ceil(p.steps, sps));
        p.start = grp.blocks; grp.blocks += p.t1 * p.t2 * p.splits;
        grp.slab_off[i] = grp.slab_floats; grp.slab_floats += p.splits * grp.range_floats[i];
    }
}

// another problem of the launch adds to the same output: its tiles keep their atomics even when the token axis is not cut
static inline const float* tn_colsum(const ap_tn_problem& q) { return q.colsum_A; }
static inline const float* tn_colsum(const ap_tn8_problem&) { return nullptr; }        // (ap_quantize_bf8 forms the fp8 bias gradient)
template <class P> static inline int tn_shared_out(const P* problems, int count, int i) {
    for (int j = 0; j < count; ++j)
        if (j != i && (problems[j].C == problems[i].C || (tn_colsum(problems[i]) && tn_colsum(problems[j]) == tn_colsum(problems[i])))) return 1;
    return 0;
}

static inline int tn_validate(const ap_tn_problem* problems, int count, int max_count) {
    if (!problems) return AP_ERR_NULL;
    if (count <= 0 || count > max_count) return AP_ERR_SHAPE;
    for (int i = 0; i < count; ++i) {
        const ap_tn_problem& q = problems[i];
        if (!q.A || !q.B || !q.C) return AP_ERR_NULL;
        if (q.M <= 0 || q.N1 <= 0 || q.N2 <= 0 || q.M > AP_MAX_ROWS) return AP_ERR_SHAPE;
        if ((q.lda & 7) || q.lda < q.N1 || q.ldc < q.N2) return AP_ERR_SHAPE;
        if (!q.b_patch && ((q.ldb & 7) || q.ldb < q.N2)) return AP_ERR_SHAPE;         // patch-addressed B has no leading dimension
    }
    return AP_OK;
}

// Placement: one (problem, token split) = one XCD.  Greedy packing of the groups, largest first (stable), onto the least loaded of the
// 8 XCDs; the launch is 8 * (largest load) workgroups, the unused ids return at once.  A group that does not fit the least loaded XCD
// any more is CUT over XCDs where the kernel allows it (consecutive tiles of the 192 x 192 kernel share their A column block: with six
// blocks in a launch its table is nearly full -- 240 of 256 slots).  false = does not fit the table or the resident capacity (more than
// `cap` slots per XCD would start a second round of workgroups): the caller keeps the contiguous-range placement.
static inline bool tn_place(const TnTiles* pl, int count, int cap, bool may_cut, unsigned short* e, int table_len, int shift, int& blocks) {
    struct G { int p, s, n; };
    G g[TN_MAP_MAX]; int ng = 0;
    for (int i = 0; i < count; ++i) {
        if (pl[i].tiles * pl[i].splits > (1 << shift)) return false;
        for (int s = 0; s < pl[i].splits; ++s) { if (ng == table_len) return false; g[ng++] = G{i, s, pl[i].tiles}; }
    }
    for (int i = 1; i < ng; ++i) {                       // insertion sort by size, descending, stable
        const G v = g[i]; int j = i - 1;
        while (j >= 0 && g[j].n < v.n) { g[j + 1] = g[j]; --j; }
        g[j + 1] = v;
    }
    int load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < table_len; ++i) e[i] = TN_MAP_IDLE;
    for (int i = 0; i < ng; ++i) {
        for (int t = 0; t < g[i].n;) {
            int x = 0;
            for (int k = 1; k < 8; ++k) if (load[k] < load[x]) x = k;
            int take = g[i].n - t;
            if (take > cap - load[x]) { if (!may_cut) return false; take = cap - load[x]; }
            if (take <= 0 || (load[x] + take) * 8 > table_len) return false;
            for (int u = 0; u < take; ++u) e[(load[x] + u) * 8 + x] = (unsigned short)((g[i].p << shift) | (g[i].s * g[i].n + t + u));
            load[x] += take; t += take;
        }
    }
    int mx = 0;
    for (int k = 0; k < 8; ++k) if (load[k] > mx) mx = load[k];
    blocks = mx * 8;
    return true;
}
static_assert(T8_MAP_MAX <= TN_MAP_MAX, "tn_place sorts at most TN_MAP_MAX groups");

// ---- the 128 x 128-tile kernels (reduction steps of TN_STEP tokens)
// ap_gemm_tn_acc: about `target_blocks` workgroups, token ranges of at least 4 steps
static inline TnItemPlan tn_single_plan(int M, int N1, int N2, int target_blocks) {
    TnItemPlan p = {tn_ceil(N1, 128), tn_ceil(N2, 128), tn_ceil(M, TN_STEP), 0, 0, 0, 0};
    const int want = tn_ceil(target_blocks, p.t1 * p.t2);
    tn_split(p, want < p.steps / 4 ? want : p.steps / 4);
    return p;
}
// Grouped launch: token splits per problem such that the launch fills `capacity` resident workgroups once.  Two 256-thread workgroups
// are resident per CU: the launch should fill that single wave of workgroups as fully as possible but never spill into a second one
// (measured on the D1 blocks: 450 workgroups 125 us, 540 -> 175 us).
static inline int tn128_plan(const ap_tn_problem* problems, int count, int capacity, TnGroupPlan& grp) {
    if (const int rc = tn_validate(problems, count, TN_MAX_GROUP); rc != AP_OK) return rc;
    int max_steps = 8;
    for (int i = 0; i < count; ++i) {
        const ap_tn_problem& q = problems[i];
        grp.p[i] = TnItemPlan{tn_ceil(q.N1, 128), tn_ceil(q.N2, 128), tn_ceil(q.M, TN_STEP), 0, 0, 0, 0};
        grp.range_floats[i] = (size_t)q.N1 * q.N2 + (q.colsum_A ? (size_t)q.N1 : 0);
        if (grp.p[i].steps > max_steps) max_steps = grp.p[i].steps;
        if (q.b_patch) {            // whole patch rows in 16-byte chunks, inside the exactness bound of the magic division (gemm_epi.h)
            const ap_patch_map* m = q.b_patch;
            if (m->group <= 1 || m->kseg <= 1 || (q.N2 & 7) || (m->kseg & 7) || q.N2 % m->kseg ||
                (int64_t)q.M >= (int64_t)(0xFFFFFFFFu / (unsigned)m->group)) return AP_ERR_SHAPE;
        }
    }
    // smallest steps-per-workgroup (>= 8) whose block count fits the resident capacity (binary search: the block count is monotone)
    int lo = 8, hi = max_steps;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (tn_group_blocks(grp, count, mid) <= capacity) hi = mid; else lo = mid + 1;
    }
    tn_group_cut(grp, count, lo);
    return AP_OK;
}
static inline bool tn128_place(const TnGroupPlan& grp, int cap, TnMap& map, int& blocks) {
    TnTiles pl[TN_MAX_GROUP];
    for (int i = 0; i < grp.count; ++i) pl[i] = TnTiles{grp.p[i].t1 * grp.p[i].t2, grp.p[i].splits};
    return tn_place(pl, grp.count, cap, false, map.e, TN_MAP_MAX, TN_MAP_SHIFT, blocks);
}

// ---- the 192 x 192-tile kernels: every width a multiple of 192, whole K-tiles of `ktile` tokens (64 of bf16, 128 of fp8).  The token
// axis is cut into ranges of `ksps` K-tiles, the smallest (>= `floor`) that leaves at most one work item per CU and fits the placement.
static inline bool t8_search(int count, int n_cu, int floor, const int* ksteps, T8Plan& out) {
    if (count <= 0 || count > AP_TN_MAX_GROUP) return false;
    int64_t work = 0; int max_k = 1;
    for (int i = 0; i < count; ++i) {
        work += (int64_t)out.pl[i].tiles * ksteps[i];
        if (ksteps[i] > max_k) max_k = ksteps[i];
    }
    out.ksps = tn_ceil(work, n_cu);
    if (out.ksps < floor) out.ksps = floor;
    for (; out.ksps <= max_k; ++out.ksps) {
        int64_t items = 0;
        for (int i = 0; i < count; ++i) { out.pl[i].splits = tn_ceil(ksteps[i], out.ksps); items += (int64_t)out.pl[i].tiles * out.pl[i].splits; }
        if (items <= n_cu && tn_place(out.pl, count, n_cu / 8, true, out.map.e, T8_MAP_MAX, T8_MAP_SHIFT, out.blocks)) return true;
    }
    return false;
}
template <class P> static inline bool t8_plan(const P* problems, int count, int n_cu, int ktile, int floor, T8Plan& out) {
    int ksteps[AP_TN_MAX_GROUP];
    for (int i = 0; i < count && i < AP_TN_MAX_GROUP; ++i) {
        out.pl[i].tiles = (problems[i].N1 / 192) * (problems[i].N2 / 192); ksteps[i] = problems[i].M / ktile;
        out.shared_out[i] = tn_shared_out(problems, count, i);
    }
    return t8_search(count, n_cu, floor, ksteps, out);
}
// bf16: plain row-major operands, M >= 4096 (enabled: AP_GEMM_TN_8P); tn8_plan is given problems that fit
static inline bool tn8_fits(const ap_tn_problem& q, int enabled) {
    if (!enabled || !q.A || !q.B || !q.C || q.b_patch || q.N1 <= 0 || q.N2 <= 0) return false;
    if (q.N1 % 192 || q.N2 % 192 || q.M % 64 || q.M < 4096 || (q.lda & 7) || (q.ldb & 7) || q.lda < q.N1 || q.ldb < q.N2 || q.ldc < q.N2) return false;
    return !(q.colsum_weight && (reinterpret_cast<uintptr_t>(q.colsum_weight) & 3));
}
static inline bool tn8_plan(const ap_tn_problem* problems, int count, int n_cu, T8Plan& out) { return t8_plan(problems, count, n_cu, 64, 8, out); }
// fp8: one A format per launch, every problem of the launch or none
static inline bool tf8_plan(const ap_tn8_problem* problems, int count, int n_cu, int enabled, T8Plan& out) {
    for (int i = 0; i < count; ++i) {
        const ap_tn8_problem& q = problems[i];
        if (!enabled || q.a_fmt != problems[0].a_fmt || q.N1 % 192 || q.N2 % 192 || q.M % 128 || q.M < 4096) return false;
    }
    return t8_plan(problems, count, n_cu, 128, 4, out);
}

// ---- the 128 x 128-tile fp8 kernel (gemm_tn_fp8.h): K-steps of 128 tokens, widths multiples of 128
static inline int tf_plan(const ap_tn8_problem* problems, int count, int capacity, TnGroupPlan& grp) {
    if (!problems) return AP_ERR_NULL;
    if (count <= 0 || count > AP_TN_MAX_GROUP) return AP_ERR_SHAPE;
    int max_k = 4;
    for (int i = 0; i < count; ++i) {
        const ap_tn8_problem& q = problems[i];
        if (!q.A || !q.B || !q.C || !q.dq_a || !q.dq_b) return AP_ERR_NULL;
        if (q.M <= 0 || q.N1 <= 0 || q.N2 <= 0 || q.M > AP_MAX_ROWS) return AP_ERR_SHAPE;
        if ((q.lda & 15) || (q.ldb & 15) || q.lda < q.N1 || q.ldb < q.N2 || q.ldc < q.N2) return AP_ERR_SHAPE;
        if ((reinterpret_cast<uintptr_t>(q.A) & 15) || (reinterpret_cast<uintptr_t>(q.B) & 15)) return AP_ERR_SHAPE;
        if (q.N1 % 128 || q.N2 % 128 || (q.a_fmt != AP_FP8_E5M2 && q.a_fmt != AP_FP8_E4M3)) return AP_ERR_UNSUPPORTED;
        grp.p[i] = TnItemPlan{q.N1 / 128, q.N2 / 128, tn_ceil(q.M, 128), 0, 0, 0, tn_shared_out(problems, count, i)};
        grp.range_floats[i] = (size_t)q.N1 * q.N2;
        if (grp.p[i].steps > max_k) max_k = grp.p[i].steps;
    }
    // K-steps per workgroup (>= 4): the smallest time in rounds of resident workgroups (`capacity`: two 256-thread workgroups per CU, 32 KB of
    // LDS each), ceil(blocks / capacity) * (sps + 4) (the 4: a partial tile's epilogue and its atomics in K-step units) -- a launch with
    // more tiles than resident slots is cut along the tokens too, so its last round is not a nearly empty second wave of whole-axis workgroups
    int lo = 4;
    int64_t best = -1;
    for (int sps = 4; sps <= max_k; ++sps) {
        const int64_t cost = ((tn_group_blocks(grp, count, sps) + capacity - 1) / capacity) * (sps + 4);
        if (best < 0 || cost < best) { best = cost; lo = sps; }
    }
    tn_group_cut(grp, count, lo);
    return AP_OK;
}

// the LayerNorm riders of a launch: the items checked, the table filled (`first` is the launch's to set) and its workgroups counted
static inline int tn_ln_table(const ap_ln_reduce* ln_items, int ln_count, TnLn& ln, int& lblocks) {
    if (ln_count < 0 || ln_count > AP_LN_MAX_BATCH || (ln_count > 0 && !ln_items)) return AP_ERR_SHAPE;
    for (int i = 0; i < ln_count; ++i) {
        if (!ln_items[i].partial || !ln_items[i].dgamma || !ln_items[i].dbeta) return AP_ERR_NULL;
        if (ln_items[i].n_partial <= 0 || ln_items[i].C <= 0) return AP_ERR_SHAPE;
    }
    ln = TnLn{};                                        // (unused entries: null, 0)
    ln.count = ln_count; lblocks = 0;
    for (int i = 0; i < ln_count; ++i) {
        const ap_ln_reduce& q = ln_items[i];
        ln.it[i] = TnLnItem{q.partial, q.dgamma, q.dbeta, q.n_partial, q.C}; lblocks += (2 * q.C + 31) / 32;
    }
    return AP_OK;
}

// The launches of ap_gemm_tn_acc_grouped_ln, in order: launch k takes the problems order[first .. first + count) of the caller's group.
// The 192 x 192-tile LDS-DMA kernel takes the problems that fit it, with the LayerNorm riders; the rest of the group -- e.g. the
// 486-wide attention-weight projection of an outlooker block -- goes on in launches of the 128 x 128-tile kernel, 8 problems each,
// the riders with the first launch of all.  Where the 192 x 192 kernel takes nothing (no problem fits it, no ksps places them, or the
// deterministic mode, which takes at most 8 problems) a group of up to 8 stays one launch in its own order; a larger one is cut in
// the order rest, then fit.  (The order matters: the placement's sort is stable.)
enum { TN_KERNEL_8P = 0, TN_KERNEL_128 = 1 };
struct TnLaunch { int kernel, first, count, riders; };
struct TnDispatch { TnLaunch l[1 + AP_TN_MAX_GROUP / TN_MAX_GROUP]; int n; int order[AP_TN_MAX_GROUP]; T8Plan p8; };
static inline void tn_dispatch(const ap_tn_problem* problems, int count, bool deterministic, int n_cu, int enabled8, TnDispatch& d) {
    ap_tn_problem fit[AP_TN_MAX_GROUP];
    int ifit[AP_TN_MAX_GROUP], irest[AP_TN_MAX_GROUP], nfit = 0, nrest = 0;
    for (int i = 0; i < count; ++i) {
        if (!deterministic && tn8_fits(problems[i], enabled8)) { fit[nfit] = problems[i]; ifit[nfit++] = i; } else irest[nrest++] = i;
    }
    const bool on8 = nfit > 0 && tn8_plan(fit, nfit, n_cu, d.p8);
    int n = 0;
    d.n = 0;
    if (on8) {
        for (int i = 0; i < nfit; ++i) d.order[n++] = ifit[i];
        d.l[d.n++] = TnLaunch{TN_KERNEL_8P, 0, nfit, 1};
    }
    if (on8 || (!deterministic && count > TN_MAX_GROUP)) {
        const int first = n;
        for (int i = 0; i < nrest; ++i) d.order[n++] = irest[i];
        for (int i = 0; i < nfit && !on8; ++i) d.order[n++] = ifit[i];
        for (int i0 = first; i0 < count; i0 += TN_MAX_GROUP, ++d.n)
            d.l[d.n] = TnLaunch{TN_KERNEL_128, i0, count - i0 < TN_MAX_GROUP ? count - i0 : TN_MAX_GROUP, d.n == 0};
    } else {
        for (int i = 0; i < count; ++i) d.order[i] = i;
        d.l[d.n++] = TnLaunch{TN_KERNEL_128, 0, count, 1};
    }
}
