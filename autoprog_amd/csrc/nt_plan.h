// Host-side planning of the NT launches (gemm.hip: ap_gemm_nt, ap_gemm_nt_fp8): which kernel family takes a product, with which tile, grid
// and LDS, and every refusal.  Plain C++17, no HIP: the CU count, the run-time switches and the answer to "is the GELU table available?"
// come in as arguments (gemm.hip supplies them), so tests/host/nt_plan_check.cpp plans on a CPU.  A plan is launchable as it stands or it
// carries an error code; gemm.hip only turns it into kernel arguments.  The constants that planner and kernels share: gemm_nt_const.h.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../include/autoprog_hip.h"
#include "gemm_nt_const.h"

// the epilogue of a launch as plain facts (gemm.hip fills them from its EpiArgs; gelu = 4 arrives as gelu = 3 + noside)
struct NtEpi { bool bias, preact, dgelu_of, mul_by, mul8, row_scale, residual, q8, q8_scale; int ldr, gelu, noside; };
// the run-time switches, read once per process (nt_switches_from).  rules: AP_GEMM_NT_RULE = "N,K,variant[,lds_epi];..." (lds_epi -1: unset)
struct NtRule { int n, k, variant, lds_epi; };
struct NtSwitches { int mode8p, bm224, ws, skinny, tile, allow192, lds_epi, dbg, nrules; NtRule rules[16]; };
enum { NT_SKINNY = 0, NT_WS = 1, NT_8P = 2, NT_TILE = 3, NT_FP8_TILE = 4 };
// variant: 1 - 11 the k_gemm_nt tile shapes (nt_tile_shape), 20 / 21 the 8-phase kernel with 256 x 192 / 256 x 256 tiles (bm: 256 or 224).
// grid_y: the skinny kernel only.  tab: the launch carries the GELU table pointer.  flavour: 8-phase launches.  ws_epi .. per_xcd: WS.
struct NtPlan { int status, family, variant, bm, bn, ntiles, tiles_n, grid, grid_y, lds_bytes, lds_epi, prefetch, flavour, tab, ws_epi, n_slices, n_items, per_xcd; };

static inline void nt_parse_rules(const char* e, NtSwitches& s) {
    s.nrules = 0;
    while (e && *e && s.nrules < 16) {
        NtRule r = {0, 0, 0, -1};
        int used = 0;
        if (sscanf(e, "%d,%d,%d%n", &r.n, &r.k, &r.variant, &used) < 3) break;
        e += used;
        if (*e == ',') { int u2 = 0; if (sscanf(e, ",%d%n", &r.lds_epi, &u2) == 1) e += u2; }
        s.rules[s.nrules++] = r;
        if (*e == ';') ++e;
    }
}
// env: name -> value or null (getenv)
template <class Env> static inline NtSwitches nt_switches_from(Env env) {
    const auto num = [&](const char* name, int dflt) { const char* e = env(name); return e ? atoi(e) : dflt; };
    const auto is = [&](const char* name, char c) { const char* e = env(name); return e && e[0] == c; };
    NtSwitches s = {};
    s.mode8p = num("AP_GEMM_8P", 1);                    // 0: never the 8-phase kernel; 1 (default): nt_use_8p; 2: the gelu' launches too
    s.bm224 = num("AP_GEMM_BM224", 1);                  // 0: 256-row tiles everywhere
    s.ws = !is("AP_GEMM_WS", '0');                      // 0: never the weight-stationary kernel
    s.skinny = !is("AP_GEMM_NT_NO_SKINNY", '1');
    s.tile = num("AP_GEMM_NT_TILE", 0);                 // forces a variant
    s.allow192 = is("AP_GEMM_NT_192", '1');
    s.lds_epi = env("AP_GEMM_LDS_EPI") ? is("AP_GEMM_LDS_EPI", '1') : -1;       // 0 / 1 forces the direct / the LDS-staged epilogue
    s.dbg = num("AP_GEMM_DBG", 0);
    // tuning aid: AP_GEMM_NT_RULE overrides the choice for exact (N, K) pairs, so that a candidate can be timed INSIDE the training step
    // (bench.py AP_GEMM_TABLE=1) instead of in a cache-warm microbenchmark
    nt_parse_rules(env("AP_GEMM_NT_RULE"), s);
    return s;
}

static inline int nt_ceil(int a, int b) { return (a + b - 1) / b; }
static inline bool nt_is_8p(int variant) { return variant == 20 || variant == 21; }
static inline int nt_flavour(const NtEpi& e, bool tab) {        // g8_flavour() of gemm8p.h on the facts
    return (e.bias ? G8_BIAS : 0) | (e.gelu ? G8_GELU : 0) | (e.dgelu_of ? G8_DGELU : 0) | (e.row_scale ? G8_RS : 0) | (e.residual ? G8_RES : 0) |
           (e.mul_by ? G8_MUL : 0) | (e.mul8 ? G8_MUL8 : 0) | ((e.gelu == 3 && tab) ? G8_GTAB : 0) | ((e.q8 && !e.gelu) ? G8_Q8 : 0) | (e.noside ? G8_NOSIDE : 0);
}
static inline bool nt_has224(int flavour) {
    const int with224[] = {G8_FLAVOURS_224};
    for (int f : with224) if (f == flavour) return true;
    return false;
}
// variant, block tile and wave grid of the k_gemm_nt instantiations; any other variant is the 128 x 128 tile (variant 1)
#define NT_TILE_SHAPES(X) X(2, 128, 64, 2, 2) X(3, 64, 128, 2, 2) X(4, 64, 64, 2, 2) X(5, 256, 128, 4, 2) X(6, 128, 128, 2, 4) X(7, 256, 128, 2, 2) \
                          X(8, 128, 256, 2, 2) X(9, 256, 256, 2, 4) X(10, 128, 192, 2, 2) X(11, 64, 192, 2, 2)
struct NtTile { int variant, tm, tn, wm, wn; };
static inline NtTile nt_tile_shape(int variant) {
#define NT_SHAPE_ROW(...) {__VA_ARGS__},
    static const NtTile t[] = {NT_TILE_SHAPES(NT_SHAPE_ROW)};
#undef NT_SHAPE_ROW
    for (const NtTile& v : t) if (v.variant == variant) return v;
    return NtTile{1, 128, 128, 2, 2};
}

// Where the persistent 8-phase kernel is picked (measured INSIDE the training step, tools/instep_8p.sh; profiles/r03_gemm_instep_*):
// every launch with K % 64 == 0, M >= 4096 and N a multiple of 192 (256 x 192 tiles) or N >= 1024 (256 x 256 tiles, last column tile
// masked) -- 384 x 1152 plain 38.3 -> 30.7 us, + residual 45.3 -> 41.0, fc1 + GELU 61.5 -> 56.0, qkv 39.0 -> 35.0, the K = 192
// outlooker shapes 5 - 15 % -- except the gelu' epilogue, whose staged second operand still costs more than it saves (60.6 -> 62.3).
// K counts 2-byte elements (byte pairs of an fp8 launch).  -> 0 (no), 192 or 256 (block tile width)
static inline int nt_use_8p(int M, int N, int K, int ldc, const NtEpi& e, int ncu, int mode) {
    if (mode == 0 || (K & 63) || K < 128 || M < 4096 || (N & 7) || (ldc & 7) || (e.residual && (e.ldr & 7))) return 0;
    if (e.dgelu_of && (mode < 2 || e.residual)) return 0;
    if ((e.mul_by || e.mul8) && e.residual) return 0;
    int bn = N >= 1024 ? 256 : (N % 192 == 0 ? 192 : (N % 256 == 0 ? 256 : 0));
    if (N >= 384 && N % 192 == 0) {
        // both widths tile N: the persistent grid walks ceil(tiles / #CU) rounds of tiles, a 256-wide tile costs ~1.3 of a 192-wide one.
        // N = 1152 (4.5 -> 5 column tiles of 256): 25088 rows 2 x 1.3 against 3 rounds -> 256; the AutoProg stages' 8192 / 18432 rows
        // (128 / 192 px) one round against one, two against two -> 192 (12.2 against 13.8 us, 21.3 against 25.5); 12800 rows (160 px) one
        // round of 250 tiles against two of 300 -> 256 (16.3 against 21.5): tools/sweep_nt.py, AP_GEMM_NT_TILE = 20 / 21.
        const int64_t mt = (M + 255) / 256;
        const int64_t r192 = (mt * (N / 192) + ncu - 1) / ncu, r256 = (mt * ((N + 255) / 256) + ncu - 1) / ncu;
        bn = (r192 * 10 < r256 * 13) ? 192 : 256;
        // (N = 768, the D5 widths, at 50176 rows = batch 64: 784 tiles of 192 are 3.06 -> FOUR rounds, 588 of 256 three: 64.2 against 67.1 us
        // at K = 768, 231 against 241 - 257 at K = 3072; at 48608 rows three rounds of 192: 54.0 against 63.1.  N = 384 / 576 stay on 192.)
    }
    return N < 192 ? 0 : bn;
}

// The plan of one launch.  K, lda, ldb as the entry point takes them (bytes of an fp8 launch).  table(): is the GELU table available?  Its
// first call per device builds the table and synchronises the stream, and inside a capture it refuses -- so it is asked only where a
// table kernel is about to be chosen, never for a launch that cannot use it.
template <class Table>
static inline NtPlan nt_plan(int M, int N, int K, int lda, int ldb, int ldc, const NtEpi& e, bool fp8, int ncu, const NtSwitches& s, Table&& table) {
    NtPlan p = {};
    const auto fail = [&p](int rc) { p.status = rc; return p; };
    const auto ask = [&] { p.tab = table() ? 1 : 0; return p.tab != 0; };
    const int align = fp8 ? 15 : 7;                     // 16-byte chunks: 8 bf16, 16 e4m3
    if (M <= 0 || N <= 0 || K <= 0 || M > AP_MAX_ROWS) return fail(AP_ERR_SHAPE);          // (tile counts (M + tile - 1) / tile are formed in int)
    if ((K & align) || (lda & align) || (ldb & align) || lda < K || ldb < K || ldc < N) return fail(AP_ERR_SHAPE);
    if (e.residual && e.ldr < N) return fail(AP_ERR_SHAPE);
    if (e.mul_by + e.dgelu_of + e.mul8 > 1) return fail(AP_ERR_SHAPE);
    if (!e.noside && (e.gelu < 0 || e.gelu > 3 || (e.gelu >= 2 && !e.preact))) return fail(AP_ERR_SHAPE);
    if (fp8 && e.q8 && (!e.q8_scale || !e.gelu)) return fail(AP_ERR_SHAPE);
    // gelu = 4 (noside): the value of mode 3 in `out`, no side store -- the table flavours of the 8-phase and the weight-stationary kernel only
    if (e.noside && (e.mul_by || e.dgelu_of || e.mul8 || e.residual || e.q8 || !e.bias)) return fail(AP_ERR_UNSUPPORTED);
    // q8 of a bf16 launch: the output a second time as e4m3 bytes, for the fp8 input-gradient product that consumes it.  Exists in the
    // 8-phase kernel's mul_by8 flavours only (the input gradient of fc2); which kernel may carry a q8 at all is ruled below, after the choice
    if (!fp8 && e.q8 && (!e.q8_scale || !e.mul8 || e.bias || e.gelu || e.residual || (ldc & 15))) return fail(AP_ERR_UNSUPPORTED);
    const int K2 = fp8 ? K / 2 : K;                     // the kernels' element is 2 bytes
    // an fp8 launch runs on the 8-phase kernel where the bf16 launch of these dimensions would (whole 128-byte K-tiles), else on its tile kernel
    const int bn8 = (fp8 && ((K & 127) || e.dgelu_of)) ? 0 : nt_use_8p(M, N, K2, ldc, e, ncu, s.mode8p);
    const int pick8 = bn8 == 192 ? 20 : bn8 ? 21 : 0;
    int variant = pick8, rule_epi = -1;
    if (!fp8) {
        if (s.skinny && M <= 256) {          // (K = 1000: the head's input gradient ran on three 128 x 128 workgroups, 31 us, before)
            if (e.noside || e.q8) return fail(AP_ERR_UNSUPPORTED);       // (a gelu = 4 caller falls back to gelu = 3 with a side buffer)
            p.family = NT_SKINNY; p.grid = nt_ceil(N, 32); p.grid_y = nt_ceil(M, 64); p.lds_bytes = 8 * 64 * SK_STRIDE * (int)sizeof(float);
            return p;
        }
        // K = 192 with a GELU-table or a stored-derivative epilogue at many rows (the Outlooker's MLP): the weight-stationary kernel
        if (s.ws && K == WS_K && N % WS_BN == 0 && M % WS_BM == 0 && M >= 16384 && !(ldc & 15) && !(lda & 7) && !(ldb & 7) &&
            !(e.dgelu_of || e.mul_by || e.row_scale || e.residual || e.q8)) {
            int epi = -1;
            if (e.gelu == 3 && (e.preact || e.noside) && !e.mul8) { if (ask()) epi = e.noside ? 2 : 0; }
            else if (!e.gelu && e.mul8 && !e.bias) epi = 1;
            if (epi >= 0 && N / WS_BN <= ncu / 8) {
                p.family = NT_WS; p.ws_epi = epi; p.n_slices = N / WS_BN; p.n_items = M / WS_BM;
                p.per_xcd = (ncu / 8) / p.n_slices;                  // tile streams per XCD: 10 for three slices on 32 CUs (two CUs per XCD stay idle)
                p.grid = ncu & ~7; p.lds_bytes = WS_LDS_BYTES(epi);
                return p;
            }
        }
        // tile selection, measured on the VOLO-D1 shape list (tools/bench_gemm.py, AP_GEMM_NT_TILE sweep): narrow / short problems want small
        // tiles (more workgroups, 4-6 waves/SIMD, no wasted columns at N = 192/486/576), the rest 128x128
        variant = s.tile;
        if (variant == 0) {
            // 128x192 tiles (wave tile 64x96: 17 % fewer LDS bytes per FLOP, direct epilogue), AP_GEMM_NT_192=1: faster with cache-warm
            // operands (33.9 vs 37.2 us on the dfc1 shape when the same buffers are reused back to back) but the training step, whose
            // operands come from HBM, is 0.3 ms SLOWER with them -> off by default
            if (s.allow192 && N % 192 == 0 && N >= 384 && M >= 4096 && !e.gelu && !e.dgelu_of && !e.residual && K >= 384) variant = 10;
            else if (pick8) variant = pick8;                                         // persistent 8-phase kernel (gemm8p.h)
            else if (N <= 512 && K <= 256) variant = 4;                              // 64x64
            else if (N <= 256 || ((N % 128 != 0) && (N % 64 == 0))) variant = 2;     // 128x64
            else variant = 1;                                                        // 128x128
            for (int i = 0; i < s.nrules; ++i)
                if (s.rules[i].n == N && s.rules[i].k == K) { variant = s.rules[i].variant; rule_epi = s.rules[i].lds_epi; }
        }
        // the 8-phase kernel takes whole 8-column chunks and whole K-tiles only
        if (nt_is_8p(variant) && ((K & 63) || (N & 7) || (ldc & 7) || (e.residual && (e.ldr & 7)))) variant = 1;
        if (e.noside && (!nt_is_8p(variant) || !ask())) return fail(AP_ERR_UNSUPPORTED);
    }
    // the e4m3 side output exists in the 8-phase kernel only, and only where nt_use_8p takes the launch: a forced tile (AP_GEMM_NT_TILE), a
    // rule (AP_GEMM_NT_RULE), AP_GEMM_NT_192 or the fallback above may have picked a kernel that never writes it -- refused, not silently skipped
    if (e.q8 && !(bn8 && nt_is_8p(variant))) return fail(AP_ERR_UNSUPPORTED);
    if (nt_is_8p(variant)) {
        if (e.gelu == 3) ask();
        p.family = NT_8P; p.variant = variant; p.bn = variant == 20 ? 192 : 256; p.bm = 256; p.flavour = nt_flavour(e, p.tab != 0);
        p.tiles_n = nt_ceil(N, p.bn); p.ntiles = nt_ceil(M, 256) * p.tiles_n; p.lds_bytes = G8_LDS_BYTES;
        const int cap = ncu & ~7;
        // 224-row tiles where they put more CUs to work inside ONE round of the persistent grid (a launch of fewer tiles than CUs takes
        // about one tile's time whatever the number of idle CUs: tools/tile_rounds_probe.py): VOLO-D1's N = 384 products at 25088 rows,
        // 98 x 2 = 196 tiles of 256 rows -> 112 x 2 = 224 tiles of 224
        const int t224 = nt_ceil(M, 224) * p.tiles_n;
        if (s.bm224 && !fp8 && p.bn == 192 && nt_has224(p.flavour) && p.ntiles < cap && t224 <= cap && t224 > p.ntiles) { p.bm = 224; p.ntiles = t224; }
        const int want = (p.ntiles + 7) & ~7;           // a multiple of 8: the kernel deals tiles per XCD label
        p.grid = want < cap ? want : cap;
        return p;
    }
    // epilogue flavour: the LDS-staged one (fully coalesced 16-B rows) wins on 128x128 / 64x64 tiles, the direct one (64-B row segments, no
    // LDS round trip) on the 128x64 tiles of the N = 576 shapes
    const NtTile t = nt_tile_shape(variant);               // (fp8: its one tile kernel, 128 x 128 with the LDS-staged epilogue)
    p.family = fp8 ? NT_FP8_TILE : NT_TILE; p.variant = t.variant; p.bm = t.tm; p.bn = t.tn;
    p.lds_epi = fp8 ? 1 : rule_epi >= 0 ? rule_epi != 0 : s.lds_epi >= 0 ? s.lds_epi : (variant != 2 && variant != 10);
    // the 128 x 128 tile whose epilogue reads ONE more tile: the prefetching instantiation
    p.prefetch = !fp8 && t.variant == 1 && p.lds_epi && e.residual != (e.dgelu_of || e.mul_by) && !(s.dbg & 2);
    p.tiles_n = nt_ceil(N, t.tn); p.ntiles = nt_ceil(M, t.tm) * p.tiles_n; p.grid = p.ntiles;
    return p;
}
