// Plans a fixed list of attention, outlook and LayerNorm launches with csrc/attn_plan.h and csrc/ln_plan.h on the CPU, the way the entry
// points of mhsa.hip, outlook.hip and layernorm.hip do, at 256, 304 and 64 CUs, parses a list of fake environments with csrc/switches.h, and
// prints both as one JSON document (tests/test_attn_ln_plan_host.py compares with tests/golden/attn_ln_plans.json); `--record FILE` writes
// that document to FILE instead.  A plan prints as one short string -- the kernel with its template arguments, then the launch geometry; a
// grid that depends on the CU count as 256/304/64 -- and the plans of one group (a direction, a head dim, a setting) share a line.  Beside
// the print, every plan is checked against the invariants listed at the check_* functions.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include "../../autoprog_amd/csrc/attn_plan.h"
#include "../../autoprog_amd/csrc/ln_plan.h"

#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, "attn_ln_plan_check: %s: ", current.c_str()); fprintf(stderr, __VA_ARGS__); \
                                               fprintf(stderr, " [%s]\n", #cond); exit(1); } } while (0)
static std::string current;
static const int CUS[] = {256, 304, 64};
typedef std::vector<std::pair<std::string, std::string>> Entries;
static std::vector<std::pair<std::string, Entries>> groups;             // group -> (case -> plan), in the order they were put
static Entries switch_rows;

// "AP_MHSA_FLASH=1 AP_OUTLOOK_P=0" -> the switches, through the reader the library hands getenv to
static ApSwitches switches_of(const std::string& spec) {
    std::map<std::string, std::string> env;
    std::istringstream in(spec);
    for (std::string t; in >> t;) env[t.substr(0, t.find('='))] = t.substr(t.find('=') + 1);
    return ap_switches_from([&](const char* name) { const auto it = env.find(name); return it == env.end() ? nullptr : it->second.c_str(); });
}
static std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
static std::string fmt(const char* f, ...) {
    char buf[512];
    va_list ap; va_start(ap, f); vsnprintf(buf, sizeof buf, f, ap); va_end(ap);
    return buf;
}
static void put(const std::string& group, const std::string& name, const std::string& plan) {
    for (auto& g : groups) if (g.first == group) { g.second.emplace_back(name, plan); return; }
    groups.push_back({group, {{name, plan}}});
}
// "256" where the three agree, else "256/304/64"
static std::string per_cu(const int (&v)[3]) { return v[0] == v[1] && v[1] == v[2] ? std::to_string(v[0]) : fmt("%d/%d/%d", v[0], v[1], v[2]); }
static std::string with_env(const std::string& name, const char* env) { return *env ? name + ", " + env : name; }

// ---- attention.  A launchable plan asks for no more LDS than it opts in to (64 KB need no opt-in); 1 <= grid <= items; a persistent grid
// is a multiple of 8 or the item count; the workspace is 4 B per (image, head, query) on the blocked path and 0 elsewhere -- and since
// ap_mhsa_bwd_workspace and ap_mhsa_bwd both plan with mhsa_plan(ATTN_BWD, ...), two plans of the same arguments are equal
static std::string mhsa_text(const MhsaPlan& p, const std::string& grid) {
    if (p.status != AP_OK) return fmt("refused %d", p.status);
    if (p.family == MHSA_FLASH) return fmt("flash ws=%zu", p.ws_bytes);
    const std::string k = p.family == MHSA_FWD ? fmt("k_mhsa_fwd<%d,%d>", p.nt, p.hdt) : p.family == MHSA_FWD_P ? fmt("k_mhsa_fwd_p<%d>", p.nt) :
                          p.family == MHSA_BWD ? fmt("k_mhsa_bwd<%d>", p.hdt) : p.family == MHSA_BWD_DS ? fmt("k_mhsa_bwd_ds<%d>", p.nt / 2) : fmt("k_class_attn<%d>", p.hdt / 8);
    return k + " grid=" + grid + fmt(" block=%d lds=%d optin=%d", p.block, p.lds_bytes, p.lds_optin);
}
static void check_mhsa(int dir, int B, int N, int heads, int hd, int cus, const ApSwitches& sw, bool fp8, const MhsaPlan& p) {
    REQUIRE(p.status == AP_OK || p.status == AP_ERR_SHAPE || p.status == AP_ERR_UNSUPPORTED, "status %d", p.status);
    const MhsaPlan again = mhsa_plan(dir, B, N, heads, hd, cus, sw, fp8);
    REQUIRE(!memcmp(&again, &p, sizeof p), "a second plan of the same arguments differs");
    if (p.status != AP_OK) return;
    REQUIRE(p.ws_bytes == (dir == ATTN_BWD && p.family == MHSA_FLASH ? (size_t)4 * B * heads * N : 0), "workspace %zu", p.ws_bytes);
    REQUIRE(p.fp8 == 0 || p.family == MHSA_FLASH, "fp8 on family %d", p.family);
    if (p.family == MHSA_FLASH) return;
    REQUIRE(p.items == B * heads && p.grid >= 1 && p.grid <= p.items, "grid %d of %d items", p.grid, p.items);
    REQUIRE(p.lds_bytes > 0 && p.lds_bytes <= (p.lds_optin ? p.lds_optin : 64 * 1024), "LDS %d, opt-in %d", p.lds_bytes, p.lds_optin);
    REQUIRE(p.nt >= 2 && p.nt <= 16 && p.nt * 16 >= N && (p.hdt == 32 || p.hdt == 64) && p.hdt >= hd, "nt %d hd %d", p.nt, p.hdt);
    if (p.family == MHSA_FWD_P || p.family == MHSA_BWD_DS) {
        REQUIRE(p.grid % 8 == 0 || p.grid == p.items, "persistent grid %d of %d items", p.grid, p.items);
        REQUIRE(p.block == 1024 && p.hdt == 32 && p.nt >= 8 && p.nt <= 14, "block %d nt %d", p.block, p.nt);
    }
}
static void mhsa_case(int dir, int B, int N, int heads, int hd, const char* env, bool fp8 = false) {
    const ApSwitches sw = switches_of(env);
    const std::string group = with_env(fmt("mhsa %s%s hd=%d %dx%d", dir == ATTN_FWD ? "fwd" : "bwd", fp8 ? " fp8" : "", hd, B, heads), env);
    MhsaPlan p[3]; int grid[3];
    for (int i = 0; i < 3; ++i) {
        current = group + fmt(" N=%d @%d", N, CUS[i]);
        p[i] = mhsa_plan(dir, B, N, heads, hd, CUS[i], sw, fp8);
        check_mhsa(dir, B, N, heads, hd, CUS[i], sw, fp8, p[i]);
        grid[i] = p[i].grid; p[i].grid = 0;
        REQUIRE(!memcmp(&p[i], &p[0], sizeof p[0]), "more than the grid depends on the CU count");
    }
    put(group, fmt("N=%d", N), mhsa_text(p[0], per_cu(grid)));
}
static void class_attn_case(int B, int N, int heads, int hd) {
    current = fmt("class_attn hd=%d N=%d", hd, N);
    const MhsaPlan p = class_attn_plan(B, N, heads, hd);
    if (p.status == AP_OK) REQUIRE(p.grid == B * heads && p.block == 256 && p.lds_bytes <= 64 * 1024 && p.lds_bytes >= (N + 2048) * 4, "grid %d LDS %d", p.grid, p.lds_bytes);
    put(fmt("class_attn hd=%d %dx%d", hd, B, heads), fmt("N=%d", N), mhsa_text(p, std::to_string(p.grid)));
}

// ---- outlook.  LDS <= the opt-in (64 KB need none); 1 <= grid <= items, items = B * nstrips * heads with nstrips strips of sr rows covering
// the h window rows; a persistent grid is a multiple of 8 or the item count, and its tables fit the instantiation; a backward plan on the
// gather kernels carries the dlogits launch
static std::string olk_text(const OutlookPlan& p, const std::string& grid) {
    static const char* names[] = {"k_outlook_p<512,3,1>", "k_outlook_p<256,5,2>", "k_outlook_gather_mfma", "k_outlook_gather"};
    if (p.status != AP_OK) return fmt("refused %d", p.status);
    std::string t = fmt("%s sr=%d items=%d grid=", names[p.family], p.sr, p.nitems) + grid + fmt(" lds=%d optin=%d", p.lds_bytes, p.lds_optin);
    if (p.family <= OLK_P256) t += fmt(" wp_shift=%d", p.wp_shift);
    if (p.dl_grid) t += fmt(" + k_outlook_dlogits sr=%d grid=%d lds=%d optin=%d", p.dl_sr, p.dl_grid, p.dl_lds, p.dl_optin);
    return t;
}
static void check_outlook(int dir, int B, int H, int W, int heads, const OutlookPlan& p) {
    REQUIRE(p.status == AP_OK || p.status == AP_ERR_SHAPE || p.status == AP_ERR_UNSUPPORTED, "status %d", p.status);
    if (p.status != AP_OK) return;
    const int h = (H + 1) / 2, w = (W + 1) / 2;
    REQUIRE(p.sr >= 1 && p.sr <= h && p.nstrips == (h + p.sr - 1) / p.sr && p.nitems == B * p.nstrips * heads, "sr %d, %d strips, %d items", p.sr, p.nstrips, p.nitems);
    REQUIRE(p.grid >= 1 && p.grid <= p.nitems, "grid %d of %d items", p.grid, p.nitems);
    REQUIRE(p.lds_bytes > 0 && p.lds_bytes <= (p.lds_optin ? p.lds_optin : 64 * 1024), "LDS %d, opt-in %d", p.lds_bytes, p.lds_optin);
    if (p.family == OLK_P512 || p.family == OLK_P256) {
        const int T = p.block, nsu = p.family == OLK_P512 ? 3 : 5, npu = p.family == OLK_P512 ? 1 : 2;
        REQUIRE(p.grid % 8 == 0 || p.grid == p.nitems, "persistent grid %d of %d items", p.grid, p.nitems);
        REQUIRE(w <= 32 && p.sr <= 3 && (2 * p.sr + 3) * (2 * w + 1) * 4 <= nsu * T && (p.sr + 1) * w * OKK <= npu * T && p.lds_bytes <= 80 * 1024, "tables of sr %d at %d threads", p.sr, T);
        REQUIRE(p.wp_shift == (w <= 16 ? 4 : 5) && p.dl_grid == 0, "wp_shift %d", p.wp_shift);
    } else {
        REQUIRE(p.block == OGT && p.grid == p.nitems, "grid %d of %d items", p.grid, p.nitems);
        if (dir == ATTN_BWD) REQUIRE(p.dl_sr >= 1 && p.dl_sr <= h && p.dl_nstrips == (h + p.dl_sr - 1) / p.dl_sr && p.dl_grid == B * p.dl_nstrips * heads &&
                                     p.dl_lds > 0 && p.dl_lds <= (p.dl_optin ? p.dl_optin : 64 * 1024), "dlogits: sr %d grid %d LDS %d", p.dl_sr, p.dl_grid, p.dl_lds);
        else REQUIRE(p.dl_grid == 0 && p.dl_lds == 0, "a forward plan with a dlogits launch");
    }
}
static void outlook_case(int dir, int B, int H, int W, int heads, const char* env) {
    const ApSwitches sw = switches_of(env);
    const std::string group = with_env(fmt("outlook %s B=%d heads=%d", dir == ATTN_FWD ? "fwd" : "bwd", B, heads), env);
    OutlookPlan p[3]; int grid[3];
    for (int i = 0; i < 3; ++i) {
        current = group + fmt(" %dx%d @%d", H, W, CUS[i]);
        p[i] = outlook_plan(dir, B, H, W, heads, CUS[i], sw);
        check_outlook(dir, B, H, W, heads, p[i]);
        grid[i] = p[i].grid; p[i].grid = 0;
        REQUIRE(!memcmp(&p[i], &p[0], sizeof p[0]), "more than the grid depends on the CU count");
    }
    put(group, fmt("%dx%d", H, W), olk_text(p[0], per_cu(grid)));
}

// ---- LayerNorm.  A launch has 1 <= grid <= ceil(rows / rows per workgroup), G lanes x V chunks cover the row, LDS <= 64 KB (no kernel opts
// in), the instantiation exists; the backward writes n_partial = grid <= LN_MAX_PARTIAL rows of partials; rows = 0 launches nothing
enum { K_FWD, K_FWD_FP8, K_BWD, K_BWD_PARTIAL, K_BWD_POOL };
static const int64_t LN_ROWS[] = {0, 1, 300, 25088, 100352};
static void ln_case(int kind, int C, const char* env) {
    static const char* kinds[] = {"fwd", "fwd fp8", "bwd", "bwd partial", "bwd pool"};
    const ApSwitches sw = switches_of(env);
    const bool bwd = kind >= K_BWD;
    std::string grids, text;
    for (const int64_t rows : LN_ROWS) {
        current = with_env(fmt("ln %s C=%d rows=%lld", kinds[kind], C, (long long)rows), env);
        const LnPlan p = bwd ? ln_bwd_plan(rows, C, sw, kind == K_BWD_POOL) : ln_fwd_plan(rows, C, sw, kind == K_FWD_FP8);
        REQUIRE(p.status == AP_OK || p.status == AP_ERR_SHAPE || p.status == AP_ERR_UNSUPPORTED, "status %d", p.status);
        if (p.status == AP_OK && rows <= 0) REQUIRE(p.grid == 0 && p.n_partial == 0, "grid %d without rows", p.grid);
        if (p.status == AP_OK && rows > 0) {
            const int64_t per_block = (int64_t)(256 / p.G) * (bwd ? 1 : sw.ln_fwd_rpg);
            REQUIRE(p.G >= 8 && p.G <= 64 && !(p.G & (p.G - 1)) && p.V >= 1 && p.V <= 4 && p.G * p.V * 8 >= C, "G %d V %d", p.G, p.V);
            REQUIRE(p.grid >= 1 && p.grid <= (rows + per_block - 1) / per_block && p.block == 256, "grid %d", p.grid);
            REQUIRE(p.lds_bytes > 0 && p.lds_bytes <= 64 * 1024, "LDS %d", p.lds_bytes);
            REQUIRE(bwd ? (p.family == LN_BWD || p.family == LN_BWD_PF) : (p.family == LN_FWD || p.family == LN_FWD_LP), "family %d", p.family);
            REQUIRE(p.n_partial == (bwd ? p.grid : 0) && p.n_partial <= LN_MAX_PARTIAL, "%d partial rows", p.n_partial);
            if (p.family == LN_FWD_LP) REQUIRE(p.V <= 3, "k_ln_fwd_lp<%d>", p.V);
            if (p.family == LN_BWD_PF) REQUIRE(p.V <= 2 && (p.OCC == 1 || (p.OCC == 4 && p.V == 1 && p.U == 2)) && (!p.pool || (p.V == 1 && p.U == 2 && p.OCC == 1)),
                                               "k_ln_bwd_pf<%d, %d, %d, %d>", p.V, p.U, p.OCC, p.pool);
            REQUIRE((kind == K_BWD_POOL) == (p.pool != 0), "pool %d", p.pool);
        }
        // the kernel of a width does not depend on the row count; the grid (= the backward's partial rows) does
        const std::string k = p.status != AP_OK ? fmt("refused %d", p.status) : !p.grid ? "" :
                              (p.family == LN_FWD ? fmt("k_ln_fwd<%d,%d>", p.V, p.U) : p.family == LN_FWD_LP ? fmt("k_ln_fwd_lp<%d>", p.V) : p.family == LN_BWD ? fmt("k_ln_bwd<%d,%d>", p.V, p.U) :
                               fmt("k_ln_bwd_pf<%d,%d,%d,%d>", p.V, p.U, p.OCC, p.pool)) + fmt(" G=%d lds=%d", p.G, p.lds_bytes);
        if (!k.empty()) { REQUIRE(text.empty() || text == k, "the kernel depends on the row count"); text = k; }
        grids += (grids.empty() ? "" : "/") + std::to_string(p.status == AP_OK ? p.grid : 0);
    }
    put(with_env(fmt("ln %s", kinds[kind]), env), fmt("C=%d", C), text.rfind("refused", 0) == 0 ? text : text + " grid=" + grids);
}

// ---- switches: every name unset, valid, invalid and at its boundaries
static void switches_case(const char* env) {
    const ApSwitches s = switches_of(env);
    current = std::string("switches ") + env;
    REQUIRE(s.ln_fwd_rpg >= 1 && s.ln_bwd_grid >= 1 && s.ln_bwd_grid <= LN_MAX_PARTIAL && s.conv_grid >= 1 && s.conv_wgrad_grid >= 1 && s.conv7_grid >= 1 &&
            s.conv7_wgrad_grid >= 1 && (s.conv_waves == 4 || s.conv_waves == 8) && (s.mlp_fused_v == 1 || s.mlp_fused_v == 2), "a value out of its range");
    switch_rows.emplace_back(env, fmt("%d %d %d | %d %d %d %d | %d %d %d %d %d %d | %d %d %d %d %d %d %d %d | %d %d | %d %d %d %d", s.mhsa_flash, s.mhsa_fwd_p, s.mhsa_bwd_ds, s.outlook_p,
         s.outlook_mfma, s.outlook_sr, s.outlook_srw, s.ln_fwd_lp, s.ln_fwd_rpg, s.ln_fwd_wide, s.ln_bwd_pf, s.ln_bwd_grid, s.ln_bwd_grid_set, s.conv_grid, s.conv_waves,
         s.conv_wgrad_grid, s.conv_wgrad_p, s.conv128_grid, s.conv7_grid, s.conv7_wgrad_grid, s.conv_abl, s.mlp_fused_v, s.gelu_table, s.tn_8p, s.tn_group_blocks,
         s.tn_blocks, s.tn_place));
}
static const char* const switch_envs[] = {
    "",
    "AP_MHSA_FLASH=1 AP_MHSA_FWD_P=0 AP_MHSA_BWD_DS=0", "AP_MHSA_FLASH=0 AP_MHSA_FWD_P=2 AP_MHSA_BWD_DS=x", "AP_MHSA_FLASH=10 AP_MHSA_FWD_P=-1 AP_MHSA_BWD_DS=", "AP_MHSA_FLASH=yes",
    "AP_OUTLOOK_P=0 AP_OUTLOOK_MFMA=0 AP_OUTLOOK_SR=1 AP_OUTLOOK_SRW=2", "AP_OUTLOOK_P=2 AP_OUTLOOK_MFMA=1 AP_OUTLOOK_SR=2 AP_OUTLOOK_SRW=0", "AP_OUTLOOK_P=x AP_OUTLOOK_MFMA=-1 AP_OUTLOOK_SR=-3 AP_OUTLOOK_SRW=99",
    "AP_LN_FWD_LP=0 AP_LN_FWD_RPG=4 AP_LN_FWD_WIDE=1", "AP_LN_FWD_LP=x AP_LN_FWD_RPG=0 AP_LN_FWD_WIDE=x", "AP_LN_FWD_RPG=-2", "AP_LN_FWD_RPG=1",
    "AP_LN_BWD_PF=0 AP_LN_BWD_GRID=8", "AP_LN_BWD_PF=2 AP_LN_BWD_GRID=1", "AP_LN_BWD_PF=3 AP_LN_BWD_GRID=1024", "AP_LN_BWD_PF=-1 AP_LN_BWD_GRID=1025", "AP_LN_BWD_GRID=2000", "AP_LN_BWD_GRID=0",
    "AP_LN_BWD_GRID=", "AP_LN_BWD_GRID=x",
    "AP_CONV_GRID=3 AP_CONV_WAVES=4 AP_CONV_WGRAD_GRID=3 AP_CONV_WGRAD_P=0", "AP_CONV_GRID=0 AP_CONV_WAVES=8 AP_CONV_WGRAD_GRID=0 AP_CONV_WGRAD_P=2",
    "AP_CONV_GRID=-5 AP_CONV_WAVES=5 AP_CONV_WGRAD_GRID=x AP_CONV_WGRAD_P=x", "AP_CONV_GRID=1 AP_CONV_WAVES=4x AP_CONV_WGRAD_GRID=1",
    "AP_CONV128_GRID=3 AP_CONV7_GRID=3 AP_CONV7_WGRAD_GRID=3 AP_CONV_ABL=7", "AP_CONV128_GRID=0 AP_CONV7_GRID=0 AP_CONV7_WGRAD_GRID=0 AP_CONV_ABL=x",
    "AP_CONV128_GRID=-1 AP_CONV7_GRID=-1 AP_CONV7_WGRAD_GRID=-1 AP_CONV_ABL=-1", "AP_CONV128_GRID=1 AP_CONV7_GRID=1 AP_CONV7_WGRAD_GRID=1",
    "AP_MLP_FUSED_V=1 AP_GELU_TABLE=0", "AP_MLP_FUSED_V=2 AP_GELU_TABLE=1", "AP_MLP_FUSED_V=12 AP_GELU_TABLE=01", "AP_MLP_FUSED_V=0 AP_GELU_TABLE=x", "AP_MLP_FUSED_V= AP_GELU_TABLE=",
    "AP_GEMM_TN_8P=0 AP_GEMM_TN_GROUP_BLOCKS=64 AP_GEMM_TN_BLOCKS=128 AP_GEMM_TN_PLACE=0", "AP_GEMM_TN_8P=x AP_GEMM_TN_GROUP_BLOCKS=-1 AP_GEMM_TN_BLOCKS=0 AP_GEMM_TN_PLACE=2",
};

#define SWITCH_FIELDS "mhsa_flash mhsa_fwd_p mhsa_bwd_ds | outlook_p outlook_mfma outlook_sr outlook_srw | ln_fwd_lp ln_fwd_rpg ln_fwd_wide ln_bwd_pf ln_bwd_grid ln_bwd_grid_set | " \
                      "conv_grid conv_waves conv_wgrad_grid conv_wgrad_p conv128_grid conv7_grid conv7_wgrad_grid conv_abl | mlp_fused_v gelu_table | tn_8p tn_group_blocks tn_blocks tn_place"
static std::string object_of(const Entries& e, const char* sep) {
    std::string t = "{";
    for (size_t i = 0; i < e.size(); ++i) t += (i ? sep : "") + ("\"" + e[i].first + "\": \"" + e[i].second + "\"");
    return t + "}";
}

int main(int argc, char** argv) {
    for (const char* env : switch_envs) switches_case(env);
    // ---- attention: both sides of N = 96 | 97 (7 tiles), 112 | 113, 208 | 209 (13 tiles), 224 | 225 (nt 14 | 16), 256 | 257 (blocked)
    const int Ns[] = {1, 96, 97, 112, 113, 196, 197, 208, 209, 224, 225, 256, 257, 784};
    const int items[][2] = {{64, 12}, {1, 6}, {25, 12}};               // B x heads = 768, 6, 300
    for (const int dir : {ATTN_FWD, ATTN_BWD})
        for (const int hd : {32, 48, 64})
            for (const auto& bh : items)
                for (const int N : Ns) mhsa_case(dir, bh[0], N, bh[1], hd, "");
    for (const int N : Ns) {
        for (const int hd : {32, 48, 64}) mhsa_case(ATTN_FWD, 1, N, 6, hd, "", true);
        for (const int hd : {32, 64}) {
            for (const int dir : {ATTN_FWD, ATTN_BWD}) mhsa_case(dir, 64, N, 12, hd, "AP_MHSA_FLASH=1");
            mhsa_case(ATTN_FWD, 1, N, 6, hd, "AP_MHSA_FLASH=1", true);
            mhsa_case(ATTN_FWD, 1, N, 6, hd, "AP_MHSA_FLASH=0", true);
        }
        mhsa_case(ATTN_FWD, 64, N, 12, 32, "AP_MHSA_FWD_P=0");
        mhsa_case(ATTN_BWD, 64, N, 12, 32, "AP_MHSA_BWD_DS=0");
    }
    mhsa_case(ATTN_FWD, 0, 196, 12, 32, ""); mhsa_case(ATTN_BWD, 64, 0, 12, 32, ""); mhsa_case(ATTN_FWD, 64, 196, 12, 40, ""); mhsa_case(ATTN_BWD, 64, 300, 12, 40, "");
    for (const int hd : {32, 48, 64, 40})
        for (const int N : {1, 196, 14272, 14336, 14337}) class_attn_case(128, N, 12, hd);          // (the scores of 14336 keys + 8 KB are 64 KB)
    // ---- outlook: (28, 66) has w = 33 and leaves the persistent kernels
    const int HW[][2] = {{2, 2}, {7, 5}, {14, 14}, {28, 28}, {56, 56}, {28, 66}};
    const char* const olk_envs[] = {"", "AP_OUTLOOK_P=0", "AP_OUTLOOK_P=2", "AP_OUTLOOK_P=0 AP_OUTLOOK_MFMA=0", "AP_OUTLOOK_SR=1", "AP_OUTLOOK_SR=2", "AP_OUTLOOK_P=0 AP_OUTLOOK_SRW=2"};
    for (const char* env : olk_envs)
        for (const int dir : {ATTN_FWD, ATTN_BWD})
            for (const int heads : {1, 6})
                for (const auto& hw : HW) {
                    outlook_case(dir, 128, hw[0], hw[1], heads, env);
                    if (!*env) outlook_case(dir, 1, hw[0], hw[1], heads, env);
                }
    outlook_case(ATTN_FWD, 0, 28, 28, 6, ""); outlook_case(ATTN_BWD, 1, 2, 1000, 1, "AP_OUTLOOK_P=0");
    // ---- LayerNorm: C / 8 chunks on G lanes x V -- both sides of V = 1 | 2 (512 | 520), 2 | 4 (1024 | 1032 .. 1536), 2048 | 2056, 12: no whole chunks
    const int Cs[] = {8, 96, 192, 256, 384, 512, 520, 768, 1000, 1024, 1536, 2048, 2056, 12};
    for (const int C : Cs) {
        for (const int kind : {K_FWD, K_FWD_FP8, K_BWD, K_BWD_PARTIAL, K_BWD_POOL}) ln_case(kind, C, "");
        for (const char* env : {"AP_LN_FWD_LP=0", "AP_LN_FWD_RPG=4", "AP_LN_FWD_WIDE=1"}) ln_case(K_FWD, C, env);
        for (const char* env : {"AP_LN_BWD_PF=0", "AP_LN_BWD_PF=2", "AP_LN_BWD_PF=3", "AP_LN_BWD_GRID=8", "AP_LN_BWD_GRID=2000"})
            for (const int kind : {K_BWD, K_BWD_POOL}) ln_case(kind, C, env);
    }
    std::string out = "{\"switch_fields\": \"" SWITCH_FIELDS "\",\n\"switches\": " + object_of(switch_rows, ",\n ") + ",\n\"ln_rows\": \"0/1/300/25088/100352\",\n\"plans\": {\n";
    for (size_t i = 0; i < groups.size(); ++i) out += (i ? ",\n" : "") + ("\"" + groups[i].first + "\": " + object_of(groups[i].second, ", "));
    out += "\n}}\n";
    if (argc == 3 && !strcmp(argv[1], "--record")) {
        FILE* f = fopen(argv[2], "w");
        if (!f) { perror(argv[2]); return 1; }
        fputs(out.c_str(), f); fclose(f);
    } else fputs(out.c_str(), stdout);
    return 0;
}
