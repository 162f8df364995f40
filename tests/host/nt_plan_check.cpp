// Plans a fixed list of NT launches with csrc/nt_plan.h on the CPU, the way gemm.hip's nt_launch does, at 256, 304 and 64 CUs, and prints
// the plans as JSON (tests/test_nt_plan_host.py compares with tests/golden/nt_plans.json); `--record FILE` writes that document to FILE
// instead.  Beside the print, every plan is checked against the invariants listed at check_plan.  The switches come from strings, through
// the same nt_switches_from that reads the environment in the library; the GELU table is a counting callable.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include "../../autoprog_amd/csrc/nt_plan.h"

#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, "nt_plan_check: %s: ", current.c_str()); fprintf(stderr, __VA_ARGS__); \
                                               fprintf(stderr, " [%s]\n", #cond); exit(1); } } while (0)
static std::string current;

// "bias gelu=3 preact res=384": the facts of an epilogue.  gelu=4 arrives as the entry point hands it on (gelu 3, noside, no preact); q8 comes
// with its scale (q8noscale: without); res without a number: ldr = N
static NtEpi epi_of(const std::string& spec, int N) {
    NtEpi e = {};
    std::istringstream in(spec);
    for (std::string t; in >> t;) {
        if (t == "bias") e.bias = true;
        else if (t == "preact") e.preact = true;
        else if (t == "dgelu") e.dgelu_of = true;
        else if (t == "mul") e.mul_by = true;
        else if (t == "mul8") e.mul8 = true;
        else if (t == "rs") e.row_scale = true;
        else if (t == "q8") e.q8 = e.q8_scale = true;
        else if (t == "q8noscale") e.q8 = true;
        else if (t.rfind("res", 0) == 0) { e.residual = true; e.ldr = t.size() > 4 ? atoi(t.c_str() + 4) : N; }
        else if (t == "gelu=4") { e.gelu = 3; e.noside = 1; }
        else if (t.rfind("gelu=", 0) == 0) e.gelu = atoi(t.c_str() + 5);
        else { fprintf(stderr, "nt_plan_check: unknown epilogue token %s\n", t.c_str()); exit(1); }
    }
    return e;
}
// "AP_GEMM_8P=0 AP_GEMM_NT_RULE=1152,384,2,0" -> the switches
static NtSwitches switches_of(const std::string& spec) {
    std::map<std::string, std::string> env;
    std::istringstream in(spec);
    for (std::string t; in >> t;) env[t.substr(0, t.find('='))] = t.substr(t.find('=') + 1);
    return nt_switches_from([&](const char* name) { const auto it = env.find(name); return it == env.end() ? nullptr : it->second.c_str(); });
}

// dimensions as the entry point takes them (K, lda, ldb in bytes for fp8); lda = ldb = K and ldc = N rounded up to 8 where 0
struct Case { const char* name; int M, N, K; const char* epi; const char* env; bool fp8, table; int ldc, lda; };
static const Case cases[] = {
    // ---- the 8-phase kernel: 224-row tiles, the width rule (r192 * 10 against r256 * 13), its thresholds
    {"25088x384x384 plain", 25088, 384, 384, "", ""},
    {"25088x384x384 bias", 25088, 384, 384, "bias", ""},
    {"25088x384x384 bias rs res", 25088, 384, 384, "bias rs res", ""},
    {"25088x384x384 plain, AP_GEMM_BM224=0", 25088, 384, 384, "", "AP_GEMM_BM224=0"},
    {"25088x1152x384 plain", 25088, 1152, 384, "", ""},
    {"8192x1152x384 plain", 8192, 1152, 384, "", ""},
    {"18432x1152x384 plain", 18432, 1152, 384, "", ""},
    {"12800x1152x384 plain", 12800, 1152, 384, "", ""},
    {"50176x768x768 plain", 50176, 768, 768, "", ""},
    {"48608x768x768 plain", 48608, 768, 768, "", ""},
    {"25088x1536x384 bias gelu=3 preact", 25088, 1536, 384, "bias gelu=3 preact", "", false, true},
    {"25088x1536x384 bias gelu=3 preact, no table", 25088, 1536, 384, "bias gelu=3 preact", "", false, false},
    {"25088x1536x384 bias gelu=2 preact", 25088, 1536, 384, "bias gelu=2 preact", "", false, true},
    {"25088x384x1536 dgelu", 25088, 384, 1536, "dgelu", ""},
    {"25088x384x1536 dgelu, AP_GEMM_8P=2", 25088, 384, 1536, "dgelu", "AP_GEMM_8P=2"},
    {"25088x384x1536 mul8 res", 25088, 384, 1536, "mul8 res", ""},
    {"25088x1152x384 plain, AP_GEMM_8P=0", 25088, 1152, 384, "", "AP_GEMM_8P=0"},
    {"4095x384x384 plain", 4095, 384, 384, "", ""},
    {"4096x384x384 plain", 4096, 384, 384, "", ""},
    {"8192x384x64 plain", 8192, 384, 64, "", ""},
    {"8192x384x128 plain", 8192, 384, 128, "", ""},
    {"8192x384x200 plain", 8192, 384, 200, "", ""},
    {"8192x184x256 plain", 8192, 184, 256, "", ""},
    {"8192x192x256 plain", 8192, 192, 256, "", ""},
    {"8192x1016x384 plain", 8192, 1016, 384, "", ""},
    {"8192x1024x384 plain", 8192, 1024, 384, "", ""},
    {"8192x1030x384 plain", 8192, 1030, 384, "", ""},
    {"8192x1032x384 plain", 8192, 1032, 384, "", ""},
    {"8192x384x384 bias res=388", 8192, 384, 384, "bias res=388", ""},
    // ---- skinny
    {"128x384x1000 plain", 128, 384, 1000, "", ""},
    {"128x384x1000 bias gelu=4", 128, 384, 1000, "bias gelu=4", "", false, true},
    {"128x384x1000 plain, AP_GEMM_NT_NO_SKINNY=1", 128, 384, 1000, "", "AP_GEMM_NT_NO_SKINNY=1"},
    {"256x384x384 plain", 256, 384, 384, "", ""},
    {"257x384x384 plain", 257, 384, 384, "", ""},
    // ---- weight-stationary
    {"100352x576x192 bias gelu=3 preact", 100352, 576, 192, "bias gelu=3 preact", "", false, true},
    {"100352x576x192 bias gelu=3 preact, no table", 100352, 576, 192, "bias gelu=3 preact", "", false, false},
    {"100352x576x192 bias gelu=3 preact, AP_GEMM_WS=0", 100352, 576, 192, "bias gelu=3 preact", "AP_GEMM_WS=0", false, true},
    {"100352x576x192 bias gelu=4", 100352, 576, 192, "bias gelu=4", "", false, true},
    {"100352x192x192 mul8", 100352, 192, 192, "mul8", ""},
    {"100352x192x192 mul8 rs", 100352, 192, 192, "mul8 rs", ""},
    {"100352x1728x192 mul8 (nine slices)", 100352, 1728, 192, "mul8", ""},
    {"100352x1728x192 bias gelu=4 (nine slices)", 100352, 1728, 192, "bias gelu=4", "", false, true},
    {"16320x576x192 mul8", 16320, 576, 192, "mul8", ""},
    {"16383x576x192 mul8", 16383, 576, 192, "mul8", ""},
    {"16384x576x192 mul8", 16384, 576, 192, "mul8", ""},
    {"16384x576x192 mul8, ldc 584", 16384, 576, 192, "mul8", "", false, false, 584},
    // ---- the k_gemm_nt tiles
    {"300x384x384 plain", 300, 384, 384, "", ""},
    {"300x384x384 plain, AP_GEMM_LDS_EPI=0", 300, 384, 384, "", "AP_GEMM_LDS_EPI=0"},
    {"3136x576x384 plain", 3136, 576, 384, "", ""},
    {"3136x576x384 plain, AP_GEMM_LDS_EPI=1", 3136, 576, 384, "", "AP_GEMM_LDS_EPI=1"},
    {"3136x576x384 bias gelu=3 preact", 3136, 576, 384, "bias gelu=3 preact", "", false, true},
    {"25088x486x192 plain", 25088, 486, 192, "", ""},
    {"3000x512x256 plain", 3000, 512, 256, "", ""},
    {"3000x576x256 plain", 3000, 576, 256, "", ""},
    {"3000x384x384 bias res", 3000, 384, 384, "bias res", ""},
    {"3000x384x384 bias res, AP_GEMM_DBG=2", 3000, 384, 384, "bias res", "AP_GEMM_DBG=2"},
    {"3000x384x384 dgelu res", 3000, 384, 384, "dgelu res", ""},
    {"3000x384x1536 mul", 3000, 384, 1536, "mul", ""},
    {"25088x1152x384 plain, AP_GEMM_NT_192=1", 25088, 1152, 384, "", "AP_GEMM_NT_192=1"},
    {"25088x1152x384 plain, AP_GEMM_NT_TILE=5", 25088, 1152, 384, "", "AP_GEMM_NT_TILE=5"},
    {"25088x1152x384 plain, AP_GEMM_NT_TILE=20", 25088, 1152, 384, "", "AP_GEMM_NT_TILE=20"},
    {"25088x1152x200 plain, AP_GEMM_NT_TILE=20", 25088, 1152, 200, "", "AP_GEMM_NT_TILE=20"},
    {"25088x1152x384 plain, rule 1152,384,2,0", 25088, 1152, 384, "", "AP_GEMM_NT_RULE=1152,384,2,0"},
    {"25088x1152x384 plain, rules 384,384,4;1152,384,11,1", 25088, 1152, 384, "", "AP_GEMM_NT_RULE=384,384,4;1152,384,11,1"},
    {"25088x1152x384 plain, rule and AP_GEMM_NT_TILE=3", 25088, 1152, 384, "", "AP_GEMM_NT_RULE=1152,384,2,0 AP_GEMM_NT_TILE=3"},
    // ---- q8 of a bf16 launch and gelu = 4: accepted by the 8-phase kernel (and WS, above), refused everywhere else
    {"25088x1152x384 mul8 q8", 25088, 1152, 384, "mul8 q8", ""},
    {"25088x1152x384 mul8 rs q8", 25088, 1152, 384, "mul8 rs q8", ""},
    {"25088x1152x384 mul8 q8, AP_GEMM_NT_TILE=1", 25088, 1152, 384, "mul8 q8", "AP_GEMM_NT_TILE=1"},
    {"25088x1152x384 mul8 q8, rule 1152,384,2,0", 25088, 1152, 384, "mul8 q8", "AP_GEMM_NT_RULE=1152,384,2,0"},
    {"25088x1152x384 mul8 q8, AP_GEMM_NT_192=1", 25088, 1152, 384, "mul8 q8", "AP_GEMM_NT_192=1"},
    {"25088x1152x384 mul8 q8, AP_GEMM_8P=0", 25088, 1152, 384, "mul8 q8", "AP_GEMM_8P=0"},
    {"3000x1152x384 mul8 q8, AP_GEMM_NT_TILE=20", 3000, 1152, 384, "mul8 q8", "AP_GEMM_NT_TILE=20"},
    {"128x1152x384 mul8 q8", 128, 1152, 384, "mul8 q8", ""},
    {"25088x1152x384 mul8 bias q8", 25088, 1152, 384, "mul8 bias q8", ""},
    {"25088x1152x384 mul8 q8noscale", 25088, 1152, 384, "mul8 q8noscale", ""},
    {"4096x192x128 mul8 q8", 4096, 192, 128, "mul8 q8", ""},
    {"4095x192x128 mul8 q8", 4095, 192, 128, "mul8 q8", ""},
    {"4096x200x128 mul8 q8", 4096, 200, 128, "mul8 q8", ""},
    {"4096x192x128 mul8 q8, ldc 200", 4096, 192, 128, "mul8 q8", "", false, false, 200},
    {"4096x192x64 mul8 q8", 4096, 192, 64, "mul8 q8", ""},
    {"25088x1536x384 bias gelu=4", 25088, 1536, 384, "bias gelu=4", "", false, true},
    {"25088x1536x384 bias gelu=4, no table", 25088, 1536, 384, "bias gelu=4", "", false, false},
    {"25088x1536x384 bias gelu=4, AP_GEMM_NT_TILE=1", 25088, 1536, 384, "bias gelu=4", "AP_GEMM_NT_TILE=1", false, true},
    {"25088x1536x384 gelu=4 without bias", 25088, 1536, 384, "gelu=4", "", false, true},
    {"3000x1536x384 bias gelu=4", 3000, 1536, 384, "bias gelu=4", "", false, true},
    // ---- fp8 (K in bytes)
    {"fp8 25088x1152x384", 25088, 1152, 384, "", "", true},
    {"fp8 25088x1152x320", 25088, 1152, 320, "", "", true},
    {"fp8 25088x1152x320 bias gelu=1 q8", 25088, 1152, 320, "bias gelu=1 q8", "", true},
    {"fp8 25088x1536x384 bias gelu=3 preact q8", 25088, 1536, 384, "bias gelu=3 preact q8", "", true, true},
    {"fp8 25088x1536x384 bias gelu=3 preact q8, no table", 25088, 1536, 384, "bias gelu=3 preact q8", "", true, false},
    {"fp8 25088x1536x320 bias gelu=3 preact", 25088, 1536, 320, "bias gelu=3 preact", "", true, true},
    {"fp8 25088x384x384 bias res", 25088, 384, 384, "bias res", "", true},
    {"fp8 25088x1152x384 dgelu", 25088, 1152, 384, "dgelu", "", true},
    {"fp8 25088x1152x384, AP_GEMM_8P=0", 25088, 1152, 384, "", "AP_GEMM_8P=0", true},
    {"fp8 4096x192x256 bias gelu=1 q8", 4096, 192, 256, "bias gelu=1 q8", "", true},
    {"fp8 4096x192x128 bias gelu=1 q8", 4096, 192, 128, "bias gelu=1 q8", "", true},
    {"fp8 128x384x1024", 128, 384, 1024, "", "", true},
    // ---- refused shapes
    {"300x384x388 (K % 8)", 300, 384, 388, "", ""},
    {"300x384x384, ldc 380", 300, 384, 384, "", "", false, false, 380},
    {"300x384x384, lda 380", 300, 384, 384, "", "", false, false, 0, 380},
    {"300x384x384 bias res=380", 300, 384, 384, "bias res=380", ""},
    {"300x384x384 mul dgelu", 300, 384, 384, "mul dgelu", ""},
    {"300x384x384 bias gelu=2 (no preact)", 300, 384, 384, "bias gelu=2", ""},
    {"300x384x384 bias gelu=5", 300, 384, 384, "bias gelu=5 preact", ""},
    {"2147483400x384x384 (beyond AP_MAX_ROWS)", 2147483400, 384, 384, "", ""},
    {"fp8 300x384x392 (K % 16)", 300, 384, 392, "", "", true},
    {"fp8 25088x1152x384 bias q8 (no gelu)", 25088, 1152, 384, "bias q8", "", true},
};

static const char* family_name(int f) {
    static const char* names[] = {"skinny", "ws", "8p", "tile", "fp8_tile"};
    return names[f];
}

// grid > 0; an 8-phase grid is a multiple of 8 and at most ncu & ~7; ntiles = ceil(M / bm) * ceil(N / bn) where the kernel walks tiles; a plan
// with q8 or noside is an 8-phase plan or a WS plan with epi 2; WS: n_slices * per_xcd <= ncu / 8; the table is asked for gelu = 3 only
static void check_plan(const Case& c, const NtEpi& e, int ncu, const NtPlan& p, int asks) {
    REQUIRE(e.gelu == 3 || asks == 0, "%d asks at gelu %d", asks, e.gelu);
    REQUIRE(p.status == AP_OK || p.status == AP_ERR_SHAPE || p.status == AP_ERR_UNSUPPORTED, "status %d", p.status);
    if (p.status != AP_OK) return;
    REQUIRE(p.family >= NT_SKINNY && p.family <= NT_FP8_TILE && p.grid > 0, "family %d grid %d", p.family, p.grid);
    REQUIRE(!p.tab || asks > 0, "a table pointer nobody asked for");
    if (p.family == NT_8P) REQUIRE(p.grid % 8 == 0 && p.grid <= (ncu & ~7) && (p.bm == 256 || p.bm == 224) && (p.bn == 192 || p.bn == 256), "grid %d tile %d x %d", p.grid, p.bm, p.bn);
    if (p.family == NT_8P || p.family == NT_TILE || p.family == NT_FP8_TILE)
        REQUIRE(p.tiles_n == nt_ceil(c.N, p.bn) && p.ntiles == nt_ceil(c.M, p.bm) * p.tiles_n, "%d tiles, %d across, of %d x %d", p.ntiles, p.tiles_n, p.bm, p.bn);
    if (p.family == NT_TILE || p.family == NT_FP8_TILE) REQUIRE(p.grid == p.ntiles, "grid %d for %d tiles", p.grid, p.ntiles);
    if (e.q8 || e.noside) REQUIRE(p.family == NT_8P || (p.family == NT_WS && p.ws_epi == 2 && !e.q8), "family %d cannot emit it", p.family);
    if (p.family == NT_WS) REQUIRE(p.n_slices > 0 && p.per_xcd > 0 && p.n_slices * p.per_xcd <= ncu / 8 && p.n_slices * WS_BN == c.N && p.n_items * WS_BM == c.M,
                                   "%d slices x %d per XCD, %d items", p.n_slices, p.per_xcd, p.n_items);
}

// what AP_GEMM_NT_RULE strings parse to
static void check_rules() {
    current = "rule strings";
    NtSwitches s = switches_of("AP_GEMM_NT_RULE=384,384,4;1152,384,11,1");
    REQUIRE(s.nrules == 2 && s.rules[0].n == 384 && s.rules[0].variant == 4 && s.rules[0].lds_epi == -1 && s.rules[1].k == 384 && s.rules[1].variant == 11 && s.rules[1].lds_epi == 1, "two rules");
    REQUIRE(switches_of("AP_GEMM_NT_RULE=1152,384").nrules == 0 && switches_of("").nrules == 0 && switches_of("AP_GEMM_NT_RULE=x").nrules == 0, "no rule");
    std::string many = "AP_GEMM_NT_RULE=";
    for (int i = 0; i < 20; ++i) many += std::to_string(8 * i + 8) + ",64,1;";
    s = switches_of(many);
    REQUIRE(s.nrules == 16 && s.rules[15].n == 128, "at most 16 rules");
    s = switches_of("");
    REQUIRE(s.mode8p == 1 && s.bm224 == 1 && s.ws == 1 && s.skinny == 1 && s.tile == 0 && s.allow192 == 0 && s.lds_epi == -1 && s.dbg == 0, "defaults");
}

int main(int argc, char** argv) {
    check_rules();
    std::string out = "[\n";
    char buf[1024];
    bool first = true;
    for (const Case& c : cases) {
        const NtEpi e = epi_of(c.epi, c.N);
        const NtSwitches s = switches_of(c.env);
        for (const int ncu : {256, 304, 64}) {
            current = std::string(c.name) + " @" + std::to_string(ncu);
            int asks = 0;
            const int lda = c.lda ? c.lda : c.K, ldc = c.ldc ? c.ldc : (c.N + 7) & ~7;
            const NtPlan p = nt_plan(c.M, c.N, c.K, lda, c.K, ldc, e, c.fp8, ncu, s, [&] { ++asks; return c.table; });
            check_plan(c, e, ncu, p, asks);
            snprintf(buf, sizeof buf, "%s{\"case\": \"%s\", \"cus\": %d, \"status\": %d, \"family\": \"%s\", \"variant\": %d, \"bm\": %d, \"bn\": %d, \"ntiles\": %d, "
                     "\"tiles_n\": %d, \"grid\": %d, \"grid_y\": %d, \"lds_bytes\": %d, \"lds_epi\": %d, \"prefetch\": %d, \"flavour\": %d, \"tab\": %d, \"ws_epi\": %d, "
                     "\"n_slices\": %d, \"n_items\": %d, \"per_xcd\": %d, \"asks\": %d}", first ? "" : ",\n", c.name, ncu, p.status,
                     p.status == AP_OK ? family_name(p.family) : "none", p.variant, p.bm, p.bn, p.ntiles, p.tiles_n, p.grid, p.grid_y, p.lds_bytes, p.lds_epi, p.prefetch,
                     p.flavour, p.tab, p.ws_epi, p.n_slices, p.n_items, p.per_xcd, asks);
            out += buf; first = false;
        }
    }
    out += "\n]\n";
    if (argc == 3 && !strcmp(argv[1], "--record")) {
        FILE* f = fopen(argv[2], "w");
        if (!f) { perror(argv[2]); return 1; }
        fputs(out.c_str(), f); fclose(f);
    } else fputs(out.c_str(), stdout);
    return 0;
}
