// Plans a fixed list of weight-gradient launches with csrc/tn_plan.h on the CPU, the way gemm.hip's entry points do, and prints them as
// JSON (tests/test_tn_plan_host.py compares with tests/golden/tn_plans.json); `--record FILE` writes that document to FILE instead.
// Beside the print, every placement table and every token cut is checked against the invariants listed at check_table / check_cut.
// Pointers are made-up addresses: planning never reads through them.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../autoprog_amd/csrc/tn_plan.h"

static std::string out;
static void put(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
static void put(const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    out += buf;
}
#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, "tn_plan_check: %s: ", current.c_str()); fprintf(stderr, __VA_ARGS__); \
                                               fprintf(stderr, " [%s]\n", #cond); exit(1); } } while (0)
static std::string current;

static uintptr_t next_addr = 0x100000;
template <class T> static T* fake() { next_addr += 0x10000; return reinterpret_cast<T*>(next_addr); }

static unsigned long long fnv1a(const unsigned short* e, int n) {
    unsigned long long h = 0xcbf29ce484222325ull;
    for (int i = 0; i < n; ++i)
        for (int b = 0; b < 2; ++b) { h ^= (e[i] >> (8 * b)) & 0xFFu; h *= 0x100000001b3ull; }
    return h;
}

// every (problem, split, tile) exactly once, everything else idle, at most `cap` entries per XCD column, blocks = 8 * (largest column),
// and -- where a group may not be cut -- all tiles of one (problem, split) in one column
static void check_table(const unsigned short* e, int table_len, int shift, int blocks, int cap, const TnTiles* pl, int count, bool may_cut) {
    REQUIRE(blocks >= 0 && blocks <= table_len && blocks % 8 == 0, "blocks %d", blocks);
    std::vector<std::vector<int>> column(count);
    int load[8] = {0, 0, 0, 0, 0, 0, 0, 0}, total = 0, placed = 0;
    for (int i = 0; i < count; ++i) { column[i].assign((size_t)pl[i].tiles * pl[i].splits, -1); total += pl[i].tiles * pl[i].splits; }
    for (int b = 0; b < table_len; ++b) {
        if (e[b] == TN_MAP_IDLE) continue;
        REQUIRE(b < blocks, "entry %d beyond the launch of %d", b, blocks);
        const int p = e[b] >> shift, idx = e[b] & ((1 << shift) - 1);
        REQUIRE(p < count && idx < (int)column[p].size(), "entry %d names problem %d item %d", b, p, idx);
        REQUIRE(column[p][idx] < 0, "problem %d item %d placed twice", p, idx);
        column[p][idx] = b % 8; ++load[b % 8]; ++placed;
    }
    REQUIRE(placed == total, "%d of %d items placed", placed, total);
    int mx = 0;
    for (int x = 0; x < 8; ++x) { REQUIRE(load[x] <= cap, "XCD %d holds %d > %d", x, load[x], cap); if (load[x] > mx) mx = load[x]; }
    REQUIRE(blocks == 8 * mx, "blocks %d, largest column %d", blocks, mx);
    if (!may_cut)
        for (int i = 0; i < count; ++i)
            for (int k = 0; k < (int)column[i].size(); ++k)
                REQUIRE(column[i][k] == column[i][k / pl[i].tiles * pl[i].tiles], "problem %d split %d lies on two XCDs", i, k / pl[i].tiles);
}
// no token range is empty and none is missing
static void check_cut(int steps, int sps, int splits) {
    REQUIRE(sps > 0 && splits > 0 && (long long)(splits - 1) * sps < steps && steps <= (long long)splits * sps, "steps %d sps %d splits %d", steps, sps, splits);
}

static void put_ints(const char* key, const std::vector<long long>& v) {
    put("\"%s\": [", key);
    for (size_t i = 0; i < v.size(); ++i) put("%s%lld", i ? ", " : "", v[i]);
    put("]");
}
struct Row { int sps, splits, tiles, start, shared_out; };
static void put_rows(const std::vector<Row>& rows) {
    put("\"problems\": [");
    for (size_t i = 0; i < rows.size(); ++i)
        put("%s{\"sps\": %d, \"splits\": %d, \"tiles\": %d, \"start\": %d, \"shared_out\": %d}", i ? ", " : "", rows[i].sps, rows[i].splits, rows[i].tiles,
            rows[i].start, rows[i].shared_out);
    put("]");
}
static void put_8p(const char* kernel, const T8Plan& p8, int count, const std::vector<long long>& which, int lblocks, int n_cu, const std::vector<int>& ksteps) {
    check_table(p8.map.e, T8_MAP_MAX, T8_MAP_SHIFT, p8.blocks, n_cu / 8, p8.pl, count, true);
    std::vector<Row> rows;
    long long items = 0;
    for (int i = 0; i < count; ++i) {
        check_cut(ksteps[i], p8.ksps, p8.pl[i].splits);
        items += (long long)p8.pl[i].tiles * p8.pl[i].splits;
        rows.push_back(Row{p8.ksps, p8.pl[i].splits, p8.pl[i].tiles, -1, p8.shared_out[i]});
    }
    REQUIRE(items <= n_cu, "%lld items on %d CUs", items, n_cu);
    put("{\"kernel\": \"%s\", ", kernel); put_ints("which", which);
    put(", \"riders\": 1, \"grid\": %d, \"table_blocks\": %d, \"digest\": \"%016llx\", ", p8.blocks + lblocks, p8.blocks, fnv1a(p8.map.e, p8.blocks));
    put_rows(rows); put("}");
}

static void begin_case(const std::string& name, int n_cu) {
    current = name + "@" + std::to_string(n_cu);
    put("%s  {\"case\": \"%s\", \"cus\": %d, ", out.size() > 2 ? ",\n" : "", name.c_str(), n_cu);
}

struct Switches { int enabled8 = 1, place = 1, capacity = 0; };      // AP_GEMM_TN_8P, AP_GEMM_TN_PLACE, AP_GEMM_TN_GROUP_BLOCKS (0: two per CU)

// ap_gemm_tn_acc_grouped_ln
static void plan_bf16(const std::string& name, int n_cu, const ap_tn_problem* problems, int count, const std::vector<ap_ln_reduce>& riders, int ln_count,
                      bool deterministic, Switches sw = Switches()) {
    begin_case(name, n_cu);
    const int capacity = sw.capacity > 0 ? sw.capacity : 2 * n_cu;
    TnLn ln; int lblocks = 0;
    int rc = tn_ln_table(riders.empty() ? nullptr : riders.data(), ln_count, ln, lblocks);
    if (rc == AP_OK) rc = tn_validate(problems, count, AP_TN_MAX_GROUP);
    if (rc != AP_OK) { put("\"rc\": %d, \"launches\": []}", rc); return; }
    static TnDispatch d;
    tn_dispatch(problems, count, deterministic, n_cu, sw.enabled8, d);
    std::string launches;
    std::vector<bool> seen(count, false);
    std::swap(out, launches);
    for (int k = 0; k < d.n && rc == AP_OK; ++k) {
        const TnLaunch& L = d.l[k];
        std::vector<long long> which;
        std::vector<ap_tn_problem> sub;
        for (int i = 0; i < L.count; ++i) {
            const int pi = d.order[L.first + i];
            REQUIRE(pi >= 0 && pi < count && !seen[pi], "launch %d takes problem %d", k, pi);
            seen[pi] = true; which.push_back(pi); sub.push_back(problems[pi]);
        }
        REQUIRE(L.riders == (k == 0), "launch %d riders %d", k, L.riders);
        if (L.kernel == TN_KERNEL_8P) {
            std::vector<int> ksteps;
            for (const ap_tn_problem& q : sub) ksteps.push_back(q.M / 64);
            put("%s", k ? ", " : ""); put_8p("8p", d.p8, L.count, which, lblocks, n_cu, ksteps);
            continue;
        }
        static TnGroupPlan gp;
        rc = tn128_plan(sub.data(), L.count, capacity, gp);
        if (rc != AP_OK) break;
        bool any_patch = false;
        for (const ap_tn_problem& q : sub) any_patch = any_patch || q.b_patch;
        TnMap map; int mblocks = 0;
        const bool placed = !any_patch && sw.place && tn128_place(gp, 2 * n_cu / 8, map, mblocks);
        std::vector<Row> rows; std::vector<long long> offs;
        TnTiles pl[TN_MAX_GROUP];
        int start = 0;
        for (int i = 0; i < L.count; ++i) {
            const TnItemPlan& p = gp.p[i];
            check_cut(p.steps, p.sps, p.splits);
            REQUIRE(p.steps == (sub[i].M + 63) / 64 && p.start == start, "problem %d steps %d start %d", i, p.steps, p.start);
            pl[i] = TnTiles{p.t1 * p.t2, p.splits}; start += p.t1 * p.t2 * p.splits;
            rows.push_back(Row{p.sps, p.splits, p.t1 * p.t2, p.start, p.shared_out}); offs.push_back((long long)gp.slab_off[i]);
        }
        REQUIRE(start == gp.blocks, "blocks %d", gp.blocks);
        if (placed) check_table(map.e, TN_MAP_MAX, TN_MAP_SHIFT, mblocks, 2 * n_cu / 8, pl, L.count, false);
        put("%s{\"kernel\": \"%s\", ", k ? ", " : "", placed ? "128map" : any_patch ? "128patch" : "128"); put_ints("which", which);
        // (without a table the riders get a launch of their own)
        put(", \"riders\": %d, \"grid\": %d, ", L.riders, placed ? mblocks + (L.riders ? lblocks : 0) : gp.blocks);
        if (placed) put("\"table_blocks\": %d, \"digest\": \"%016llx\", ", mblocks, fnv1a(map.e, mblocks));
        if (deterministic) { put("\"slab_floats\": %lld, ", (long long)gp.slab_floats); put_ints("slab_off", offs); put(", "); }
        put_rows(rows); put("}");
    }
    std::swap(out, launches);
    if (rc != AP_OK) launches.clear();
    else for (int i = 0; i < count; ++i) REQUIRE(seen[i], "problem %d is in no launch", i);
    put("\"rc\": %d, \"launches\": [", rc);
    out += launches + "]}";
}

// ap_gemm_tn8_acc_grouped_ln
static void plan_fp8(const std::string& name, int n_cu, const ap_tn8_problem* problems, int count, bool deterministic, Switches sw = Switches()) {
    begin_case(name, n_cu);
    TnLn ln; int lblocks = 0;
    int rc = tn_ln_table(nullptr, 0, ln, lblocks);
    static TnGroupPlan gp;
    if (rc == AP_OK) rc = tf_plan(problems, count, 2 * n_cu, gp);
    if (rc != AP_OK) { put("\"rc\": %d, \"launches\": []}", rc); return; }
    std::vector<long long> which;
    for (int i = 0; i < count; ++i) which.push_back(i);
    put("\"rc\": 0, \"launches\": [");
    static T8Plan p8;
    if (!deterministic && tf8_plan(problems, count, n_cu, sw.enabled8, p8)) {
        std::vector<int> ksteps;
        for (int i = 0; i < count; ++i) ksteps.push_back(problems[i].M / 128);
        put_8p("8p_fp8", p8, count, which, lblocks, n_cu, ksteps);
    } else {
        std::vector<Row> rows; std::vector<long long> offs;
        int start = 0;
        for (int i = 0; i < count; ++i) {
            const TnItemPlan& p = gp.p[i];
            check_cut(p.steps, p.sps, p.splits);
            REQUIRE(p.steps == (problems[i].M + 127) / 128 && p.start == start, "problem %d steps %d start %d", i, p.steps, p.start);
            start += p.t1 * p.t2 * p.splits;
            rows.push_back(Row{p.sps, p.splits, p.t1 * p.t2, p.start, p.shared_out}); offs.push_back((long long)gp.slab_off[i]);
        }
        REQUIRE(start == gp.blocks, "blocks %d", gp.blocks);
        put("{\"kernel\": \"fp8\", "); put_ints("which", which); put(", \"riders\": 1, \"grid\": %d, ", gp.blocks + lblocks);
        if (deterministic) { put("\"slab_floats\": %lld, ", (long long)gp.slab_floats); put_ints("slab_off", offs); put(", "); }
        put_rows(rows); put("}");
    }
    put("]}");
}

// ap_gemm_tn_acc
static void plan_single(const std::string& name, int n_cu, int M, int N1, int N2, int target_blocks) {
    begin_case(name, n_cu);
    const TnItemPlan p = tn_single_plan(M, N1, N2, target_blocks);
    check_cut(p.steps, p.sps, p.splits);
    put("\"rc\": 0, \"launches\": [{\"kernel\": \"single\", \"which\": [0], \"riders\": 0, \"grid\": %d, ", p.t1 * p.t2 * p.splits);
    put_rows({Row{p.sps, p.splits, p.t1 * p.t2, p.start, p.shared_out}}); put("}]}");
}

static ap_tn_problem bf16_problem(int M, int N1, int N2, bool colsum, int lda = 0, int ldb = 0) {
    ap_tn_problem q;
    memset(&q, 0, sizeof q);
    q.A = fake<ap_bf16>(); q.lda = lda ? lda : (N1 + 7) / 8 * 8;
    q.B = fake<ap_bf16>(); q.ldb = ldb ? ldb : (N2 + 7) / 8 * 8;
    q.C = fake<float>(); q.ldc = N2;
    q.M = M; q.N1 = N1; q.N2 = N2;
    q.colsum_A = colsum ? fake<float>() : nullptr;
    return q;
}
static ap_tn8_problem fp8_problem(int M, int N1, int N2, int a_fmt) {
    ap_tn8_problem q;
    memset(&q, 0, sizeof q);
    q.A = fake<unsigned char>(); q.lda = N1; q.B = fake<unsigned char>(); q.ldb = N2; q.C = fake<float>(); q.ldc = N2;
    q.M = M; q.N1 = N1; q.N2 = N2; q.a_fmt = a_fmt; q.dq_a = fake<float>(); q.dq_b = fake<float>();
    return q;
}
static std::vector<ap_ln_reduce> make_riders(int n, int c_even, int c_odd) {
    std::vector<ap_ln_reduce> r;
    for (int k = 0; k < n; ++k) r.push_back(ap_ln_reduce{fake<float>(), 8, k % 2 ? c_odd : c_even, fake<float>(), fake<float>()});
    return r;
}

int main(int argc, char** argv) {
    const char* record = argc == 3 && !strcmp(argv[1], "--record") ? argv[2] : nullptr;
    if (argc != 1 && !record) { fprintf(stderr, "usage: %s [--record FILE]\n", argv[0]); return 2; }
    const std::vector<ap_ln_reduce> none;
    out = "[\n";

    // one VOLO-D1 transformer block, six of them, one outlooker block
    std::vector<ap_tn_problem> block, six, outlooker;
    const int tb[4][2] = {{1152, 384}, {384, 384}, {1152, 384}, {384, 1152}}, ob[5][2] = {{192, 192}, {486, 192}, {192, 192}, {576, 192}, {192, 576}};
    for (int b = 0; b < 6; ++b)
        for (const auto& s : tb) {
            six.push_back(bf16_problem(25088, s[0], s[1], true));
            if (b == 0) block.push_back(six.back());
        }
    for (const auto& s : ob) outlooker.push_back(bf16_problem(100352, s[0], s[1], true));
    const std::vector<ap_ln_reduce> riders3 = make_riders(3, 192, 192), riders12 = make_riders(12, 192, 384), riders13 = make_riders(13, 192, 384);
    // the group of test_gemm_tn_8p_launch_of_many_blocks_is_unsplit_and_exact
    std::vector<ap_tn_problem> many;
    for (int i = 0; i < 24; ++i) many.push_back(bf16_problem(4096, i < 20 ? 384 : 768, i < 20 ? 576 : 384, i % 2 != 0, 768, 576));
    many.push_back(bf16_problem(4096, 384, 384, false, 768, 576));
    many.push_back(bf16_problem(4096, 384, 384, false, 768, 576));
    many.back().C = many[24].C;
    many.push_back(bf16_problem(4096, 486, 192, true, 768, 576));
    // the ragged shapes of test_gemm_tn_acc_grouped
    std::vector<ap_tn_problem> ragged;
    {
        const int s[10][4] = {{3136, 1152, 384, 1}, {3136, 384, 384, 1}, {3136, 1152, 384, 0}, {3136, 384, 1152, 1}, {1000, 486, 192, 1}, {77, 32, 96, 0},
                              {4000, 192, 192, 1}, {130, 1000, 384, 1}, {500, 16, 64, 1}, {2048, 576, 192, 0}};
        for (const auto& r : s) ragged.push_back(bf16_problem(r[0], r[1], r[2], r[3] != 0));
    }
    std::vector<ap_tn_problem> wide, wide72, nine;
    for (int i = 0; i < 8; ++i) wide.push_back(bf16_problem(12544, 3072, 768, false));
    for (int i = 0; i < 8; ++i) wide72.push_back(bf16_problem(12544, 1536, 768, false));       // 72 tiles each: one problem per XCD where an XCD holds 76
    for (int i = 0; i < 9; ++i) nine.push_back(bf16_problem(25088, 384, 384, true));
    std::vector<ap_tn8_problem> f128 = {fp8_problem(5000, 512, 1024, AP_FP8_E5M2), fp8_problem(5000, 1024, 512, AP_FP8_E5M2)};
    std::vector<ap_tn8_problem> f192 = {fp8_problem(12544, 768, 3072, AP_FP8_E5M2), fp8_problem(12544, 3072, 768, AP_FP8_E5M2),
                                        fp8_problem(12544, 768, 768, AP_FP8_E5M2), fp8_problem(12544, 768, 2304, AP_FP8_E5M2)};
    std::vector<ap_tn8_problem> fmixed = f192;
    fmixed[2].a_fmt = AP_FP8_E4M3;
    Switches off8; off8.enabled8 = 0;

    for (const int n_cu : {256, 304, 64}) {
        plan_bf16("1 transformer block", n_cu, block.data(), 4, none, 0, false);
        plan_bf16("2 six transformer blocks", n_cu, six.data(), 24, riders12, 12, false);
        plan_bf16("3 outlooker block with riders", n_cu, outlooker.data(), 5, riders3, 3, false);
        plan_bf16("4 many blocks, shared output, 486 wide, 12 riders", n_cu, many.data(), (int)many.size(), riders12, 12, false);
        plan_bf16("5 ten ragged shapes", n_cu, ragged.data(), 10, none, 0, false);
        plan_bf16("6 eight 3072x768, AP_GEMM_TN_8P=0", n_cu, wide.data(), 8, none, 0, false, off8);
        plan_bf16("6 eight 1536x768, AP_GEMM_TN_8P=0", n_cu, wide72.data(), 8, none, 0, false, off8);
        plan_bf16("7 eight 3072x768", n_cu, wide.data(), 8, none, 0, false);
        plan_single("8 single 25088 1152x384", n_cu, 25088, 1152, 384, 384);
        plan_single("8 single 200 384x384", n_cu, 200, 384, 384, 384);
        plan_bf16("9 deterministic transformer block", n_cu, block.data(), 4, none, 0, true);
        plan_bf16("9 deterministic nine problems", n_cu, nine.data(), 9, none, 0, true);
        plan_fp8("10 fp8 128-multiples, ragged tokens", n_cu, f128.data(), 2, false);
        plan_fp8("11 fp8 8-phase", n_cu, f192.data(), 4, false);
        plan_fp8("11 fp8 mixed formats", n_cu, fmixed.data(), 4, false);

        plan_bf16("12 null problems", n_cu, nullptr, 4, none, 0, false);
        plan_bf16("12 count 0", n_cu, block.data(), 0, none, 0, false);
        plan_bf16("12 count 33", n_cu, six.data(), 33, none, 0, false);
        std::vector<ap_tn_problem> bad = block;
        bad[1].A = nullptr;
        plan_bf16("12 null A", n_cu, bad.data(), 4, none, 0, false);
        bad = block; bad[2].lda = 1156;
        plan_bf16("12 lda not a multiple of 8", n_cu, bad.data(), 4, none, 0, false);
        bad = block; bad[3].ldc = 1151;
        plan_bf16("12 ldc < N2", n_cu, bad.data(), 4, none, 0, false);
        bad = block; bad[0].M = 0;
        plan_bf16("12 M = 0", n_cu, bad.data(), 4, none, 0, false);
        std::vector<ap_ln_reduce> r = riders3;
        r[1].C = 0;
        plan_bf16("12 rider with C = 0", n_cu, block.data(), 4, r, 3, false);
        r = riders3; r[2].dgamma = nullptr;
        plan_bf16("12 rider with null dgamma", n_cu, block.data(), 4, r, 3, false);
        plan_bf16("12 thirteen riders", n_cu, block.data(), 4, riders13, 13, false);
        std::vector<ap_tn8_problem> f200 = f128;
        f200[1].N1 = 200; f200[1].lda = 208;
        plan_fp8("12 fp8 width 200", n_cu, f200.data(), 2, false);
    }
    out += "\n]\n";
    if (record) {
        FILE* f = fopen(record, "w");
        if (!f || fputs(out.c_str(), f) < 0 || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", record); return 1; }
    } else fputs(out.c_str(), stdout);
    return 0;
}
