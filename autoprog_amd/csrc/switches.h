// The run-time switches of the library outside nt_plan.h (NtSwitches), read once per process and in one place.  Plain C++17, no HIP:
// ap_switches_from() takes the environment as a callable, so tests/host/attn_ln_plan_check.cpp parses a fake one on a CPU.  The library's
// copy is ap_switches() (common.h); no entry point reads the environment itself.  What each value selects: DESIGN.md §3 "Run-time switches".
#pragma once
#include <stdlib.h>

struct ApSwitches {
    int mhsa_flash, mhsa_fwd_p, mhsa_bwd_ds;                            // attn_plan.h: mhsa_plan
    int outlook_p, outlook_mfma, outlook_sr, outlook_srw;               // attn_plan.h: outlook_plan
    int ln_fwd_lp, ln_fwd_rpg, ln_fwd_wide, ln_bwd_pf, ln_bwd_grid, ln_bwd_grid_set;      // ln_plan.h
    int conv_grid, conv_waves, conv_wgrad_grid, conv_wgrad_p, conv128_grid, conv7_grid, conv7_wgrad_grid, conv_abl;
    int mlp_fused_v, gelu_table;
    int tn_8p, tn_group_blocks, tn_blocks, tn_place;                    // gemm.hip: the weight-gradient launches
};

// env: name -> value or null (getenv)
template <class Env> static inline ApSwitches ap_switches_from(Env env) {
    const auto num = [&](const char* name, int dflt) { const char* e = env(name); return e ? atoi(e) : dflt; };
    const auto is = [&](const char* name, char c) { const char* e = env(name); return e && e[0] == c; };
    const auto cap = [&](const char* name, int dflt) { const int v = num(name, dflt); return v < 1 ? dflt : v; };     // a grid cap: < 1 is the default
    ApSwitches s = {};
    s.mhsa_flash = is("AP_MHSA_FLASH", '1');            // 1: the blocked kernels of mhsa_flash.hip at every shape; anything else: mhsa_flash()
    s.mhsa_fwd_p = num("AP_MHSA_FWD_P", 1);             // 0: one workgroup per (image, head), never the persistent forward
    s.mhsa_bwd_ds = num("AP_MHSA_BWD_DS", 1);           // 0: the two-pass backward
    s.outlook_p = num("AP_OUTLOOK_P", 1);               // 1: persistent, 512 threads (256 where the tables do not fit); 2: 256 threads; 0: one item per workgroup
    s.outlook_mfma = num("AP_OUTLOOK_MFMA", 1);         // 0: the scalar gather kernel (with AP_OUTLOOK_P=0)
    s.outlook_sr = num("AP_OUTLOOK_SR", 0);             // > 0: the strip height every outlook kernel but dlogits starts its search from
    s.outlook_srw = num("AP_OUTLOOK_SRW", 0);           // > 0: the same for k_outlook_dlogits
    s.ln_fwd_lp = num("AP_LN_FWD_LP", 1);               // 0: never the low-register forward
    s.ln_fwd_rpg = num("AP_LN_FWD_RPG", 1); if (s.ln_fwd_rpg < 1) s.ln_fwd_rpg = 1;       // rows per lane group and workgroup
    s.ln_fwd_wide = num("AP_LN_FWD_WIDE", 0);           // 1: the backward's wide lane groups in the forward
    s.ln_bwd_pf = num("AP_LN_BWD_PF", 1);               // 0: trip by trip; 1: pipelined; 2: pipelined, twice the rows per trip; 3: 1 at four workgroups per SIMD
    s.ln_bwd_grid = num("AP_LN_BWD_GRID", 768); if (s.ln_bwd_grid < 1 || s.ln_bwd_grid > 1024) s.ln_bwd_grid = 768;
    s.ln_bwd_grid_set = env("AP_LN_BWD_GRID") != nullptr;              // set at all, even to a value out of range: no 512 cap at V >= 2
    s.conv_grid = cap("AP_CONV_GRID", 256);
    s.conv_waves = num("AP_CONV_WAVES", 8) == 4 ? 4 : 8;
    s.conv_wgrad_grid = cap("AP_CONV_WGRAD_GRID", 512);
    s.conv_wgrad_p = num("AP_CONV_WGRAD_P", 1);
    s.conv128_grid = num("AP_CONV128_GRID", 0);         // < 1: not forced, one workgroup per CU
    s.conv7_grid = cap("AP_CONV7_GRID", 512);
    s.conv7_wgrad_grid = cap("AP_CONV7_WGRAD_GRID", 512);
    s.conv_abl = num("AP_CONV_ABL", 0);                 // ablation bits, builds with -DAP_EXPERIMENTS=1 only
    s.mlp_fused_v = is("AP_MLP_FUSED_V", '1') ? 1 : 2;  // 1: the one-wave-per-SIMD kernel; 2: producer / consumer waves
    s.gelu_table = !is("AP_GELU_TABLE", '0');
    s.tn_8p = num("AP_GEMM_TN_8P", 1);
    s.tn_group_blocks = num("AP_GEMM_TN_GROUP_BLOCKS", 0);
    s.tn_blocks = num("AP_GEMM_TN_BLOCKS", 384);        // measured optimum: atomics vs parallelism
    s.tn_place = num("AP_GEMM_TN_PLACE", 1);
    return s;
}
