// Host-side planning of the attention and outlook launches (mhsa.hip, outlook.hip): which kernel takes a shape, with which instantiation,
// grid and LDS, and every refusal that depends on the shape.  Plain C++17, no HIP: the CU count and the run-time switches come in as
// arguments, so tests/host/attn_ln_plan_check.cpp plans on a CPU.  A plan is launchable as it stands or it carries an error code; the entry
// points check their pointers, plan, and turn the plan into one launch.  The constants that planner and kernels share: attn_const.h.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/autoprog_hip.h"
#include "attn_const.h"
#include "switches.h"

enum { ATTN_FWD = 0, ATTN_BWD = 1 };
static inline int attn_min(int a, int b) { return a < b ? a : b; }

// ---- multi-head self-attention
enum { MHSA_FLASH = 0, MHSA_FWD = 1, MHSA_FWD_P = 2, MHSA_BWD = 3, MHSA_BWD_DS = 4, MHSA_CLASS = 5 };
// nt: token tiles of 16 in the LDS image, the NT of k_mhsa_fwd<NT, HD> / k_mhsa_fwd_p<NT> and twice the NP of k_mhsa_bwd_ds<NP>.
// hdt: the HD template argument (32 or 64); k_class_attn_*<PARTS>: PARTS = hdt / 8.  lds_optin: what ap_allow_lds is asked for (0: nothing).
// MHSA_FLASH: grids and LDS are formed by mhsa_flash.hip; fp8: the launch writes the e4m3 side output; ws_bytes: the backward's workspace,
// filled for every valid (B, N, heads) whatever the head dim (the workspace query does not refuse one).
struct MhsaPlan { int status, family, nt, hdt, items, grid, block, lds_bytes, lds_optin, fp8; size_t ws_bytes; };

// N <= 256 with head_dim 32 / 64: one workgroup holds the whole head in LDS (mhsa.hip); anything else (448-px inputs, head_dim 48 of
// VOLO-D4/D5) goes to the key/query-blocked kernels of mhsa_flash.hip.  AP_MHSA_FLASH=1 forces the blocked path (parity tests run both on
// the same inputs).
static inline bool mhsa_flash(int N, int hd, const ApSwitches& sw) { return sw.mhsa_flash || N > 256 || hd == 48; }

static inline MhsaPlan mhsa_plan(int dir, int B, int N, int heads, int hd, int cus, const ApSwitches& sw, bool want_fp8) {
    MhsaPlan p = {};
    const auto fail = [&p](int rc) { p.status = rc; return p; };
    if (B <= 0 || N <= 0 || heads <= 0) return fail(AP_ERR_SHAPE);
    const bool flash = mhsa_flash(N, hd, sw);
    if (flash && dir == ATTN_BWD) p.ws_bytes = (size_t)B * heads * N * sizeof(float);          // delta = rowsum(dO * O) per (image, head, query)
    if (hd != 32 && hd != 48 && hd != 64) return fail(AP_ERR_UNSUPPORTED);
    if (want_fp8 && !flash) return fail(AP_ERR_UNSUPPORTED);            // the e4m3 side output exists in the blocked kernel only
    p.items = B * heads; p.hdt = hd == 32 ? 32 : 64; p.fp8 = want_fp8;
    if (flash) { p.family = MHSA_FLASH; return p; }
    p.nt = 2 * ((N + 31) / 32);
    const int ntile = (N + 15) / 16;
    if (dir == ATTN_FWD) {
        const int lds = 2 * p.nt * 16 * hd * 2;         // K and V (Q in the same rows), bf16
        const int p_cu = cus & ~7;                      // whole XCD groups (xcd_remap)
        // head_dim 32 and 7 .. 13 query tiles: the persistent kernel with loader waves (AP_MHSA_FWD_P=0: one workgroup per (image, head))
        if (hd == 32 && sw.mhsa_fwd_p && ntile >= 7 && ntile <= 16 - FP_LOADERS && p_cu >= 8) {
            p.family = MHSA_FWD_P; p.block = 1024; p.grid = attn_min(p.items, p_cu); p.lds_bytes = 2 * lds;
            return p;
        }
        p.family = MHSA_FWD; p.block = 256; p.grid = p.items; p.lds_bytes = lds;
        if (hd != 32 && p.nt >= 14) p.lds_optin = 96 * 1024;            // the two instantiations whose head does not fit 64 KB
        return p;
    }
    const int lds = 4 * p.nt * 16 * hd * 2 + 2 * p.nt * 16 * 4;
    const int lds_ds = lds + 2 * p.nt * 16 * 4 + ntile * 16 * DS_STR * 2;
    const int ds_cu = cus >= 8 ? cus & ~7 : cus;        // whole XCD groups (xcd_remap)
    p.lds_optin = 160 * 1024;
    // default for head_dim 32 and 7 .. 13 token tiles (N = 97 .. 208): dS through LDS, loader waves (AP_MHSA_BWD_DS=0: the two-pass kernel)
    if (hd == 32 && sw.mhsa_bwd_ds && ntile <= 16 - DS_LOADERS && ntile >= 7 && p.nt * 16 * 4 <= 5 * 64 * DS_LOADERS && p.nt * 16 <= DS_STR - 8 &&
        lds_ds <= 160 * 1024) {
        p.family = MHSA_BWD_DS; p.block = 1024; p.grid = attn_min(p.items, ds_cu); p.lds_bytes = lds_ds;
        return p;
    }
    p.family = MHSA_BWD; p.block = 512; p.grid = p.items; p.lds_bytes = lds;
    return p;
}

// class attention (one query per image and head), both directions: scores of all keys + KS * HDP = 2048 floats for both PARTS
static inline MhsaPlan class_attn_plan(int B, int N, int heads, int hd) {
    MhsaPlan p = {};
    if (B <= 0 || N <= 0 || heads <= 0) { p.status = AP_ERR_SHAPE; return p; }
    if (hd != 32 && hd != 48 && hd != 64) { p.status = AP_ERR_UNSUPPORTED; return p; }
    const size_t lds = ((size_t)((N + 63) & ~63) + 64 * 32) * sizeof(float);
    if (lds > 64 * 1024) { p.status = AP_ERR_UNSUPPORTED; return p; }
    p.family = MHSA_CLASS; p.hdt = hd == 32 ? 32 : 64; p.items = p.grid = B * heads; p.block = 256; p.lds_bytes = (int)lds;
    return p;
}

// ---- outlook attention
enum { OLK_P512 = 0, OLK_P256 = 1, OLK_GATHER_MFMA = 2, OLK_GATHER = 3 };
// sr: window rows per strip; nstrips, nitems = B * nstrips * heads; wp_shift: the persistent kernels' OlkArgs.  A backward plan on the
// gather kernels is two launches: the gather (on dY, transposed probabilities) and k_outlook_dlogits, whose geometry is dl_*.
struct OutlookPlan { int status, family, sr, nstrips, nitems, wp_shift, grid, block, lds_bytes, lds_optin, dl_sr, dl_nstrips, dl_grid, dl_lds, dl_optin; };
static inline int olk_optin(int lds) { return lds > 64 * 1024 ? 160 * 1024 : 0; }            // the one-item-per-workgroup kernels ask only past 64 KB

// the one-item-per-workgroup kernels: the forced strip height (an AP_OUTLOOK_SR* value) or the kernel's measured default, at most h, lowered
// until the strip's LDS image leaves two workgroups per CU (78 KB)
template <class Lds> static inline int olk_strip(int forced, int dflt, int h, Lds lds_of) {
    int sr = attn_min(forced > 0 ? forced : dflt, h);
    while (sr > 1 && lds_of(sr) > 78 * 1024) --sr;
    return sr;
}
// geometry of a persistent launch of k_outlook_p<T, NSU, NPU>: the tallest strip (<= 3 window rows) whose tables fit the instantiation and
// whose LDS image leaves two workgroups per CU; -> sr (0: this shape stays on the one-item-per-workgroup kernels)
static inline int olk_pick(int H, int W, bool bwd, int T, int NSU, int NPU, int forced, int& lds) {
    const int h = (H + 1) / 2, w = (W + 1) / 2, pw = 2 * w + 1;
    if (w > 32) return 0;
    for (int sr = attn_min(forced > 0 ? forced : 3, h); sr >= 1; --sr) {
        const int npix = (2 * sr + 3) * pw;
        if (npix * 4 > NSU * T || (sr + 1) * w * OKK > NPU * T) continue;
        const int npixl = (2 * sr + 3) * olk_pws(pw);
        size_t b = (size_t)npixl * OHD * 2 + (size_t)(sr + 1) * w * OPZ * 2;
        if (bwd) b += (size_t)pad_npix(npixl) * OHD * 2 + (((size_t)sr * w * OPP * 2 + 15) & ~(size_t)15);
        if (b <= 80 * 1024) { lds = (int)b; return sr; }
    }
    return 0;
}

static inline OutlookPlan outlook_plan(int dir, int B, int H, int W, int heads, int cus, const ApSwitches& sw) {
    OutlookPlan p = {};
    const auto fail = [&p](int rc) { p.status = rc; return p; };
    if (B <= 0 || H <= 0 || W <= 0 || heads <= 0) return fail(AP_ERR_SHAPE);
    const bool bwd = dir == ATTN_BWD;
    const int h = (H + 1) / 2, w = (W + 1) / 2, pw = 2 * w + 1;
    // AP_OUTLOOK_P: 1 (default) the persistent kernels with 512-thread workgroups (256 where a shape's tables do not fit 512 threads);
    // 2 the 256-thread instantiations; 0 the one-item-per-workgroup kernels
    if (sw.outlook_p) {
        if (sw.outlook_p == 1 && (p.sr = olk_pick(H, W, bwd, 512, 3, 1, sw.outlook_sr, p.lds_bytes)) != 0) { p.family = OLK_P512; p.block = 512; }
        else if ((p.sr = olk_pick(H, W, bwd, 256, 5, 2, sw.outlook_sr, p.lds_bytes)) != 0) { p.family = OLK_P256; p.block = 256; }
    }
    if (p.sr) {
        p.nstrips = (h + p.sr - 1) / p.sr; p.nitems = B * p.nstrips * heads; p.wp_shift = w <= 16 ? 4 : 5; p.lds_optin = 160 * 1024;
        int per_cu = attn_min(160 * 1024 / p.lds_bytes, 2048 / p.block);
        if (per_cu < 1) per_cu = 1;
        p.grid = attn_min(p.nitems, cus * per_cu) & ~7;                 // a multiple of 8: the XCD-contiguous item walk
        if (p.grid < 8) p.grid = 8;
        if (p.grid > p.nitems) p.grid = p.nitems;
        return p;
    }
    // strips of sr window rows: a strip re-stages 3 halo pixel rows and one halo window row, so taller strips waste less; 4 rows keep ~3000
    // workgroups x 256 lanes in flight at 28x28 / B = 128 and 3 workgroups per CU (LDS)
    const auto lds_g = [&](int sr) { return (size_t)pad_npix((2 * sr + 3) * pw) * OHD * 2 + (size_t)(sr + 1) * w * OPP * 4; };
    const auto lds_m = [&](int sr) { return (size_t)(2 * sr + 3) * pw * OHD * 2 + (size_t)(sr + 1) * w * OPZ * 2; };
    const auto lds_d = [&](int sr) { return 2 * ((size_t)pad_npix((2 * sr + 1) * pw) * OHD * 2) + (size_t)sr * w * OPP * 4; };
    p.family = OLK_GATHER; p.block = OGT; p.sr = olk_strip(sw.outlook_sr, 4, h, lds_g);
    if (lds_g(p.sr) > 160 * 1024) return fail(AP_ERR_UNSUPPORTED);
    p.lds_bytes = (int)lds_g(p.sr); p.lds_optin = olk_optin(p.lds_bytes);
    if (sw.outlook_mfma) {
        const int srm = olk_strip(sw.outlook_sr, 3, h, lds_m);          // 3 window rows: 50.4 us forward at 28 x 28 / B = 128 (4: 58.6, 2: 50.3)
        if (lds_m(srm) <= 160 * 1024) { p.family = OLK_GATHER_MFMA; p.sr = srm; p.lds_bytes = (int)lds_m(srm); p.lds_optin = 160 * 1024; }
    }
    p.nstrips = (h + p.sr - 1) / p.sr; p.nitems = p.grid = B * p.nstrips * heads;
    if (bwd) {
        p.dl_sr = olk_strip(sw.outlook_srw, 4, h, lds_d);
        // (never reached: the gather's image of one window row is the larger one, and it was refused above)
        if (lds_d(p.dl_sr) > 160 * 1024) return fail(AP_ERR_UNSUPPORTED);
        p.dl_nstrips = (h + p.dl_sr - 1) / p.dl_sr; p.dl_grid = B * p.dl_nstrips * heads; p.dl_lds = (int)lds_d(p.dl_sr); p.dl_optin = olk_optin(p.dl_lds);
    }
    return p;
}
