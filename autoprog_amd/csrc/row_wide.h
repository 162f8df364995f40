// The core of the kernels that keep a row wider than 1024 columns in LDS: k_soft_ce_wide (softce.hip), k_softmax_topk_wide (topk.hip),
// k_distill_wide (distill.hip).  Also the wave reductions and the bf16 order code, which the narrow register kernels of topk.hip and
// distill.hip use as well.
//
// A TEAM of WPR waves owns a row: one wave up to RW_TEAM1_MAXLD columns (four rows per workgroup), four waves beyond (one row per
// workgroup).  The row is read from global memory ONCE, in 16-byte chunks, and staged in LDS; every later walk reads LDS.  The rules:
//   * thread tt of a team owns chunks tt, tt + T, .. (T = 64 WPR): it is the only thread that ever writes or reads them, so the row itself
//     needs no barrier -- the teams' reductions meet in a few words of LDS (lane 0 of a wave writes, one barrier, folded in wave order);
//   * every wave reaches every barrier: a row beyond M is clamped to row M - 1 and computed like any other, only its stores are masked;
//   * loads are clamped and unconditional (no exec-masked blocks around them); a repeated chunk is dropped by the `q < nch` in front of
//     the consumer, padding columns by the consumer's own masks.
// Fixed reduction order (one DPP tree per wave, then the waves of a team in index order): bit-reproducible.
#pragma once
#include <type_traits>
#include "common.h"

#define RW_TEAM1_MAXLD 4096        // a wave per row up to here, four waves per row beyond
#define RW_MAXLD 65536             // 2 B per column of LDS: 128 KB, one workgroup per CU

// ---- wave reductions on the DPP path (no LDS crossbar round trip per step): lanes of a quad, the two halves of a row of 16 and the row
// mirrored, then lane 15 of rows 0 / 2 into rows 1 / 3 and lane 31 into rows 2 / 3 -- lane 63 ends with the whole wave, read back as a
// wave-uniform value.  Rows that a step does not write keep `old`: 0 for the sums and the keys (the identity), the value itself for the
// float maximum.  One fixed order for every row: the float sum is bit-reproducible.
#define RW_DPP(old, x, ctrl, rows) __builtin_amdgcn_update_dpp((int)(old), (int)(x), ctrl, rows, 0xf, false)
#define RW_DPP_F(old, x, ctrl, rows) __builtin_bit_cast(float, RW_DPP(__builtin_bit_cast(int, old), __builtin_bit_cast(int, x), ctrl, rows))
__device__ __forceinline__ unsigned rw_wave_maxu(unsigned v) {
    v = max(v, (unsigned)RW_DPP(0, v, 0xb1, 0xf));                // quad_perm [1, 0, 3, 2]
    v = max(v, (unsigned)RW_DPP(0, v, 0x4e, 0xf));                // quad_perm [2, 3, 0, 1]
    v = max(v, (unsigned)RW_DPP(0, v, 0x141, 0xf));               // row_half_mirror
    v = max(v, (unsigned)RW_DPP(0, v, 0x140, 0xf));               // row_mirror: every lane of a row holds the row's maximum
    v = max(v, (unsigned)RW_DPP(0, v, 0x142, 0xa));               // row_bcast15 into rows 1 and 3
    v = max(v, (unsigned)RW_DPP(0, v, 0x143, 0xc));               // row_bcast31 into rows 2 and 3
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ float rw_wave_sum(float v) {
    v += RW_DPP_F(0.f, v, 0xb1, 0xf);
    v += RW_DPP_F(0.f, v, 0x4e, 0xf);
    v += RW_DPP_F(0.f, v, 0x141, 0xf);
    v += RW_DPP_F(0.f, v, 0x140, 0xf);
    v += RW_DPP_F(0.f, v, 0x142, 0xa);
    v += RW_DPP_F(0.f, v, 0x143, 0xc);
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ float rw_wave_max(float v) {
    v = fmaxf(v, RW_DPP_F(v, v, 0xb1, 0xf));
    v = fmaxf(v, RW_DPP_F(v, v, 0x4e, 0xf));
    v = fmaxf(v, RW_DPP_F(v, v, 0x141, 0xf));
    v = fmaxf(v, RW_DPP_F(v, v, 0x140, 0xf));
    v = fmaxf(v, RW_DPP_F(v, v, 0x142, 0xa));
    v = fmaxf(v, RW_DPP_F(v, v, 0x143, 0xc));
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// ---- the bf16 order code.  Two bf16 of a word -> their two 16-bit CODES, whose unsigned order is the values' order (-0 is +0 first, then
// positive: u ^ 0x8000, negative: ~u).  A column's KEY is (code << 16) | (0xFFFF - column): the keys of a row are distinct and their
// unsigned maximum is the largest value at its smallest column.
__device__ __forceinline__ unsigned rw_encode2(unsigned w) {
    const unsigned m = w & 0x7fff7fffu;
    const unsigned nz = (m + 0x7fff7fffu) & 0x80008000u;          // bit 15 of a half: its magnitude is not zero (no carry between the halves)
    w &= nz | 0x7fff7fffu;                                        // -0 -> +0: equal logits are equal codes
    const unsigned s = (w >> 15) & 0x00010001u;
    return w ^ (s * 0x7fffu + 0x80008000u);                       // negative: ^ 0xffff, positive: ^ 0x8000
}
// the class a key names, clamped into [0, C) whatever the row held
__device__ __forceinline__ int rw_key_class(unsigned key, int C) { return min((int)(0xffffu - (key & 0xffffu)), C - 1); }

// ---- where a thread of a 256-thread workgroup stands: its wave and lane, its team and its place in it (tw: wave of the team, tt: thread of
// the team), and the team's row, clamped (live: the row exists)
struct RwTeam {
    int wave, lane, team, tw, tt;
    int64_t row;
    bool live;
};
template <int WPR>
__device__ __forceinline__ RwTeam rw_team(int64_t M) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int team = wave / WPR, tw = wave % WPR, tt = tw * 64 + lane;
    const int64_t row_raw = (int64_t)blockIdx.x * (4 / WPR) + team;
    return {wave, lane, team, tw, tt, min(row_raw, M - 1), row_raw < M};
}

// ---- the staging walk: chunks tt, tt + T, .. < nch of a row come through registers, U = 4 in flight, the loads of the next batch issued
// before the previous one is consumed.  f(q, chunk) runs once for every chunk q the thread owns: it stores what the later walks need and
// takes what can be had on the way.  (k_distill_wide, which walks two rows together, keeps this loop written out: through this template it
// measured 3 % (hard) and 7 % (soft) slower at 21 848 columns -- the compiler then waits for the next batch before it consumes this one.)
template <int T, class F>
__device__ __forceinline__ void rw_stage(const u32x4* g, int nch, int tt, F&& f) {
    constexpr int U = 4;
    u32x4 cur[U], nxt[U];
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u] = g[min(tt + T * u, nch - 1)];            // clamped, unconditional
    for (int base = 0; base < nch; base += U * T) {
        const bool more = base + U * T < nch;                                    // team-uniform: one branch around the whole batch
        if (more) {
#pragma unroll
            for (int u = 0; u < U; ++u) nxt[u] = g[min(base + U * T + tt + T * u, nch - 1)];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = base + tt + T * u;
            if (q < nch) f(q, cur[u]);
        }
        if (more) {
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        }
    }
}

// ---- the launch shape: what selects the team (`width`: a leading dimension, or the columns that are read) and the row count give the
// rows per workgroup (4 / WPR) and the grid; go(WPR as an integral constant, blocks) launches its family's <1> or <4> kernel with the LDS
// bytes that family needs and returns the status.
template <class GO>
static int rw_launch(int width, int64_t M, GO&& go) {
    const int rpb = width <= RW_TEAM1_MAXLD ? 4 : 1;
    const int64_t blocks = (M + rpb - 1) / rpb;
    if (blocks > 0x7fffffffLL) return AP_ERR_SHAPE;
    if (rpb == 1) return go(std::integral_constant<int, 4>{}, (unsigned)blocks);
    return go(std::integral_constant<int, 1>{}, (unsigned)blocks);
}
