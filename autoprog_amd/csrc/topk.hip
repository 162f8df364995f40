// Row-wise softmax + top-K over bf16 logits: the (class, score) pairs of a token-label target from a teacher's logits, one pass.
//   idx[o + k] = class of the k-th largest logit of row r = (b, n) among columns 0 .. C-1 (equal logits: ascending class),
//   val[o + k] = softmax(inv_temp * x)[idx[o + k]] over all C columns,       o = b * o_sb + n * o_sn,  k < K <= 16.
// HBM-bound by design: 2 B per (row, class) in, 8 K bytes per row out; the row is read from global memory ONCE.
//
// Order and tie rule in one integer.  A bf16 value becomes a 16-bit CODE whose unsigned order is the value's order (-0 is +0 first,
// then positive: u ^ 0x8000, negative: ~u), and a column's KEY is (code << 16) | (0xFFFF - column): keys of a row are distinct, and
// their unsigned maximum is the largest value at its smallest column.  Round j of the selection is "the largest key strictly below
// the winner of round j-1": with t = key - prev (mod 2^32) every key below prev maps above every key that is not, in order, so a
// round is one subtraction and one maximum per column and nothing is ever removed from anyone's registers.  prev = 0 is round 0.
// The value comes back out of the winning key, so the K scores need no second lookup.
// Columns C .. ld-1 are replaced by the code of -inf before any use: they add exp(-inf) = 0 to the sum, and behind every valid column
// of the same value in the order -- K <= C, so none of them is ever selected.  A NaN or an all -inf row gives unspecified scores;
// the stored class is clamped into [0, C) whatever the keys were.
// Statistics in fp32, maximum subtracted ((x - max) is exact for bf16 operands), fixed reduction order (one DPP tree per wave, then the
// waves of a team in index order): bit-reproducible.  No atomics, no workspace; plain grids (one workgroup per row group).
#include "common.h"

#define TK_MAXK 16
#define TK_SR 2                    // narrow kernel: rows per wave, all of their loads issued before the first is reduced
#define TK_NARROW_MAXLD 1024       // a row in one wave's registers: 2 chunks of 8 columns per lane
#define TK_TEAM1_MAXLD 4096        // LDS rows: a wave per row up to here (4 rows per workgroup), four waves per row beyond
#define TK_MAXLD 65536             // 2 B per column of LDS: 128 KB, one workgroup per CU
#define TK_NEG_INF_CODE 0x007fu    // ~0xff80

// two bf16 of a word -> their two codes
__device__ __forceinline__ unsigned tk_encode2(unsigned w) {
    const unsigned m = w & 0x7fff7fffu;
    const unsigned nz = (m + 0x7fff7fffu) & 0x80008000u;          // bit 15 of a half: its magnitude is not zero (no carry between the halves)
    w &= nz | 0x7fff7fffu;                                        // -0 -> +0: equal logits are equal codes
    const unsigned s = (w >> 15) & 0x00010001u;
    return w ^ (s * 0x7fffu + 0x80008000u);                       // negative: ^ 0xffff, positive: ^ 0x8000
}
// one chunk (columns c0 .. c0+7) with its columns >= C replaced by -inf (only the last chunks of a row take the branch)
__device__ __forceinline__ u32x4 tk_mask8(u32x4 v, int c0, int C) {
    if (c0 + 8 > C) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const unsigned lo = c0 + 2 * w < C ? (v[w] & 0xffffu) : 0xff80u;
            const unsigned hi = c0 + 2 * w + 1 < C ? (v[w] & 0xffff0000u) : 0xff800000u;
            v[w] = lo | hi;
        }
    }
    return v;
}
__device__ __forceinline__ u32x4 tk_encode8(const u32x4& v) {
    u32x4 o;
#pragma unroll
    for (int w = 0; w < 4; ++w) o[w] = tk_encode2(v[w]);
    return o;
}
// code << 16 (low half zero) -> the value
__device__ __forceinline__ float tk_code_value(unsigned hi) {
    return __uint_as_float(hi ^ ((int)hi < 0 ? 0x80000000u : 0xffff0000u));
}
// max over the 8 columns of chunk q of (key - prev)
__device__ __forceinline__ unsigned tk_chunk_round(const u32x4& o, int q, unsigned prev, unsigned t) {
    const unsigned cc = 0xffffu - 8u * (unsigned)q;               // 0xFFFF - column of the chunk's first element
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        t = max(t, ((o[w] << 16) | (cc - 2 * w)) - prev);
        t = max(t, ((o[w] & 0xffff0000u) | (cc - 2 * w - 1)) - prev);
    }
    return t;
}
// Wave reductions on the DPP path (no LDS crossbar round trip per step): lanes of a quad, the two halves of a row of 16 and the row mirrored,
// then lane 15 of rows 0 / 2 into rows 1 / 3 and lane 31 into rows 2 / 3 -- lane 63 ends with the whole wave, read back as a wave-uniform value.
// One fixed order for every row: the float sum is bit-reproducible.
#define TK_DPP(x, ctrl, rows) __builtin_amdgcn_update_dpp(0, (int)(x), ctrl, rows, 0xf, false)
__device__ __forceinline__ unsigned tk_wave_max(unsigned v) {
    v = max(v, (unsigned)TK_DPP(v, 0xb1, 0xf));                  // quad_perm [1, 0, 3, 2]
    v = max(v, (unsigned)TK_DPP(v, 0x4e, 0xf));                  // quad_perm [2, 3, 0, 1]
    v = max(v, (unsigned)TK_DPP(v, 0x141, 0xf));                 // row_half_mirror
    v = max(v, (unsigned)TK_DPP(v, 0x140, 0xf));                 // row_mirror: every lane of a row holds the row's maximum
    v = max(v, (unsigned)TK_DPP(v, 0x142, 0xa));                 // row_bcast15 into rows 1 and 3 (others read 0: the identity)
    v = max(v, (unsigned)TK_DPP(v, 0x143, 0xc));                 // row_bcast31 into rows 2 and 3
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ float tk_wave_sum(float v) {
#define TK_DPP_F(x, ctrl, rows) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), ctrl, rows, 0xf, false))
    v += TK_DPP_F(v, 0xb1, 0xf);
    v += TK_DPP_F(v, 0x4e, 0xf);
    v += TK_DPP_F(v, 0x141, 0xf);
    v += TK_DPP_F(v, 0x140, 0xf);
    v += TK_DPP_F(v, 0x142, 0xa);
    v += TK_DPP_F(v, 0x143, 0xc);
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
// lane k < K holds the winner of round k in `mine`; se = sum_c exp(inv_temp (x_c - max)), scale = inv_temp * log2(e)
__device__ __forceinline__ void tk_store(unsigned mine, unsigned first, float scale, float se, int lane, int K, int C, int64_t row, int rows_per_batch,
                                         int* __restrict__ idx, float* __restrict__ val, int64_t o_sb, int64_t o_sn) {
    if (lane < K) {
        // (wave-uniform; the 64-bit division is ~100 instructions, more than two selection rounds)
        const int64_t b = row <= 0x7fffffffLL ? (int64_t)((unsigned)row / (unsigned)rows_per_batch) : row / rows_per_batch, n = row - b * rows_per_batch;
        const int64_t o = b * o_sb + n * o_sn + lane;
        const float mx = tk_code_value(first & 0xffff0000u);
        const float e = __builtin_amdgcn_exp2f((tk_code_value(mine & 0xffff0000u) - mx) * scale);
        idx[o] = min((int)(0xffffu - (mine & 0xffffu)), C - 1);
        val[o] = e / se;
    }
}

// ---------------------------------------------------------------------------------------------------------------- ld <= 1024
// One wave per row, TK_SR rows per wave: lane l owns chunks l and l + 64 (16 columns), their keys live in 16 registers.
__global__ void __launch_bounds__(256)
k_softmax_topk(const bf16_t* __restrict__ logits, int ld, int C, int K, float scale, int* __restrict__ idx, float* __restrict__ val,
               int64_t o_sb, int64_t o_sn, int rows_per_batch, int64_t M) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * TK_SR;
    if (row0 >= M) return;                                        // (whole waves; no barrier in this kernel)
    const int nch = ld >> 3;
    u32x4 raw[TK_SR][2];
#pragma unroll
    for (int r = 0; r < TK_SR; ++r) {
        const u32x4* xg = reinterpret_cast<const u32x4*>(logits + min(row0 + r, M - 1) * ld);
#pragma unroll
        for (int i = 0; i < 2; ++i) raw[r][i] = xg[min(lane + 64 * i, nch - 1)];       // clamped, unconditional; a repeated chunk is masked below
    }
#pragma unroll
    for (int r = 0; r < TK_SR; ++r) {
        const int64_t row = row0 + r;
        if (row >= M) break;
        unsigned key[16];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int q = lane + 64 * i;
            raw[r][i] = tk_mask8(raw[r][i], q < nch ? 8 * q : C, C);                   // a chunk beyond the row: all -inf
            const u32x4 o = tk_encode8(raw[r][i]);
            const unsigned cc = 0xffffu - 8u * (unsigned)q;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                key[8 * i + 2 * w] = (o[w] << 16) | (cc - 2 * w);
                key[8 * i + 2 * w + 1] = (o[w] & 0xffff0000u) | (cc - 2 * w - 1);
            }
        }
        unsigned prev = 0, mine = 0, first = 0;
        for (int j = 0; j < K; ++j) {
            unsigned t = 0;
#pragma unroll
            for (int e = 0; e < 16; ++e) t = max(t, key[e] - prev);
            prev += tk_wave_max(t);
            if (j == 0) first = prev;
            mine = lane == j ? prev : mine;
        }
        const float mx = tk_code_value(first & 0xffff0000u);
        float se = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {                                                  // (the values from the masked words themselves: one operation each)
            const unsigned w = raw[r][e >> 2][e & 3];
            se += __builtin_amdgcn_exp2f((bf_lo(w) - mx) * scale);
            se += __builtin_amdgcn_exp2f((bf_hi(w) - mx) * scale);
        }
        se = tk_wave_sum(se);
        tk_store(mine, first, scale, se, lane, K, C, row, rows_per_batch, idx, val, o_sb, o_sn);
    }
}

// ---------------------------------------------------------------------------------------------------------------- 1024 < ld <= 65 536
// The row is staged in LDS once, as codes, in 16-byte chunks (the loads of the next batch issued before the previous one is encoded and
// written), round 0 on the way.  A TEAM of WPR waves owns a row; thread tt of the team owns chunks tt, tt + T, ..: it is the only
// thread that ever writes or reads them, so the row itself needs no barrier -- the rounds and the sum meet in a few words of LDS
// (one barrier each, double-buffered; every wave reaches every barrier: rows beyond M are clamped and only their stores are masked).
template <int T>
__device__ __forceinline__ unsigned tk_stage(const u32x4* __restrict__ xg, u32x4* xs, int nch, int C, int tt) {
    constexpr int U = 4;
    unsigned t = 0;
    u32x4 cur[U], nxt[U];
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u] = xg[min(tt + T * u, nch - 1)];          // clamped, unconditional
    for (int base = 0; base < nch; base += U * T) {
        const bool more = base + U * T < nch;                                    // team-uniform: one branch around the whole batch
        if (more) {
#pragma unroll
            for (int u = 0; u < U; ++u) nxt[u] = xg[min(base + U * T + tt + T * u, nch - 1)];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = base + tt + T * u;
            if (q < nch) {
                const u32x4 o = tk_encode8(tk_mask8(cur[u], 8 * q, C));
                xs[q] = o;
                t = tk_chunk_round(o, q, 0u, t);
            }
        }
        if (more) {
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        }
    }
    return t;
}

template <int WPR>
__global__ void __launch_bounds__(256)
k_softmax_topk_wide(const bf16_t* __restrict__ logits, int ld, int C, int K, float scale, int* __restrict__ idx, float* __restrict__ val,
                    int64_t o_sb, int64_t o_sn, int rows_per_batch, int64_t M) {
    extern __shared__ __attribute__((aligned(16))) u32x4 tk_rows[];             // [4 / WPR][ld / 8] codes
    __shared__ unsigned red_k[2][4];
    __shared__ float red_s[4];
    constexpr int T = 64 * WPR;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int team = wave / WPR, tw = wave % WPR, tt = tw * 64 + lane;
    const int64_t row_raw = (int64_t)blockIdx.x * (4 / WPR) + team;
    const bool live = row_raw < M;
    const int64_t row = min(row_raw, M - 1);
    const int nch = ld >> 3;
    u32x4* xs = tk_rows + (size_t)team * nch;
    unsigned prev = 0, mine = 0, first = 0;
    for (int j = 0; j < K; ++j) {
        unsigned t = 0;
        if (j == 0) {
            t = tk_stage<T>(reinterpret_cast<const u32x4*>(logits + row * ld), xs, nch, C, tt);
        } else {
#pragma unroll 2
            for (int q = tt; q < nch; q += T) t = tk_chunk_round(xs[q], q, prev, t);
        }
        t = tk_wave_max(t);
        if (WPR > 1) {
            if (lane == 0) red_k[j & 1][wave] = t;
            __syncthreads();
            t = red_k[j & 1][team * WPR];
#pragma unroll
            for (int w = 1; w < WPR; ++w) t = max(t, red_k[j & 1][team * WPR + w]);
        }
        prev += t;
        if (j == 0) first = prev;
        mine = lane == j ? prev : mine;
    }
    const float mx = tk_code_value(first & 0xffff0000u);
    float se = 0.f;
#pragma unroll 2
    for (int q = tt; q < nch; q += T) {
        const u32x4 o = xs[q];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            se += __builtin_amdgcn_exp2f((tk_code_value(o[w] << 16) - mx) * scale);
            se += __builtin_amdgcn_exp2f((tk_code_value(o[w] & 0xffff0000u) - mx) * scale);
        }
    }
    se = tk_wave_sum(se);
    if (WPR > 1) {
        if (lane == 0) red_s[wave] = se;
        __syncthreads();
        se = red_s[team * WPR];
#pragma unroll
        for (int w = 1; w < WPR; ++w) se += red_s[team * WPR + w];
    }
    if (live && tw == 0) tk_store(mine, first, scale, se, lane, K, C, row, rows_per_batch, idx, val, o_sb, o_sn);
}

extern "C" int ap_softmax_topk_rows(const ap_bf16* logits, int ld, int C, int K, float inv_temp, int* idx, float* val, int64_t o_sb, int64_t o_sn,
                                    int rows_per_batch, int64_t M, ap_stream_t stream) {
    if (M < 0 || C <= 0 || ld < C || (ld & 7) || K < 1 || K > TK_MAXK || K > C || rows_per_batch <= 0) return AP_ERR_SHAPE;
    if (!(inv_temp > 0.f) || !(inv_temp < 3.0e38f)) return AP_ERR_SHAPE;
    if (ld > TK_MAXLD) return AP_ERR_UNSUPPORTED;
    if (M == 0) return AP_OK;
    if (!logits || !idx || !val) return AP_ERR_NULL;
    if ((uintptr_t)logits & 15) return AP_ERR_SHAPE;                            // rows are moved in 16-byte chunks
    const float scale = inv_temp * 1.44269504088896341f;
    const bf16_t* x = reinterpret_cast<const bf16_t*>(logits);
    (void)hipGetLastError();
    if (ld <= TK_NARROW_MAXLD) {
        const int64_t blocks = (M + 4 * TK_SR - 1) / (4 * TK_SR);
        if (blocks > 0x7fffffffLL) return AP_ERR_SHAPE;
        hipLaunchKernelGGL(k_softmax_topk, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, ld, C, K, scale, idx, val, o_sb, o_sn, rows_per_batch, M);
        return ap_check_launch();
    }
    const bool team1 = ld <= TK_TEAM1_MAXLD;
    const int rpb = team1 ? 4 : 1;
    const int64_t blocks = (M + rpb - 1) / rpb;
    if (blocks > 0x7fffffffLL) return AP_ERR_SHAPE;
    const size_t lds = (size_t)rpb * ld * sizeof(bf16_t);
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute((const void*)k_softmax_topk_wide<4>, hipFuncAttributeMaxDynamicSharedMemorySize, TK_MAXLD * (int)sizeof(bf16_t));
        attr = true;
    }
    if (team1)
        hipLaunchKernelGGL(k_softmax_topk_wide<1>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, x, ld, C, K, scale, idx, val, o_sb, o_sn, rows_per_batch, M);
    else
        hipLaunchKernelGGL(k_softmax_topk_wide<4>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, x, ld, C, K, scale, idx, val, o_sb, o_sn, rows_per_batch, M);
    return ap_check_launch();
}
