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
#include "row_wide.h"

#define TK_MAXK 16
#define TK_SR 2                    // narrow kernel: rows per wave, all of their loads issued before the first is reduced
#define TK_NARROW_MAXLD 1024       // a row in one wave's registers: 2 chunks of 8 columns per lane
#define TK_NEG_INF_CODE 0x007fu    // ~0xff80

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
    for (int w = 0; w < 4; ++w) o[w] = rw_encode2(v[w]);
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
// lane k < K holds the winner of round k in `mine`; se = sum_c exp(inv_temp (x_c - max)), scale = inv_temp * log2(e)
__device__ __forceinline__ void tk_store(unsigned mine, unsigned first, float scale, float se, int lane, int K, int C, int64_t row, int rows_per_batch,
                                         int* __restrict__ idx, float* __restrict__ val, int64_t o_sb, int64_t o_sn) {
    if (lane < K) {
        // (wave-uniform; the 64-bit division is ~100 instructions, more than two selection rounds)
        const int64_t b = row <= 0x7fffffffLL ? (int64_t)((unsigned)row / (unsigned)rows_per_batch) : row / rows_per_batch, n = row - b * rows_per_batch;
        const int64_t o = b * o_sb + n * o_sn + lane;
        const float mx = tk_code_value(first & 0xffff0000u);
        const float e = __builtin_amdgcn_exp2f((tk_code_value(mine & 0xffff0000u) - mx) * scale);
        idx[o] = rw_key_class(mine, C);
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
            prev += rw_wave_maxu(t);
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
        se = rw_wave_sum(se);
        tk_store(mine, first, scale, se, lane, K, C, row, rows_per_batch, idx, val, o_sb, o_sn);
    }
}

// ---------------------------------------------------------------------------------------------------------------- 1024 < ld <= 65 536
// The row is staged in LDS once, as codes, round 0 on the way (the staging walk, the team and their rules: row_wide.h).  The rounds and the
// sum meet in a few words of LDS (one barrier each, double-buffered; none for a team of one wave).
template <int WPR>
__global__ void __launch_bounds__(256)
k_softmax_topk_wide(const bf16_t* __restrict__ logits, int ld, int C, int K, float scale, int* __restrict__ idx, float* __restrict__ val,
                    int64_t o_sb, int64_t o_sn, int rows_per_batch, int64_t M) {
    extern __shared__ __attribute__((aligned(16))) u32x4 tk_rows[];             // [4 / WPR][ld / 8] codes
    __shared__ unsigned red_k[2][4];
    __shared__ float red_s[4];
    constexpr int T = 64 * WPR;
    const RwTeam g = rw_team<WPR>(M);
    const int wave = g.wave, lane = g.lane, team = g.team, tw = g.tw, tt = g.tt;
    const int nch = ld >> 3;
    u32x4* xs = tk_rows + (size_t)team * nch;
    unsigned prev = 0, mine = 0, first = 0;
    for (int j = 0; j < K; ++j) {
        unsigned t = 0;
        if (j == 0) {
            rw_stage<T>(reinterpret_cast<const u32x4*>(logits + g.row * ld), nch, tt, [&](int q, const u32x4& v) {
                const u32x4 o = tk_encode8(tk_mask8(v, 8 * q, C));
                xs[q] = o;
                t = tk_chunk_round(o, q, 0u, t);
            });
        } else {
#pragma unroll 2
            for (int q = tt; q < nch; q += T) t = tk_chunk_round(xs[q], q, prev, t);
        }
        t = rw_wave_maxu(t);
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
    se = rw_wave_sum(se);
    if (WPR > 1) {
        if (lane == 0) red_s[wave] = se;
        __syncthreads();
        se = red_s[team * WPR];
#pragma unroll
        for (int w = 1; w < WPR; ++w) se += red_s[team * WPR + w];
    }
    if (g.live && tw == 0) tk_store(mine, first, scale, se, lane, K, C, g.row, rows_per_batch, idx, val, o_sb, o_sn);
}

extern "C" int ap_softmax_topk_rows(const ap_bf16* logits, int ld, int C, int K, float inv_temp, int* idx, float* val, int64_t o_sb, int64_t o_sn,
                                    int rows_per_batch, int64_t M, ap_stream_t stream) {
    if (M < 0 || C <= 0 || ld < C || (ld & 7) || K < 1 || K > TK_MAXK || K > C || rows_per_batch <= 0) return AP_ERR_SHAPE;
    if (!(inv_temp > 0.f) || !(inv_temp < 3.0e38f)) return AP_ERR_SHAPE;
    if (ld > RW_MAXLD) return AP_ERR_UNSUPPORTED;
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
    return rw_launch(ld, M, [&](auto wpr, unsigned blocks) {
        constexpr int WPR = decltype(wpr)::value;
        const size_t lds = (size_t)(4 / WPR) * ld * sizeof(bf16_t);
        if constexpr (WPR == 4) {                                                // (four rows of a one-wave team are 32 KB at the most)
            if (const int rc = ap_allow_lds<k_softmax_topk_wide<4>>(RW_MAXLD * (int)sizeof(bf16_t)); rc != AP_OK) return rc;
        }
        hipLaunchKernelGGL(k_softmax_topk_wide<WPR>, dim3(blocks), dim3(256), lds, (hipStream_t)stream, x, ld, C, K, scale, idx, val, o_sb, o_sn, rows_per_batch, M);
        return ap_check_launch();
    });
}
