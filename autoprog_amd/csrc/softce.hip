// Dense soft-target cross entropy, forward + gradient in one pass over (logits, target):
//   row_loss = lse*sum_c t - sum_c t*x ;  dx = gscale*(softmax(x)*sum_c t - t)
// (loss/cross_entropy.py:35-36; token-label targets are CLASS-major [B,C,2+N] while logits are
// token-major [B*N,C], loss/cross_entropy.py:147-148 -- the transpose is done through LDS).
// HBM-bound: logits 2 B + target 4 B + dlogits 2 B per (row, class).
//
// Block = one (batch, tile of TN=16 tokens).  Phase A: the target tile is read coalesced along
// the token axis (16 consecutive fp32 = 64 B per class) and stored token-major in LDS with an
// odd row stride.  Phase B: each wave owns 4 rows; lanes stride over classes (coalesced logits),
// keep the row in registers, reduce max / sum-exp / sum t / sum t*x with wavefront shuffles.
#include "row_wide.h"

#define CE_TN 16
#define CE_MAXV 8          // classes per lane pairs: supports C <= 64*2*CE_MAXV = 1024

__global__ void __launch_bounds__(256)
k_soft_ce(const bf16_t* __restrict__ logits, int ldx, const float* __restrict__ target, int64_t t_sb, int64_t t_sc,
          int64_t t_sn, int rows_per_batch, float* __restrict__ row_loss, bf16_t* __restrict__ dlogits,
          float gscale, int64_t M, int C, int tiles_per_batch, float mix_lam, int mix_batches, const float* __restrict__ lam_dev = nullptr) {
    if (lam_dev) mix_lam = lam_dev[0];                   // the step's lam from device memory (graph replay; lam = 1: lam t + 0 t' = t exactly)
    extern __shared__ __attribute__((aligned(16))) float tt[];      // [CE_TN][Cp] Cp odd
    const int Cp = C | 1;
    const int64_t b = blockIdx.x / tiles_per_batch;
    const int n0 = (blockIdx.x % tiles_per_batch) * CE_TN;
    const int ntok = min(CE_TN, rows_per_batch - n0);
    // the logits of this wave's (up to) four rows are requested FIRST: they do not depend on the target tile, so their latency hides
    // behind phase A (clamped, unconditional 4-byte loads; columns beyond C are masked where they are used)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned lraw[CE_TN / 4][CE_MAXV];
#pragma unroll
    for (int r = 0; r < CE_TN / 4; ++r) {
        const int64_t rowc = min(b * rows_per_batch + n0 + min(wave + 4 * r, ntok - 1), M - 1);
        const bf16_t* xr = logits + rowc * ldx;
#pragma unroll
        for (int i = 0; i < CE_MAXV; ++i) lraw[r][i] = *reinterpret_cast<const unsigned*>(xr + min(2 * (lane + 64 * i), ldx - 2));
    }
    // ---- phase A: target tile -> LDS (token-major)
    {
        const int tn = threadIdx.x & (CE_TN - 1), cl = threadIdx.x / CE_TN;     // 16 classes per pass
        const int tnc = min(tn, ntok - 1);                                       // lanes beyond the tile's tokens read a valid token (never stored)
        const float* tb = target + b * t_sb + (int64_t)(n0 + tnc) * t_sn;
        // mix-token: the image-level label of sample b is lam * t[b] + (1 - lam) * t[B-1-b] (loss/cross_entropy.py:151-152)
        const float* tb2 = mix_batches > 0 ? target + (int64_t)(mix_batches - 1 - b) * t_sb + (int64_t)(n0 + tnc) * t_sn : tb;
        const float lam2 = mix_batches > 0 ? 1.0f - mix_lam : 0.f, lam1 = mix_batches > 0 ? mix_lam : 1.0f;
        // CE_INFLIGHT independent loads in flight per thread: the tile is 63 four-byte loads per thread, and every batch exposes one memory
        // latency (one load per iteration: 63 latencies; 8 per batch: 8; 32 per batch: 2)
        constexpr int CSTEP = 256 / CE_TN;
        constexpr int CE_INFLIGHT = 32;
        const bool mixed = mix_batches > 0;
        for (int c0 = cl; c0 < C; c0 += CE_INFLIGHT * CSTEP) {
            float v[CE_INFLIGHT], v2[CE_INFLIGHT];
#pragma unroll
            for (int u = 0; u < CE_INFLIGHT; ++u) {
                const int c = min(c0 + u * CSTEP, C - 1);                       // clamped: unconditional loads (no exec-masked blocks)
                v[u] = tb[(int64_t)c * t_sc];
                v2[u] = mixed ? tb2[(int64_t)c * t_sc] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < CE_INFLIGHT; ++u) {
                const int c = c0 + u * CSTEP;
                if (tn < ntok && c < C) tt[tn * Cp + c] = lam1 * v[u] + lam2 * v2[u];
            }
        }
    }
    __syncthreads();
    // ---- phase B
#pragma unroll
    for (int r = 0; r < CE_TN / 4; ++r) {
        const int tn = wave + 4 * r;
        const int64_t row = b * rows_per_batch + n0 + tn;
        if (tn >= ntok || row >= M) break;
        const float* tr = tt + tn * Cp;
        float xv[CE_MAXV][2];
        float mx = -3.0e38f;
#pragma unroll
        for (int i = 0; i < CE_MAXV; ++i) {
            const int c = 2 * (lane + 64 * i);
            const unsigned u = lraw[r][i];
            xv[i][0] = c < C ? bf_lo(u) : -3.0e38f;
            xv[i][1] = c + 1 < C ? bf_hi(u) : -3.0e38f;
            mx = fmaxf(mx, fmaxf(xv[i][0], xv[i][1]));
        }
        mx = group_max<64>(mx);
        float se = 0.f, st = 0.f, stx = 0.f;
#pragma unroll
        for (int i = 0; i < CE_MAXV; ++i) {
            const int c = 2 * (lane + 64 * i);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (c + k < C) {
                    const float t = tr[c + k];
                    se += __expf(xv[i][k] - mx);
                    st += t;
                    stx += t * xv[i][k];
                }
            }
        }
        se = group_sum<64>(se); st = group_sum<64>(st); stx = group_sum<64>(stx);
        const float lse = mx + __logf(se);
        if (lane == 0) row_loss[row] = lse * st - stx;
        bf16_t* dr = dlogits + row * ldx;
#pragma unroll
        for (int i = 0; i < CE_MAXV; ++i) {
            const int c = 2 * (lane + 64 * i);
            if (c < ldx) {      // ldx is even (multiple of 8): pairs never straddle the row end
                float d0 = 0.f, d1 = 0.f;
                if (c < C) d0 = gscale * (__expf(xv[i][0] - lse) * st - tr[c]);
                if (c + 1 < C) d1 = gscale * (__expf(xv[i][1] - lse) * st - tr[c + 1]);
                *reinterpret_cast<unsigned*>(dr + c) = pack_bf2(d0, d1);
            }
        }
    }
}

// The same loss on the token-label target in its SOURCE form.  The reference builds the dense class-major [B,C,2+N] tensor from
// top-K (class, score) label maps plus label smoothing on the GPU every step (main_prog.py:994-1004, tlt create_token_label_target)
// and the dense kernel above then reads 4 B per (row, class) of it -- 101 MB at B = 128.  Here a row's target is
//     t[c] = (1 - s) * sum_k [idx_k == c] * val_k + s / C
// formed in registers from its K pairs: logits in, dlogits out, nothing else.  One wave per row, a lane owns class pairs
// 2 (lane + 64 i).  Pairs of row r = (b, n), b = r / rows_per_batch, sit at pairs + b * p_sb + n * p_sn (K entries each).
// mix_batches = B > 0 (the mix-token class target, loss/cross_entropy.py:150-152: lam * t[b] + (1 - lam) * t[B-1-b]): lanes K .. 2K-1
// hold the pairs of the same slot of image B-1-b weighted 1 - lam, the row's own are weighted lam -- 2K <= CE_MAXK pairs, no
// concatenated / flipped / scaled copies of the label maps on the host side.
#define CE_MAXK 16
#define CE_SR 4            // rows per wave, all of their loads issued before the first is reduced

// GT = true: the class row of TokenLabelGTCrossEntropy (loss/cross_entropy.py:62-89), one row per image (rows_per_batch = 1).  Its target is
//     t_b = ratio_b * dense(slot 1) + (1 - ratio_b) * dense(slot 0),   ratio_b = 0.9 - 0.4 * [argmax dense(slot 0) == argmax dense(slot 1)]
// and, mixed, lam * t_b + (1 - lam) * t_{B-1-b} with the partner's OWN ratio: every weight row sums to 1, so the smoothing term stays s / C
// and the row is up to 4 K weighted pairs, K <= CE_GT_MAXK.  Lane 8 g + k (< 32) holds pair k of group g:
//     g = 0  own slot 1      lam * ratio_b                  g = 2  partner slot 1   (1 - lam) * ratio_{B-1-b}
//     g = 1  own slot 0      lam * (1 - ratio_b)            g = 3  partner slot 0   (1 - lam) * (1 - ratio_{B-1-b})
// (unmixed: groups 0 and 1, weights ratio_b and 1 - ratio_b).  The argmax of a slot, decided here per group of 8 lanes: a class's score is
// the fp32 sum of its pairs' val in ascending k (indices outside [0, C) add nothing); the argmax is the SMALLEST class among those of the
// largest score, and class 0 when no score is positive (every class then holds s / C).  Scores are assumed non-negative.
// idx1 / val1 point at slot 1 of image 0, d0 is the offset from slot 1 to slot 0, p_sb the image stride.  Every lane loads (clamped to a
// pair of the row's own slot 1); a pair outside [0, C) leaves (-1, 0).  All 64 lanes must be active (cross-lane reads).
#define CE_GT_MAXK 8
__device__ __forceinline__ void ce_gt_pairs(const int* __restrict__ idx1, const float* __restrict__ val1, int K, int64_t p_sb, int64_t d0, int64_t b,
                                            int mix_batches, float mix_lam, float smoothing, int C, int lane, int& my_i, float& my_v) {
    const bool mixed = mix_batches > 0;
    const int g = lane >> 3, k = lane & 7;
    const bool want = lane < 32 && k < K && (g < 2 || mixed);
    const int64_t img = (mixed && (g & 2)) ? (int64_t)(mix_batches - 1) - b : b;
    const int64_t po = want ? img * p_sb + ((g & 1) ? d0 : 0) + k : b * p_sb;
    int ci = idx1[po];
    float cv = val1[po];
    const bool ok = want && ci >= 0 && ci < C;
    ci = ok ? ci : -1;
    cv = ok ? cv : 0.f;
    // the score of this lane's class inside its group: the K x K compare, pairs in ascending k
    float sc = 0.f;
#pragma unroll
    for (int j = 0; j < CE_GT_MAXK; ++j) {
        const int oi = __shfl(ci, (lane & ~7) | j, 64);
        const float ov = __shfl(cv, (lane & ~7) | j, 64);
        sc += oi == ci ? ov : 0.f;
    }
    sc = ok ? sc : -1.0f;
    float best = sc;
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) best = fmaxf(best, __shfl_xor(best, o, 64));
    int am = (ok && best > 0.f && sc == best) ? ci : 0x7fffffff;
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) am = min(am, __shfl_xor(am, o, 64));
    am = am == 0x7fffffff ? 0 : am;
    const float ratio = am == __shfl_xor(am, 8, 64) ? 0.5f : 0.9f;          // 0.9 - 0.4 * [the two slots agree]
    float wgt = (g & 1) ? 1.0f - ratio : ratio;
    if (mixed) wgt *= (g & 2) ? 1.0f - mix_lam : mix_lam;
    my_i = ci;
    my_v = cv * wgt * (1.0f - smoothing);
}

// GT: one row per wave (the B class rows are latency, not traffic), p_sn carries d0 (rows_per_batch = 1 leaves it free), idx / val point at slot 1
template <bool GT>
__global__ void __launch_bounds__(256)
k_soft_ce_sparse(const bf16_t* __restrict__ logits, int ldx, const int* __restrict__ idx, const float* __restrict__ val, int K,
                 int64_t p_sb, int64_t p_sn, int rows_per_batch, float smoothing, float* __restrict__ row_loss,
                 bf16_t* __restrict__ dlogits, float gscale, int64_t M, int C, float mix_lam, int mix_batches, const float* __restrict__ lam_dev = nullptr) {
    if (lam_dev) mix_lam = lam_dev[0];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int SR = GT ? 1 : CE_SR;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * SR;
    if (row0 >= M) return;
    const int KK = GT ? (mix_batches > 0 ? 32 : 16) : (mix_batches > 0 ? 2 * K : K);       // lanes that may hold a pair of the row
    unsigned lraw[SR][CE_MAXV];
    int my_i[SR];
    float my_v[SR];
#pragma unroll
    for (int r = 0; r < SR; ++r) {
        const int64_t row = min(row0 + r, M - 1);
        const bf16_t* xr = logits + row * ldx;
#pragma unroll
        for (int i = 0; i < CE_MAXV; ++i) lraw[r][i] = *reinterpret_cast<const unsigned*>(xr + min(2 * (lane + 64 * i), ldx - 2));
        if constexpr (GT) {
            ce_gt_pairs(idx, val, K, p_sb, p_sn, row, mix_batches, mix_lam, smoothing, C, lane, my_i[r], my_v[r]);
        } else {
            const int64_t b = row / rows_per_batch, n = row - b * rows_per_batch;
            const bool other = lane >= K;                                // (mix) the partner image's pairs
            const int64_t po = ((mix_batches > 0 && other) ? (int64_t)(mix_batches - 1) - b : b) * p_sb + n * p_sn + (other ? lane - K : lane);
            const float wgt = mix_batches > 0 ? (other ? 1.0f - mix_lam : mix_lam) : 1.0f;
            my_i[r] = lane < KK ? idx[po] : -1;                          // lane k holds pair k of the row
            my_v[r] = lane < KK ? val[po] * wgt * (1.0f - smoothing) : 0.f;
        }
    }
    const float base = smoothing / (float)C;
#pragma unroll
    for (int r = 0; r < SR; ++r) {
        const int64_t row = row0 + r;
        if (row >= M) break;
        float xv[CE_MAXV][2], tv[CE_MAXV][2];
        float mx = -3.0e38f;
#pragma unroll
        for (int i = 0; i < CE_MAXV; ++i) {
            const int c = 2 * (lane + 64 * i);
            xv[i][0] = c < C ? bf_lo(lraw[r][i]) : -3.0e38f;
            xv[i][1] = c + 1 < C ? bf_hi(lraw[r][i]) : -3.0e38f;
            tv[i][0] = c < C ? base : 0.f;
            tv[i][1] = c + 1 < C ? base : 0.f;
            mx = fmaxf(mx, fmaxf(xv[i][0], xv[i][1]));
        }
        // the K pairs are wave-uniform once read with v_readlane: class ci = 2 * (owner + 64 * slot) + (ci & 1) lives in ONE lane
        for (int k = 0; k < KK; ++k) {
            const int ci = __builtin_amdgcn_readlane(my_i[r], k);
            const float cv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_v[r]), k));
            if (ci < 0 || ci >= C) continue;
            const int owner = (ci >> 1) & 63, slot = ci >> 7, odd = ci & 1;
            const float add = lane == owner ? cv : 0.f;
#pragma unroll
            for (int i = 0; i < CE_MAXV; ++i) { tv[i][0] += (i == slot && !odd) ? add : 0.f; tv[i][1] += (i == slot && odd) ? add : 0.f; }
        }
        mx = group_max<64>(mx);
        float se = 0.f, st = 0.f, stx = 0.f;
#pragma unroll
        for (int i = 0; i < CE_MAXV; ++i)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (2 * (lane + 64 * i) + k < C) {
                    se += __expf(xv[i][k] - mx);
                    st += tv[i][k];
                    stx += tv[i][k] * xv[i][k];
                }
            }
        se = group_sum<64>(se); st = group_sum<64>(st); stx = group_sum<64>(stx);
        const float lse = mx + __logf(se);
        if (lane == 0) row_loss[row] = lse * st - stx;
        bf16_t* dr = dlogits + row * ldx;
#pragma unroll
        for (int i = 0; i < CE_MAXV; ++i) {
            const int c = 2 * (lane + 64 * i);
            if (c < ldx) {
                float d0 = 0.f, d1 = 0.f;
                if (c < C) d0 = gscale * (__expf(xv[i][0] - lse) * st - tv[i][0]);
                if (c + 1 < C) d1 = gscale * (__expf(xv[i][1] - lse) * st - tv[i][1]);
                *reinterpret_cast<unsigned*>(dr + c) = pack_bf2(d0, d1);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- rows wider than 1024
// ldx > 64 * 2 * CE_MAXV: a row no longer fits one wave's registers (21 843 classes: 43.7 KB of bf16).  The row is staged in LDS ONCE
// by the walk of row_wide.h (its teams, its rules) and every later walk reads LDS: logits once in, gradient once out, whatever the caches
// do.  Three walks: maximum (while staging), sums, gradient -- the exact max-then-sum order of the narrow kernels, no running rescale.
//   WPR = 1 (ldx <= RW_TEAM1_MAXLD): four rows per workgroup, 4 * ldx * 2 B of LDS (<= 32 KB);
//   WPR = 4: one row per workgroup, ldx * 2 B of LDS -- three workgroups per CU at 21 848 columns, one at RW_MAXLD = 65 536.
// Plain grid, one workgroup per row group; two barriers per workgroup.  The wave reductions stay the xor butterflies of the narrow
// kernels (group_max / group_sum: the DPP tree adds in another order).  Padding columns C .. ldx-1 of the logits reach LDS and
// registers but are replaced by a select before any use; their gradient is stored as zeros with the last chunks of the row.
//   SPARSE: a lane owns the 8 classes of a 16-byte chunk (16-byte stores).  The pairs sit one per lane (as in k_soft_ce_sparse);
//     sum t = s + sum_k v_k and sum t x = (s / C) sum x + sum_k v_k x[i_k] need no scan, and in the gradient walk a wave's 64 chunks
//     are one 512-class window: one ballot per window finds the pairs inside it, and each of those lands in ONE (lane, element).
//   DENSE: a lane owns a class pair (the 4-byte mapping of k_soft_ce) and reads its two target values straight from global memory
//     through (t_sb, t_sc, t_sn) -- any strides, coalesced when the target is row-major [M, C] (t_sc = 1: timm's Mixup target).  The
//     target is walked twice (sums, gradient): 8 B per class of one row, the second walk comes from L2.  The class-major token-label
//     tensor (t_sn = 1) is correct here and uncoalesced; it takes k_soft_ce_wide_cm below where its token tile fits LDS.
// the dense target of class pairs g = tt, tt + T, .. < ngr, four pairs per lane in flight, the next batch requested before f(g, t0, t1)
// runs on the previous one.  mixed: t = lam1 * t[b] + lam2 * t[B-1-b] (one wave-uniform branch per batch)
template <int T, class F>
__device__ __forceinline__ void ce_wide_walk_target(const float* __restrict__ tb, const float* __restrict__ tb2, bool mixed, float lam1, float lam2,
                                                    int64_t t_sc, int C, int ngr, int tt, F&& f) {
    constexpr int U = 4;
    float cur[U][2], nxt[U][2];
    auto load = [&](float (&o)[U][2], int base) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = 2 * (base + tt + T * u);
            const int64_t o0 = (int64_t)min(c, C - 1) * t_sc, o1 = (int64_t)min(c + 1, C - 1) * t_sc;
            o[u][0] = tb[o0];
            o[u][1] = tb[o1];
        }
        if (mixed) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = 2 * (base + tt + T * u);
                const int64_t o0 = (int64_t)min(c, C - 1) * t_sc, o1 = (int64_t)min(c + 1, C - 1) * t_sc;
                o[u][0] = lam1 * o[u][0] + lam2 * tb2[o0];
                o[u][1] = lam1 * o[u][1] + lam2 * tb2[o1];
            }
        }
    };
    load(cur, 0);
    for (int base = 0; base < ngr; base += U * T) {
        const bool more = base + U * T < ngr;
        if (more) load(nxt, base + U * T);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int g = base + tt + T * u;
            if (g < ngr) f(g, cur[u][0], cur[u][1]);
        }
        if (more) {
#pragma unroll
            for (int u = 0; u < U; ++u) { cur[u][0] = nxt[u][0]; cur[u][1] = nxt[u][1]; }
        }
    }
}

//   GT (SPARSE only): the class row of TokenLabelGTCrossEntropy -- the pairs and their weights come from ce_gt_pairs (up to 32 lanes), p_sn
//     carries the offset from slot 1 to slot 0 and rows_per_batch is 1; everything behind the prologue is the SPARSE row body.
template <int WPR, bool DENSE, bool GT = false>
__global__ void __launch_bounds__(256)
k_soft_ce_wide(const bf16_t* __restrict__ logits, int ldx, const float* __restrict__ target, int64_t t_sb, int64_t t_sc, int64_t t_sn,
               const int* __restrict__ idx, const float* __restrict__ val, int K, int64_t p_sb, int64_t p_sn, float smoothing,
               int rows_per_batch, float* __restrict__ row_loss, bf16_t* __restrict__ dlogits, float gscale, int64_t M, int C,
               float mix_lam, int mix_batches, const float* __restrict__ lam_dev) {
    static_assert(!(GT && DENSE), "the GT class rows exist on the sparse target only");
    if (lam_dev) mix_lam = lam_dev[0];
    extern __shared__ __attribute__((aligned(16))) u32x4 ce_wide_rows[];       // [4 / WPR][ldx / 8]
    __shared__ float red_mx[4], red_a[4], red_b[4], red_c[4];
    constexpr int T = 64 * WPR;
    const RwTeam g = rw_team<WPR>(M);
    const int wave = g.wave, lane = g.lane, team = g.team, tw = g.tw, tt = g.tt;
    const bool live = g.live;
    const int64_t row = g.row;
    const int nch = ldx >> 3;
    u32x4* xs = ce_wide_rows + (size_t)team * nch;
    const int64_t b = row / rows_per_batch, n = row - b * rows_per_batch;
    const bool mixed = mix_batches > 0;
    // SPARSE: lane k holds pair k of the row (lanes K .. 2K-1: the partner image's, weighted 1 - lam); a pair outside [0, C) is dropped here
    int my_i = -1;
    float my_v = 0.f;
    if constexpr (GT) {
        ce_gt_pairs(idx, val, K, p_sb, p_sn, row, mix_batches, mix_lam, smoothing, C, lane, my_i, my_v);
    } else if (!DENSE) {
        const int KK = mixed ? 2 * K : K;
        const bool other = lane >= K;
        const int64_t po = ((mixed && other) ? (int64_t)(mix_batches - 1) - b : b) * p_sb + n * p_sn + (other ? lane - K : lane);
        const float wgt = mixed ? (other ? 1.0f - mix_lam : mix_lam) : 1.0f;
        if (lane < KK) { my_i = idx[po]; my_v = val[po] * wgt * (1.0f - smoothing); }
        if (my_i < 0 || my_i >= C) { my_i = -1; my_v = 0.f; }
    }
    // ---- walk 1: global -> LDS, the maximum on the way
    float mx = -3.0e38f;
    rw_stage<T>(reinterpret_cast<const u32x4*>(logits + row * ldx), nch, tt, [&](int q, const u32x4& v) {
        xs[q] = v;
        float f[8];
        unpack8(v, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) mx = fmaxf(mx, 8 * q + j < C ? f[j] : -3.0e38f);
    });
    mx = group_max<64>(mx);
    if (lane == 0) red_mx[wave] = mx;
    __syncthreads();
    mx = red_mx[team * WPR];
#pragma unroll
    for (int w = 1; w < WPR; ++w) mx = fmaxf(mx, red_mx[team * WPR + w]);
    // ---- walk 2: sum exp, sum t, sum t x
    const float* tb = DENSE ? target + b * t_sb + n * t_sn : nullptr;
    const float* tb2 = (DENSE && mixed) ? target + (int64_t)(mix_batches - 1 - b) * t_sb + n * t_sn : tb;
    const float lam1 = mix_lam, lam2 = 1.0f - mix_lam;
    const unsigned* xw = reinterpret_cast<const unsigned*>(xs);
    float se = 0.f, st = 0.f, stx = 0.f;
    if (DENSE) {
        ce_wide_walk_target<T>(tb, tb2, mixed, lam1, lam2, t_sc, C, (C + 1) >> 1, tt, [&](int p, float t0, float t1) {
            const unsigned w = xw[p];
            const float x0 = bf_lo(w), x1 = bf_hi(w);
            se += __expf(x0 - mx); st += t0; stx += t0 * x0;                      // 2 p < C always
            if (2 * p + 1 < C) { se += __expf(x1 - mx); st += t1; stx += t1 * x1; }
        });
    } else {
        float sx = 0.f;
#pragma unroll 2
        for (int q = tt; q < nch; q += T) {
            float f[8];
            unpack8(xs[q], f);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (8 * q + j < C) { se += __expf(f[j] - mx); sx += f[j]; }
        }
        st = sx;                                                                  // (reduced below; scaled after)
    }
    se = group_sum<64>(se); st = group_sum<64>(st); stx = group_sum<64>(stx);
    if (lane == 0) { red_a[wave] = se; red_b[wave] = st; red_c[wave] = stx; }
    __syncthreads();
    se = red_a[team * WPR]; st = red_b[team * WPR]; stx = red_c[team * WPR];
#pragma unroll
    for (int w = 1; w < WPR; ++w) { se += red_a[team * WPR + w]; st += red_b[team * WPR + w]; stx += red_c[team * WPR + w]; }
    const float base = smoothing / (float)C;
    if (!DENSE) {
        // t = base + the pairs: sum t = C base + sum_k v_k,  sum t x = base sum x + sum_k v_k x[i_k]  (every wave of the team, same values)
        const float xk = bf2f(reinterpret_cast<const bf16_t*>(xs)[max(my_i, 0)]);
        const float pst = group_sum<64>(my_v), pstx = group_sum<64>(my_i >= 0 ? my_v * xk : 0.f);
        stx = base * st + pstx;
        st = base * (float)C + pst;
    }
    const float lse = mx + __logf(se);
    if (live && tt == 0) row_loss[row] = lse * st - stx;
    // ---- walk 3: the gradient, columns C .. ldx-1 as zeros
    bf16_t* dr = dlogits + row * ldx;
    if (DENSE) {
        ce_wide_walk_target<T>(tb, tb2, mixed, lam1, lam2, t_sc, C, ldx >> 1, tt, [&](int p, float t0, float t1) {
            const unsigned w = xw[p];
            const int c = 2 * p;
            float d0 = 0.f, d1 = 0.f;
            if (c < C) d0 = gscale * (__expf(bf_lo(w) - lse) * st - t0);
            if (c + 1 < C) d1 = gscale * (__expf(bf_hi(w) - lse) * st - t1);
            if (live) *reinterpret_cast<unsigned*>(dr + c) = pack_bf2(d0, d1);
        });
    } else {
        const int my_win = my_i >= 0 ? my_i >> 9 : -1;
        for (int q0 = 0; q0 < nch; q0 += T) {
            const int q = q0 + tt;
            float tv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) tv[j] = base;
            // this wave's 64 chunks are classes [512 win, 512 win + 512); the pairs are wave-uniform once read with v_readlane
            unsigned long long hits = __ballot(my_win == (q0 >> 6) + tw);
            while (hits) {
                const int k = __builtin_ctzll(hits);
                hits &= hits - 1;
                const int ci = __builtin_amdgcn_readlane(my_i, k);
                const float cv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_v), k));
                const float add = lane == ((ci >> 3) & 63) ? cv : 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) tv[j] += (j == (ci & 7)) ? add : 0.f;
            }
            if (q < nch) {
                float f[8], d[8];
                unpack8(xs[q], f);
#pragma unroll
                for (int j = 0; j < 8; ++j) d[j] = 8 * q + j < C ? gscale * (__expf(f[j] - lse) * st - tv[j]) : 0.f;
                if (live) st16_nt(dr + 8 * q, pack8(d));
            }
        }
    }
}

// The class-major token-label tensor [B, C, 2 + N] (t_sn = 1) at 1024 < ldx <= 128 * MAXV: k_soft_ce's own structure with more class
// pairs per lane (k_soft_ce itself stays as it is, bit for bit, for the rows it takes).  The 16-token target tile is transposed
// through LDS -- 16 * (C | 1) * 4 B, which is what bounds this form: 70 KB at 1100 classes (two workgroups per CU), 160 KB at
// CE_WIDE_CM_MAXC -- and a wave keeps its four logits rows in registers (MAXV words each).  Wider class-major targets take
// k_soft_ce_wide through their strides.
#define CE_WIDE_CM_MAXC 2559
template <int MAXV>
__global__ void __launch_bounds__(256)
k_soft_ce_wide_cm(const bf16_t* __restrict__ logits, int ldx, const float* __restrict__ target, int64_t t_sb, int64_t t_sc,
                  int64_t t_sn, int rows_per_batch, float* __restrict__ row_loss, bf16_t* __restrict__ dlogits,
                  float gscale, int64_t M, int C, int tiles_per_batch, float mix_lam, int mix_batches, const float* __restrict__ lam_dev) {
    if (lam_dev) mix_lam = lam_dev[0];
    extern __shared__ __attribute__((aligned(16))) float ce_cm_tile[];      // [CE_TN][Cp] Cp odd
    const int Cp = C | 1;
    const int64_t b = blockIdx.x / tiles_per_batch;
    const int n0 = (blockIdx.x % tiles_per_batch) * CE_TN;
    const int ntok = min(CE_TN, rows_per_batch - n0);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // the logits of this wave's (up to) four rows first: their latency hides behind phase A (clamped, unconditional 4-byte loads)
    unsigned lraw[CE_TN / 4][MAXV];
#pragma unroll
    for (int r = 0; r < CE_TN / 4; ++r) {
        const int64_t rowc = min(b * rows_per_batch + n0 + min(wave + 4 * r, ntok - 1), M - 1);
        const bf16_t* xr = logits + rowc * ldx;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) lraw[r][i] = *reinterpret_cast<const unsigned*>(xr + min(2 * (lane + 64 * i), ldx - 2));
    }
    // ---- phase A: target tile -> LDS (token-major), 32 independent loads in flight per thread
    {
        const int tn = threadIdx.x & (CE_TN - 1), cl = threadIdx.x / CE_TN;
        const int tnc = min(tn, ntok - 1);
        const bool mixed = mix_batches > 0;
        const float* tb = target + b * t_sb + (int64_t)(n0 + tnc) * t_sn;
        const float* tb2 = mixed ? target + (int64_t)(mix_batches - 1 - b) * t_sb + (int64_t)(n0 + tnc) * t_sn : tb;
        const float lam2 = mixed ? 1.0f - mix_lam : 0.f, lam1 = mixed ? mix_lam : 1.0f;
        constexpr int CSTEP = 256 / CE_TN, INFLIGHT = 32;
        for (int c0 = cl; c0 < C; c0 += INFLIGHT * CSTEP) {
            float v[INFLIGHT], v2[INFLIGHT];
#pragma unroll
            for (int u = 0; u < INFLIGHT; ++u) v[u] = tb[(int64_t)min(c0 + u * CSTEP, C - 1) * t_sc];
            if (mixed) {
#pragma unroll
                for (int u = 0; u < INFLIGHT; ++u) v2[u] = tb2[(int64_t)min(c0 + u * CSTEP, C - 1) * t_sc];
            } else {
#pragma unroll
                for (int u = 0; u < INFLIGHT; ++u) v2[u] = 0.f;
            }
#pragma unroll
            for (int u = 0; u < INFLIGHT; ++u) {
                const int c = c0 + u * CSTEP;
                if (tn < ntok && c < C) ce_cm_tile[tn * Cp + c] = lam1 * v[u] + lam2 * v2[u];
            }
        }
    }
    __syncthreads();
    // ---- phase B
#pragma unroll
    for (int r = 0; r < CE_TN / 4; ++r) {
        const int tn = wave + 4 * r;
        const int64_t row = b * rows_per_batch + n0 + tn;
        if (tn >= ntok || row >= M) break;
        const float* tr = ce_cm_tile + tn * Cp;
        float mx = -3.0e38f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = 2 * (lane + 64 * i);
            mx = fmaxf(mx, fmaxf(c < C ? bf_lo(lraw[r][i]) : -3.0e38f, c + 1 < C ? bf_hi(lraw[r][i]) : -3.0e38f));
        }
        mx = group_max<64>(mx);
        float se = 0.f, st = 0.f, stx = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = 2 * (lane + 64 * i);
            if (c < C) { const float x = bf_lo(lraw[r][i]), t = tr[c]; se += __expf(x - mx); st += t; stx += t * x; }
            if (c + 1 < C) { const float x = bf_hi(lraw[r][i]), t = tr[c + 1]; se += __expf(x - mx); st += t; stx += t * x; }
        }
        se = group_sum<64>(se); st = group_sum<64>(st); stx = group_sum<64>(stx);
        const float lse = mx + __logf(se);
        if (lane == 0) row_loss[row] = lse * st - stx;
        bf16_t* dr = dlogits + row * ldx;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = 2 * (lane + 64 * i);
            if (c < ldx) {      // ldx is even: pairs never straddle the row end
                float d0 = 0.f, d1 = 0.f;
                if (c < C) d0 = gscale * (__expf(bf_lo(lraw[r][i]) - lse) * st - tr[c]);
                if (c + 1 < C) d1 = gscale * (__expf(bf_hi(lraw[r][i]) - lse) * st - tr[c + 1]);
                *reinterpret_cast<unsigned*>(dr + c) = pack_bf2(d0, d1);
            }
        }
    }
}

// loss = wa * sum(a[0:na]) + wb * sum(b[0:nb]) in one workgroup (the two CE terms of the token-label loss, loss/cross_entropy.py:154-156)
__global__ void __launch_bounds__(1024)
k_loss_combine(const float* __restrict__ a, int64_t na, float wa, const float* __restrict__ b, int64_t nb, float wb, float* __restrict__ out) {
    __shared__ float red[16];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < na; i += 1024) s += wa * a[i];
    for (int64_t i = threadIdx.x; i < nb; i += 1024) s += wb * b[i];
    s = group_sum<64>(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) t += red[w];
        out[0] = t;
    }
}

extern "C" int ap_loss_combine(const float* a, int64_t na, float wa, const float* b, int64_t nb, float wb, float* out, ap_stream_t stream) {
    if (!a || !out || (nb > 0 && !b)) return AP_ERR_NULL;
    if (na < 0 || nb < 0) return AP_ERR_SHAPE;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_loss_combine, dim3(1), dim3(1024), 0, (hipStream_t)stream, a, na, wa, b, nb, wb, out);
    return ap_check_launch();
}

// rows wider than the register kernels take: k_soft_ce_wide, a team of one wave per row up to RW_TEAM1_MAXLD columns and of four beyond
template <bool DENSE, bool GT = false>
static int ce_wide_launch(const ap_bf16* logits, int ldx, const float* target, int64_t t_sb, int64_t t_sc, int64_t t_sn, const int* idx, const float* val,
                          int K, int64_t p_sb, int64_t p_sn, float smoothing, int rows_per_batch, float* row_loss, ap_bf16* dlogits, float grad_scale,
                          int64_t M, int C, float mix_lam, int mix_batches, const float* mix_lam_dev, ap_stream_t stream) {
    if (ldx > RW_MAXLD) return AP_ERR_UNSUPPORTED;
    if (((uintptr_t)logits | (uintptr_t)dlogits) & 15) return AP_ERR_SHAPE;       // rows are moved in 16-byte chunks
    if (M == 0) return AP_OK;
    return rw_launch(ldx, M, [&](auto wpr, unsigned blocks) {
        constexpr int WPR = decltype(wpr)::value;
        const size_t lds = (size_t)(4 / WPR) * ldx * sizeof(bf16_t);
        if constexpr (WPR == 4) {                                                // (four rows of a one-wave team are 32 KB at the most)
            if (const int rc = ap_allow_lds<k_soft_ce_wide<4, DENSE, GT>>(RW_MAXLD * (int)sizeof(bf16_t)); rc != AP_OK) return rc;
        }
        (void)hipGetLastError();
        hipLaunchKernelGGL((k_soft_ce_wide<WPR, DENSE, GT>), dim3(blocks), dim3(256), lds, (hipStream_t)stream, logits, ldx, target, t_sb, t_sc, t_sn, idx, val, K,
                           p_sb, p_sn, smoothing, rows_per_batch, row_loss, dlogits, grad_scale, M, C, mix_lam, mix_batches, mix_lam_dev);
        return ap_check_launch();
    });
}

// the class-major token-label tensor while its 16-token tile fits LDS: 12 or 20 class pairs per lane
static int ce_wide_cm_launch(const ap_bf16* logits, int ldx, const float* target, int64_t t_sb, int64_t t_sc, int64_t t_sn, int rows_per_batch,
                             float* row_loss, ap_bf16* dlogits, float grad_scale, int64_t M, int C, float mix_lam, int mix_batches,
                             const float* mix_lam_dev, ap_stream_t stream) {
    if (M == 0) return AP_OK;
    const int tiles = (rows_per_batch + CE_TN - 1) / CE_TN;
    const int64_t blocks = (M / rows_per_batch) * tiles;
    if (blocks > 0x7fffffffLL) return AP_ERR_SHAPE;
    const size_t lds = (size_t)CE_TN * (C | 1) * sizeof(float);
    (void)hipGetLastError();
    if (const int rc = ldx <= 128 * 12 ? ap_allow_lds<k_soft_ce_wide_cm<12>>(160 * 1024) : ap_allow_lds<k_soft_ce_wide_cm<20>>(160 * 1024); rc != AP_OK) return rc;
    if (ldx <= 128 * 12)
        hipLaunchKernelGGL(k_soft_ce_wide_cm<12>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, logits, ldx, target, t_sb, t_sc, t_sn, rows_per_batch,
                           row_loss, dlogits, grad_scale, M, C, tiles, mix_lam, mix_batches, mix_lam_dev);
    else
        hipLaunchKernelGGL(k_soft_ce_wide_cm<20>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, logits, ldx, target, t_sb, t_sc, t_sn, rows_per_batch,
                           row_loss, dlogits, grad_scale, M, C, tiles, mix_lam, mix_batches, mix_lam_dev);
    return ap_check_launch();
}

extern "C" int ap_soft_ce_fwd_bwd(const ap_bf16* logits, int ldx, const float* target, int64_t t_sb, int64_t t_sc,
                                  int64_t t_sn, int rows_per_batch, float* row_loss, ap_bf16* dlogits,
                                  float grad_scale, int64_t M, int C, float mix_lam, int mix_batches, ap_stream_t stream) {
    return ap_soft_ce_fwd_bwd_dev(logits, ldx, target, t_sb, t_sc, t_sn, rows_per_batch, row_loss, dlogits, grad_scale, M, C, mix_lam, mix_batches, nullptr, stream);
}

extern "C" int ap_soft_ce_fwd_bwd_dev(const ap_bf16* logits, int ldx, const float* target, int64_t t_sb, int64_t t_sc,
                                      int64_t t_sn, int rows_per_batch, float* row_loss, ap_bf16* dlogits,
                                      float grad_scale, int64_t M, int C, float mix_lam, int mix_batches, const float* mix_lam_dev, ap_stream_t stream) {
    if (!logits || !target || !row_loss || !dlogits) return AP_ERR_NULL;
    if (mix_batches != 0 && (mix_batches < 0 || (int64_t)mix_batches * rows_per_batch != M)) return AP_ERR_SHAPE;
    if (C <= 0 || ldx < C || (ldx & 7) || rows_per_batch <= 0 || M < 0 || M % rows_per_batch) return AP_ERR_SHAPE;
    if (ldx > 64 * 2 * CE_MAXV && t_sn == 1 && rows_per_batch > 1 && C <= CE_WIDE_CM_MAXC && ldx <= 128 * 20)
        return ce_wide_cm_launch(logits, ldx, target, t_sb, t_sc, t_sn, rows_per_batch, row_loss, dlogits, grad_scale, M, C, mix_lam, mix_batches, mix_lam_dev, stream);
    if (ldx > 64 * 2 * CE_MAXV)
        return ce_wide_launch<true>(logits, ldx, target, t_sb, t_sc, t_sn, nullptr, nullptr, 0, 0, 0, 0.f, rows_per_batch, row_loss, dlogits, grad_scale, M, C,
                                    mix_lam, mix_batches, mix_lam_dev, stream);
    if (M == 0) return AP_OK;
    const int tiles = (rows_per_batch + CE_TN - 1) / CE_TN;
    const int64_t blocks = (M / rows_per_batch) * tiles;
    if (blocks > 0x7fffffffLL) return AP_ERR_SHAPE;
    const size_t lds = (size_t)CE_TN * (C | 1) * sizeof(float);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_soft_ce, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, logits, ldx, target, t_sb, t_sc,
                       t_sn, rows_per_batch, row_loss, dlogits, grad_scale, M, C, tiles, mix_lam, mix_batches, mix_lam_dev);
    return ap_check_launch();
}

extern "C" int ap_soft_ce_sparse_fwd_bwd(const ap_bf16* logits, int ldx, const int* idx, const float* val, int K, int64_t p_sb, int64_t p_sn,
                                         int rows_per_batch, float smoothing, float* row_loss, ap_bf16* dlogits, float grad_scale,
                                         int64_t M, int C, float mix_lam, int mix_batches, ap_stream_t stream) {
    return ap_soft_ce_sparse_fwd_bwd_dev(logits, ldx, idx, val, K, p_sb, p_sn, rows_per_batch, smoothing, row_loss, dlogits, grad_scale, M, C, mix_lam, mix_batches,
                                         nullptr, stream);
}

extern "C" int ap_soft_ce_sparse_fwd_bwd_dev(const ap_bf16* logits, int ldx, const int* idx, const float* val, int K, int64_t p_sb, int64_t p_sn,
                                             int rows_per_batch, float smoothing, float* row_loss, ap_bf16* dlogits, float grad_scale,
                                             int64_t M, int C, float mix_lam, int mix_batches, const float* mix_lam_dev, ap_stream_t stream) {
    if (!logits || !idx || !val || !row_loss || !dlogits) return AP_ERR_NULL;
    if (C <= 0 || ldx < C || (ldx & 7) || rows_per_batch <= 0 || M < 0 || K <= 0 || K > CE_MAXK || smoothing < 0.f || smoothing >= 1.f) return AP_ERR_SHAPE;
    if (mix_batches != 0 && (mix_batches < 0 || (int64_t)mix_batches * rows_per_batch != M || 2 * K > CE_MAXK)) return AP_ERR_SHAPE;
    if (ldx > 64 * 2 * CE_MAXV)
        return ce_wide_launch<false>(logits, ldx, nullptr, 0, 0, 0, idx, val, K, p_sb, p_sn, smoothing, rows_per_batch, row_loss, dlogits, grad_scale, M, C,
                                     mix_lam, mix_batches, mix_lam_dev, stream);
    if (M == 0) return AP_OK;
    if ((M + 4 * CE_SR - 1) / (4 * CE_SR) > 0x7fffffffLL) return AP_ERR_SHAPE;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_soft_ce_sparse<false>, dim3((unsigned)((M + 4 * CE_SR - 1) / (4 * CE_SR))), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const bf16_t*>(logits), ldx,
                       idx, val, K, p_sb, p_sn, rows_per_batch, smoothing, row_loss, reinterpret_cast<bf16_t*>(dlogits), grad_scale, M, C, mix_lam, mix_batches, mix_lam_dev);
    return ap_check_launch();
}

// the class rows of TokenLabelGTCrossEntropy: B rows, one per image (include/autoprog_hip.h)
extern "C" int ap_soft_ce_sparse_gt_fwd_bwd(const ap_bf16* logits, int ldx, const int* idx, const float* val, int K, int64_t p_sb, int64_t p_s0, int64_t p_s1,
                                            float smoothing, float* row_loss, ap_bf16* dlogits, float grad_scale, int64_t B, int C, float mix_lam,
                                            int mix_batches, const float* mix_lam_dev, ap_stream_t stream) {
    if (!logits || !idx || !val || !row_loss || !dlogits) return AP_ERR_NULL;
    if (C <= 0 || ldx < C || (ldx & 7) || B < 0 || K <= 0 || K > CE_GT_MAXK || smoothing < 0.f || smoothing >= 1.f) return AP_ERR_SHAPE;
    if (mix_batches != 0 && (mix_batches < 0 || (int64_t)mix_batches != B)) return AP_ERR_SHAPE;
    // the kernels address slot 1 as the base and slot 0 relative to it (their p_sn; one row per image)
    if (ldx > 64 * 2 * CE_MAXV)
        return ce_wide_launch<false, true>(logits, ldx, nullptr, 0, 0, 0, idx + p_s1, val + p_s1, K, p_sb, p_s0 - p_s1, smoothing, 1, row_loss, dlogits, grad_scale,
                                           B, C, mix_lam, mix_batches, mix_lam_dev, stream);
    if (B == 0) return AP_OK;
    if ((B + 3) / 4 > 0x7fffffffLL) return AP_ERR_SHAPE;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_soft_ce_sparse<true>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const bf16_t*>(logits), ldx,
                       idx + p_s1, val + p_s1, K, p_sb, p_s0 - p_s1, 1, smoothing, row_loss, reinterpret_cast<bf16_t*>(dlogits), grad_scale, B, C, mix_lam, mix_batches,
                       mix_lam_dev);
    return ap_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------- validation statistics
// ap_classify_stats: cross entropy against a hard label and the rank of the label's logit, one wave per row (lanes stride over the classes: coalesced
// 2-byte loads, any ld), xor-butterfly reductions, every lane ends with the full sums (bit-equal across lanes) and lane 0 stores.  The row is read
// twice (maximum + rank, then the exponentials): 2 KB that stay in the cache -- a validation pass launches this once per batch.
__global__ void __launch_bounds__(256)
k_classify_stats(const bf16_t* __restrict__ logits, int ld, int C, const int64_t* __restrict__ labels, float* __restrict__ loss,
                 int* __restrict__ rank, int64_t rows) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                              // (whole waves; no barrier in this kernel)
    const int64_t lab = labels[row];
    if (lab < 0 || lab >= C) {                            // padding: nothing is read through the label
        if (lane == 0) { loss[row] = 0.f; rank[row] = -1; }
        return;
    }
    const bf16_t* z = logits + row * ld;
    const float zl = bf2f(z[lab]);
    float mx = -3.0e38f;
    int above = 0;
    for (int c = lane; c < C; c += 64) {
        const float v = bf2f(z[c]);
        mx = fmaxf(mx, v);
        above += v > zl ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        above += __shfl_xor(above, o, 64);
    }
    float se = 0.f;
    for (int c = lane; c < C; c += 64) se += expf(bf2f(z[c]) - mx);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o, 64);
    if (lane == 0) { loss[row] = (mx - zl) + logf(se); rank[row] = above; }
}

extern "C" int ap_classify_stats(const ap_bf16* logits, int ld, int n_classes, const int64_t* labels, float* loss, int* rank, int64_t rows,
                                 ap_stream_t stream) {
    if (rows < 0 || n_classes <= 0 || ld < n_classes) return AP_ERR_SHAPE;
    if (rows == 0) return AP_OK;
    if (!logits || !labels || !loss || !rank) return AP_ERR_NULL;
    if ((rows + 3) / 4 > 0x7fffffffLL) return AP_ERR_SHAPE;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_classify_stats, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const bf16_t*>(logits), ld, n_classes, labels, loss, rank, rows);
    return ap_check_launch();
}
