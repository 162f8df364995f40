// bf16 MFMA GEMMs for the Linear layers of the VOLO/DeiT hot path (models/volo.py:67,68,71,
// 156,158,180,182,253,256,258,547,553 and their autograd backward).
//
//   ap_gemm_nt     C[M,N]  = epi(A[M,K] . B[N,K]^T)      forward (B = weight) and input-gradient
//                                                        (B = pre-transposed weight) GEMMs
//   ap_gemm_tn_acc C[N1,N2] += A[M,N1]^T . B[M,N2]       weight gradients, fp32 accumulate
//
// Both use v_mfma_f32_16x16x32_bf16 (lane maps pinned on hardware by tools/probe, profiles/
// r01_hw_probe.txt): A operand lane l holds A[row l&15][k 8*(l>>4)+j], B operand B[k][col l&15],
// accumulator D[row 4*(l>>4)+r][col l&15].
//
// gemm_nt: 128x128x64 tile, 4 waves (2x2) x 64x64 per wave.  Operands are staged global ->
// registers -> LDS (16-byte chunks) with the 16-B chunk index XORed by (row&7): ds_write_b128 of a
// row and ds_read_b128 of an MFMA fragment are both bank-conflict free.  The MFMA is issued as
// D = W_frag (A operand) x X_frag (B operand) so that a lane ends with 4 CONSECUTIVE output columns
// of one output row -> 8-byte bf16 stores and vector loads of bias / residual in the epilogue.
// The next K tile's global loads are issued before the MFMAs of the current one.
//
// gemm_tn: the reduction runs over the token axis, which is the SLOW axis of both operands, so
// fragments are fetched with ds_read_b64_tr_b16 (hardware transpose) from row-major [64 tok][128]
// LDS tiles; the chunk swizzle f(row) keeps those transposed reads conflict free.  The token range
// is split across blockIdx.z and partial tiles are added with fp32 atomics (few MB per call).
#include <mutex>
#include <algorithm>
#include <cstring>
#include "common.h"
#include <type_traits>
#include "gemm_epi.h"
#include "gemm8p.h"
#include "gemm_ws.h"
#include "gemm_tn8p.h"
#include "gemm_tn_fp8.h"
#include "nt_plan.h"
#include "tn_plan.h"
// (the measured-and-rejected kernels of rounds 1 and 2 -- LDS-DMA rings, persistent 256-row tiles, the ring weight-gradient kernel -- and
// their AP_GEMM_NT_P / _RING / _DMA, AP_GEMM_TN_RING switches live under tools/gemm_lab/rejected/, outside the product library)
#include <cstdlib>
#include <cstdio>

#ifndef AP_ABL
#define AP_ABL 0
#endif
#define SBM 128
#define SBN 128
#define SBK 64

// Register-staged multi-workgroup kernel, templated on the block tile TM x TN and the wave grid WGM x WGN
// (wave tile (TM/WGM) x (TN/WGN), BK = 64).  Variants are selected per shape by ap_gemm_nt.
// PRE = true: the instantiation used when the epilogue READS a second tile (residual, or the stored pre-activation of gelu'): that
// tile is prefetched under the last K step (see "epilogue input prefetch" below).  PRE = false is the plain kernel, unchanged.
// amdgpu_waves_per_eu: the PRE kernel keeps the register budget of the plain one (three workgroups of the 128x128 tile per CU);
// without the hint the scheduler spends a wave of occupancy on interleaving the erf evaluations of the epilogue chunks.
// PATCH = 1: the rows of A are patches of an NHWC feature map (PatchMap, gemm_epi.h); PATCH = 2: the rows of C are (the input gradient
// of such a patch convolution, written straight into the feature-map layout; plain epilogue only).
// FP8 = true: A and B hold OCP e4m3 bytes (configs[4] "mixed MFMA fp8 GEMM / bf16 accum" -> fp32 accumulate here).  The kernel is
// launched with K, lda, ldb counted in PAIRS of bytes, so staging, swizzle and addressing are the bf16 kernel's; a 16-byte fragment is
// 16 K positions = two v_mfma_f32_16x16x32_fp8_fp8 on its 8-byte halves (the same K set on both operands), and the accumulators are
// scaled by the two dequantisation factors in the epilogue.
template <int TM, int TN, int WGM, int WGN, bool DEPI = true, int PF = 1, bool PRE = false, int PATCH = 0, bool FP8 = false>
__global__ void __launch_bounds__(WGM * WGN * 64) __attribute__((amdgpu_waves_per_eu((PRE && TM * TN == 128 * 128 && WGM * WGN == 4) ? 3 : 1)))
k_gemm_nt(const bf16_t* __restrict__ A, int lda, const bf16_t* __restrict__ B, int ldb, bf16_t* __restrict__ C, int ldc,
          int M, int N, int K, int tiles_n, int ntiles, EpiArgs ep) {
    constexpr int NTH = WGM * WGN * 64;
    constexpr int MT = TM / WGM / 16, NT = TN / WGN / 16;
    constexpr int NA = TM * 8 / NTH, NB = TN * 8 / NTH;              // 16-B chunks per thread per K step
    constexpr int EROWS_RAW = ((TM + TN) * 32 / TN) / 16 * 16;        // rows of the fp32 staging tile that fit the LDS
    constexpr int EROWS = EROWS_RAW < TM ? EROWS_RAW : TM;
    constexpr int PASSES = (TM + EROWS - 1) / EROWS;
    static_assert(TM * 8 % NTH == 0 && TN * 8 % NTH == 0, "staging split");
    static_assert(PATCH != 2 || (!DEPI && !PRE), "patch-addressed C rows: staged plain epilogue only");
    static_assert((TM / WGM) % 16 == 0 && (TN / WGN) % 16 == 0, "wave tile");
    static_assert(EROWS >= 16 && EROWS % 16 == 0, "epilogue pass split");
    __shared__ __attribute__((aligned(16))) bf16_t smem_nt[(TM + TN) * SBK];       // A tile | B tile; reused by the epilogue
    bf16_t* sA = smem_nt;
    bf16_t* sB = smem_nt + TM * SBK;
    const int tile = xcd_remap(blockIdx.x, ntiles);
    const int m0 = (tile / tiles_n) * TM, n0 = (tile % tiles_n) * TN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int fr = lane & 15, g = lane >> 4;

    // staging assignment: rows (tid>>3) + (NTH/8)*i, chunk kc = tid&7
    const int srow = tid >> 3, kc = tid & 7;
    const bf16_t* ga[NA];
    const bf16_t* gb[NB];
    int soffa[NA], soffb[NB];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int r = srow + (NTH / 8) * i;
        ga[i] = A + (PATCH == 1 ? patch_row(ep.pm, min(m0 + r, M - 1)) : (int64_t)min(m0 + r, M - 1) * lda) + kc * 8;
        soffa[i] = r * SBK + ((kc ^ (r & 7)) << 3);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int r = srow + (NTH / 8) * i;
        gb[i] = B + (int64_t)min(n0 + r, N - 1) * ldb + kc * 8;
        soffb[i] = r * SBK + ((kc ^ (DEPI ? key_b(r) : key_a(r))) << 3);
    }
    // PF register sets: the global loads of the next PF K steps are in flight while one step is computed.  PF = 2 was tried on
    // the small tiles (K = 192..576, 3..9 steps) and LOST inside the training step (fc1+gelu of the outlooker 96 -> 111 us,
    // 192x576 plain 40.6 -> 45.3), and on the 128x128 tile (38.9 -> 64.6 us on the dfc1 shape): the extra 16-32 VGPRs cost a
    // wave (or two) per SIMD, and three co-resident workgroups already keep three K steps of loads in flight.  Default 1.
    u32x4 ra0[NA], rb0[NB], ra1[PF > 1 ? NA : 1], rb1[PF > 1 ? NB : 1];
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    // K % 64 == 0 (every Linear of the models except the 1000-class heads): unconditional loads.  The per-lane `ok ? load : 0`
    // of the ragged-K path compiles to one exec-masked branch block with 8 register zeroings per load pair.
    const bool kfull = (K & (SBK - 1)) == 0;
    auto gload = [&](u32x4* ra, u32x4* rb, int k0) {
        if (kfull) {
            const int ka = PATCH == 1 ? patch_col(ep.pm, k0) : k0;      // uniform: a 64-wide K step never straddles a kernel row
#pragma unroll
            for (int i = 0; i < NA; ++i) ra[i] = ld16(ga[i] + ka);
#pragma unroll
            for (int i = 0; i < NB; ++i) rb[i] = ld16(gb[i] + k0);
        } else {
            const bool ok = (k0 + kc * 8) < K;
#pragma unroll
            for (int i = 0; i < NA; ++i) ra[i] = ok ? ld16(ga[i] + k0) : zero4;
#pragma unroll
            for (int i = 0; i < NB; ++i) rb[i] = ok ? ld16(gb[i] + k0) : zero4;
        }
    };

    f32x4 acc[NT][MT];
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < MT; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // Epilogue input prefetch.  The residual tile (or the stored pre-activation of the gelu' epilogue) is TM x TN bf16 = NPRE
    // 16-byte chunks per thread, no more than the A/B staging registers hold -- and those are dead once the last K step has
    // been written to the LDS.  Loading the epilogue's input there, under the last step's MFMAs, takes its HBM latency out of
    // the epilogue (384x384 + residual: 32.7 us against 19.6 us plain before this, for 19 MB more traffic).  Full tiles only.
    constexpr int NPRE = TM * TN / 8 / NTH;
    constexpr int CPR_E = TN / 8;
    const bf16_t* emul = ep.dgelu_of ? ep.dgelu_of : ep.mul_by;          // the factor tile (gelu' input or stored derivative), else the residual
    const bf16_t* esrc = emul ? emul : ep.residual;
    const int elds = emul ? ldc : ep.ldr;
    // (the staged epilogue's (pass, iteration) -> chunk map is the row-major one only when a pass is a whole number of thread sweeps)
    // The chunks live in the staging registers themselves (chunk c in ra0[c] / rb0[c - NA]): no register beyond the main loop's.
    constexpr bool PFOK = PRE && !DEPI && PF == 1 && (NPRE <= NA + NB) && ((EROWS * (TN / 8)) % NTH == 0) && (TM % EROWS == 0) && (NTH % (TN / 8) == 0);
    static_assert(PFOK || !PRE, "PRE is instantiated only for tiles whose staged epilogue sweeps whole rows of chunks");
    const bool pf = PFOK && esrc != nullptr && (emul == nullptr || ep.residual == nullptr) && (ldc & 7) == 0 && (elds & 7) == 0 &&
                    m0 + TM <= M && n0 + TN <= N && !(ep.dbg & 2);
    auto pre = [&](int c) -> u32x4& { return c < NA ? ra0[c < NA ? c : 0] : rb0[c >= NA && c < NA + NB ? c - NA : 0]; };
    // addresses = one uniform tile base (+ a uniform per-chunk step) + ONE 32-bit per-thread offset: a single VGPR across the main loop
    auto eload = [&]() {
        // the row-major chunk order of the staged epilogue: chunk c of thread tid is (row tid / CPR_E + c * NTH / CPR_E, column chunk
        // tid % CPR_E) -- NTH % CPR_E == 0, a thread keeps its column chunk across the sweeps
        const bf16_t* tbase = esrc + (int64_t)m0 * elds + n0;
        const unsigned toff = (unsigned)((tid / CPR_E) * elds + 8 * (tid % CPR_E));
#pragma unroll
        for (int c = 0; c < NPRE; ++c) pre(c) = ld16(tbase + c * (NTH / CPR_E) * elds + toff);
    };

    // one K step: registers -> LDS, refill the same register set with step `refill_k`, MFMAs
    // (mode 0: a refill always follows; 1: the last step, the epilogue prefetch takes the refill's place; 2: decided at run time)
    // PATCH = 1 with ep.abn: this thread's chunk kc holds channels 8 kc .. + 7 of a 64-channel pixel in EVERY K step (a 64-deep step is one pixel)
    float bsc[PATCH == 1 ? 8 : 1], bsh[PATCH == 1 ? 8 : 1];
    bool a_bn = false;
    if constexpr (PATCH == 1) {
        a_bn = ep.abn.mean != nullptr;
        if (a_bn) bn_in_consts(ep.abn, kc * 8, bsc, bsh);
    }
    auto step = [&](u32x4* ra, u32x4* rb, int refill_k, auto mode) {
        if constexpr (PATCH == 1) {
            if (a_bn) {
#pragma unroll
                for (int i = 0; i < NA; ++i) ra[i] = bn_in_apply(ra[i], bsc, bsh);
            }
        }
#pragma unroll
        for (int i = 0; i < NA; ++i) st16(sA + soffa[i], ra[i]);
#pragma unroll
        for (int i = 0; i < NB; ++i) st16(sB + soffb[i], rb[i]);
        __syncthreads();
        if constexpr (mode.value == 0) gload(ra, rb, refill_k);
        else if constexpr (mode.value == 1) { if (pf) eload(); }
        else if (refill_k < K) gload(ra, rb, refill_k);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 xf[MT], wf[NT];
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                const int r = wm * (TM / WGM) + t * 16 + fr;
                xf[t] = as_bf16x8(ld16(sA + r * SBK + (((ks * 4 + g) ^ (r & 7)) << 3)));
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                // DEPI: fragment t of pair P = t>>1 holds weight rows 32P + 8q + 4(t&1) + p for MFMA row 4q + p, so a
                // lane's 4 + 4 accumulator registers of the pair are 8 CONSECUTIVE output columns
                const int r = DEPI ? wn * (TN / WGN) + 32 * (t >> 1) + 8 * (fr >> 2) + 4 * (t & 1) + (fr & 3)
                                   : wn * (TN / WGN) + t * 16 + fr;
                wf[t] = as_bf16x8(ld16(sB + r * SBK + (((ks * 4 + g) ^ (DEPI ? key_b(r) : key_a(r))) << 3)));
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    if constexpr (FP8) {
                        typedef __attribute__((ext_vector_type(2))) long l64x2;
                        const l64x2 wv = __builtin_bit_cast(l64x2, wf[nt]), xv = __builtin_bit_cast(l64x2, xf[mt]);
                        acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(wv[0], xv[0], acc[nt][mt], 0, 0, 0);
                        acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(wv[1], xv[1], acc[nt][mt], 0, 0, 0);
                    } else acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt], xf[mt], acc[nt][mt], 0, 0, 0);
                }
        }
        __syncthreads();
    };
    gload(ra0, rb0, 0);
    if constexpr (PF > 1) {
        if (SBK < K) gload(ra1, rb1, SBK);
        for (int k0 = 0; k0 < K; k0 += 2 * SBK) {
            step(ra0, rb0, k0 + 2 * SBK, std::integral_constant<int, 2>{});
            if (k0 + SBK < K) step(ra1, rb1, k0 + 3 * SBK, std::integral_constant<int, 2>{});
        }
    } else {
        if constexpr (PFOK) {
            for (int k0 = SBK; k0 < K; k0 += SBK) step(ra0, rb0, k0, std::integral_constant<int, 0>{});
            step(ra0, rb0, K, std::integral_constant<int, 1>{});
        } else {
            for (int k0 = 0; k0 < K; k0 += SBK) step(ra0, rb0, k0 + SBK, std::integral_constant<int, 2>{});
        }
    }
#if (AP_ABL & 128)
    if (ep.dbg & 1) {                     // ablation build only (AP_GEMM_DBG=1): main loop without the epilogue
        float sacc = 0.f;
#pragma unroll
        for (int a = 0; a < NT; ++a)
#pragma unroll
            for (int b = 0; b < MT; ++b) sacc += acc[a][b][0] + acc[a][b][1] + acc[a][b][2] + acc[a][b][3];
        if (sacc == 12345.678f) C[0] = 1;
        return;
    }
#endif

    if constexpr (FP8) {
        const float dq = ep.dq_a[0] * ep.dq_b[0];
#pragma unroll
        for (int a = 0; a < NT; ++a)
#pragma unroll
            for (int b = 0; b < MT; ++b) acc[a][b] *= dq;
    }
    // ---------------------------------------------------------------- epilogue
    // PASSES passes of EROWS rows: accumulators -> fp32 [EROWS][TN] tile in LDS (16-B chunk swizzle) -> every
    // thread finishes 8 consecutive columns of a row with 16-byte coalesced global accesses
    const bool vec_ok = ((ldc & 7) == 0) && (ep.residual == nullptr || (ep.ldr & 7) == 0);
    if constexpr (DEPI) {
        // direct epilogue: no LDS round trip.  Lane (fr, g) owns, per fragment pair, columns 8g..8g+7 of row fr:
        // one wave instruction stores 16 rows x 64 contiguous bytes.
        static_assert(NT % 2 == 0, "N-permuted fragments come in pairs");
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int m = m0 + wm * (TM / WGM) + mt * 16 + fr;
#pragma unroll
            for (int pr = 0; pr < NT / 2; ++pr) {
                const int n = n0 + wn * (TN / WGN) + 32 * pr + 8 * g;
                if (m >= M || n >= N) continue;
                float v[8];
                v[0] = acc[2 * pr][mt][0]; v[1] = acc[2 * pr][mt][1]; v[2] = acc[2 * pr][mt][2]; v[3] = acc[2 * pr][mt][3];
                v[4] = acc[2 * pr + 1][mt][0]; v[5] = acc[2 * pr + 1][mt][1]; v[6] = acc[2 * pr + 1][mt][2]; v[7] = acc[2 * pr + 1][mt][3];
                epi_chunk(v, m, n, N, ldc, vec_ok, ep, C);
            }
        }
        return;
    }
    float* ctile = reinterpret_cast<float*>(smem_nt);
    constexpr int CPR = TN / 8;
    constexpr int IPP = (EROWS * CPR + NTH - 1) / NTH;                // chunks per thread per pass
#pragma unroll 1
    for (int pass = 0; pass < PASSES; ++pass) {
        const int prow0 = pass * EROWS;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int rt = wm * (TM / WGM) + mt * 16;                 // first row of this 16-row fragment within the tile
            if (rt >= prow0 && rt < prow0 + EROWS) {
                const int r = rt - prow0 + fr;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int c16 = (wn * (TN / WGN) + nt * 16) / 4 + g;
                    *reinterpret_cast<f32x4*>(ctile + r * TN + ((c16 ^ (r & 7)) << 2)) = acc[nt][mt];
                }
            }
        }
        __syncthreads();
        if constexpr (!PFOK) {
#pragma unroll 2
            for (int id = tid; id < EROWS * CPR; id += NTH) {
                const int r = id / CPR, j = id - r * CPR;
                const int m = m0 + prow0 + r, n = n0 + 8 * j;
                if (prow0 + r >= TM || m >= M || n >= N) continue;
                float v[8];
                const f32x4 lo = *reinterpret_cast<const f32x4*>(ctile + r * TN + (((2 * j) ^ (r & 7)) << 2));
                const f32x4 hi = *reinterpret_cast<const f32x4*>(ctile + r * TN + (((2 * j + 1) ^ (r & 7)) << 2));
                v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3]; v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
                if constexpr (PATCH == 2) st16(C + patch_row(ep.pm, m) + patch_col(ep.pm, n), pack8(v));      // N % 8 == 0, plain epilogue (host-checked)
                else epi_chunk(v, m, n, N, ldc, vec_ok, ep, C);
            }
        } else {
            // UNR chunks at a time in a ROLLED loop (a fully unrolled sweep holds 4 chunks of erf / gelu' temporaries); the
            // prefetched chunks are consumed in order, so after each group the rest move down by UNR registers
            constexpr int UNR = (IPP % 2 == 0) ? 2 : 1;
#pragma unroll 1
            for (int it0 = 0; it0 < IPP; it0 += UNR) {
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const int id = tid + NTH * (it0 + u);
                    const int r = id / CPR, j = id - r * CPR;
                    const int m = m0 + prow0 + r, n = n0 + 8 * j;
                    if (m >= M || n >= N) continue;
                    float v[8];
                    const f32x4 lo = *reinterpret_cast<const f32x4*>(ctile + r * TN + (((2 * j) ^ (r & 7)) << 2));
                    const f32x4 hi = *reinterpret_cast<const f32x4*>(ctile + r * TN + (((2 * j + 1) ^ (r & 7)) << 2));
                    v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3]; v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
                    epi_chunk(v, m, n, N, ldc, vec_ok, ep, C, pre(u), pf);
                }
#pragma unroll
                for (int c = 0; c + UNR < NPRE; ++c) pre(c) = pre(c + UNR);
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------ gemm_nt for very few rows (M <= 256)
// The class-attention blocks and the heads work on ONE token per image (M = batch = 128).  As 128x128 tiles these are
// 3-9 workgroups walking K serially, one exposed memory latency per 64-deep step: 19-51 us inside the training step for
// 0.04-0.1 GFLOP.  Here: 64x32 output tile per workgroup (24-72 workgroups), the 8 waves split K into 32-deep chunks, each
// wave loads its MFMA fragments straight from global memory with up to three chunks in flight, partial sums meet in LDS.
__global__ void __launch_bounds__(512)
k_gemm_nt_skinny(const bf16_t* __restrict__ A, int lda, const bf16_t* __restrict__ B, int ldb, bf16_t* __restrict__ C, int ldc,
                 int M, int N, int K, EpiArgs ep) {
    extern __shared__ __attribute__((aligned(16))) float sk_part[];          // [8 waves][64][SK_STRIDE]
    const int n0 = blockIdx.x * 32, m0 = blockIdx.y * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, g = lane >> 4;
    const int nch = (K + 31) >> 5;            // the last chunk may be partial (K % 8 == 0: whole 16-byte pieces; lanes beyond K load zeros)
    const bf16_t* arow[4];
    const bf16_t* brow[2];
#pragma unroll
    for (int t = 0; t < 4; ++t) arow[t] = A + (int64_t)min(m0 + t * 16 + fr, M - 1) * lda + g * 8;
#pragma unroll
    for (int t = 0; t < 2; ++t) brow[t] = B + (int64_t)min(n0 + t * 16 + fr, N - 1) * ldb + g * 8;
    f32x4 acc[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    for (int c0 = wave; c0 < nch; c0 += 24) {          // rounds of up to 3 chunks per wave, chunks interleaved over the waves
        u32x4 xa[3][4], wb[3][2];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int ch = c0 + 8 * r;
            const bool ok = ch < nch && ch * 32 + g * 8 < K;
#pragma unroll
            for (int t = 0; t < 4; ++t) xa[r][t] = ok ? ld16(arow[t] + ch * 32) : zero4;
#pragma unroll
            for (int t = 0; t < 2; ++t) wb[r][t] = ok ? ld16(brow[t] + ch * 32) : zero4;
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
                    acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(wb[r][nt]), as_bf16x8(xa[r][mt]), acc[nt][mt], 0, 0, 0);
    }
    float* mine = sk_part + wave * 64 * SK_STRIDE;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
            *reinterpret_cast<f32x4*>(mine + (mt * 16 + fr) * SK_STRIDE + nt * 16 + 4 * g) = acc[nt][mt];
    __syncthreads();
    if (tid < 256) {
        const int r = tid >> 2, j = tid & 3;
        const int m = m0 + r, n = n0 + 8 * j;
        if (m < M && n < N) {
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < 8; ++w) {
                const float* p = sk_part + (w * 64 + r) * SK_STRIDE + 8 * j;
                const f32x4 lo = *reinterpret_cast<const f32x4*>(p), hi = *reinterpret_cast<const f32x4*>(p + 4);
                v[0] += lo[0]; v[1] += lo[1]; v[2] += lo[2]; v[3] += lo[3]; v[4] += hi[0]; v[5] += hi[1]; v[6] += hi[2]; v[7] += hi[3];
            }
            const bool vec_ok = ((ldc & 7) == 0) && (ep.residual == nullptr || (ep.ldr & 7) == 0);
            epi_chunk(v, m, n, N, ldc, vec_ok, ep, C);
        }
    }
}


// ------------------------------------------------------------------------------------ wgrad
#define TM 64          // tokens per step (MFMA reduction)
__device__ __forceinline__ int tn_swz(int row) { return ((row & 3) << 1) | (((row >> 3) & 1) << 3); }

__device__ __forceinline__ bf16x8 tr_frag(const bf16_t* tile, int row0, int col0, int lane) {
    // fragment for MFMA 16x16x32 whose k axis is the tile ROW axis: rows row0+8g..+7, cols col0..+15
    const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
    const int r1 = row0 + 8 * g + q, r2 = r1 + 4;
    const int j = (col0 >> 3) + (p >> 1);
    const bf16_t* a1 = tile + r1 * 128 + ((j ^ tn_swz(r1)) << 3) + (p & 1) * 4;
    const bf16_t* a2 = tile + r2 * 128 + ((j ^ tn_swz(r2)) << 3) + (p & 1) * 4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(a1));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(a2));
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

// same fragment from a per-lane base offset computed once outside the token loop: the swizzle term is
// lane-constant (it depends on q = (lane&15)>>2 and g&1 only), so every read of the loop is
// base[t] + compile-time immediate (ks*32 rows, +4 rows for the second half)
__device__ __forceinline__ int tr_base(int col0, int lane) {
    const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
    const int r1 = 8 * g + q;
    const int j = (col0 >> 3) + (p >> 1);
    return r1 * 128 + ((j ^ tn_swz(r1)) << 3) + (p & 1) * 4;
}
__device__ __forceinline__ bf16x8 tr_frag_at(const bf16_t* tile, int base, int ks) {
    const bf16_t* a1 = tile + base + ks * 32 * 128;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(a1));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(a1 + 4 * 128));
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

// one weight-gradient problem of a (possibly grouped) launch
struct TnArgs {
    const bf16_t* A; const bf16_t* B; float* C; float* colsum;
    int lda, ldb, ldc, M, N1, N2, steps_per_split, t1, t2, nblocks, start;
    const bf16_t* cs_weight;    // per-token weights of the fused column sum (bf16 [M], nullptr = ones)
    float cs_scale;             // factor applied to the column sums
    float alpha;                // factor applied to the product
    float* slab;                // deterministic mode: partial tiles [splits][N1][N2] (+ [splits][N1] column sums behind them), else nullptr
    int splits;
    PatchMap pb;                // pb.group != 0: the rows of B are patches of an NHWC feature map (gemm_epi.h)
};
// deterministic mode: partial results are STORED per token split and summed in split order by k_tn_reduce
struct TnDet { float* slab; float* cs_slab; };
struct TnGroup { TnArgs p[TN_MAX_GROUP]; int count; };
static_assert(TM == TN_STEP, "tn_plan.h counts the reduction steps of these kernels");
// (the placement table TnMap of a grouped launch, entry b = problem << 12 | split * tiles + tile of workgroup b: tn_plan.h)

template <bool BPATCH = false, bool BBN = false>
__device__ __forceinline__ void tn_tile(const bf16_t* __restrict__ A, int lda, const bf16_t* __restrict__ B, int ldb, float* __restrict__ C, int ldc,
                                        int M, int N1, int N2, int steps_per_split, float* __restrict__ colsum, int t1, int t2, int nblocks, int block,
                                        bf16_t* sA, bf16_t* sB, const bf16_t* __restrict__ cs_weight = nullptr, float cs_scale = 1.0f,
                                        float* __restrict__ slab = nullptr, int splits = 1, float alpha = 1.0f,
                                        const PatchMap pb = PatchMap{0, 0, 0, 0, 0, 0u, 0u}, const BnIn bbn = BnIn{nullptr, nullptr, nullptr, nullptr}) {
    // XCD-aware decode: workgroups that share an XCD (and its L2) get consecutive ids, i.e. all output
    // tiles of the SAME token split, so each token range is fetched from HBM by one L2 only
    // (before: 347 MB of beyond-L2 traffic for 77 MB of operands on the qkv shape)
    const int id = nblocks > 0 ? xcd_remap(block, nblocks) : block;        // nblocks <= 0: `block` is already split * tiles + tile (TnMap)
    const int bz = id / (t1 * t2), tl = id - bz * (t1 * t2);
    const int by = tl / t1, bx = tl - by * t1;
    const int n0 = bx * 128, k0 = by * 128;
    const int step_begin = bz * steps_per_split;
    const int total_steps = (M + TM - 1) / TM;
    const int step_end = min(total_steps, step_begin + steps_per_split);
    if (step_begin >= step_end) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave >> 1, wk = wave & 1;
    const int srow = tid >> 4, j = tid & 15;            // 4 chunks: rows srow + 16*i, chunk j
    const bool a_ok = (n0 + j * 8) < N1, b_ok = (k0 + j * 8) < N2;
    // two register sets: the loads of steps t+1 and t+2 are in flight while step t is computed
    // (rocprof: 1.4 waves/SIMD resident, 42 % of wave cycles parked waiting for the single prefetch)
    u32x4 ra0[4], rb0[4], ra1[4], rb1[4];
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    // full token steps: unconditional loads; the guarded form compiles to an exec-masked branch block with register zeroing
    // around every load
    // (columns beyond N1 / N2 only feed output rows / columns that are never stored: their chunk index is clamped into the
    // row instead of being guarded, so ragged tiles -- N = 192, 486, 576 -- take the fast path too)
    const int ca = min(n0 + j * 8, lda - 8), cb = min(k0 + j * 8, ldb - 8);
    // per-token weights of the fused column sum travel with the operands (same prefetch distance): loading them inside the MFMA loop
    // made the loop wait for ALL older loads -- the operand prefetch included -- and cost 0.8 ms per training step
    // (branch-free: a guarded load compiles to an exec-masked block, and the wait-count pass then drains the operand prefetch at its join)
    const bool cs_w = (colsum != nullptr) && (cs_weight != nullptr) && (by == 0) && (wk == 0);
    const bf16_t* wsrc = (cs_weight != nullptr) ? cs_weight : A;                  // any valid address when there are no weights
    const int wmax = (cs_weight != nullptr) ? ((M + 7) & ~7) - 8 : 0;            // the weight vector is padded to a multiple of 8 tokens
    // only the few waves that own a column-sum (wk == 0 of the by == 0 tiles) of a weighted problem load them: a PROVABLY wave-uniform
    // branch (readfirstlane), so the other waves neither issue the two extra loads per step nor wait for them
    const bool cs_w_u = __builtin_amdgcn_readfirstlane((int)cs_w) != 0;
    auto wload = [&](u32x4* rw, int step) {
        if (cs_w_u) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) rw[ks] = ld16(wsrc + min(step * TM + ks * 32 + 8 * (lane >> 4), wmax));
        }
    };
    // patch-addressed B (the weight gradient of a k x k / stride k convolution: B rows are patches of the layer input): the column part
    // of the address is fixed per thread, the row part costs one multiply-high per load
    // (a separate instantiation: the extra address registers cost the grouped kernel its second workgroup per CU)
    constexpr bool b_patch = BPATCH;
    const int cbp = b_patch ? patch_col(pb, min(k0 + j * 8, N2 - 8)) : 0;
    auto brow = [&](int m) { return b_patch ? patch_row(pb, m) + cbp : (int64_t)m * ldb + cb; };
    auto gload = [&](u32x4* ra, u32x4* rb, int step) {
        if (step < step_end && (step + 1) * TM <= M) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = step * TM + srow + 16 * i;
                ra[i] = ld16(A + (int64_t)m * lda + ca);
                rb[i] = ld16(B + brow(m));
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = step * TM + srow + 16 * i;
            const bool ok = (m < M) && (step < step_end);
            ra[i] = (ok && a_ok) ? ld16(A + (int64_t)m * lda + n0 + j * 8) : zero4;
            rb[i] = (ok && b_ok) ? ld16(B + (b_patch ? brow(min(m, M - 1)) : (int64_t)m * ldb + k0 + j * 8)) : zero4;
        }
    };
    f32x4 acc[4][4];     // [nt][kt]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // optional fused bias gradient: column sums of A = A^T . 1, one extra MFMA per A fragment with an
    // all-ones B fragment, done only by the wk==0 waves of the blockIdx.y==0 tiles
    const bool do_colsum = (colsum != nullptr) && (by == 0) && (wk == 0);
    f32x4 csum[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) csum[a] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const u32x4 ones_u = {0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u};
    const bf16x8 ones = __builtin_bit_cast(bf16x8, ones_u);

    int abase[4], bbase[4], woff[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        abase[t] = tr_base(wn * 64 + t * 16, lane);
        bbase[t] = tr_base(wk * 64 + t * 16, lane);
        const int r = srow + 16 * t;
        woff[t] = r * 128 + ((j ^ tn_swz(r)) << 3);
    }
    // BBN (a patch instantiation of its own: as a run-time branch its 16 registers doubled the time of EVERY patch launch, 67 -> 130 us):
    // the B rows are relu(bn(.)) of the 64-channel map that is read; chunk j of a 128-column tile is channels 8 (j & 7) .. + 7
    float tsc[BBN ? 8 : 1], tsh[BBN ? 8 : 1];
    if constexpr (BBN) bn_in_consts(bbn, (j & 7) * 8, tsc, tsh);
    auto stage_and_compute = [&](u32x4* ra, u32x4* rb, u32x4* rw, int refill_step) {
        const u32x4 wcur[2] = {rw[0], rw[1]};          // this step's weights (the refill below overwrites the set)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            st16(sA + woff[i], ra[i]);
            if constexpr (BBN) rb[i] = bn_in_apply(rb[i], tsc, tsh);
            st16(sB + woff[i], rb[i]);
        }
        __syncthreads();
        gload(ra, rb, refill_step);
        wload(rw, refill_step);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 af[4], bfr[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                af[t] = tr_frag_at(sA, abase[t], ks);
                bfr[t] = tr_frag_at(sB, bbase[t], ks);
            }
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
                    acc[nt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[nt], bfr[kt], acc[nt][kt], 0, 0, 0);
            if (do_colsum) {
                const bf16x8 wfrag = cs_w ? __builtin_bit_cast(bf16x8, wcur[ks]) : ones;       // element j <-> token 8g + j of this k-step
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) csum[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[nt], wfrag, csum[nt], 0, 0, 0);
            }
        }
        __syncthreads();
    };
    u32x4 rw0[2] = {zero4, zero4}, rw1[2] = {zero4, zero4};
    gload(ra0, rb0, step_begin);
    wload(rw0, step_begin);
    gload(ra1, rb1, step_begin + 1);
    wload(rw1, step_begin + 1);
    for (int step = step_begin; step < step_end; step += 2) {
        stage_and_compute(ra0, rb0, rw0, step + 2);
        if (step + 1 < step_end) stage_and_compute(ra1, rb1, rw1, step + 3);
    }
    const int fr = lane & 15, g = lane >> 4;
    // deterministic mode: this split's partial tile / column sums are STORED (k_tn_reduce adds the splits in order)
    float* cs_out = slab ? slab + (int64_t)splits * N1 * N2 + (int64_t)bz * N1 : colsum;
    if (do_colsum && fr == 0) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + wn * 64 + nt * 16 + 4 * g + r;
                if (n < N1) { if (slab) cs_out[n] = csum[nt][r] * cs_scale; else atomicAdd(cs_out + n, csum[nt][r] * cs_scale); }
            }
    }
    if (slab) {
        float* part = slab + (int64_t)bz * N1 * N2;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                const int kk = k0 + wk * 64 + kt * 16 + fr;
                if (kk >= N2) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = n0 + wn * 64 + nt * 16 + 4 * g + r;
                    if (n < N1) part[(int64_t)n * N2 + kk] = acc[nt][kt][r] * alpha;
                }
            }
        return;
    }
#if (AP_ABL & 64)
    {   // ablation: no atomics (keep the accumulators live)
        float sacc = 0.f;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) sacc += acc[nt][kt][0] + acc[nt][kt][1] + acc[nt][kt][2] + acc[nt][kt][3];
        if (sacc == 12345.678f) C[0] = 1.f;
        return;
    }
#endif
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const int kk = k0 + wk * 64 + kt * 16 + fr;
            if (kk >= N2) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + wn * 64 + nt * 16 + 4 * g + r;
                if (n < N1) atomicAdd(C + (int64_t)n * ldc + kk, acc[nt][kt][r] * alpha);
            }
        }
}

__global__ void __launch_bounds__(256)
k_gemm_tn(const bf16_t* __restrict__ A, int lda, const bf16_t* __restrict__ B, int ldb, float* __restrict__ C, int ldc,
          int M, int N1, int N2, int steps_per_split, float* __restrict__ colsum, int t1, int t2, int nblocks) {
    __shared__ __attribute__((aligned(16))) bf16_t sA[TM * 128];
    __shared__ __attribute__((aligned(16))) bf16_t sB[TM * 128];
    tn_tile(A, lda, B, ldb, C, ldc, M, N1, N2, steps_per_split, colsum, t1, t2, nblocks, blockIdx.x, sA, sB);
}

// Several weight gradients in ONE launch (all Linear layers of a block): the workgroups of the launch are shared
// between the problems, so each problem is split over fewer token ranges -> longer reduction loops and
// (#problems)x fewer fp32 atomics than one launch per problem (atomics were 12-17 us of a 34-53 us launch).
__global__ void __launch_bounds__(256)
k_gemm_tn_grouped(TnGroup grp) {
    __shared__ __attribute__((aligned(16))) bf16_t sA[TM * 128];
    __shared__ __attribute__((aligned(16))) bf16_t sB[TM * 128];
    int pi = 0;
#pragma unroll
    for (int i = 1; i < TN_MAX_GROUP; ++i)
        if (i < grp.count && (int)blockIdx.x >= grp.p[i].start) pi = i;
    const TnArgs& a = grp.p[pi];
    tn_tile(a.A, a.lda, a.B, a.ldb, a.C, a.ldc, a.M, a.N1, a.N2, a.steps_per_split, a.colsum, a.t1, a.t2, a.nblocks,
            (int)blockIdx.x - a.start, sA, sB, a.cs_weight, a.cs_scale, a.slab, a.splits, a.alpha);
}
// LayerNorm dgamma / dbeta reductions riding in the grouped launch (ap_gemm_tn_acc_grouped_ln): the workgroups behind the placement
// table add the partial rows k_ln_bwd left (column sums of [nblocks][2 C]) -- the block's own reduction launch (5.8 us, 19 per step,
// nothing but latency) disappears into a launch that has idle workgroup slots anyway.  (TnLn, the table of these riders: tn_plan.h)
__device__ __forceinline__ void tn_ln_role(const TnLn& ln, int blk, float* red) {          // red: >= (blockDim.x / 32) * 33 floats of LDS
    int y = 0, b0 = 0;
    for (int i = 0; i + 1 < ln.count; ++i) {                                     // which reduction this workgroup belongs to
        const int nb = (2 * ln.it[i].C + 31) / 32;
        if (y == i && blk >= b0 + nb) { b0 += nb; y = i + 1; }
    }
    const float* __restrict__ partial = ln.it[y].partial;
    const int nblocks = ln.it[y].nblocks, C = ln.it[y].C, C2 = 2 * C;
    const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5, RG = (int)blockDim.x >> 5;      // 32 columns x RG row groups
    const int c = (blk - b0) * 32 + cx;
    if ((blk - b0) * 32 >= C2) return;
    float s = 0.f;
    if (c < C2) {
        int b = ry;
        for (; b + 15 * RG < nblocks; b += 16 * RG) {                            // 16 loads in flight per thread
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = partial[(int64_t)(b + u * RG) * C2 + c];
#pragma unroll
            for (int u = 0; u < 16; ++u) s += v[u];
        }
        for (; b < nblocks; b += RG) s += partial[(int64_t)b * C2 + c];
    }
    red[ry * 33 + cx] = s;
    __syncthreads();
    if (ry == 0 && c < C2) {
        float t = 0.f;
        for (int r = 0; r < RG; ++r) t += red[r * 33 + cx];
        if (c < C) ln.it[y].dgamma[c] += t; else ln.it[y].dbeta[c - C] += t;
    }
}

// the same with the host-made placement table (one (problem, split) per XCD)
__global__ void __launch_bounds__(256)
k_gemm_tn_grouped_map(TnGroup grp, TnMap map, TnLn ln) {
    __shared__ __attribute__((aligned(16))) bf16_t sA[TM * 128];
    __shared__ __attribute__((aligned(16))) bf16_t sB[TM * 128];
    if ((int)blockIdx.x >= ln.first) { tn_ln_role(ln, (int)blockIdx.x - ln.first, reinterpret_cast<float*>(sA)); return; }
    const unsigned e = map.e[blockIdx.x];
    if (e == TN_MAP_IDLE) return;
    const TnArgs& a = grp.p[e >> 12];
    tn_tile(a.A, a.lda, a.B, a.ldb, a.C, a.ldc, a.M, a.N1, a.N2, a.steps_per_split, a.colsum, a.t1, a.t2, 0,
            (int)(e & 0xFFFu), sA, sB, a.cs_weight, a.cs_scale, a.slab, a.splits, a.alpha);
}

// the 192 x 192-tile, LDS-DMA weight-gradient kernel (gemm_tn8p.h) with the same placement table and LayerNorm riders
// (up to AP_TN_MAX_GROUP = 32 problems -- the Linear layers of six transformer blocks, or of two and four outlooker blocks -- and one work item per CU: its own, smaller
// placement table T8Map, entry = problem << 11 | split * tiles + tile (tn_plan.h); the three arguments stay under 4 KB)
struct T8Group { T8Item p[AP_TN_MAX_GROUP]; int tiles[AP_TN_MAX_GROUP]; };
static_assert(sizeof(T8Group) + sizeof(T8Map) + sizeof(TnLn) <= 4096, "kernel arguments of k_gemm_tn_8p");
static_assert(sizeof(TnGroup) + sizeof(TnMap) + sizeof(TnLn) <= 4096, "kernel arguments of k_gemm_tn_grouped_map");
__global__ void __launch_bounds__(512, 2)
k_gemm_tn_8p(T8Group grp, T8Map map, TnLn ln) {
    extern __shared__ __attribute__((aligned(16))) unsigned char t8_smem[];
    if ((int)blockIdx.x >= ln.first) { tn_ln_role(ln, (int)blockIdx.x - ln.first, reinterpret_cast<float*>(t8_smem)); return; }
    const unsigned e = map.e[blockIdx.x];
    if (e == TN_MAP_IDLE) return;
    const int pi = e >> T8_MAP_SHIFT, idx = e & ((1u << T8_MAP_SHIFT) - 1u), tiles = grp.tiles[pi];
    t8_item(grp.p[pi], idx % tiles, idx / tiles, t8_smem);
}
// its fp8 flavour (gemm_tn8p.h, FP8): the same placement table and riders; AF = the format of A (every problem of a launch)
struct T8GroupF8 { T8ItemF8 p[AP_TN_MAX_GROUP]; int tiles[AP_TN_MAX_GROUP]; };
static_assert(sizeof(T8GroupF8) + sizeof(T8Map) + sizeof(TnLn) <= 4096, "kernel arguments of k_gemm_tn_8p_fp8");
template <int AF>
__global__ void __launch_bounds__(512, 2)
k_gemm_tn_8p_fp8(T8GroupF8 grp, T8Map map, TnLn ln) {
    extern __shared__ __attribute__((aligned(16))) unsigned char t8_smem[];
    if ((int)blockIdx.x >= ln.first) { tn_ln_role(ln, (int)blockIdx.x - ln.first, reinterpret_cast<float*>(t8_smem)); return; }
    const unsigned e = map.e[blockIdx.x];
    if (e == TN_MAP_IDLE) return;
    const int pi = e >> T8_MAP_SHIFT, idx = e & ((1u << T8_MAP_SHIFT) - 1u), tiles = grp.tiles[pi];
    t8_item<true, AF>(grp.p[pi], idx % tiles, idx / tiles, t8_smem);
}

// one weight gradient whose B rows are patches of an NHWC feature map (PatchMap): a k x k / stride k convolution's dW
template <bool BBN>
__global__ void __launch_bounds__(256)
k_gemm_tn_patch(TnArgs a, BnIn bbn) {
    __shared__ __attribute__((aligned(16))) bf16_t sA[TM * 128];
    __shared__ __attribute__((aligned(16))) bf16_t sB[TM * 128];
    tn_tile<true, BBN>(a.A, a.lda, a.B, a.ldb, a.C, a.ldc, a.M, a.N1, a.N2, a.steps_per_split, a.colsum, a.t1, a.t2, a.nblocks,
                  (int)blockIdx.x, sA, sB, a.cs_weight, a.cs_scale, a.slab, a.splits, a.alpha, a.pb, bbn);
}

// deterministic mode, second pass: C[n][k] += sum over splits (in split order) of the stored partial tiles; same for the column sums
__global__ void __launch_bounds__(256)
k_tn_reduce(TnGroup grp) {
    for (int pi = 0; pi < grp.count; ++pi) {
        const TnArgs& a = grp.p[pi];
        const int64_t nmat = (int64_t)a.N1 * a.N2, ntot = nmat + (a.colsum ? a.N1 : 0);
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < ntot; i += (int64_t)gridDim.x * 256) {
            if (i < nmat) {
                float acc = 0.f;
                for (int z = 0; z < a.splits; ++z) acc += a.slab[(int64_t)z * nmat + i];
                const int64_t n = i / a.N2, k = i - n * a.N2;
                a.C[n * a.ldc + k] += acc;
            } else {
                const int64_t n = i - nmat;
                float acc = 0.f;
                for (int z = 0; z < a.splits; ++z) acc += a.slab[(int64_t)a.splits * nmat + (int64_t)z * a.N1 + n];
                a.colsum[n] += acc;
            }
        }
    }
}


// the fp8 weight-gradient kernel (gemm_tn_fp8.h): workgroups [start, start + tiles * splits) of the launch belong to problem i (split-major),
// the LayerNorm riders behind them
struct TfGroup { TfItem p[AP_TN_MAX_GROUP]; int count; };
static_assert(sizeof(TfGroup) + sizeof(TnLn) <= 4096, "kernel arguments of k_gemm_tn_fp8");
__global__ void __launch_bounds__(256)
k_gemm_tn_fp8(TfGroup grp, TnLn ln) {
    __shared__ __attribute__((aligned(16))) unsigned char tf_smem[32768];
    if ((int)blockIdx.x >= ln.first) { tn_ln_role(ln, (int)blockIdx.x - ln.first, reinterpret_cast<float*>(tf_smem)); return; }
    int pi = 0;
    for (int i = 1; i < AP_TN_MAX_GROUP; ++i)
        if (i < grp.count && (int)blockIdx.x >= grp.p[i].start) pi = i;
    const TfItem& it = grp.p[pi];
    const int local = (int)blockIdx.x - it.start;
    if (it.a_fmt == AP_FP8_E5M2) tf_tile<AP_FP8_E5M2>(it, local % it.tiles, local / it.tiles, tf_smem);
    else tf_tile<AP_FP8_E4M3>(it, local % it.tiles, local / it.tiles, tf_smem);
}


// the GELU table of gemm_epi.h (gelu = 3 launches of the 8-phase kernel): a static device array, filled once per process on the stream of
// its first use (no allocation inside the library; AP_GELU_TABLE=0: the row phase evaluates the functions instead)
__device__ unsigned g8_gelu_table[2 * GQ_TAB_N];
__global__ void __launch_bounds__(256) k_build_gelu_table(unsigned* tab) {
    const unsigned idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < 2 * GQ_TAB_N) tab[idx] = gq_tab_entry(idx);
}
// (not static: csrc/mlp_fused.hip reads the same table; declared in gemm_epi.h)
// Built once per device, synchronously (the build used to be enqueued on the stream of its first use -- if that first use sat inside
// a stream capture the kernel was only RECORDED and later eager launches read an unbuilt table; launches on another stream had no dependency
// on it).  While `st` is capturing nothing can be built or waited for: the caller gets nullptr and takes the arithmetic path for that launch.
const unsigned* g8_gelu_table_ptr(hipStream_t st) {
    static std::mutex mu;
    static int state[16] = {0};                 // per device -- 0: not built, 1: built, -1: switched off
    static unsigned* ptr[16] = {nullptr};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) { (void)hipGetLastError(); return nullptr; }
    std::lock_guard<std::mutex> lock(mu);
    if (state[dev] == 0) {
        if (!ap_switches().gelu_table) { state[dev] = -1; return nullptr; }
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
        if (cs != hipStreamCaptureStatusNone) return nullptr;
        if (hipGetSymbolAddress(reinterpret_cast<void**>(&ptr[dev]), HIP_SYMBOL(g8_gelu_table)) != hipSuccess || !ptr[dev]) { (void)hipGetLastError(); state[dev] = -1; return nullptr; }
        hipLaunchKernelGGL(k_build_gelu_table, dim3(2 * GQ_TAB_N / 256), dim3(256), 0, st, ptr[dev]);
        if (hipStreamSynchronize(st) != hipSuccess) { (void)hipGetLastError(); state[dev] = -1; return nullptr; }
        state[dev] = 1;
    }
    return state[dev] == 1 ? ptr[dev] : nullptr;
}

// launch of the persistent 8-phase kernel (gemm8p.h): one instantiation per epilogue flavour of the training step, a generic one
// (EF = -1: the flavour is read from the arguments on the device) for anything else
template <int NT1, int EF, bool FP8 = false, int BM = 256>
static int g8_go(const G8Args& ga, const EpiArgs& ep, int grid, hipStream_t st) {
    AP_LAUNCH_LDS((k_gemm_nt_8p<NT1, EF, FP8, BM>), dim3(grid), dim3(512), G8_LDS_BYTES, st, ga, ep);
    return ap_check_launch();
}
// the instantiations of one tile shape: the first EF of the list that equals the flavour, or is the generic -1, takes the launch -- so -1
// stands last in a list; a list without it (the 224-row tiles) refuses any other flavour
template <int NT1, bool FP8, int BM, int... EF>
static int g8_pick(int flavour, const G8Args& ga, const EpiArgs& ep, int grid, hipStream_t st) {
    int rc = AP_ERR_UNSUPPORTED;
    (void)(... || ((EF < 0 || EF == flavour) && ((rc = g8_go<NT1, EF, FP8, BM>(ga, ep, grid, st)), true)));
    return rc;
}
// bf16, 256-row tiles: the flavours of the training step and of the forward-only passes ...
#define G8_FLAVOURS_BF16 0, G8_BIAS, G8_RS, G8_BIAS | G8_GELU, G8_BIAS | G8_GELU | G8_RS, G8_BIAS | G8_GELU | G8_GTAB, G8_BIAS | G8_GELU | G8_RS | G8_GTAB, \
    G8_BIAS | G8_GELU | G8_GTAB | G8_NOSIDE, G8_BIAS | G8_GELU | G8_RS | G8_GTAB | G8_NOSIDE, G8_DGELU, G8_DGELU | G8_RS, G8_MUL, G8_MUL | G8_RS, G8_MUL8, \
    G8_MUL8 | G8_RS, G8_MUL8 | G8_Q8, G8_MUL8 | G8_RS | G8_Q8, G8_BIAS | G8_RES, G8_BIAS | G8_RS | G8_RES, -1
// ... fp8 (ap_gemm_nt_fp8: the forward Linear layers of the configs[4] step): the flavours a transformer block's forward uses; the 224-row
// list is G8_FLAVOURS_224 (gemm_nt_const.h): nt_plan.h plans such tiles for those flavours only (no generic instantiation)
#define G8_FLAVOURS_FP8 0, G8_BIAS, G8_BIAS | G8_GELU, G8_BIAS | G8_GELU | G8_RS, G8_BIAS | G8_GELU | G8_GTAB, G8_BIAS | G8_GELU | G8_RS | G8_GTAB, G8_BIAS | G8_RES, \
    G8_BIAS | G8_RS | G8_RES, -1

// ---- NT products: which kernel is launched, with which tile and grid, and what is refused is planned by nt_plan.h; here its plans become
// kernel arguments.  The run-time switches (read once per process), the device's CU count and the GELU table are handed to the planner.
static const NtSwitches& nt_switches() { static const NtSwitches s = nt_switches_from(getenv); return s; }
static NtEpi nt_facts(const EpiArgs& ep) {
    return NtEpi{ep.bias != nullptr, ep.preact != nullptr, ep.dgelu_of != nullptr, ep.mul_by != nullptr, ep.mul8 != nullptr, ep.row_scale != nullptr,
                 ep.residual != nullptr, ep.q8 != nullptr, ep.q8_scale != nullptr, ep.ldr, ep.gelu, ep.noside};
}
template <int EPI>
static int ws_go(const WsArgs& a, const EpiArgs& ep, int grid, hipStream_t st) {
    AP_LAUNCH_LDS(k_gemm_nt_ws<EPI>, dim3(grid), dim3(512), WS_LDS_BYTES(EPI), st, a, ep);
    return ap_check_launch();
}
template <int BM_, int BN_, int WM_, int WN_>
static void nt_tile_go(const NtPlan& p, const bf16_t* A, int lda, const bf16_t* B, int ldb, bf16_t* C, int ldc, int M, int N, int K, const EpiArgs& ep, hipStream_t st) {
    if (p.lds_epi) hipLaunchKernelGGL((k_gemm_nt<BM_, BN_, WM_, WN_, false>), dim3(p.grid), dim3(WM_ * WN_ * 64), 0, st, A, lda, B, ldb, C, ldc, M, N, K, p.tiles_n, p.ntiles, ep);
    else hipLaunchKernelGGL((k_gemm_nt<BM_, BN_, WM_, WN_, true>), dim3(p.grid), dim3(WM_ * WN_ * 64), 0, st, A, lda, B, ldb, C, ldc, M, N, K, p.tiles_n, p.ntiles, ep);
}
// plan and launch.  K, lda, ldb as the entry point took them: the kernels of an fp8 launch count them in byte PAIRS (their element is 2 bytes)
static int nt_launch(const bf16_t* A, int lda, const bf16_t* B, int ldb, bf16_t* C, int ldc, int M, int N, int K, EpiArgs& ep, bool fp8, hipStream_t st) {
    const unsigned* tab = nullptr;
    const NtPlan p = nt_plan(M, N, K, lda, ldb, ldc, nt_facts(ep), fp8, ap_cu_count(), nt_switches(), [&] { return (tab = g8_gelu_table_ptr(st)) != nullptr; });
    if (p.status != AP_OK) return p.status;
    (void)hipGetLastError();
    if (p.tab) ep.gelu_tab = tab;
    if (fp8) { lda /= 2; ldb /= 2; K /= 2; }
    switch (p.family) {
        case NT_SKINNY:
            AP_LAUNCH_LDS(k_gemm_nt_skinny, dim3(p.grid, p.grid_y), dim3(512), p.lds_bytes, st, A, lda, B, ldb, C, ldc, M, N, K, ep);
            break;
        case NT_8P: {
            const G8Args ga = {A, lda, B, ldb, C, ldc, M, N, K, p.tiles_n, p.ntiles};
            if (g8_flavour(ep) != p.flavour) return AP_ERR_LAUNCH;         // (the instantiation is picked by the plan's flavour, the generic kernel reads g8_flavour)
            if (p.bm == 224) return g8_pick<1, false, 224, G8_FLAVOURS_224>(p.flavour, ga, ep, p.grid, st);
            if (fp8) return p.bn == 192 ? g8_pick<1, true, 256, G8_FLAVOURS_FP8>(p.flavour, ga, ep, p.grid, st) : g8_pick<2, true, 256, G8_FLAVOURS_FP8>(p.flavour, ga, ep, p.grid, st);
            return p.bn == 192 ? g8_pick<1, false, 256, G8_FLAVOURS_BF16>(p.flavour, ga, ep, p.grid, st) : g8_pick<2, false, 256, G8_FLAVOURS_BF16>(p.flavour, ga, ep, p.grid, st);
        }
        case NT_WS: {
            const WsArgs a = {A, lda, B, ldb, C, ldc, M, N, p.n_slices, p.n_items, p.per_xcd};
            return p.ws_epi == 0 ? ws_go<0>(a, ep, p.grid, st) : p.ws_epi == 2 ? ws_go<2>(a, ep, p.grid, st) : ws_go<1>(a, ep, p.grid, st);
        }
        case NT_TILE:
#define NT_CASE(V, ...) case V: nt_tile_go<__VA_ARGS__>(p, A, lda, B, ldb, C, ldc, M, N, K, ep, st); break;
            switch (p.variant) {
                NT_TILE_SHAPES(NT_CASE)
                default:
                    if (p.prefetch) hipLaunchKernelGGL((k_gemm_nt<128, 128, 2, 2, false, 1, true>), dim3(p.grid), dim3(256), 0, st, A, lda, B, ldb, C, ldc, M, N, K, p.tiles_n, p.ntiles, ep);
                    else nt_tile_go<128, 128, 2, 2>(p, A, lda, B, ldb, C, ldc, M, N, K, ep, st);
            }
#undef NT_CASE
            break;
        default:                // NT_FP8_TILE
            hipLaunchKernelGGL((k_gemm_nt<128, 128, 2, 2, false, 1, false, 0, true>), dim3(p.grid), dim3(256), 0, st, A, lda, B, ldb, C, ldc, M, N, K, p.tiles_n, p.ntiles, ep);
            break;
    }
    return ap_check_launch();
}

extern "C" {

// the epilogue of a launch without ap_gemm_epilogue: everything off, one row per DropPath scale
static EpiArgs epi_none() {
    EpiArgs ep = {};
    ep.rows_per_scale = 1;
    return ep;
}
// the fields of ap_gemm_epilogue that every entry point takes (what else it takes, and what it refuses, is the entry point's or the planner's)
static void epi_common(EpiArgs& ep, const ap_gemm_epilogue& epi) {
    ep.bias = epi.bias; ep.gelu = epi.gelu; ep.preact = epi.preact_out; ep.dgelu_of = epi.dgelu_of;
    ep.row_scale = epi.row_scale; ep.rows_per_scale = epi.rows_per_scale > 0 ? epi.rows_per_scale : 1;
    ep.residual = epi.residual; ep.ldr = epi.ldr;
    ep.q8 = epi.q8_out; ep.q8_scale = epi.q8_scale; ep.q8_amax = epi.q8_amax;
}

int ap_gemm_nt(const ap_bf16* A, int lda, const ap_bf16* B, int ldb, ap_bf16* C, int ldc, int M, int N, int K,
               const ap_gemm_epilogue* epi, ap_stream_t stream) {
    if (!A || !B || !C) return AP_ERR_NULL;
    EpiArgs ep = epi_none();
    ep.dbg = nt_switches().dbg;                 // AP_GEMM_DBG (ablation aid of k_gemm_nt)
    if (epi) {
        epi_common(ep, *epi);
        ep.mul_by = epi->mul_by; ep.mul8 = epi->mul_by8;
        // gelu = 4: the value of mode 3 in `out`, no side store (forward-only launches); preact_out is ignored
        if (ep.gelu == 4) { ep.gelu = 3; ep.noside = 1; ep.preact = nullptr; }
    }
    return nt_launch(A, lda, B, ldb, C, ldc, M, N, K, ep, false, (hipStream_t)stream);
}

int ap_gemm_nt_fp8(const unsigned char* A, int lda, const unsigned char* B, int ldb, ap_bf16* C, int ldc, int M, int N, int K,
                   const float* dq_a, const float* dq_b, const ap_gemm_epilogue* epi, ap_stream_t stream) {
    if (!A || !B || !C || !dq_a || !dq_b) return AP_ERR_NULL;
    EpiArgs ep = epi_none();
    ep.dq_a = dq_a; ep.dq_b = dq_b;
    if (epi) epi_common(ep, *epi);
    return nt_launch(reinterpret_cast<const bf16_t*>(A), lda, reinterpret_cast<const bf16_t*>(B), ldb, C, ldc, M, N, K, ep, true, (hipStream_t)stream);
}

// does a launch of these dimensions emit its output a second time as e4m3 (q8_out)?  The plan of the canonical launch under the process's
// switches -- bf16: mul_by8 + q8 (the input gradient of fc2), fp8: bias + gelu + q8 (fc1's forward); operands with lda = ldb = K
int ap_gemm_nt_q8_ok(int M, int N, int K, int ldc, int fp8) {
    NtEpi e = {};
    e.q8 = e.q8_scale = true;
    if (fp8) { e.bias = e.preact = true; e.gelu = 1; } else e.mul8 = true;
    return nt_plan(M, N, K, K, K, ldc, e, fp8 != 0, ap_cu_count(), nt_switches(), [] { return true; }).status == AP_OK;
}

static bool patch_map_device(const ap_patch_map* map, PatchMap& pm) {
    if (!map || map->group < 1 || map->kseg < 1) return false;
    pm.group = map->group; pm.gstride = map->group_stride; pm.rstride = map->row_stride; pm.kseg = map->kseg; pm.kstride = map->kseg_stride;
    pm.gmagic = map->group == 1 ? 0xFFFFFFFFu : (unsigned)(0xFFFFFFFFu / (unsigned)map->group) + 1u;      // group 1: q = m - (m != 0 ? 0 : 0) handled below
    pm.kmagic = map->kseg == 1 ? 0xFFFFFFFFu : (unsigned)(0xFFFFFFFFu / (unsigned)map->kseg) + 1u;
    return map->group > 1 && map->kseg > 1;         // d = 1 has no exact 32-bit magic; no caller needs it
}

int ap_gemm_nt_patch(const ap_bf16* A, const ap_bf16* B, int ldb, ap_bf16* C, int ld, int M, int N, int K,
                     const float* bias, const ap_patch_map* map, int side, ap_stream_t stream) {
    return ap_gemm_nt_patch_bn(A, nullptr, B, ldb, C, ld, M, N, K, bias, map, side, stream);
}

int ap_gemm_nt_patch_bn(const ap_bf16* A, const ap_bn_input* a_bn, const ap_bf16* B, int ldb, ap_bf16* C, int ld, int M, int N, int K,
                        const float* bias, const ap_patch_map* map, int side, ap_stream_t stream) {
    if (!A || !B || !C || !map) return AP_ERR_NULL;
    if (a_bn && (side != 1 || !a_bn->mean || !a_bn->rstd || !a_bn->gamma || !a_bn->beta)) return AP_ERR_NULL;
    if (M <= 0 || N <= 0 || K <= 0 || M > AP_MAX_ROWS || (K & 7) || (ldb & 7) || ldb < K) return AP_ERR_SHAPE;
    EpiArgs ep = epi_none();
    if (!patch_map_device(map, ep.pm)) return AP_ERR_SHAPE;
    if ((int64_t)M >= (int64_t)(0xFFFFFFFFu / (unsigned)map->group)) return AP_ERR_SHAPE;       // exactness bound of the magic division
    (void)hipGetLastError();
    if (side == 1) {            // A rows are patches; C plain [M, ld]
        if ((K & 63) || (map->kseg & 63) || K % map->kseg || ld < N) return AP_ERR_SHAPE;
        ep.bias = bias;
        if (a_bn) ep.abn = BnIn{a_bn->mean, a_bn->rstd, a_bn->gamma, a_bn->beta};       // (64-channel pixels: kseg % 64 == 0 is checked above)
        const int tm = (M + 127) / 128, tn = (N + 63) / 64, nt = tm * tn;
        hipLaunchKernelGGL((k_gemm_nt<128, 64, 2, 2, true, 1, false, 1>), dim3(nt), dim3(256), 0, (hipStream_t)stream, A, K, B, ldb, C, ld, M, N, K, tn, nt, ep);
    } else if (side == 2) {     // C rows are patches (input gradient); A plain [M, ld]
        if (bias || (N & 7) || (map->kseg & 7) || N % map->kseg || (ld & 7) || ld < K) return AP_ERR_SHAPE;
        const int tm = (M + 127) / 128, tn = (N + 127) / 128, nt = tm * tn;
        hipLaunchKernelGGL((k_gemm_nt<128, 128, 2, 2, false, 1, false, 2>), dim3(nt), dim3(256), 0, (hipStream_t)stream, A, ld, B, ldb, C, N, M, N, K, tn, nt, ep);
    } else return AP_ERR_SHAPE;
    return ap_check_launch();
}

// ---- weight gradients: what is launched and how it is cut and placed is planned by tn_plan.h; here its plans become kernel arguments.
// The run-time switches and the device's CU count are read here and handed to the planner.
static int tn_8p_enabled() { return ap_switches().tn_8p; }
static int tn_capacity() {               // resident workgroups of the 128 x 128-tile kernels, two per CU (AP_GEMM_TN_GROUP_BLOCKS forces a number)
    const int forced = ap_switches().tn_group_blocks;
    return forced > 0 ? forced : 2 * ap_cu_count();
}

int ap_gemm_tn_acc(const ap_bf16* A, int lda, const ap_bf16* B, int ldb, float* C, int ldc, int M, int N1, int N2,
                   float* colsum_A, ap_stream_t stream) {
    if (!A || !B || !C) return AP_ERR_NULL;
    if (M <= 0 || N1 <= 0 || N2 <= 0 || M > AP_MAX_ROWS) return AP_ERR_SHAPE;
    if ((lda & 7) || (ldb & 7) || lda < N1 || ldb < N2 || ldc < N2) return AP_ERR_SHAPE;
    const TnItemPlan p = tn_single_plan(M, N1, N2, ap_switches().tn_blocks);
    const int blocks = p.t1 * p.t2 * p.splits;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_gemm_tn, dim3(blocks), dim3(256), 0, (hipStream_t)stream, A, lda, B, ldb, C, ldc, M, N1, N2, p.sps, colsum_A, p.t1, p.t2, blocks);
    return ap_check_launch();
}

// the arguments of the 128 x 128-tile kernels from a plan (slabs of the deterministic mode: the caller's)
static int tn_group_args(const ap_tn_problem* problems, int count, TnGroupPlan& plan, TnGroup& grp) {
    if (const int rc = tn128_plan(problems, count, tn_capacity(), plan); rc != AP_OK) return rc;
    grp.count = count;
    for (int i = 0; i < count; ++i) {
        const ap_tn_problem& q = problems[i];
        const TnItemPlan& p = plan.p[i];
        TnArgs& a = grp.p[i];
        a.A = reinterpret_cast<const bf16_t*>(q.A); a.B = reinterpret_cast<const bf16_t*>(q.B); a.C = q.C; a.colsum = q.colsum_A;
        a.lda = q.lda; a.ldb = q.ldb; a.ldc = q.ldc; a.M = q.M; a.N1 = q.N1; a.N2 = q.N2;
        a.steps_per_split = p.sps; a.t1 = p.t1; a.t2 = p.t2; a.nblocks = p.t1 * p.t2 * p.splits; a.start = p.start;
        a.cs_weight = reinterpret_cast<const bf16_t*>(q.colsum_weight);
        a.cs_scale = tn_cs_scale(q.colsum_weight, q.colsum_scale);
        a.alpha = tn_alpha(q.alpha);
        a.slab = nullptr; a.splits = p.splits;
        a.pb = PatchMap{0, 0, 0, 0, 0, 0u, 0u};
        if (q.b_patch) patch_map_device(q.b_patch, a.pb);          // (the plan has checked the map)
    }
    for (int i = count; i < TN_MAX_GROUP; ++i) { grp.p[i] = grp.p[0]; grp.p[i].start = 0x7fffffff; grp.p[i].nblocks = 0; }
    return AP_OK;
}

size_t ap_gemm_tn_grouped_workspace(const ap_tn_problem* problems, int count) {
    TnGroupPlan plan; TnGroup grp;
    return tn_group_args(problems, count, plan, grp) == AP_OK ? plan.slab_floats * sizeof(float) : 0;
}

int ap_gemm_tn_acc_grouped(const ap_tn_problem* problems, int count, void* workspace, size_t ws_bytes, ap_stream_t stream) {
    return ap_gemm_tn_acc_grouped_ln(problems, count, nullptr, 0, workspace, ws_bytes, stream);
}

// the 192 x 192-tile kernel (tn_plan.h: tn8_plan) with the LayerNorm riders behind its table
static int tn_launch_8p(const ap_tn_problem* problems, int count, const T8Plan& plan, TnLn ln, int lblocks, ap_stream_t stream) {
    T8Group g8;
    for (int i = 0; i < count; ++i) {
        const ap_tn_problem& q = problems[i];
        T8Item& t = g8.p[i];
        t.A = reinterpret_cast<const bf16_t*>(q.A); t.B = reinterpret_cast<const bf16_t*>(q.B); t.C = q.C; t.colsum = q.colsum_A;
        t.cs_weight = reinterpret_cast<const bf16_t*>(q.colsum_weight);
        t.lda = q.lda; t.ldb = q.ldb; t.ldc = q.ldc; t.M = q.M; t.t2 = q.N2 / 192; t.ksteps = q.M / 64; t.ksps = plan.ksps;
        t.alpha = tn_alpha(q.alpha); t.cs_scale = tn_cs_scale(q.colsum_weight, q.colsum_scale);
        t.shared_out = plan.shared_out[i];
        g8.tiles[i] = plan.pl[i].tiles;
    }
    for (int i = count; i < AP_TN_MAX_GROUP; ++i) { g8.p[i] = g8.p[0]; g8.tiles[i] = 1; }
    ln.first = plan.blocks;
    if (const int rc = ap_allow_lds<k_gemm_tn_8p>(T8_LDS_BYTES); rc != AP_OK) return rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_gemm_tn_8p, dim3(plan.blocks + lblocks), dim3(512), T8_LDS_BYTES, (hipStream_t)stream, g8, plan.map, ln);
    return ap_check_launch();
}

// the 128 x 128-tile kernels: at most TN_MAX_GROUP problems, optional deterministic mode
static int tn_grouped_128(const ap_tn_problem* problems, int count, const ap_ln_reduce* ln_items, int ln_count,
                          void* workspace, size_t ws_bytes, ap_stream_t stream) {
    bool ln_done = ln_count == 0;
    TnGroupPlan plan; TnGroup grp;
    if (const int rc = tn_group_args(problems, count, plan, grp); rc != AP_OK) return rc;
    const int blocks = plan.blocks;
    if (workspace) {                                  // deterministic: stored partial tiles + ordered reduce instead of fp32 atomics
        if (ws_bytes < plan.slab_floats * sizeof(float)) return AP_ERR_SHAPE;
        for (int i = 0; i < count; ++i) grp.p[i].slab = reinterpret_cast<float*>(workspace) + plan.slab_off[i];
    }
    (void)hipGetLastError();
    bool any_patch = false;
    for (int i = 0; i < count; ++i) any_patch = any_patch || problems[i].b_patch != nullptr;
    if (any_patch) {
        if (count != 1) return AP_ERR_UNSUPPORTED;                  // a patch-addressed problem is launched on its own
        BnIn bbn = BnIn{nullptr, nullptr, nullptr, nullptr};
        if (problems[0].b_bn) {
            const ap_bn_input* q = problems[0].b_bn;
            if (!q->mean || !q->rstd || !q->gamma || !q->beta) return AP_ERR_NULL;
            if (problems[0].b_patch->kseg % 64 || problems[0].N2 % 64) return AP_ERR_SHAPE;         // 64-channel pixels, whole pixels per patch row
            bbn = BnIn{q->mean, q->rstd, q->gamma, q->beta};
        }
        if (problems[0].b_bn) hipLaunchKernelGGL(k_gemm_tn_patch<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, grp.p[0], bbn);
        else hipLaunchKernelGGL(k_gemm_tn_patch<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, grp.p[0], bbn);
    } else {
        const int cap = 2 * ap_cu_count() / 8;                                                                  // resident workgroups per XCD
        TnMap map; int mblocks = 0;
        if (ap_switches().tn_place && tn128_place(plan, cap, map, mblocks)) {
            TnLn ln; int lblocks = 0;
            tn_ln_table(ln_items, ln_count, ln, lblocks);           // (checked by the entry point)
            ln.first = mblocks;
            hipLaunchKernelGGL(k_gemm_tn_grouped_map, dim3(mblocks + lblocks), dim3(256), 0, (hipStream_t)stream, grp, map, ln);
            ln_done = true;
        } else hipLaunchKernelGGL(k_gemm_tn_grouped, dim3(blocks), dim3(256), 0, (hipStream_t)stream, grp);
    }
    if (!ln_done) {                                    // no placement table (or a patch-addressed problem): the reductions get their own launch
        const int rc2 = ap_layernorm_bwd_reduce_batched(ln_items, ln_count, stream);
        if (rc2 != AP_OK) return rc2;
    }
    if (workspace) hipLaunchKernelGGL(k_tn_reduce, dim3(1024), dim3(256), 0, (hipStream_t)stream, grp);
    return ap_check_launch();
}

int ap_gemm_tn_acc_grouped_ln(const ap_tn_problem* problems, int count, const ap_ln_reduce* ln_items, int ln_count,
                              void* workspace, size_t ws_bytes, ap_stream_t stream) {
    TnLn ln; int lblocks = 0;
    if (const int rc = tn_ln_table(ln_items, ln_count, ln, lblocks); rc != AP_OK) return rc;
    if (const int rc = tn_validate(problems, count, AP_TN_MAX_GROUP); rc != AP_OK) return rc;
    TnDispatch d;
    tn_dispatch(problems, count, workspace != nullptr, workspace ? 0 : ap_cu_count(), tn_8p_enabled(), d);
    for (int k = 0; k < d.n; ++k) {
        const TnLaunch& l = d.l[k];
        ap_tn_problem sub[AP_TN_MAX_GROUP];
        for (int i = 0; i < l.count; ++i) sub[i] = problems[d.order[l.first + i]];
        const int rc = l.kernel == TN_KERNEL_8P ? tn_launch_8p(sub, l.count, d.p8, ln, lblocks, stream)
                                                : tn_grouped_128(sub, l.count, l.riders ? ln_items : nullptr, l.riders ? ln_count : 0, workspace, ws_bytes, stream);
        if (rc != AP_OK) return rc;
    }
    return AP_OK;
}

// ---- fp8 weight gradients (gemm_tn_fp8.h)
static int tf_group_args(const ap_tn8_problem* problems, int count, TnGroupPlan& plan, TfGroup& grp) {
    if (const int rc = tf_plan(problems, count, 2 * ap_cu_count(), plan); rc != AP_OK) return rc;       // (validates every problem)
    grp.count = count;
    for (int i = 0; i < count; ++i) {
        const ap_tn8_problem& q = problems[i];
        const TnItemPlan& p = plan.p[i];
        TfItem& t = grp.p[i];
        t.A = q.A; t.B = q.B; t.C = q.C; t.slab = nullptr; t.dq_a = q.dq_a; t.dq_b = q.dq_b;
        t.lda = q.lda; t.ldb = q.ldb; t.ldc = q.ldc; t.M = q.M; t.N1 = q.N1; t.N2 = q.N2;
        t.t2 = p.t2; t.ksteps = p.steps; t.ksps = p.sps; t.splits = p.splits; t.tiles = p.t1 * p.t2;
        t.start = p.start; t.alpha = tn_alpha(q.alpha); t.a_fmt = q.a_fmt; t.shared_out = p.shared_out;
    }
    for (int i = count; i < AP_TN_MAX_GROUP; ++i) { grp.p[i] = grp.p[0]; grp.p[i].start = 0x7fffffff; }
    return AP_OK;
}

size_t ap_gemm_tn8_grouped_workspace(const ap_tn8_problem* problems, int count) {
    TnGroupPlan plan; TfGroup grp;
    return tf_group_args(problems, count, plan, grp) == AP_OK ? plan.slab_floats * sizeof(float) : 0;
}

int ap_gemm_tn8_acc_grouped(const ap_tn8_problem* problems, int count, void* workspace, size_t ws_bytes, ap_stream_t stream) {
    return ap_gemm_tn8_acc_grouped_ln(problems, count, nullptr, 0, workspace, ws_bytes, stream);
}

int ap_gemm_tn8_acc_grouped_ln(const ap_tn8_problem* problems, int count, const ap_ln_reduce* ln_items, int ln_count,
                               void* workspace, size_t ws_bytes, ap_stream_t stream) {
    TnLn ln; int lblocks = 0;
    if (const int rc = tn_ln_table(ln_items, ln_count, ln, lblocks); rc != AP_OK) return rc;
    TnGroupPlan plan; TfGroup grp;
    if (const int rc = tf_group_args(problems, count, plan, grp); rc != AP_OK) return rc;
    const int blocks = plan.blocks;
    T8Plan p8;
    if (!workspace && tf8_plan(problems, count, ap_cu_count(), tn_8p_enabled(), p8)) {        // atomic mode: the 8-phase flavour when every problem fits it
        T8GroupF8 g8;
        for (int i = 0; i < count; ++i) {
            const ap_tn8_problem& q = problems[i];
            T8ItemF8& t = g8.p[i];
            t.A = q.A; t.B = q.B; t.C = q.C; t.dq_a = q.dq_a; t.dq_b = q.dq_b;
            t.lda = q.lda; t.ldb = q.ldb; t.ldc = q.ldc; t.M = q.M; t.t2 = q.N2 / 192; t.ksteps = q.M / 128; t.ksps = p8.ksps;
            t.alpha = tn_alpha(q.alpha);
            t.shared_out = p8.shared_out[i];
            g8.tiles[i] = p8.pl[i].tiles;
        }
        for (int i = count; i < AP_TN_MAX_GROUP; ++i) { g8.p[i] = g8.p[0]; g8.tiles[i] = 1; }
        const int mb8 = p8.blocks;
        ln.first = mb8;
        const bool e5 = problems[0].a_fmt == AP_FP8_E5M2;
        if (const int rca = e5 ? ap_allow_lds<k_gemm_tn_8p_fp8<AP_FP8_E5M2>>(T8_LDS_BYTES) : ap_allow_lds<k_gemm_tn_8p_fp8<AP_FP8_E4M3>>(T8_LDS_BYTES); rca != AP_OK) return rca;
        (void)hipGetLastError();
        if (e5)
            hipLaunchKernelGGL(k_gemm_tn_8p_fp8<AP_FP8_E5M2>, dim3(mb8 + lblocks), dim3(512), T8_LDS_BYTES, (hipStream_t)stream, g8, p8.map, ln);
        else
            hipLaunchKernelGGL(k_gemm_tn_8p_fp8<AP_FP8_E4M3>, dim3(mb8 + lblocks), dim3(512), T8_LDS_BYTES, (hipStream_t)stream, g8, p8.map, ln);
        return ap_check_launch();
    }
    if (workspace) {                                  // deterministic: stored partial tiles + ordered reduce instead of fp32 atomics
        if (ws_bytes < plan.slab_floats * sizeof(float)) return AP_ERR_SHAPE;
        for (int i = 0; i < count; ++i) grp.p[i].slab = reinterpret_cast<float*>(workspace) + plan.slab_off[i];
    }
    ln.first = blocks;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_gemm_tn_fp8, dim3(blocks + lblocks), dim3(256), 0, (hipStream_t)stream, grp, ln);
    if (workspace) {                                  // the ordered sum of the splits: k_tn_reduce, TN_MAX_GROUP problems per launch
        for (int i0 = 0; i0 < count; i0 += TN_MAX_GROUP) {
            TnGroup rg;
            rg.count = std::min(TN_MAX_GROUP, count - i0);
            for (int i = 0; i < TN_MAX_GROUP; ++i) {
                const TfItem& t = grp.p[i0 + std::min(i, rg.count - 1)];
                TnArgs& a = rg.p[i];
                memset(&a, 0, sizeof(a));
                a.C = t.C; a.ldc = t.ldc; a.N1 = t.N1; a.N2 = t.N2; a.slab = t.slab; a.splits = t.splits; a.colsum = nullptr;
                a.start = i < rg.count ? 0 : 0x7fffffff;
            }
            hipLaunchKernelGGL(k_tn_reduce, dim3(1024), dim3(256), 0, (hipStream_t)stream, rg);
        }
    }
    return ap_check_launch();
}

}  // extern "C"
