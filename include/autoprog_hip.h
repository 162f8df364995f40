/*
 * autoprog_hip.h -- C ABI of libautoprog_hip.so: the MI355X (gfx950) kernels behind the
 * AutoProg VOLO/DeiT training hot path.
 *
 * The reference (changlin31/AutoProg) has no FFI/plugin ABI: its hot path is Python
 * nn.Modules calling ATen ops.  This header is therefore
 * build-defined (row B2); each entry point names the reference call site whose device
 * arithmetic it replaces (file:line relative to the reference tree).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer borrowed for the call; nothing is allocated,
 *     freed or synchronised inside; work is enqueued on `stream` (a hipStream_t)
 *   - bf16 tensors are passed as uint16_t*, row-major, leading dimension in ELEMENTS and a
 *     multiple of 8 (16-byte rows); fp32 statistics / parameters / gradients are float*
 *   - return 0 on success, a negative AP_ERR_* otherwise (no exceptions cross the ABI)
 *   - entry points are re-entrant and thread-compatible; the only process-wide state is a handful of tuning switches
 *     (AP_* environment variables, each read once into a function-local static) and one-time hipFuncSetAttribute calls
 */
#ifndef AUTOPROG_HIP_H
#define AUTOPROG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ap_stream_t;          /* hipStream_t */
typedef uint16_t ap_bf16;

enum {
    AP_OK = 0,
    AP_ERR_SHAPE = -1,        /* a size/stride violates the documented constraints */
    AP_ERR_UNSUPPORTED = -2,  /* valid request outside what the kernels implement  */
    AP_ERR_LAUNCH = -3,       /* hipGetLastError() != hipSuccess after a launch    */
    AP_ERR_NULL = -4          /* a required pointer is NULL                         */
};

/* Operand sizes ("Operand size limits").  Row, image and element counts passed as int64_t are good for any operand that fits device
 * memory: every address is formed in 64 bits, and the kernels whose grid grows with the row count return AP_ERR_SHAPE beyond 2^31 - 1
 * workgroups (the losses, top-K, the distillation loss, ap_classify_stats: 2^31 - 1 rows or more).  Row counts passed as int (M of the
 * GEMMs, of ap_gemm_tn_acc* / ap_gemm_tn8_acc_grouped and of ap_colsum_acc) must not exceed AP_MAX_ROWS: the tile counts (M + tile - 1) / tile
 * are formed in int.  AP_ERR_SHAPE beyond. */
#define AP_MAX_ROWS 0x7fffff00       /* 2^31 - 256 */

int ap_abi_version(void);
const char* ap_error_string(int code);

/* ---- calibration probes of the device a measurement runs on (no reference call site: bench.py `calibration`, next to the timing
 * loop of main_prog.py:1007-1008,1061-1064).  ap_calib_copy: dst[0:bytes) = src[0:bytes) with 16 bytes per lane (bytes % 16 == 0);
 * ap_calib_mfma: 256 workgroups x 4 waves, each `iters` trips of 16 independent v_mfma_f32_16x16x32_bf16 on operands read once from
 * seed (>= 2048 bf16) -- 256 * 4 * iters * 16 * 16384 FLOP; sink receives nothing unless a sum hits a sentinel (keeps the loop alive) */
int ap_calib_copy(const void* src, void* dst, int64_t bytes, ap_stream_t stream);
int ap_calib_mfma(const ap_bf16* seed, float* sink, int iters, ap_stream_t stream);

/* ---- precision plumbing (apex O1 casts, main_prog.py:491: fp32 master -> 16-bit) ------- */
int ap_cast_f32_bf16(const float* src, ap_bf16* dst, int64_t n, ap_stream_t stream);
int ap_cast_bf16_f32(const ap_bf16* src, float* dst, int64_t n, ap_stream_t stream);
/* dst[c*ld_dst + r] = bf16(src[r*cols + c]); columns rows..ld_dst-1 of dst are zeroed */
int ap_cast_transpose_f32_bf16(const float* src, ap_bf16* dst, int rows, int cols, int ld_dst, ap_stream_t stream);

/* ---- per-step input resize of progressive / supernet training (main_prog.py:973-974,1908-1910:
 * F.interpolate(input, size=(r,r), mode='bilinear', align_corners=False)) fused with the stem's NCHW fp32 -> NHWC bf16 conversion:
 * x [B,C,Hi,Wi] fp32 -> y [B,Ho,Wo,C] bf16.  Ho = Hi, Wo = Wi is the plain layout change + cast. */
int ap_resize_bilinear_nhwc(const float* x, ap_bf16* y, int B, int C, int Hi, int Wi, int Ho, int Wo, ap_stream_t stream);

/* ---- DropPath masks of a whole forward pass (timm DropPath behind models/volo.py:128,218: mask = floor(keep + U), y = x * mask / keep):
 * uniform [sites,B] in [0,1), keep [sites] -> factor [sites,B] = mask/keep, mask [sites,B] in {0,1}, and (tokens > 0) token_mask
 * [sites, token_row] bf16 with token_mask[s, b*tokens + t] = mask[s,b], zero padding up to token_row (a multiple of 8 >= B*tokens) */
int ap_droppath_masks(const float* uniform, const float* keep, float* factor, float* mask, ap_bf16* token_mask, int sites, int B,
                      int tokens, int token_row, ap_stream_t stream);

/* ---- LayerNorm (nn.LayerNorm: models/volo.py:122,131,213,221,290,297,550) ------------- */
int ap_layernorm_fwd(const ap_bf16* x, const float* gamma, const float* beta, ap_bf16* y,
                     float* mean, float* rstd, int64_t rows, int C, float eps, ap_stream_t stream);
/* the same with a second copy of the output as OCP e4m3 bytes for an fp8 GEMM (configs[4]): y8 = sat(y * q_scale[0]),
 * q_amax[0] = max(q_amax[0], max |y|) (nullable) -- what ap_quantize_fp8 would produce from y, without its pass over y */
int ap_layernorm_fwd_fp8(const ap_bf16* x, const float* gamma, const float* beta, ap_bf16* y, unsigned char* y8, const float* q_scale,
                         float* q_amax, float* mean, float* rstd, int64_t rows, int C, float eps, ap_stream_t stream);
/* dx = dres + d(LN)/dx ; dgamma/dbeta are ACCUMULATED (+=).  `workspace` (device, caller-owned,
 * >= ap_layernorm_bwd_workspace() bytes) holds per-workgroup partial sums for the deterministic
 * two-pass column reduction. */
size_t ap_layernorm_bwd_workspace(int64_t rows, int C);
int ap_layernorm_bwd(const ap_bf16* dy, const ap_bf16* x, const float* gamma, const float* mean,
                     const float* rstd, const ap_bf16* dres /*nullable*/, ap_bf16* dx,
                     float* dgamma, float* dbeta, int64_t rows, int C,
                     void* workspace, size_t ws_bytes, ap_stream_t stream);
/* the same without the dgamma / dbeta reduction: the per-workgroup partial rows stay in `workspace` (which must live until the
 * batched reduction ran), *n_partial receives their count; ap_layernorm_bwd_reduce_batched then reduces up to AP_LN_MAX_BATCH
 * LayerNorms (all of one block) in ONE launch: dgamma / dbeta += column sums of the partial rows */
#define AP_LN_MAX_BATCH 12
typedef struct ap_ln_reduce { const float* partial; int n_partial; int C; float* dgamma; float* dbeta; } ap_ln_reduce;
int ap_layernorm_bwd_partial(const ap_bf16* dy, const ap_bf16* x, const float* gamma, const float* mean, const float* rstd,
                             const ap_bf16* dres, ap_bf16* dx, int64_t rows, int C, void* workspace, size_t ws_bytes, int* n_partial,
                             ap_stream_t stream);
/* (ABI version 6) the same for the LayerNorm whose output also feeds a 2 x 2 ceil-mode average pool (OutlookAttention, models/volo.py:75,87):
 * rows = B*H*W tokens of a [B,H,W,C] grid, and the incoming gradient of token (b, y, x) is dy + pool_grad[b, y/2, x/2] / count (count = pixels
 * under the pooled cell) -- the pool's backward rides in the kernel instead of a pass of its own over dy (ap_avgpool2_bwd_acc).
 * AP_ERR_UNSUPPORTED where the pipelined one-chunk-per-lane kernel does not apply (C > 512): call ap_avgpool2_bwd_acc + the plain form. */
int ap_layernorm_bwd_partial_pool(const ap_bf16* dy, const ap_bf16* pool_grad, int B, int H, int W, const ap_bf16* x, const float* gamma,
                                  const float* mean, const float* rstd, const ap_bf16* dres, ap_bf16* dx, int C, void* workspace, size_t ws_bytes,
                                  int* n_partial, ap_stream_t stream);
int ap_layernorm_bwd_reduce_batched(const ap_ln_reduce* items, int count, ap_stream_t stream);

/* ---- Linear layers (nn.Linear: models/volo.py:67,68,71,156,158,180,182,253,256,258,547,553)
 * C[M,N] = epilogue( A[M,K] . B[N,K]^T )   bf16 in, fp32 MFMA accumulate, bf16 out
 * epilogue order: +bias[n]; GELU (optionally also storing the pre-activation); * gelu'(h[m,n]);
 * * row_scale[m / rows_per_scale] (DropPath, timm); + residual[m,n]
 * Only the N logical columns are written: columns N .. ldc-1 of C (and of preact_out / q8_out, whose leading dimension is ldc) keep what
 * they held, also inside the last 16-byte chunk when N % 8 != 0; nothing is read from the columns K .. lda-1 / K .. ldb-1 of A / B, the
 * columns N .. ldr-1 of residual or N .. ldc-1 of dgelu_of / mul_by / mul_by8 in a way that reaches the output (padding may hold anything) */
/* Patch addressing: a k x k / stride k convolution on an NHWC feature map [B,H,W,C] (PatchEmbed.proj, Downsample:
 * models/volo.py:368-372,383-396) is a GEMM whose row m = (b, i, j) and column kk = (dy, dx, c) live at element offset
 *   (m / group) * group_stride + (m % group) * row_stride + (kk / kseg) * kseg_stride + (kk % kseg)
 * with group = W/k output columns, group_stride = k*W*C, row_stride = k*C, kseg = k*C, kseg_stride = W*C (H % k == 0). */
typedef struct ap_patch_map { int group, group_stride, row_stride, kseg, kseg_stride; } ap_patch_map;
/* side 1: C[M, ld] = A_patches[M, K] . B[N, K]^T + bias   (forward; K % 64 == 0, kseg % 64 == 0)
 * side 2: C_patches[M, N] = A[M, ld >= K] . B[N, K]^T        (input gradient written in place of the feature map; bias NULL) */
int ap_gemm_nt_patch(const ap_bf16* A, const ap_bf16* B, int ldb, ap_bf16* C, int ld, int M, int N, int K,
                     const float* bias, const ap_patch_map* map, int side, ap_stream_t stream);
/* (ABI version 6) side = 1 with a_bn: the A rows are relu(bn(.)) of the 64-channel NHWC map that is read (the activation between the last
 * stem convolution and PatchEmbed.proj, models/volo.py:364-372, is never materialised); a_bn NULL: ap_gemm_nt_patch */
struct ap_bn_input;
int ap_gemm_nt_patch_bn(const ap_bf16* A, const struct ap_bn_input* a_bn, const ap_bf16* B, int ldb, ap_bf16* C, int ld, int M, int N, int K,
                        const float* bias, const ap_patch_map* map, int side, ap_stream_t stream);

typedef struct ap_gemm_epilogue {
    const float* bias;          /* [N] or NULL */
    int gelu;                   /* 1: out = gelu_erf(v) (models/volo.py:157); 2: the same, and preact_out receives gelu'(v) instead of v;
                                 * 3 (ABI version 6): as 2, but preact_out is an UNSIGNED CHAR [M, ldc] tensor of 8-bit fixed-point codes
                                 * code = clamp(rint(202 * gelu'(v)) + 26, 0, 255), i.e. gelu' = (code - 26) / 202 on [-0.1287, 1.1337] (gelu' lives in
                                 * [-0.1290, 1.1290]; 0, 1/2 and 1 are exact codes): half the bytes of the bf16 derivative, |error| <= 1/404;
                                 * 4 (forward-only launches, additive in ABI version 7): `out` holds exactly the bits mode 3 stores there and nothing
                                 * else is written -- preact_out is ignored and may be NULL.  Needs a bias; no residual / mul_by / dgelu_of / q8_out.
                                 * Taken by the launches the 8-phase kernel or the weight-stationary kernel serves with the GELU table;
                                 * AP_ERR_UNSUPPORTED for any other launch (M <= 256, K % 64 != 0, M < 4096, AP_GELU_TABLE=0, ...): the caller then
                                 * issues mode 3 with a side buffer */
    ap_bf16* preact_out;        /* with gelu: also store v (the pre-activation; gelu = 2: its activation derivative) here, ld = ldc */
    const ap_bf16* dgelu_of;    /* out = v * gelu'(dgelu_of[m,n]) (backward of the above), ld = ldc */
    const float* row_scale;     /* [ceil(M/rows_per_scale)] or NULL */
    int rows_per_scale;
    const ap_bf16* residual;    /* [M,N] with leading dimension ldr, or NULL */
    int ldr;
    const ap_bf16* mul_by;      /* out = v * mul_by[m,n] (ld = ldc), applied where dgelu_of is: the backward of gelu = 2, whose forward stored
                                 * gelu'(h) -- the only thing the backward needs of h (autograd of models/volo.py:157) -- so that it is a
                                 * multiplication instead of ~18 instructions per element; not together with dgelu_of.  (ABI version 3) */
    const unsigned char* mul_by8; /* (ABI version 6) as mul_by with the 8-bit codes a gelu = 3 forward stored: out = v * (mul_by8[m,n] - 26) / 202, ld = ldc
                                 * bytes; not together with mul_by / dgelu_of */
    unsigned char* q8_out;      /* ap_gemm_nt_fp8 with gelu (ABI version 4), ap_gemm_nt with mul_by8 and nothing else but row_scale (version 6:   */
                                /* the input gradient of fc2, operand of fc1's fp8 input-gradient product; AP_ERR_UNSUPPORTED for any other launch */
                                /* or one the 8-phase kernel does not take): the output a second time as OCP e4m3 bytes [M, ldc] --             */
    const float* q8_scale;      /* q8_out = sat(out * q8_scale[0]), q8_amax[0] = max(q8_amax[0], max |out|) (nullable) -- the operand of the */
    float* q8_amax;             /* fp8 GEMM that consumes this activation, without a quantisation pass.  Launches of the 8-phase kernel only */
                                /* (M >= 4096, K % 128 == 0, N as for ap_gemm_nt): AP_ERR_UNSUPPORTED otherwise -- also from ap_gemm_nt, which  */
                                /* since ABI version 6 takes q8_out on its mul_by8 launches and refuses it on any launch whose kernel cannot     */
                                /* write it (a forced tile variant included)                                                                     */
} ap_gemm_epilogue;
int ap_gemm_nt(const ap_bf16* A, int lda, const ap_bf16* B, int ldb, ap_bf16* C, int ldc,
               int M, int N, int K, const ap_gemm_epilogue* epi, ap_stream_t stream);
/* Would a launch of these dimensions emit q8_out?  1 / 0: the launch plan (csrc/nt_plan.h) of the canonical q8 launch under the process's
 * switches on the current device -- fp8 = 0: ap_gemm_nt with mul_by8 + q8_out, fp8 = 1: ap_gemm_nt_fp8 (K in bytes) with bias + gelu + q8_out;
 * lda = ldb = K.  Nothing is launched.  (An added symbol: the ABI version stays 7.) */
int ap_gemm_nt_q8_ok(int M, int N, int K, int ldc, int fp8);
/* ---- (ABI version 7) the MLP of a block in ONE launch: Mlp.forward, models/volo.py:147-167 (fc1 -> GELU -> fc2) with the residual add and
 * DropPath scale of its call sites (:143 Outlooker, :233 Transformer), and -- the same kernel, backward = 1 -- the two input-gradient products
 * of its backward pass.  The hidden activation never makes the trip to memory and back between the two products; it still LEAVES (the weight
 * gradients read it).  Rounding points and K order are those of the two ap_gemm_nt launches it replaces: results are bit-identical to
 *     forward : a = ap_gemm_nt(x, wa, bias1, gelu = 3 -> codes, row_scale_hidden);  out = ap_gemm_nt(a, wb, bias2, row_scale_out, residual)
 *     backward: dh = ap_gemm_nt(x = dL/dout, wa = fc2.weight^T copy, mul_by8 = codes, row_scale_hidden);  out = ap_gemm_nt(dh, wb = fc1.weight^T copy)
 * Built for c = 384, hidden = 3 c, m % 128 == 0 (VOLO-D1's transformer stages at any batch of 128-row blocks): AP_ERR_UNSUPPORTED otherwise,
 * and for a forward launch while the GELU table cannot be had (AP_GELU_TABLE=0; a stream capture in front of its first build) -- the caller
 * then issues the two launches. */
typedef struct ap_mlp_fused_args {
    const ap_bf16* x; int ldx;               /* [m, c] */
    const ap_bf16* wa; int ldwa;             /* [hidden, c] */
    const ap_bf16* wb; int ldwb;             /* [c, hidden] */
    ap_bf16* out; int ldo;                   /* [m, c] */
    ap_bf16* hidden_out; int ldh;            /* [m, hidden]: forward gelu(h) * row_scale_hidden, backward dL/dh */
    unsigned char* codes;                    /* [m, hidden] bytes, row stride ldh: 8-bit gelu' codes (ap_gemm_epilogue.gelu = 3) -- written by the
                                              * forward, read by the backward */
    const float* bias1; const float* bias2;  /* forward: [hidden], [c] (nullable); backward: NULL */
    const float* row_scale_hidden;           /* [ceil(m / rows_per_scale)] or NULL: forward the 0/1 DropPath mask on a, backward mask / keep on dL/dh */
    const float* row_scale_out;              /* forward: mask / keep on the branch output (before the residual); backward: NULL */
    int rows_per_scale;
    const ap_bf16* residual; int ldr;        /* forward: [m, c] or NULL; backward: NULL */
    int m, c, hidden;
    int backward;
    /* forward, optional: the LayerNorm in front of fc1 (Transformer.forward, models/volo.py:233 `self.mlp(self.norm2(x))`) inside the same
     * launch.  ln_in non-NULL: x is ignored, the rows are read from ln_in [m, c], normalised with ln_gamma / ln_beta / ln_eps (bit-identical to
     * ap_layernorm_fwd), written to ln_out [m, c] (the fc1 weight gradient reads them) and their statistics to ln_mean / ln_rstd [m] */
    const ap_bf16* ln_in; int ld_ln;
    ap_bf16* ln_out; int ld_lno;
    const float* ln_gamma; const float* ln_beta; float ln_eps;
    float* ln_mean; float* ln_rstd;
} ap_mlp_fused_args;
int ap_mlp_fused(const ap_mlp_fused_args* args, ap_stream_t stream);
/* The forward of ap_mlp_fused for a pass that no backward follows (additive in ABI version 7): `out` is bit-identical to ap_mlp_fused's for
 * the same arguments; hidden_out, codes, ln_out, ln_mean and ln_rstd may be NULL and are never written.  backward must be 0 (AP_ERR_SHAPE).
 * Same shape contract (c = 384, hidden = 3 c, m % 128 == 0, the GELU table at hand; AP_MLP_FUSED_V=1 has no such kernel): AP_ERR_UNSUPPORTED
 * otherwise. */
int ap_mlp_fused_infer(const ap_mlp_fused_args* args, ap_stream_t stream);

/* ---- fp8 forward GEMM (BASELINE configs[4] "mixed MFMA fp8 GEMM"): OCP e4m3 operands, fp32 accumulation, bf16 output.
 * y = sat(x * scale[0]) -> e4m3, n % 16 == 0; amax (nullable): amax[0] = max(amax[0], max |x|) for the next step's scale */
int ap_quantize_fp8(const ap_bf16* x, unsigned char* y, int64_t n, const float* scale, float* amax, ap_stream_t stream);
/* the same for several tensors in ONE launch (the Linear weights of a model, once per optimizer step): `jobs_device` is a DEVICE array;
 * job j is scaled by scales[slot] and raises amax[slot] (n % 16 == 0) */
typedef struct ap_fp8_job { const ap_bf16* x; unsigned char* y; int64_t n; int slot; int pad_; } ap_fp8_job;
int ap_quantize_fp8_multi(const ap_fp8_job* jobs_device, int njobs, const float* scales, float* amax, ap_stream_t stream);

/* ---- test aid: fill all 160 KB of LDS of every CU with `pattern` (one workgroup per CU; scratch2: 8 bytes of device memory).  A kernel
 * that reads LDS it never wrote (padded rows of a tile) then sees NaNs instead of the previous kernel's leftovers: tests/test_gpu_kernels.py */
int ap_debug_poison_lds(unsigned pattern, unsigned* scratch2, ap_stream_t stream);
/* C = epi(dq_a[0] * dq_b[0] * A8 . B8^T): A8 [M,K], B8 [N,K] e4m3 bytes (K, lda, ldb multiples of 16), dq_* device scalars (1/scale);
 * same epilogue as ap_gemm_nt */
int ap_gemm_nt_fp8(const unsigned char* A, int lda, const unsigned char* B, int ldb, ap_bf16* C, int ldc, int M, int N, int K,
                   const float* dq_a, const float* dq_b, const struct ap_gemm_epilogue* epi, ap_stream_t stream);
/* weight gradient: C[N1,N2] += A[M,N1]^T . B[M,N2]   (fp32 accumulate into C, atomics);
 * optional fused bias gradient: colsum_A[n] += sum_m A[m,n] (NULL to skip).  Columns N2 .. ldc-1 of C are neither read nor written;
 * the columns N1 .. lda-1 / N2 .. ldb-1 of A / B may hold anything */
int ap_gemm_tn_acc(const ap_bf16* A, int lda, const ap_bf16* B, int ldb, float* C, int ldc,
                   int M, int N1, int N2, float* colsum_A, ap_stream_t stream);
/* the same for up to AP_TN_MAX_GROUP problems in ONE launch (all Linear layers of a block, or of several blocks: the
 * reference's autograd issues one addmm per layer, models/volo.py:67-71,156-158,180-182): the launch's workgroups are shared
 * between the problems, so each is split over fewer token ranges and adds fewer fp32 partial tiles atomically -- with the
 * weight gradients of ~6 transformer blocks in one launch no problem is split at all and the partial tiles are plain
 * read-add-stores (the atomics of a block's own launch were 21-27 us of its ~100).  The deterministic mode takes at most 8. */
#define AP_TN_MAX_GROUP 32
typedef struct ap_tn_problem {
    const ap_bf16* A; int lda;      /* [M,N1] */
    const ap_bf16* B; int ldb;      /* [M,N2] */
    float* C; int ldc;              /* [N1,N2] += A^T . B */
    int M, N1, N2;
    float alpha;                    /* C += alpha * A^T . B (0 is read as 1: zero-initialised structs keep the plain product) */
    float* colsum_A;                /* [N1] += colsum_scale * sum_m w[m] * A[m,n], or NULL */
    const ap_bf16* colsum_weight;   /* per-token weights w (bf16, ceil(M/8)*8 elements readable, 16-byte aligned), NULL = ones: the DropPath keep mask of the
                                     * bias gradient d/db of x + (mask/keep) * (y W^T + b), models/volo.py:230-234 */
    float colsum_scale;             /* used with colsum_weight only (1/keep) */
    const struct ap_patch_map* b_patch;   /* non-NULL: the rows of B are patches of an NHWC feature map (ldb ignored) -- the weight
                                           * gradient of a k x k / stride k convolution without a gathered copy of its input */
    const struct ap_bn_input* b_bn;       /* (ABI version 6, with b_patch, 64-channel maps) non-NULL: the B rows are relu(bn(.)) of the map that is read
                                           * -- PatchEmbed.proj's weight gradient on the PRE-BatchNorm output of the last stem convolution */
} ap_tn_problem;
/* `workspace` NULL: partial tiles of the token splits are added with fp32 atomics (results vary in the last bits from run to run).
 * `workspace` of >= ap_gemm_tn_grouped_workspace() bytes: DETERMINISTIC -- every split stores its partial tile and a second kernel adds
 * them in split order (bitwise reproducible; the mode behind AP_DETERMINISTIC=1 of the Python layer). */
size_t ap_gemm_tn_grouped_workspace(const ap_tn_problem* problems, int count);
int ap_gemm_tn_acc_grouped(const ap_tn_problem* problems, int count, void* workspace, size_t ws_bytes, ap_stream_t stream);
/* the same launch also performs up to AP_LN_MAX_BATCH deferred LayerNorm dgamma / dbeta reductions (ap_layernorm_bwd_partial) on
 * workgroups of its own: the weight gradients and the LayerNorm parameter gradients of one block in ONE launch */
int ap_gemm_tn_acc_grouped_ln(const ap_tn_problem* problems, int count, const ap_ln_reduce* ln_items, int ln_count,
                              void* workspace, size_t ws_bytes, ap_stream_t stream);
/* ---- fp8 weight gradients (configs[4]: "e4m3 fwd / e5m2 grads"): C[N1,N2] += alpha * dq_a[0] * dq_b[0] * A8[M,N1]^T . B8[M,N2]
 * A8: output gradient as OCP e5m2 (a_fmt = AP_FP8_E5M2) or e4m3 (AP_FP8_E4M3) bytes, B8: layer input as e4m3 bytes, fp32 accumulation.
 * dq_a / dq_b are DEVICE scalars (1/scale of the quantisation), read at run time (graph replays stay correct).
 * y = sat(g * scale[0]) -> e5m2 (|.| <= 57344, round to nearest even), n % 16 == 0; amax (nullable): amax[0] = max(amax[0], max |g|).
 * colsum (nullable): the bias gradient of the UN-quantised g [rows, cols] (rows * cols == n, cols % 16 == 0):
 * colsum[c] += colsum_scale * sum_r w[r] * g[r,c], w = colsum_weight (bf16 per-row weights, NULL = ones; colsum_scale then unused) */
#define AP_BF8_COLSUM_SPLITS 64
/* colsum_ws (nullable): AP_BF8_COLSUM_SPLITS * cols floats -- the row splits' partial sums are stored there and added in split order
 * (bitwise reproducible, the AP_DETERMINISTIC=1 mode); NULL: fp32 atomics */
int ap_quantize_bf8(const ap_bf16* g, unsigned char* y, int64_t n, const float* scale, float* amax, float* colsum, int rows, int cols,
                    const ap_bf16* colsum_weight, float colsum_scale, float* colsum_ws, ap_stream_t stream);
#define AP_FP8_E4M3 0
#define AP_FP8_E5M2 1
typedef struct ap_tn8_problem {
    const unsigned char* A; int lda;   /* [M,N1] bytes, format a_fmt; lda % 16 == 0 */
    const unsigned char* B; int ldb;   /* [M,N2] e4m3 bytes; ldb % 16 == 0 */
    float* C; int ldc;                 /* [N1,N2] += alpha * dq_a[0] * dq_b[0] * A^T . B */
    int M, N1, N2;                     /* N1, N2 multiples of 128 (every Linear width of VOLO-D5); any M > 0 */
    int a_fmt;                         /* AP_FP8_E5M2 or AP_FP8_E4M3 */
    float alpha;                       /* 0 is read as 1 */
    const float* dq_a; const float* dq_b;
} ap_tn8_problem;
/* `workspace` as for ap_gemm_tn_acc_grouped (NULL: fp32 atomics; >= ap_gemm_tn8_grouped_workspace() bytes: deterministic split order).
 * AP_ERR_UNSUPPORTED for a width or format outside the above (the caller then runs the bf16 product). */
size_t ap_gemm_tn8_grouped_workspace(const ap_tn8_problem* problems, int count);
int ap_gemm_tn8_acc_grouped(const ap_tn8_problem* problems, int count, void* workspace, size_t ws_bytes, ap_stream_t stream);
int ap_gemm_tn8_acc_grouped_ln(const ap_tn8_problem* problems, int count, const ap_ln_reduce* ln_items, int ln_count,
                               void* workspace, size_t ws_bytes, ap_stream_t stream);
/* bias gradient: out[n] += sum_m A[m,n] */
int ap_colsum_acc(const ap_bf16* A, int lda, float* out, int M, int N, ap_stream_t stream);

/* ---- Outlook attention core (models/volo.py:83-98: unfold, softmax, attn@v, fold) -------
 * v [B,H,W,C], logits [B*h*w, ldl] with channel = head*81 + p*9 + q (kernel 3, pad 1, stride 2),
 * y [B,H,W,C].  C = heads*hd.  ldl >= heads*81, a multiple of 8; the logits' columns heads*81 .. ldl-1 may hold anything.
 * dlogits [B*h*w, ldl] has the logits' leading dimension: its columns heads*81 .. ldl-1 are zeroed.  */
int ap_outlook_fwd(const ap_bf16* v, const ap_bf16* logits, int ldl, ap_bf16* y,
                   int B, int H, int W, int heads, int hd, float scale, ap_stream_t stream);
int ap_outlook_bwd(const ap_bf16* v, const ap_bf16* logits, int ldl, const ap_bf16* dy,
                   ap_bf16* dv, ap_bf16* dlogits, int B, int H, int W, int heads, int hd,
                   float scale, ap_stream_t stream);
/* AvgPool2d(2,2,ceil_mode=True) on NHWC tokens (models/volo.py:75,87) */
int ap_avgpool2_fwd(const ap_bf16* x, ap_bf16* y, int B, int H, int W, int C, ap_stream_t stream);
/* dx[b,y,x,:] += dpooled[b,y/2,x/2,:] / count */
int ap_avgpool2_bwd_acc(const ap_bf16* dpooled, ap_bf16* dx, int B, int H, int W, int C, ap_stream_t stream);

/* ---- Multi-head self-attention core (models/volo.py:188-197) ---------------------------
 * qkv [B,N,3C] packed (channel = which*C + head*hd + d), out [B,N,C], lse [B,heads,N].
 * head_dim 32 / 48 / 64 (VOLO-D1..D3 and DeiT: 32 / 64; VOLO-D4/D5: 48, models/volo.py:776-821), any N:
 * N <= 256 with head_dim 32 / 64 runs LDS-resident kernels, everything else key/query-blocked ones.
 * The backward of the blocked path needs ap_mhsa_bwd_workspace() bytes of device scratch (0 for the
 * resident path: `workspace` may then be NULL).                                              */
/* out_row_scale (nullable, fp32 [B]): out[b] is stored multiplied by it.  Used with the 0/1 DropPath keep mask of the projection
 * that follows: rows of dropped samples are zeros, so the projection's weight gradient dx^T out needs no masked copy of dx
 * (models/volo.py:230-234).  The backward needs nothing extra: a dropped sample arrives with dout = 0. */
int ap_mhsa_fwd(const ap_bf16* qkv, ap_bf16* out, float* lse, int B, int N, int heads, int hd,
                float scale, const float* out_row_scale, ap_stream_t stream);
/* the same with the output a second time as OCP e4m3 bytes (out8 = sat(out * q_scale[0]), q_amax[0] raised to max |out|, nullable): the
 * operand of an fp8 output projection (configs[4]).  The key/query-blocked kernel only (N > 256 or head_dim 48): AP_ERR_UNSUPPORTED else */
int ap_mhsa_fwd_fp8(const ap_bf16* qkv, ap_bf16* out, unsigned char* out8, const float* q_scale, float* q_amax, float* lse, int B, int N,
                    int heads, int hd, float scale, const float* out_row_scale, ap_stream_t stream);
/* Would ap_mhsa_fwd_fp8 take this shape?  1 / 0: the launch plan (csrc/attn_plan.h) under the process's switches (AP_MHSA_FLASH=1 sends every
 * shape to the blocked kernel).  Nothing is launched.  (An added symbol: the ABI version stays 7.) */
int ap_mhsa_fwd_emits_fp8(int N, int hd);
size_t ap_mhsa_bwd_workspace(int B, int N, int heads, int hd);
int ap_mhsa_bwd(const ap_bf16* qkv, const ap_bf16* out, const ap_bf16* dout, const float* lse,
                ap_bf16* dqkv, int B, int N, int heads, int hd, float scale,
                void* workspace, size_t ws_bytes, ap_stream_t stream);

/* ---- Class attention core (models/volo.py:264-274): one query per image ----------------
 * q [B,C] (un-scaled), kv [B,N,2C] (channel = which*C + head*hd + d), out [B,C], probs [B,heads,N]; head_dim 32 / 48 / 64.
 * Split layout (kv_cls != NULL): key 0 -- the class token -- is row b of kv_cls [B,2C] and keys 1..N-1 are the N-1 token rows of
 * kv [B,N-1,2C]: the reference concatenates the class token with the tokens before every class block (models/volo.py:304-308),
 * here that copy never happens.  dkv_cls must be given exactly when kv_cls is. */
int ap_class_attn_fwd(const ap_bf16* q, const ap_bf16* kv, const ap_bf16* kv_cls /*nullable*/, ap_bf16* out, float* probs,
                      int B, int N, int heads, int hd, float scale, ap_stream_t stream);
int ap_class_attn_bwd(const ap_bf16* q, const ap_bf16* kv, const ap_bf16* kv_cls /*nullable*/, const float* probs, const ap_bf16* dout,
                      ap_bf16* dq, ap_bf16* dkv, ap_bf16* dkv_cls /*nullable*/, int B, int N, int heads, int hd, float scale,
                      ap_stream_t stream);

/* ---- Mix-token region swap (models/volo.py:654-658, 685-689) ----------------------------
 * y = x except y[b, r0:r1, c0:c1, :] = x[B-1-b, r0:r1, c0:c1, :]  (x: [B,H,W,C])            */
int ap_mix_token_swap(const ap_bf16* x, ap_bf16* y, int B, int H, int W, int C,
                      int r0, int r1, int c0, int c1, ap_stream_t stream);
/* (ABI version 6) the same with the box in DEVICE memory: box_dev = int[4] {r0, r1, c0, c1} on the token-label grid, multiplied by `scale`
 * (2 for the token swap in front of the stages, 1 for the aux-logit swap: models/volo.py:654-658, 685-689).  Part of the graph-replayable
 * step: the box of the step is written into a device buffer in front of the replay instead of being a launch argument. */
int ap_mix_token_swap_dev(const ap_bf16* x, ap_bf16* y, int B, int H, int W, int C, const int* box_dev, int scale, ap_stream_t stream);

/* ---- Dense soft-target cross entropy (loss/cross_entropy.py:35-36, 147-156) -------------
 * logits [M,ldx] (C valid classes); target element (row,c) =
 *   target[(row / rows_per_batch)*t_sb + c*t_sc + (row % rows_per_batch)*t_sn]   (fp32)
 * row_loss[row] = -sum_c t*log_softmax(x);  dlogits = grad_scale*(softmax*sum_c t - t)
 * (columns C..ldx-1 of dlogits are zeroed).
 * mix_batches = B > 0: the target of batch b is mix_lam * t[b] + (1 - mix_lam) * t[B-1-b] (the mix-token image label,
 * loss/cross_entropy.py:151-152) -- no mixed copy of the target is materialised; 0: plain.
 * Widths (both losses, all four entry points; ldx % 8 == 0): ldx <= 1024 runs the register kernels, a row in one wave.  1024 < ldx <= 65 536
 * (ImageNet-21k: 21 843 classes; iNaturalist: 8 142 / 10 000) runs the wide kernels on the same contract -- fp32 statistics, columns C..ldx-1
 * of dlogits zeroed, mix_batches / mix_lam / mix_lam_dev, any target strides, no atomics, no workspace, no host synchronisation; they move
 * rows in 16-byte chunks: logits and dlogits 16-byte aligned (AP_ERR_SHAPE otherwise).  ldx > 65 536: AP_ERR_UNSUPPORTED (a row is staged
 * in LDS, 2 B per column of the 160 KB).  The dense wide kernel is fast on a row-major target (t_sc == 1: [M, C] soft targets) and, up to
 * 2559 classes, on the class-major token-label tensor (t_sn == 1, rows_per_batch > 1); other strides are correct and uncoalesced. */
/* Validation statistics, per row (additive in ABI version 7): logits bf16 [rows, ld], n_classes <= ld valid columns, labels int64 [rows] ->
 *   loss[row] = logsumexp(z) - z[label]                                    (fp32 accumulation)
 *   rank[row] = #{c : z[c] > z[label]}   -- STRICTLY greater: a row is top-k correct iff 0 <= rank < k.  On ties this is the most favourable
 *               of the orders torch.topk may return (its choice among equal values is unspecified); without ties the two agree.
 * A row whose label is outside [0, n_classes) gets loss = 0, rank = -1 (the padding of a last batch; nothing is read through such a label).
 * rows = 0 succeeds without a launch.  No atomics, no host synchronisation. */
int ap_classify_stats(const ap_bf16* logits, int ld, int n_classes, const int64_t* labels, float* loss, int* rank, int64_t rows,
                      ap_stream_t stream);
/* Row-wise softmax + top-K (additive in ABI version 7; csrc/topk.hip): the (class, score) pairs of a token-label target from a teacher's
 * logits.  logits bf16 [M, ld], columns 0 .. C-1 valid (C .. ld-1 are never interpreted: they may hold NaN or inf).  For row r = (b, n),
 * b = r / rows_per_batch, n = r % rows_per_batch, o = b * o_sb + n * o_sn and k < K:
 *   idx[o + k] = the class with the k-th largest logit; EQUAL logits rank by ascending class (torch.sort(descending=True, stable=True))
 *   val[o + k] = softmax(inv_temp * x)[idx[o + k]] over all C columns (fp32, maximum subtracted, fixed reduction order: bit-reproducible)
 * so the K entries are in descending order.  The strides let one launch write straight into slots of a [B, 2 + N, K] target.
 * ld % 8 == 0, logits 16-byte aligned, 1 <= K <= min(16, C), C <= ld, rows_per_batch > 0, 0 < inv_temp < inf (AP_ERR_SHAPE otherwise);
 * ld > 65 536: AP_ERR_UNSUPPORTED (rows beyond 1024 columns are staged in LDS, 2 B per column).  M = 0 succeeds without a launch.
 * A NaN among the valid columns or a row of all -inf gives unspecified values; the indices stay inside [0, C).  The row is read from
 * global memory once.  No atomics, no workspace, no allocation, no host synchronisation. */
int ap_softmax_topk_rows(const ap_bf16* logits, int ld, int C, int K, float inv_temp, int* idx, float* val, int64_t o_sb, int64_t o_sn,
                         int rows_per_batch, int64_t M, ap_stream_t stream);
/* Distillation loss of a student row against a teacher row, loss and gradient from one read of both (additive in ABI version 7;
 * csrc/distill.hip): DeiT's DistillationLoss.  student bf16 [M, ld_s], teacher bf16 [M, ld_t], columns 0 .. C-1 of both valid (C .. ld-1
 * are never interpreted: they may hold NaN or inf).  p_s = softmax(inv_temp * x_s), p_t = softmax(inv_temp * x_t), both fp32 with the
 * maximum subtracted, T = 1 / inv_temp:
 *   mode 0 (soft)   row_loss[r] = T^2 * sum_c p_t[c] (log p_t[c] - log p_s[c])        dstudent[r, c] = grad_scale * T * (p_s[c] - p_t[c])
 *   mode 1 (hard)   row_loss[r] = logsumexp(x_s) - x_s[c*]                             dstudent[r, c] = grad_scale * (softmax(x_s)[c] - [c == c*])
 *                   c* = the class of the largest teacher logit, EQUAL logits resolve to the smallest class (the tie rule of
 *                   ap_softmax_topk_rows; -0 equals +0); inv_temp is ignored.
 * A teacher row that equals the student row gives exactly zero loss in soft mode, and a gradient of at most 2^-24 * grad_scale * T * p_s[c]
 * (the rounding residue of one product).  dstudent has leading dimension ld_s; its
 * columns C .. ld_s-1 are written as zero bits.  No gradient for the teacher.
 * ld_s % 8 == 0, ld_t % 8 == 0, student / teacher / dstudent 16-byte aligned, 1 <= C <= min(ld_s, ld_t), mode 0 or 1, 0 < inv_temp < inf in
 * soft mode (AP_ERR_SHAPE otherwise); a leading dimension above 65 536: AP_ERR_UNSUPPORTED.  M = 0 succeeds without a launch.
 * The kernel is selected by round_up(C, 8) alone, so a padded operand gives the bits of the compact one: up to 1024 columns both rows sit in
 * a wave's registers; wider rows are staged in LDS -- both operands are read from global memory exactly once up to 40 704 columns; beyond
 * (soft mode) the student row is staged and read once and the teacher row is read in each of the three walks, the later two from L2.
 * A NaN among the valid columns gives unspecified values and no out-of-range access.  Fixed reduction order: two runs are bit-identical.
 * No atomics, no workspace, no allocation, no host synchronisation. */
int ap_distill_fwd_bwd(const ap_bf16* student, int ld_s, const ap_bf16* teacher, int ld_t, int C, int mode, float inv_temp,
                       float* row_loss, ap_bf16* dstudent, float grad_scale, int64_t M, ap_stream_t stream);
int ap_soft_ce_fwd_bwd(const ap_bf16* logits, int ldx, const float* target, int64_t t_sb,
                       int64_t t_sc, int64_t t_sn, int rows_per_batch, float* row_loss,
                       ap_bf16* dlogits, float grad_scale, int64_t M, int C,
                       float mix_lam, int mix_batches, ap_stream_t stream);
/* The same loss on the token-label target in its SOURCE form: the reference builds the dense [B,C,2+N] tensor on the GPU every
 * step from top-K (class, score) label maps plus label smoothing (main_prog.py:994-1004 -> tlt create_token_label_target) and
 * feeds it to loss/cross_entropy.py:136-156.  Here the target of logits row r = (b, n), b = r / rows_per_batch, is
 *   t[c] = (1 - smoothing) * sum_k [idx[o + k] == c] * val[o + k] + smoothing / C,   o = b * p_sb + n * p_sn,   k < K <= 16
 * (repeated indices accumulate, indices outside [0, C) contribute nothing); loss and gradient as ap_soft_ce_fwd_bwd.  No dense
 * target exists: 101 MB less to read per step at B = 128.
 * mix_batches = B > 0 (ABI version 5; as in ap_soft_ce_fwd_bwd): the mix-token class target of loss/cross_entropy.py:150-152,
 * t = mix_lam * t[b] + (1 - mix_lam) * t[B-1-b] -- row (b, n) takes the K pairs of its own slot weighted mix_lam and the K pairs of the
 * same slot of image B-1-b weighted 1 - mix_lam (2 K <= 16; M == B * rows_per_batch).  0: no mixing (mix_lam ignored). */
int ap_soft_ce_sparse_fwd_bwd(const ap_bf16* logits, int ldx, const int* idx, const float* val, int K, int64_t p_sb, int64_t p_sn,
                              int rows_per_batch, float smoothing, float* row_loss, ap_bf16* dlogits, float grad_scale,
                              int64_t M, int C, float mix_lam, int mix_batches, ap_stream_t stream);
/* (ABI version 6) both losses with the mix-token lam in DEVICE memory (mix_lam_dev non-NULL overrides mix_lam; pass mix_batches = B
 * always: lam = 1 gives lam t + 0 t' = t exactly) -- the graph-replayable step */
int ap_soft_ce_fwd_bwd_dev(const ap_bf16* logits, int ldx, const float* target, int64_t t_sb, int64_t t_sc, int64_t t_sn, int rows_per_batch,
                           float* row_loss, ap_bf16* dlogits, float grad_scale, int64_t M, int C, float mix_lam, int mix_batches,
                           const float* mix_lam_dev, ap_stream_t stream);
int ap_soft_ce_sparse_fwd_bwd_dev(const ap_bf16* logits, int ldx, const int* idx, const float* val, int K, int64_t p_sb, int64_t p_sn,
                                  int rows_per_batch, float smoothing, float* row_loss, ap_bf16* dlogits, float grad_scale, int64_t M, int C,
                                  float mix_lam, int mix_batches, const float* mix_lam_dev, ap_stream_t stream);
/* The class rows of TokenLabelGTCrossEntropy (loss/cross_entropy.py:62-89) on the sparse target, at every class width of the sparse loss
 * (additive in ABI version 7).  logits bf16 [B, ldx], one row per image.  Image b holds K pairs of slot s at
 * idx / val + b * p_sb + p_s + k, p_s = p_s0 for the ground-truth slot and p_s1 for the image-level slot, 1 <= K <= 8.  With
 *   dense_s[c] = (1 - smoothing) * sum_k [idx_k == c] * val_k + smoothing / C     (repeated indices accumulate, indices outside [0, C) add nothing)
 *   a_s        = argmax_c dense_s[c]
 *   ratio_b    = 0.9 - 0.4 * [a_0 == a_1]
 *   t_b        = ratio_b * dense_1 + (1 - ratio_b) * dense_0
 * the target of row b is t_b, or with mix_batches = B the mix-token class target mix_lam * t_b + (1 - mix_lam) * t_{B-1-b}, where the partner
 * image's ratio is the partner's own; loss and gradient as the sparse loss above.
 * The argmax rule: a class's score is the fp32 sum of its pairs' val, added in ascending k; the argmax is the smallest class index among
 * those with the largest score, and class 0 if no score is positive (a slot of -1 fillers: every class then holds smoothing / C).  Scores
 * are assumed non-negative.
 * Every weight row sums to 1, so the smoothing term stays smoothing / C and the row is at most 4 K weighted pairs:
 *   own slot 1      mix_lam * ratio_b                      partner slot 1   (1 - mix_lam) * ratio_{B-1-b}
 *   own slot 0      mix_lam * (1 - ratio_b)                partner slot 0   (1 - mix_lam) * (1 - ratio_{B-1-b})
 * (mix_batches = 0: the own slots with ratio_b and 1 - ratio_b; mix_lam is ignored).  mix_lam_dev non-NULL overrides mix_lam (pass
 * mix_batches = B: lam = 1 gives the unmixed bits exactly).  Columns C .. ldx-1 of the logits are never interpreted and their gradient is
 * stored as zero bits.  K outside 1 .. 8, mix_batches not in {0, B}, ldx % 8 != 0, ldx < C, smoothing outside [0, 1), rows wider than 1024
 * columns that are not 16-byte aligned: AP_ERR_SHAPE; ldx > 65 536: AP_ERR_UNSUPPORTED.  B = 0 succeeds without a launch.  Fixed reduction
 * order: two runs are bit-identical.  No atomics, no workspace, no allocation, no host synchronisation. */
int ap_soft_ce_sparse_gt_fwd_bwd(const ap_bf16* logits, int ldx, const int* idx, const float* val, int K, int64_t p_sb, int64_t p_s0, int64_t p_s1,
                                 float smoothing, float* row_loss, ap_bf16* dlogits, float grad_scale, int64_t B, int C, float mix_lam,
                                 int mix_batches, const float* mix_lam_dev, ap_stream_t stream);
/* out[0] = wa * sum(a[0:na]) + wb * sum(b[0:nb]): cls_weight * mean(row losses) + dense_weight * mean(row losses)
 * of the token-label loss (loss/cross_entropy.py:154-156) in one launch */
int ap_loss_combine(const float* a, int64_t na, float wa, const float* b, int64_t nb, float wb, float* out, ap_stream_t stream);

/* ---- small fused elementwise helpers ---------------------------------------------------- */
/* y[m,:] = x[m,:] * scale[m / rows_per_scale] */
int ap_row_scale(const ap_bf16* x, const float* scale, ap_bf16* y, int64_t M, int C,
                 int rows_per_scale, ap_stream_t stream);
/* y = a + b (b broadcast over the leading `reps` copies when b_elems < n) */
int ap_add_bcast(const ap_bf16* a, const ap_bf16* b, ap_bf16* y, int64_t n, int64_t b_elems, ap_stream_t stream);
/* out[i] += sum over reps of x[r*n + i]  (fp32 accumulate; gradient of a broadcast add).  reps <= AP_SUM_REPS_MAX (16 repetitions per
 * workgroup along the grid's y axis, which holds 65 535): AP_ERR_SHAPE beyond */
#define AP_SUM_REPS_MAX (16 * 65535)
int ap_sum_reps_acc(const ap_bf16* x, float* out, int64_t n, int reps, ap_stream_t stream);
/* out[oy, ox, c] (+)= sum_iy wy[oy*hi + iy] * sum_ix wx[ox*wi + ix] * in[(iy*wi + ix)*C + c]   (fp32 NHWC grids, dense tap matrices wy [ho, hi],
 * wx [wo, wi]): VOLO.interpolate_pos_encoding (models/volo.py:580-596 -- F.interpolate(pos_embed, scale_factor, mode="bicubic") on every
 * forward whose token grid differs from the embedding's) with the bicubic taps of that call as the matrices; with the transposed
 * matrices and accumulate = 1 its backward, added into the embedding's gradient.  hi, wi <= 64 (AP_ERR_UNSUPPORTED beyond).  (ABI version 5) */
int ap_resample_grid(const float* in, int hi, int wi, const float* wy, const float* wx, float* out, int ho, int wo, int C, int accumulate,
                     ap_stream_t stream);

/* ---- fused BatchNorm2d + ReLU of the conv stem on NHWC bf16 rows [T = B*H*W, C] (models/volo.py:355-367;
 * SURVEY.md row N3).  training != 0: batch statistics (biased variance), running stats updated with
 * `momentum` (unbiased variance) as nn.BatchNorm2d; mean/rstd are outputs saved for backward.
 * training == 0: mean/rstd are INPUTS (running_mean, 1/sqrt(running_var+eps)).  C/8 must be a power of two. */
size_t ap_bn_relu_workspace(int64_t T, int C);
int ap_bn_relu_fwd(const ap_bf16* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                   int training, float momentum, float eps, ap_bf16* y, float* mean, float* rstd, int64_t T, int C,
                   void* workspace, size_t ws_bytes, ap_stream_t stream);
/* training-mode ap_bn_relu_fwd whose batch statistics come from `partial`: n_partial rows [2][C] of per-channel sums and sums
 * of squares of x, produced by the kernel that wrote x (ap_conv3x3_c64 with stats != NULL) -- saves the pass over x.
 * y NULL: statistics only (mean, rstd, running statistics); the consumer applies the normalisation itself (ap_conv3x3_c64_bn) */
int ap_bn_relu_fwd_partials(const ap_bf16* x, const float* partial, int n_partial, const float* gamma, const float* beta,
                            float* running_mean, float* running_var, float momentum, float eps, ap_bf16* y, float* mean, float* rstd,
                            int64_t T, int C, ap_stream_t stream);
/* dx = d(relu(bn(x)))/dx . dy ; dgamma/dbeta accumulated (+=) */
int ap_bn_relu_bwd(const ap_bf16* dy, const ap_bf16* x, const float* gamma, const float* beta, const float* mean,
                   const float* rstd, ap_bf16* dx, float* dgamma, float* dbeta, int64_t T, int C,
                   void* workspace, size_t ws_bytes, ap_stream_t stream);

/* (ABI version 6) ap_bn_relu_bwd that also writes act = relu(bn(x)) ([T, C] bf16, the arithmetic of ap_bn_relu_fwd): for a forward that
 * applied the BatchNorm inside its consumer (ap_gemm_nt_patch_bn) and never stored the activation -- the weight gradient of that
 * consumer then reads a plain tensor */
int ap_bn_relu_bwd_act(const ap_bf16* dy, const ap_bf16* x, const float* gamma, const float* beta, const float* mean,
                       const float* rstd, ap_bf16* dx, ap_bf16* act, float* dgamma, float* dbeta, int64_t T, int C,
                       void* workspace, size_t ws_bytes, ap_stream_t stream);
/* (ABI version 6) ap_bn_relu_bwd whose first pass has already happened: `partial` holds n_partial rows [2][C] of per-channel partial sums
 * (sum dz | sum dz * xhat, dz = dy where the ReLU passed) -- written by ap_conv3x3_c64_bwd_stats, the input-gradient convolution that
 * produced dy -- so only the finalize (dgamma / dbeta +=) and the dx pass run.  Replaces the backward of nn.BatchNorm2d + nn.ReLU at
 * reference models/volo.py:356-366 (autograd), one pass over dy and x shorter. */
int ap_bn_relu_bwd_partials(const ap_bf16* dy, const ap_bf16* x, const float* gamma, const float* beta, const float* mean,
                            const float* rstd, const float* partial, int n_partial, ap_bf16* dx, float* dgamma, float* dbeta,
                            int64_t T, int C, void* workspace, size_t ws_bytes, ap_stream_t stream);

/* ---- stem 3x3 convolutions in HIP (reference models/volo.py:355-367: the two
 * nn.Conv2d(hidden, hidden, 3, 1, 1, bias=False) of PatchEmbed at hidden = 64).  NHWC bf16 feature maps. */
/* fp32 OIHW [64][64][3][3] -> the two bf16 operand layouts of ap_conv3x3_c64: w_fwd [tap][co][ci] and
 * w_bwd [8 - tap][ci][co] (input gradient = the same convolution on flipped, transposed weights); 9*64*64 elements each */
int ap_conv3x3_c64_pack(const float* w_oihw, ap_bf16* w_fwd, ap_bf16* w_bwd, ap_stream_t stream);
/* y[B,H,W,64] = conv3x3(x[B,H,W,64], stride 1, zero pad 1) with packed weights (w_fwd: forward; w_bwd with x = dy: dx).
 * stats (nullable): float[ap_conv3x3_c64_stat_rows(B,H,W)][2][64]; every workgroup stores the per-channel sum and sum of
 * squares of its bf16 outputs to its row (the partial batch statistics of the BatchNorm that follows: ap_bn_relu_fwd_partials) */
int ap_conv3x3_c64_stat_rows(int B, int H, int W);
int ap_conv3x3_c64(const ap_bf16* x, const ap_bf16* w_packed, ap_bf16* y, int B, int H, int W, float* stats, ap_stream_t stream);
/* the same on the PRE-BatchNorm output of the previous stem convolution: the kernel applies relu((x - mean) * rstd * gamma + beta) (the
 * arithmetic of ap_bn_relu_fwd, rounded to bf16) to its input while staging it, pixels outside the image stay zero -- the activation
 * between the two convolutions (models/volo.py:358-359, 361-362) is never materialised.  bn_in NULL: plain ap_conv3x3_c64. */
typedef struct ap_bn_input { const float* mean; const float* rstd; const float* gamma; const float* beta; } ap_bn_input;   /* [64] each */
int ap_conv3x3_c64_bn(const ap_bf16* x, const ap_bn_input* bn_in, const ap_bf16* w_packed, ap_bf16* y, int B, int H, int W, float* stats,
                      ap_stream_t stream);

/* dw_oihw[64][64][3][3] (fp32) += weight gradient of ap_conv3x3_c64: x the layer input, dy the output gradient (both
 * [B,H,W,64] NHWC bf16).  Per-workgroup partial sums go to `workspace` and are added in a fixed order: no atomics. */
size_t ap_conv3x3_c64_wgrad_workspace(int B, int H, int W);
int ap_conv3x3_c64_wgrad(const ap_bf16* x, const ap_bf16* dy, float* dw_oihw, int B, int H, int W, void* workspace, size_t ws_bytes,
                         ap_stream_t stream);
/* the same for a layer whose input was relu(bn(x)) of ap_conv3x3_c64_bn: x is the pre-BatchNorm tensor */
int ap_conv3x3_c64_wgrad_bn(const ap_bf16* x, const ap_bn_input* bn_in, const ap_bf16* dy, float* dw_oihw, int B, int H, int W, void* workspace,
                            size_t ws_bytes, ap_stream_t stream);

/* (ABI version 6) the INPUT-GRADIENT convolution of a stem layer (dz on w_bwd of ap_conv3x3_c64_pack -> da, as ap_conv3x3_c64) whose
 * epilogue also runs the first pass of the backward of the BatchNorm + ReLU BELOW the layer (a = relu(bn(z_below)), reference
 * models/volo.py:356-366): stats = float[ap_conv3x3_c64_stat_rows(B,H,W)][2][64], per-workgroup partial sums (sum dzb | sum dzb * xhat,
 * dzb = the bf16-rounded da where bn(z_below) > 0), the `partial` argument of ap_bn_relu_bwd_partials */
int ap_conv3x3_c64_bwd_stats(const ap_bf16* dz, const ap_bf16* w_packed_bwd, ap_bf16* da, int B, int H, int W, const ap_bf16* z_below,
                             const ap_bn_input* bn_below, float* stats, ap_stream_t stream);

/* ---- first stem convolution in HIP: 7x7 / stride 2 / pad 3, 3 -> 64, no bias (models/volo.py:355-357) on the space-to-depth input
 * xs[B, H, W, 16] (bf16; H, W = half the image size; channel (sy*2+sx)*3+c = pixel (2Y+sy, 2X+sx) channel c, 12..15 zero) */
/* fp32 [B,3,Hi,Wi] -> xs [B,Ho/2,Wo/2,16]: the bilinear resize of ap_resize_bilinear_nhwc written in that layout (Ho, Wo even) */
int ap_resize_bilinear_s2d16(const float* x, ap_bf16* xs, int B, int Hi, int Wi, int Ho, int Wo, ap_stream_t stream);
/* fp32 OIHW [64][3][7][7] -> packed bf16 operand (16*64*16 elements) */
int ap_conv7_pack(const float* w_oihw, ap_bf16* w_packed, ap_stream_t stream);
/* y[B,H,W,64] = conv7x7/s2(image) ; stats as for ap_conv3x3_c64: float[ap_conv7_s2d_stat_rows(B,H,W)][2][64] or NULL */
int ap_conv7_s2d_stat_rows(int B, int H, int W);
int ap_conv7_s2d(const ap_bf16* xs, const ap_bf16* w_packed, ap_bf16* y, int B, int H, int W, float* stats, ap_stream_t stream);
/* dw_oihw[64][3][7][7] (fp32) += weight gradient; dz = output gradient [B,H,W,64]; per-workgroup slabs in `workspace`, ordered reduction */
size_t ap_conv7_s2d_wgrad_workspace(int B, int H, int W);
int ap_conv7_s2d_wgrad(const ap_bf16* xs, const ap_bf16* dz, float* dw_oihw, int B, int H, int W, void* workspace, size_t ws_bytes,
                       ap_stream_t stream);
/* (ABI version 6) the same two with an explicit pixel stride (elements) of y / dz: 64 output channels written into / read from a wider
 * NHWC tensor.  The 128-wide stem of VOLO-D4 / D5 (models/volo.py:799-821: nn.Conv2d(3, 128, 7, 2, 3)) is two such launches on the
 * channel halves: weights w_oihw + h * 64 * 147, y + 64 h with ldy = 128 (stats per half: [rows][2][64]) */
int ap_conv7_s2d_ld(const ap_bf16* xs, const ap_bf16* w_packed, ap_bf16* y, int ldy, int B, int H, int W, float* stats, ap_stream_t stream);
int ap_conv7_s2d_wgrad_ld(const ap_bf16* xs, const ap_bf16* dz, int lddz, float* dw_oihw, int B, int H, int W, void* workspace, size_t ws_bytes,
                          ap_stream_t stream);

/* ---- (ABI version 6) 3x3 / stride 1 / pad 1 convolution at 128 channels in HIP: the stem of VOLO-D4 / D5 (stem_hidden_dim = 128,
 * models/volo.py:355-367,803,818; BASELINE configs[4]) -- csrc/conv128.hip: the input patch in LDS, the weights streamed in 18
 * (tap, 64-input-channel) slabs.  Contracts as the 64-channel family above.
 * pack: fp32 OIHW [128][128][3][3] -> w_fwd / w_bwd, 9 * 128 * 128 bf16 each (slab layouts of the kernel) */
int ap_conv3x3_c128_pack(const float* w_oihw, ap_bf16* w_fwd, ap_bf16* w_bwd, ap_stream_t stream);
/* y[B,H,W,128] = conv3x3(x[B,H,W,128]) (w_fwd: forward; w_bwd with x = dy: the input gradient); stats (nullable):
 * float[ap_conv3x3_c128_stat_rows(B,H,W)][2][128] partial sums / sums of squares of the bf16-rounded outputs (ap_bn_relu_fwd_partials) */
int ap_conv3x3_c128_stat_rows(int B, int H, int W);
int ap_conv3x3_c128(const ap_bf16* x, const ap_bf16* w_packed, ap_bf16* y, int B, int H, int W, float* stats, ap_stream_t stream);
/* dw_oihw[128][128][3][3] (fp32) += weight gradient: the 64-channel kernel on the four (output half, input half) quadrants */
size_t ap_conv3x3_c128_wgrad_workspace(int B, int H, int W);
int ap_conv3x3_c128_wgrad(const ap_bf16* x, const ap_bf16* dy, float* dw_oihw, int B, int H, int W, void* workspace, size_t ws_bytes,
                          ap_stream_t stream);

/* ---- fused optimizer step: AdamW (torch.optim.AdamW semantics, main_prog.py:484)
 * + n_ema <= 4 ModelEmaV2 updates (main_prog.py:1030-1033) over one flat fp32 slab of n parameters
 * (n % 4 == 0).  wd_mask[i] != 0 selects decoupled weight decay for element i; `ema` / `ema_decay`
 * are HOST arrays of n_ema device pointers / decays; `step` is the 1-based update count. */
/* sum of squares of a flat fp32 slab (16-byte aligned): out[0] = sum x[i]^2, deterministic (1024 ordered partials in `workspace` of
 * ap_sumsq_workspace() bytes).  The global gradient norm of torch.nn.utils.clip_grad_norm_ (timm dispatch_clip_grad 'norm',
 * prog/scaler.py:60-68, main_prog.py:129-132,1019-1027) is one pass over the gradient slab.  (ABI version 6) */
size_t ap_sumsq_workspace(void);
int ap_sumsq_f32(const float* x, int64_t n, float* out, void* workspace, size_t ws_bytes, ap_stream_t stream);
/* gradient clipping is folded into the update (ABI version 6): gnorm_sq (nullable DEVICE scalar = ap_sumsq_f32 of g) with max_norm > 0
 * scales the gradient by min(1, max_norm / (grad_scale * sqrt(gnorm_sq[0]) + 1e-6)) -- clip_grad_norm_ on the MEAN gradient, read on
 * the device (no host round trip); clip_value > 0 clamps every element of the scaled gradient to [-clip_value, clip_value]
 * (clip_grad_value_); 0 / NULL: no clipping */
int ap_adamw_ema_step(float* p, const float* g, float* m, float* v, const unsigned char* wd_mask, int64_t n,
                      float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                      float grad_scale /* g is multiplied by this first: 1/world_size turns the all-reduced SUM into the mean */,
                      const float* gnorm_sq, float max_norm, float clip_value,
                      const float* step_scalars_dev /* nullable DEVICE float[3] {lr, 1 - beta1^step, sqrt(1 - beta2^step)}: overrides lr / step
                                                     * (the graph-replayable step: the scheduler's lr and the step count change per replay) */,
                      float* const* ema, const float* ema_decay, int n_ema,
                      ap_bf16* p_bf16 /* nullable: bf16 copy of the updated parameters, same offsets */,
                      ap_stream_t stream);

/* ---- non-finite gradient guard of the fused step (additive in ABI version 7).  The reference trains under apex's dynamic loss scaler,
 * which skips optimizer.step() for an iteration whose backward pass produced an inf or a NaN (prog/scaler.py:20-26) while
 * ModelEmaV2.update still runs (main_prog.py:1030-1033).  ap_grad_health is one pass over the fp32 gradient slab g[n] (16-byte aligned,
 * any n) against a DEVICE table seg_off[n_seg + 1] of ascending segment bounds (seg_off[0] = 0, seg_off[n_seg] = n; one segment per
 * parameter tensor in slab order; lengths arbitrary, empty segments allowed):
 *   seg_sumsq[s]     (fp64)  sum of x^2 over the FINITE elements of segment s (x^2 formed in fp64: a finite 3e38 is an ordinary element)
 *   seg_nonfinite[s] (int32) elements of segment s whose exponent field is all ones (+-inf, NaN)
 * and the step's decision in `state`, committed by the last thread of the pass:
 *   nonfinite = this step's total; total == 0: applied += 1, consecutive = 0; else: skipped += 1, consecutive += 1;
 *   bc1 = 1 - beta1^applied, bc2_sqrt = sqrt(1 - beta2^applied) as ap_adamw_ema_step forms them (double arithmetic on the fp32 betas,
 *   rounded once to float).
 * The counters live on the device: zero the record once, the host never writes it during a run.  Deterministic: ordered partials in
 * `workspace` (ap_grad_health_workspace bytes, 8-byte aligned), no floating-point atomics; nothing is allocated. */
typedef struct ap_guard_state {
    int32_t nonfinite, applied, skipped, consecutive;
    float bc1, bc2_sqrt;
    int32_t reserved[2];
} ap_guard_state;
size_t ap_grad_health_workspace(int64_t n, int n_seg);
int ap_grad_health(const float* g, int64_t n, const int64_t* seg_off, int n_seg, double* seg_sumsq, int32_t* seg_nonfinite,
                   ap_guard_state* state, float beta1, float beta2, void* workspace, size_t ws_bytes, ap_stream_t stream);
/* ap_adamw_ema_step with the decision of ap_grad_health (same stream, launched before it): state->nonfinite == 0 is the ordinary update
 * with the record's bias corrections (`step` is only checked, of step_scalars_dev only the learning rate is read); otherwise p, m, v and
 * p_bf16 are not written at all and every EMA copy takes its lerp towards the unchanged parameters. */
int ap_adamw_ema_step_guarded(float* p, const float* g, float* m, float* v, const unsigned char* wd_mask, int64_t n,
                              float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                              const float* gnorm_sq, float max_norm, float clip_value, const float* step_scalars_dev,
                              float* const* ema, const float* ema_decay, int n_ema, ap_bf16* p_bf16, const ap_guard_state* guard,
                              ap_stream_t stream);
/* ap_adamw_ema_step / _guarded that also writes bf16 copies of EMA slabs (additive in ABI version 7).  The reference keeps its EMA copies
 * as ModelEmaV2 MODULES it can run (main_prog.py:1030-1033); a forward pass here reads bf16 weights, so an EMA slab becomes a network to
 * compute with -- a teacher -- once its bf16 copy exists.  ema_bf16 is a HOST array of 4 device pointers: entry e is the bf16 slab of
 * EMA copy e (n elements, same offsets, 8-byte aligned), written with the rounding p_bf16 gets from the lerp result in registers, or
 * NULL for "do not emit this copy" (four NULL entries: the launch of ap_adamw_ema_step / _guarded itself).  guard_or_null: NULL is ap_adamw_ema_step, otherwise ap_adamw_ema_step_guarded (a skipped step
 * moves the EMA copies and writes their bf16 copies).  Refused before anything is launched: ema_bf16 == NULL (AP_ERR_NULL); an entry
 * that is not 8-byte aligned, or a non-null entry at an index >= n_ema (AP_ERR_SHAPE). */
int ap_adamw_ema_step_ema16(float* p, const float* g, float* m, float* v, const unsigned char* wd_mask, int64_t n,
                            float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                            const float* gnorm_sq, float max_norm, float clip_value, const float* step_scalars_dev,
                            float* const* ema, const float* ema_decay, int n_ema, ap_bf16* p_bf16, ap_bf16* const* ema_bf16,
                            const ap_guard_state* guard_or_null, ap_stream_t stream);
/* The same step with one learning rate and one weight decay PER PARAMETER GROUP (additive in ABI version 7): torch.optim.AdamW with
 * param_groups -- layer-wise learning-rate decay, a head trained faster than the body, a frozen group (lr 0).  In the place of wd_mask
 * the kernel reads group_id[n], one byte per element (the same traffic), and group_tab_dev[n_groups], a DEVICE table of {lr,
 * weight_decay} fp32 pairs (8-byte aligned, 1 <= n_groups <= 256).  Element i is decayed by 1 - lr*wd and stepped by lr / (1 - beta1^t)
 * of group group_id[i]; every workgroup forms the two numbers per group once, in LDS.  Groups may change at any element: tensors of odd
 * length sit back to back in the slab.  A byte group_id[i] >= n_groups is the CALLER's error: the kernel cannot afford to check the
 * bytes and would read LDS it never wrote (no memory outside the workgroup's own table of 256 entries).
 * The `lr` and `weight_decay` arguments and step_scalars_dev[0] are NOT read; the bias corrections come from where they come in the
 * other entry points (the host's `step`, step_scalars_dev[1..2], or the guard record).  Clipping (gnorm_sq / max_norm, clip_value) and
 * grad_scale are global as before; the guard, the EMA lerps, p_bf16 and ema_bf16 are unchanged.  ema_bf16 is NULLABLE here (NULL or
 * four NULL entries: nothing is emitted), guard_or_null selects the guarded step.  With a table in which every decayed element's group
 * is {lr, wd} and every other element's {lr, 0} all outputs are bit for bit those of the entry points above.
 * Refused before anything is launched: group_id == NULL or group_tab_dev == NULL (AP_ERR_NULL); n_groups < 1 or > 256, a table that is
 * not 8-byte aligned (AP_ERR_SHAPE); and everything ap_adamw_ema_step_ema16 refuses. */
int ap_adamw_ema_step_groups(float* p, const float* g, float* m, float* v, const unsigned char* group_id, int64_t n,
                             float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                             const float* gnorm_sq, float max_norm, float clip_value, const float* step_scalars_dev,
                             float* const* ema, const float* ema_decay, int n_ema, ap_bf16* p_bf16, ap_bf16* const* ema_bf16,
                             const ap_guard_state* guard_or_null, const float* group_tab_dev, int n_groups, ap_stream_t stream);
/* ---- adaptive gradient clipping (AGC) on the flat gradient slab (additive in ABI version 7; csrc/agc.hip).  The reference's
 * `--clip-mode agc` (main_prog.py:129-132, 1019-1027) calls timm 0.4.5's adaptive_clip_grad between backward and optimizer.step().  The
 * rule below restates that function and its unitwise_norm from knowledge of the code; it is NOT byte-checked against timm (timm is not a
 * dependency of this project); tests/_agc_ref.py pins it in fp64.
 *   Units.   A parameter tensor with ndim <= 1 is one unit; a tensor with ndim >= 2 has shape[0] units, each the numel / shape[0]
 *            contiguous elements of one leading index (a Linear [out, in]: `out` rows; a conv [O, I, k, k]: O units of I k k;
 *            pos_embed [1, g, g, C] and cls_token [1, 1, C]: one unit each).  The caller describes them by a DEVICE table
 *            unit_off[n_units + 1] that ascends from 0 to n and covers the slab exactly; a unit may start at any offset mod 4.
 *   Rule.    Per unit pn = ||p||_2 and gn = grad_scale * ||g||_2 (grad_scale: the pending 1/world of a deferred data-parallel mean --
 *            the rule acts on the MEAN gradient while the slab holds the SUM; 1 otherwise).  max_norm = max(pn, eps) * clip_factor.
 *            gn < max_norm: the unit is left as it is.  Otherwise every element of g is multiplied by f = max_norm / max(gn, 1e-6)
 *            (the slab stays the SUM; the pending scale stays pending).  timm's defaults: clip_factor 0.01, eps 1e-3.
 *   Skipped. unit_skip[u] != 0 leaves unit u alone (timm's exclude_head: an excluded tensor is ONE skipped unit).
 *   Deviation 1 (non-finite units).  A unit with an inf or NaN gradient element is left bit for bit as it is and counted; timm would
 *            multiply it by 0 or NaN, turning an inf into NaN and zeroing its finite neighbours in front of the non-finite guard
 *            (ap_grad_health), which reports the finite part per tensor.
 *   Deviation 2 (arithmetic).  Both sums are of exact squares in fp64, the bound and the quotient are formed in fp64, and f is rounded
 *            to fp32 once; timm computes all of it in the gradient's dtype.  p is expected finite.
 * p (the fp32 master parameters, the same offsets as g) is only read.  Elements of units that are not clipped are never stored: they keep
 * their bits, and in a healthy run the pass is close to read-only.  unit_factor_or_null[n_units] receives the factor applied, 1.0 for
 * every unit left alone; counts_or_null[2] receives {clipped units, non-finite units} (int32; zeroed by a one-wave launch in front of the pass).
 * Units of up to ap_agc_short_max() elements are read once, one wave per unit, g kept in registers between the norm and the
 * store; a longer unit takes one workgroup and a second walk over g.  Fixed reduction order, no floating-point atomics: two launches on
 * the same inputs write the same bits.  No workspace, nothing allocated; runs under stream capture.  A table entry outside [0, n] or
 * out of order is clamped: nothing outside the slabs is read or written.
 * Refused before anything is launched: g, p, unit_off or unit_skip NULL (AP_ERR_NULL); n <= 0, n_units <= 0, g or p not 16-byte
 * aligned, unit_off not 8-byte or an output not 4-byte aligned, clip_factor or grad_scale not positive and finite, eps negative or not
 * finite (AP_ERR_SHAPE). */
int ap_agc_clip(float* g, const float* p, int64_t n, const int64_t* unit_off, const uint8_t* unit_skip, int n_units,
                float clip_factor, float eps, float grad_scale, float* unit_factor_or_null, int32_t* counts_or_null,
                ap_stream_t stream);
int ap_agc_short_max(void);
/* ---- fused LAMB + EMA step on the flat slabs, one trust ratio per parameter tensor (additive in ABI version 7; csrc/lamb.hip).  The
 * reference takes its optimizer from `--opt` (main_prog.py:119, timm's create_optimizer); `fusedlamb` / `lamb` there are apex's FusedLAMB
 * and timm's Lamb.  The rule below restates those two from knowledge of their code; it is NOT byte-checked against either (neither is a
 * dependency of this project); tests/_lamb_ref.py pins it in fp64.
 *   Per element, with t, bc1 = 1 - beta1^t and sqrt(bc2) = sqrt(1 - beta2^t) as ap_adamw_ema_step gets them (the host's `step`,
 *   step_scalars_dev[1..2], or the guard record) and wd, lr_eff of the element's group (group_tab_dev, as ap_adamw_ema_step_groups):
 *     gh = the AdamW kernel's gradient: grad_scale * g, times min(1, max_norm / (norm + 1e-6)) with gnorm_sq, or clamped to +-clip_value
 *     m' = beta1 m + (1 - beta1) gh          v' = beta2 v + (1 - beta2) gh^2
 *     r  = m' / (sqrt(v') / sqrt(bc2) + eps)
 *     u  = r / bc1 + wd * p
 *   Per parameter tensor T (the WHOLE tensor: LAMB's unit, not AGC's rows):
 *     wn = sqrt(sum p^2), un = sqrt(sum u^2)     fp64 sums of the exact squares of the fp32 values, in a fixed order
 *     phi_T = wn / un  if adapt and wn > 0 and un > 0, else 1       adapt = always_adapt or wd != 0 (wd: the group of the tensor's first element)
 *     phi_T = min(phi_T, 1) if trust_clip         phi_T is formed in fp64 and rounded to fp32 once
 *     p' = p - (lr_eff * phi_T) * u
 *   then every EMA copy e' = d e + (1 - d) p', p_bf16 and the emitted ema_bf16 copies, the bf16 roundings of the stored fp32 values.
 *   `adapt` is apex's rule without use_nvlamb; always_adapt is timm's name for switching it off; trust_clip is timm's flag.
 *   Deviation 1 (pre-normalisation).  apex divides the gradient by max(global norm / max_grad_norm, 1) by default (max_grad_norm 1.0).
 *            Here that is gnorm_sq / max_norm = 1 -- clip_grad_norm_'s coefficient min(1, c / (norm + 1e-6)); apex has no 1e-6 -- and
 *            it is off unless asked for.
 *   Deviation 2 (arithmetic).  Both libraries form the two norms in fp32 and the ratio in fp32; here the sums are exact squares in
 *            fp64, the ratio is fp64 and rounded once.  m', v' and u take fused multiply-adds where csrc/lamb.hip spells them out.
 *   Non-finite inputs follow the formula (comparisons with NaN are false: such a tensor takes phi = 1); the guard is the remedy.
 * Work is cut into chunks the HOST describes once: chunk_tab_dev[n_chunks] of {int64 start, int32 length, int32 tensor} (16 bytes each,
 * 16-byte aligned), every chunk at most ap_lamb_chunk() consecutive elements of ONE tensor, tensors ascending, the chunks of a tensor
 * consecutive; tensor_first_dev[n_tensors + 1] (int32) holds every tensor's first chunk.  Entries are clamped into [0, n): a malformed
 * table reads and writes nothing outside the slabs.  Elements no chunk covers (the slab's pad) are never written in any slab.
 * Three launches: the norms (reads p, g, m, v, group_id; two fp64 partials per chunk into `workspace`, ap_lamb_workspace(n_chunks) bytes,
 * 8-byte aligned, no initial contents assumed), the trust ratios (partials added in ascending chunk order; trust_out[3][n_tensors] =
 * wn, un, phi as fp32), the update.  g is only read.  No floating-point atomics: two calls on the same inputs write the same bits.
 * guard_or_null says non-finite: p, m, v, p_bf16 and trust_out are not written, the EMA copies take their lerp towards the unchanged p.
 * n is the number of elements the chunks may cover (any n > 0): every slab holds at least n elements, and one padded to a multiple of 4
 * may be longer than g; all fp32 slabs 16-byte, the bf16 slabs 8-byte, group_id 4-byte aligned at the same offsets.
 * ema_bf16 is nullable (an array of 4, NULL entries: not emitted).  grid_cap > 0 caps the workgroups of the two sweeping launches (0: the
 * default, 2048); `passes` selects launches for measurements (bit 0 norms, bit 1 trust ratios, bit 2 update; 0: all three).
 * Nothing is allocated; runs under stream capture.  Refused before anything is launched: a NULL slab, table, output or workspace
 * (AP_ERR_NULL); n, n_chunks or n_tensors < 1, n_ema outside 0..4, n_groups outside 1..256, step < 1, gnorm_sq without max_norm > 0, a
 * workspace that is too small, a misaligned pointer, an ema_bf16 entry at an index >= n_ema, grid_cap < 0, passes outside 0..7
 * (AP_ERR_SHAPE). */
int ap_lamb_chunk(void);
size_t ap_lamb_workspace(int n_chunks);
int ap_lamb_ema_step(float* p, const float* g, float* m, float* v, const uint8_t* group_id, int64_t n,
                     float beta1, float beta2, float eps, int step, float grad_scale,
                     const float* gnorm_sq, float max_norm, float clip_value, const float* step_scalars_dev,
                     float* const* ema, const float* ema_decay, int n_ema, ap_bf16* p_bf16, ap_bf16* const* ema_bf16_or_null,
                     const ap_guard_state* guard_or_null, const float* group_tab_dev, int n_groups,
                     const void* chunk_tab_dev, int n_chunks, const int32_t* tensor_first_dev, int n_tensors,
                     int always_adapt, int trust_clip, float* trust_out, void* workspace, size_t ws_bytes,
                     int grid_cap, int passes, ap_stream_t stream);
/* transpose `count` bf16 matrices of one slab in one launch: desc_dev = device array of
 * {int64 src_off, int64 dst_off, int rows, int cols, int ld_dst, int first_tile} (32x32 tiles, first_tile
 * = running tile prefix); dst[dst_off + c*ld_dst + r] = src[src_off + r*cols + c], pad columns zeroed */
int ap_batched_transpose_bf16(const ap_bf16* src, ap_bf16* dst, const void* desc_dev, int count, int total_tiles,
                              ap_stream_t stream);

/* ---- a loader's batch, prepared on the device in one launch (additive in ABI version 7; csrc/input_prep.hip).  What the reference does
 * between its loader and its model every step: timm's PrefetchLoader (.float().sub_(mean).div_(std), RandomErasing on the GPU), the
 * collate-time Mixup / CutMix of main_prog.py:195-207,978-979 and the resize of main_prog.py:973-974.  uint8 in, the stem's bf16 layout
 * out.  The value of source pixel (b, c, y, x), in this order:
 *   1. normalise   n = table[c][u8]: `table` is 3 x 256 fp32, (v - 255 mean[c]) / (255 std[c]) computed by the caller
 *   2. mix         (mix_enabled != 0; mode read from `params` in DEVICE memory) with the partner image B-1-b (timm's x.flip(0)):
 *                  mixup m = lam * n[b] + (1 - lam) * n[B-1-b]; cutmix m = n[B-1-b] inside rows [yl, yh) x columns [xl, xh), n[b] outside
 *   3. erase       up to n_boxes records per image in DEVICE memory (`boxes`: [B][n_boxes] records of 8 x 4 bytes: int32 top, left, h, w,
 *                  fp32 v0, v1, v2, one unused word; h == 0: no box; a later record wins where two overlap).  Inside a box the value of
 *                  channel c becomes 0 (AP_ERASE_CONST), the record's v[c] (AP_ERASE_RAND) or a standard normal that is a pure function
 *                  of (seed, b, c, y, x) (AP_ERASE_PIXEL: Philox-4x32-10 on the counter (x, y, b, 0) keyed by the seed, Box-Muller)
 *   4. resize      bilinear, align_corners = False, to Ho x Wo, with the arithmetic of ap_resize_bilinear_s2d16 / ap_resize_bilinear_nhwc
 *                  operation for operation: with no mix and no erase the output is bit-identical to those kernels fed the normalised tensor
 * params (DEVICE, 16 x 4 bytes): int32 [0] mix mode (0 none, 1 mixup, 2 cutmix), fp32 [1] lam, int32 [2..5] yl, yh, xl, xh,
 * uint32 [6..7] seed, fp32 [8] 1 - lam; the rest unused.  A graph replay sees whatever the block holds when it runs.
 * boxes_host (nullable): a host copy of the records; when given every record is checked against the image (AP_ERR_SHAPE).  The kernel
 * only ever COMPARES coordinates with a box, so a record it was not shown cannot make it read or write out of bounds.
 * u8 must be 16-byte aligned.  out_layout AP_PREP_S2D16 needs even Ho, Wo; n_boxes <= 8; B == 0 succeeds without a launch. */
enum { AP_PREP_NCHW = 0, AP_PREP_NHWC = 1 };                    /* in_layout: u8 [B,3,Hi,Wi] / [B,Hi,Wi,3] */
enum { AP_PREP_S2D16 = 0, AP_PREP_OUT_NHWC = 1 };               /* out_layout: bf16 [B,Ho/2,Wo/2,16] / [B,Ho,Wo,3] */
enum { AP_ERASE_CONST = 0, AP_ERASE_RAND = 1, AP_ERASE_PIXEL = 2 };
#define AP_PREP_MAX_BOXES 8
typedef struct ap_input_prep_args {
    const unsigned char* u8; int in_layout; int B, Hi, Wi;
    ap_bf16* out; int out_layout; int Ho, Wo;
    const float* table;              /* DEVICE fp32 [3][256] */
    const int* params;               /* DEVICE block above; NULL: no mix, seed 0 */
    int mix_enabled;                 /* 0: the mix mode of `params` is ignored (no partner image is staged) */
    const int* boxes;                /* DEVICE records, NULL with n_boxes == 0 */
    const int* boxes_host;           /* nullable host copy, validated */
    int n_boxes, erase_mode;
} ap_input_prep_args;
int ap_input_prep(const ap_input_prep_args* args, ap_stream_t stream);

/* ---- per-image crop box + horizontal flip + bilinear resize of a uint8 batch in one launch (additive in ABI version 7; csrc/crop.hip).
 * The random-resized crop and flip of the reference's loader, whose per-stage scale range it realises by rebuilding the loader
 * (main_prog.py:651-653, 1513-1515; the rebuilds at :711-712, :840-846).  u8: [B,3,Hi,Wi] (AP_PREP_NCHW) or [B,Hi,Wi,3] (AP_PREP_NHWC),
 * 16-byte aligned; out: uint8 [B,3,S,S] / [B,S,S,3] in the same layout, any S >= 1, any alignment.
 * records (DEVICE): B records of 8 int32 words: top, left, h, w, flip, then three zero words.  Image b's output is the box
 * rows [top, top + h) x columns [left, left + w) resized to S x S as if the image were cropped first (fp32, bilinear, align_corners = False;
 * NO antialiasing when scaling down, as the reference's own 224 -> r F.interpolate): for output column ox, o = flip ? S-1-ox : ox,
 * f = max((o + 0.5) * (w / S) - 0.5, 0), x0 = min(floor(f), w-1), x1 = min(x0+1, w-1), lx = f - x0; rows the same with h, never flipped;
 * v = (1-ly)*((1-lx)*p00 + lx*p01) + ly*((1-lx)*p10 + lx*p11); out = clamp(rint(v), 0, 255), half to even; every operation rounded.
 * records_host (nullable): a host copy of the records; when given every record is checked against the image before the launch
 * (h, w >= 1, the box inside Hi x Wi, flip in {0, 1}: AP_ERR_SHAPE).  The kernel clamps every record into the image, so a record it
 * was not shown on the host cannot make it read or write out of bounds; it reads nothing past the last byte of the batch.
 * AP_ERR_NULL: args, u8, out or records NULL.  AP_ERR_SHAPE: a non-positive size, a bad layout, a misaligned u8, a bad host record, more
 * than 2^40 input bytes.  AP_ERR_UNSUPPORTED: the source rows of one output row exceed the 60 KB of LDS a launch takes (the budget depends
 * on Hi, Wi, S and the layout alone, never on the records).  B == 0 succeeds without a launch.  Every check comes before the launch. */
typedef struct ap_crop_resize_args {
    const unsigned char* u8; int layout; int B, Hi, Wi;
    unsigned char* out; int S;
    const int* records;              /* DEVICE [B][8] */
    const int* records_host;         /* nullable host copy, validated */
} ap_crop_resize_args;
int ap_crop_resize_u8(const ap_crop_resize_args* args, ap_stream_t stream);

/* ---- the same launch with Pillow's ANTIALIASED bilinear / bicubic filters, byte for byte (additive in ABI version 7; csrc/resample.hip).
 * The resample of the reference's loader: timm's RandomResizedCropAndInterpolation is Pillow's Image.resize, `--train-interpolation random`
 * picks bilinear or bicubic per image (main_prog.py:211, :632-658), validation is bicubic (models/volo.py:35-44).  Arguments as
 * ap_crop_resize_u8's.  records (DEVICE): B records of 8 int32 words: top, left, h, w, flip, filter, then two zero words; filter is
 * AP_RESAMPLE_BILINEAR or AP_RESAMPLE_BICUBIC and may differ from image to image.  Image b's output is what Pillow's
 * Image.crop(box).resize((S, S), filter) gives in mode RGB: two separable passes, the horizontal one first and ROUNDED TO UINT8, the
 * vertical one on its result.  For one axis of box extent n (w or h), in float64 with every operation rounded on its own:
 *     scale = n / S;  fs = max(scale, 1.0);  support = sup0 * fs;  ss = 1.0 / fs                  sup0: 1.0 bilinear, 2.0 bicubic
 *     for o in 0 .. S-1:
 *         center = (o + 0.5) * scale
 *         xmin = max((int)(center - support + 0.5), 0);  xmax = min((int)(center + support + 0.5), n)             C truncation
 *         k[i] = filt((i + xmin - center + 0.5) * ss)  for i in 0 .. xmax - xmin - 1
 *         ww = k[0] + k[1] + ... in this order;  if ww != 0: k[i] = k[i] / ww
 *         K[i] = (int)(k[i] * 4194304.0 + (k[i] < 0 ? -0.5 : 0.5))                                2^22, C truncation
 *         out[o] = clip((2097152 + sum_i src[xmin + i] * K[i]) >> 22, 0, 255)                     int32, arithmetic shift
 *     bilinear: x = |x|;  x < 1 ? 1 - x : 0
 *     bicubic (a = -0.5): x = |x|;  x < 1 ? ((a + 2) x - (a + 3)) x x + 1 : x < 2 ? (((x - 5) x + 8) x - 4) a : 0
 * The support is clipped to the BOX, not the image: the image is cropped first, as timm's F.resized_crop does.  The flip acts on the
 * result: output column ox of a flipped image is column S - 1 - ox of the resampled box (timm resizes, then flips; resampling a mirrored
 * box gives other bytes).  Rows are never flipped.  A box with h = w = S comes back as the slice under both filters.
 * records_host (nullable): as ap_crop_resize_u8's, and the filter must be 1 or 2 (AP_ERR_SHAPE).  The kernel clamps every record into the
 * image and any other filter code to AP_RESAMPLE_BILINEAR, so a record it was not shown on the host cannot make it read or write out of
 * bounds; it reads nothing past the last byte of the batch.
 * AP_ERR_NULL, AP_ERR_SHAPE: as ap_crop_resize_u8.  AP_ERR_UNSUPPORTED: a workgroup keeps in LDS, for tr >= 1 output rows of the whole
 * image under bicubic, the box rows they read (ceil((tr - 1) Hi / S + 4 max(Hi / S, 1)) + 2, at most Hi, of Wi pixels plus 30 bytes per
 * plane), the same number of intermediate rows of 3 S bytes and both coefficient tables (S windows of ceil(2 max(Wi / S, 1)) * 2 + 1
 * int32, tr of ceil(2 max(Hi / S, 1)) * 2 + 1); when that exceeds 80 KB at tr = 1, or the runtime refuses more than 64 KB to a launch.
 * The budget depends on Hi, Wi, S and the layout alone, never on the records.  B == 0 succeeds without a launch.  Every check comes
 * before the launch. */
enum { AP_RESAMPLE_BILINEAR = 1, AP_RESAMPLE_BICUBIC = 2 };      /* word 5 of a record */
typedef struct ap_crop_resample_args {
    const unsigned char* u8; int layout; int B, Hi, Wi;
    unsigned char* out; int S;
    const int* records;              /* DEVICE [B][8] */
    const int* records_host;         /* nullable host copy, validated */
} ap_crop_resample_args;
int ap_crop_resample_u8(const ap_crop_resample_args* args, ap_stream_t stream);

/* ---- RandAugment on a uint8 batch, byte for byte what Pillow makes of an RGB image (additive in ABI version 7; csrc/randaug.hip).
 * The auto-augment step of the reference's loader (timm's rand_augment_transform, `--aa rand-m9-mstd0.5-inc1`), which sits between the
 * random-resized crop and the normalisation and whose magnitude AutoProg ramps per stage by rebuilding the loader (main_prog.py:651-656,
 * 1443-1518).  u8: [B,3,S,S] (AP_PREP_NCHW) or [B,S,S,3] (AP_PREP_NHWC), any alignment, never written; out: the same shape and layout;
 * scratch: the same size again, needed when n_layers > 1 (its contents afterwards are unspecified).  u8, out and scratch are distinct.
 * records (DEVICE): B x n_layers records of AP_RANDAUG_RECORD_WORDS = 16 int32 words, image b's layer j at record b * n_layers + j.  The
 * layers of an image are applied in order, one launch per layer.  A record:
 *     word 0      op code, AP_RA_*
 *     word 1      resample filter of AP_RA_AFFINE: AP_RESAMPLE_BILINEAR or AP_RESAMPLE_BICUBIC; 0 for the other ops
 *     word 2      int argument: Solarize's threshold t (0..256), SolarizeAdd's a, Posterize's bits
 *     word 3      float32 argument (its bit pattern): the factor f of Brightness / Contrast / Color / Sharpness
 *     words 4-15  six float64 m0 .. m5, little endian (word 4 the low half of m0): the matrix of AP_RA_AFFINE
 * fill: the colour (R, G, B) of pixels an affine op maps from outside the image.  "trunc" is C's conversion toward zero.
 *   NONE          copy.
 *   table ops     out = lut[c][in], one table of 256 entries per channel:
 *     INVERT        255 - i
 *     SOLARIZE      i < t ? i : 255 - i
 *     SOLARIZE_ADD  i < 128 ? min(255, i + a) : i
 *     POSTERIZE     i & ~(2^(8 - bits) - 1); bits = 0 gives black, bits >= 8 the identity
 *     BRIGHTNESS    blend(0, i, f)
 *     CONTRAST      blend(m, i, f) with m = trunc((double)(sum of L over the image) / (double)(S S) + 0.5),
 *                   L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16
 *     AUTOCONTRAST  lo, hi = smallest, largest value of the channel; hi <= lo: identity; else in float64, every operation rounded on its
 *                   own: scale = 255.0 / (hi - lo); offset = -lo * scale; lut[i] = clip(trunc(i * scale + offset), 0, 255)
 *     EQUALIZE      h = the channel's histogram; at most one non-empty bin: identity; step = (S S - h[last non-empty bin]) / 255 (integer);
 *                   step == 0: identity; else n = step / 2; for i = 0 .. 255: lut[i] = min(255, n / step); n += h[i]
 *   COLOR         out[c] = blend(L, in[c], f) with the pixel's own L.
 *   SHARPNESS     out = blend(smooth, in, f); smooth = in on rows and columns 0 and S - 1, elsewhere in float32, every operation rounded on
 *                 its own, k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f: ss = 0.5f; for the rows y + 1, y, y - 1 in this order:
 *                 ss += (in[x-1] * ka + in[x] * kb) + in[x+1] * kc, the centre tap k5 and every other k1; smooth = ss <= 0 ? 0 : ss >= 255 ?
 *                 255 : trunc(ss).  (Pillow's ImageFilter.SMOOTH.)
 *   blend(d, i, f)  float32, unfused: t = (float)d + f * (float)(i - d), the difference taken in int.  0 <= f <= 1: trunc(t); otherwise
 *                 t <= 0 ? 0 : t >= 255 ? 255 : trunc(t).
 *   AFFINE        float64, unfused.  For output pixel (x, y): xin = m0 (x + 0.5) + m1 (y + 0.5) + m2, yin = m3 (x + 0.5) + m4 (y + 0.5) + m5.
 *                 Unless 0 <= xin < S and 0 <= yin < S (a NaN fails this) the pixel is `fill`.  Otherwise xin -= 0.5, yin -= 0.5,
 *                 X = floor(xin), Y = floor(yin), dx = xin - X, dy = yin - Y; columns are clamped to [0, S - 1].
 *     bilinear      v1 = a + (b - a) dx on columns X, X + 1 of row clamp(Y); v2 the same on row Y + 1 if 0 <= Y + 1 < S, else v1;
 *                   out = trunc(v1 + (v2 - v1) dy)
 *     bicubic       cub(v1, v2, v3, v4, d) = v2 + d ((-v1 + v3) + d ((2 (v1 - v2) + v3 - v4) + d (-v1 + v2 - v3 + v4))); the first row value
 *                   is cub over columns X - 1 .. X + 2 of row clamp(Y - 1); rows Y, Y + 1, Y + 2 give theirs the same way if inside the
 *                   image, otherwise the value of the row before; v = cub of the four row values with dy;
 *                   out = v <= 0 ? 0 : v >= 255 ? 255 : trunc(v)
 *                 (Image.transform(size, AFFINE, m, resample, fillcolor=fill), which also serves Image.rotate.)
 * records_host (nullable): a host copy of the records; when given, an op code outside AP_RA_* or an affine record whose filter is not 1 or
 * 2 is refused (AP_ERR_SHAPE).  The kernel treats an unknown op code as AP_RA_NONE and any other filter code as AP_RESAMPLE_BILINEAR and
 * clamps every source index, so a record it was not shown on the host cannot make it read or write out of bounds.
 * AP_ERR_NULL: args, u8, out or records NULL, scratch NULL with n_layers > 1.  AP_ERR_SHAPE: B < 0 or > 65 535, S < 1 or > 16 384, a bad
 * layout, n_layers outside 1 .. AP_RANDAUG_MAX_LAYERS, aliased buffers, a bad host record.  B == 0 succeeds without a launch.  Every
 * check comes before the first launch. */
enum { AP_RA_NONE = 0, AP_RA_AUTOCONTRAST = 1, AP_RA_EQUALIZE = 2, AP_RA_INVERT = 3, AP_RA_SOLARIZE = 4, AP_RA_SOLARIZE_ADD = 5,
       AP_RA_POSTERIZE = 6, AP_RA_BRIGHTNESS = 7, AP_RA_CONTRAST = 8, AP_RA_COLOR = 9, AP_RA_SHARPNESS = 10, AP_RA_AFFINE = 11 };
enum { AP_RANDAUG_RECORD_WORDS = 16, AP_RANDAUG_MAX_LAYERS = 8 };
typedef struct ap_randaug_args {
    const unsigned char* u8; int layout; int B, S;
    unsigned char* out;
    unsigned char* scratch;          /* nullable when n_layers == 1 */
    const int* records;              /* DEVICE [B][n_layers][16] */
    const int* records_host;         /* nullable host copy, validated */
    int n_layers;
    unsigned char fill[3];
} ap_randaug_args;
int ap_randaug_u8(const ap_randaug_args* args, ap_stream_t stream);

/* ---- token labels from stored top-k label maps, ROI-aligned to each image's crop box and flipped with it, in one launch (additive in ABI
 * version 7; csrc/labelmap.hip).  The reference's published recipe (`train_autoprog.sh --token-label --token-label-data ...`) trains on
 * stored NFNet-F6 label maps, a top-5 (score, class) map per image, which its loader cuts to the image's random crop box with
 * roi_align(aligned=False, sampling_ratio=-1) on the densified maps and flips with the image before tlt's create_token_label_target
 * (main_prog.py:994-1004).  tlt and torchvision are not at hand: the rule below is this library's restatement of that forward, from
 * knowledge of those packages, not byte-checked against them; tests/_labelmap_ref.py pins it in fp64.
 * scores (DEVICE): [B][Kin][Hm][Wm], fp16 (AP_LM_F16) or fp32 (AP_LM_F32) by score_dtype, image b at element b * score_stride; scores are
 * non-negative.  classes (DEVICE): the same shape at its own class_stride, in the scores' float dtype (AP_LM_CLASS_FLOAT, converted by
 * truncation) or int32 (AP_LM_CLASS_I32); a class outside [0, C) contributes nothing.  tlt's stored half tensor [B, 2, Kin, Hm, Wm] passes
 * as two views of one buffer.  labels (DEVICE): int64 [B].  boxes (DEVICE): B records of 8 fp32 words: x1, y1, x2, y2 in map pixel
 * units, the flip as 0.0 or 1.0, then three zero words.  idx (int32) and val (fp32): [B, 2 + P P, K], contiguous -- the arrays of a
 * SparseTokenLabelTarget at the token grid P.  dropped (nullable): fp32 [B, 1 + P P].
 * An output bin of image b is the class slot (the single bin of a 1 x 1 pooling of the box, Pw = Ph = 1) or one of the P x P token bins
 * (Pw = Ph = P).  In fp64, for the x axis and the same in y:
 *     roi_w = max(x2 - x1, 1);  bin_w = roi_w / Pw;  gw = ceil(roi_w / Pw)
 *     sample ix of bin pw:  x = x1 + pw * bin_w + (ix + 0.5) * bin_w / gw
 *     a sample with x < -1 or x > Wm (or the same in y) counts but adds nothing;  x = max(x, 0);  xl = (int)x;
 *     if xl >= Wm - 1: xl = xh = Wm - 1, x = xl  else xh = xl + 1;  lx = x - xl, hx = 1 - lx
 *     dense[c] = (1 / (gh gw)) * sum over the samples, over the 4 corners (weights hy hx, hy lx, ly hx, ly lx), over k < Kin with
 *                classes[b, k, corner] == c, of weight * scores[b, k, corner]
 * Slot 0 is (labels[b], 1.0), then fillers (-1, 0.0).  Slot 1 (the class slot) and slots 2.. (the token bins) hold the K classes with
 * the largest dense[c] > 0, by descending score and equal scores by ascending class (the tie rule of ap_softmax_topk_rows), completed
 * with fillers.  With flip 1, token slot 2 + ph P + pw holds bin (ph, P - 1 - pw); rows never flip and the class slot is unaffected.
 * dropped[b][slot - 1]: the sum of dense[c] over the classes that were not kept -- keeping the top K where a bin can see more classes is a
 * stated deviation from the reference, and this makes it visible.  Raw scores are written: label smoothing is applied where the loss
 * reads the pairs.  Corners that carry the same class merge into one pair.
 * The kernel forms the sample positions and a pixel's separable weight wy[y] wx[x] / (gh gw) in fp64, products and sums in fp32, every
 * bin's sums in a fixed order and without atomics: the output is bit-reproducible.  One launch for all B (1 + P P) bins; the launch
 * geometry depends on B and P alone, never on the records.  boxes_host (nullable): a host copy of the records, validated before the
 * launch.  The kernel clamps what it indexes (a bin's pixels into the map, the samples of a pixel's weight to the 16 nearest), so a record
 * it was not shown on the host cannot make it read or write out of bounds.
 * AP_ERR_NULL: args or a required pointer NULL.  AP_ERR_SHAPE: K or Kin outside 1..8, P < 1 (or P P beyond 2^30), Hm or Wm < 1, C outside
 * 1..65536, B < 0, a bad dtype flag, a host record with x2 < x1 or y2 < y1, a non-finite word or a flip other than 0 or 1.
 * AP_ERR_UNSUPPORTED: Hm Wm Kin > 4096 (the candidates of the class slot's bin, which a workgroup keeps in LDS).  B == 0 succeeds
 * without a launch.  Every check comes before the launch. */
enum { AP_LM_F16 = 0, AP_LM_F32 = 1 };                   /* score_dtype */
enum { AP_LM_CLASS_FLOAT = 0, AP_LM_CLASS_I32 = 1 };     /* class_dtype */
typedef struct ap_label_map_crop_args {
    const void* scores; int score_dtype; int64_t score_stride;
    const void* classes; int class_dtype; int64_t class_stride;
    const int64_t* labels;           /* DEVICE [B] */
    const float* boxes;              /* DEVICE [B][8] */
    const float* boxes_host;         /* nullable host copy, validated */
    int* idx; float* val;            /* [B][2 + P P][K] */
    float* dropped;                  /* nullable, [B][1 + P P] */
    int B, Kin, Hm, Wm, P, K, C;
} ap_label_map_crop_args;
int ap_label_map_crop(const ap_label_map_crop_args* args, ap_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* AUTOPROG_HIP_H */
