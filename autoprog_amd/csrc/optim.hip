// Fused multi-tensor AdamW + up to 4 EMA updates over ONE flat fp32 parameter slab (SURVEY.md row N4;
// reference: timm create_optimizer -> torch.optim.AdamW at main_prog.py:484, ModelEmaV2.update x4 at
// main_prog.py:1030-1033 with decays 0.998 0.9986 0.999 0.9996, scripts/train_autoprog.sh:5).
// One pass: reads p,g,m,v,ema_0..3 and a 1-byte weight-decay mask, writes p,m,v,ema_0..3 (60 B per
// parameter instead of ~100 B and ~70 launches for foreach AdamW + 4 foreach lerps).  HBM-bound.
#include "common.h"
#include "slab_math.h"

// The arguments of all eight instantiations of k_adamw_ema<GUARD, E16, GROUPED>; an instantiation reads the fields of its flags and
// compiles to the code it would have without the others (`if constexpr` around every use).  The order of the fields is part of the
// code: hipcc's register allocation follows it (profiles/optim_core_refactor.txt).
//   GUARD (ap_adamw_ema_step_guarded): the bias corrections and the skip decision come from the ap_guard_state that ap_grad_health
//     committed for this step.  A skipped step (a non-finite gradient element) reads neither g, m nor v and writes neither p, m, v nor
//     p16; the EMA copies still take their lerp towards the unchanged parameters (the reference updates its ModelEma list whether or not
//     apex skipped the step, main_prog.py:1030-1033).
//   E16 (ap_adamw_ema_step_ema16): one bf16 slab per EMA copy (nullptr: that copy is not emitted).  An emitted copy is the rounding of
//     the fp32 lerp that is stored beside it (pack_bf2, as p16), from the registers that hold it: 2 bytes per parameter and copy more, no
//     second pass.  A skipped guarded step moves the EMA copies and so writes their bf16 copies as well.
//   GROUPED (ap_adamw_ema_step_groups): a device table of {lr, weight_decay} per parameter group.  The byte slab the kernel reads per
//     element (`wd_mask` otherwise) then holds the element's GROUP; lr and wd are not read.  Every workgroup forms the two numbers a
//     group contributes -- the decay factor 1 - lr*wd and the step size lr / bc1 -- once, in LDS, and the inner loop looks both up per
//     element (a float4 may straddle groups: tensors of odd length sit back to back in the slab).
struct AdamGroupEntry { float lr, wd; };
struct AdamArgs {
    float lr, beta1, beta2, eps, wd, bc1, bc2_sqrt;   // bc1 = 1-beta1^t, bc2_sqrt = sqrt(1-beta2^t)
    float gscale;                                      // gradient pre-scale (1/world_size: the data-parallel mean)
    const float* gnorm_sq;                             // device scalar: sum of squares of the UNSCALED slab (ap_sumsq_f32), or nullptr
    float max_norm;                                    // clip_grad_norm_ bound on the scaled gradient (with gnorm_sq)
    float clip_value;                                  // clip_grad_value_ bound on the scaled gradient elements (> 0), else 0
    const float* step_dev;                             // device [lr, 1 - beta1^t, sqrt(1 - beta2^t)] (graph replay), or nullptr: the host values above
    int n_ema;
    float decay[4];
    float* ema[4];
    const ap_guard_state* guard;                       // GUARD
    const AdamGroupEntry* group_tab;                   // GROUPED
    int n_groups;
    bf16_t* ema16[4];                                  // E16
};
constexpr int ADAM_MAX_GROUPS = 256;                   // one byte per element

template <bool GUARD, bool E16, bool GROUPED>
__global__ void __launch_bounds__(256)
k_adamw_ema(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
            const unsigned char* __restrict__ wd_mask, int64_t n, AdamArgs a, bf16_t* __restrict__ p16) {
    const int64_t nv = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if constexpr (GROUPED) { if (a.step_dev) { a.bc1 = a.step_dev[1]; a.bc2_sqrt = a.step_dev[2]; } }      // (the rates come from the table)
    else if (a.step_dev) { a.lr = a.step_dev[0]; a.bc1 = a.step_dev[1]; a.bc2_sqrt = a.step_dev[2]; }
    bool skip = false;
    if constexpr (GUARD) { skip = a.guard->nonfinite != 0; a.bc1 = a.guard->bc1; a.bc2_sqrt = a.guard->bc2_sqrt; }
    const float step_size = a.lr / a.bc1;
    const float2* tab = nullptr;                       // per group {1 - lr*wd, lr / bc1}
    if constexpr (GROUPED) {
        __shared__ float2 s_tab[ADAM_MAX_GROUPS];
        // the ungrouped kernel's two numbers in the forms its instructions have: the factor is ONE fma (its 1.0f - a.lr * a.wd is
        // contracted), the step size an IEEE division.  Written out, so that no choice of the compiler's separates the two kernels.
        for (int gi = threadIdx.x; gi < a.n_groups; gi += blockDim.x) {
            const AdamGroupEntry t = a.group_tab[gi];
            s_tab[gi] = make_float2(__builtin_fmaf(-t.lr, t.wd, 1.0f), t.lr / a.bc1);
        }
        __syncthreads();
        tab = s_tab;
    }
    // gradient clipping folded into the update (prog/scaler.py:60-68 -> timm dispatch_clip_grad, main_prog.py:1019-1027):
    // mode 'norm' = torch.nn.utils.clip_grad_norm_: coef = min(1, max_norm / (||g|| + 1e-6)) with ||g|| the norm of the MEAN gradient
    // (gscale * the norm of the slab, which holds the all-reduced SUM under a deferred mean); mode 'value': clamp every element
    const float gs = clip_gscale(a.gscale, a.gnorm_sq, a.max_norm);
    const float cv = a.clip_value;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
        float4 pp = reinterpret_cast<float4*>(p)[i];
        if (!skip) {
            float4 gg = reinterpret_cast<const float4*>(g)[i];
            gg.x *= gs; gg.y *= gs; gg.z *= gs; gg.w *= gs;
            if (cv > 0.f) { gg.x = fminf(fmaxf(gg.x, -cv), cv); gg.y = fminf(fmaxf(gg.y, -cv), cv); gg.z = fminf(fmaxf(gg.z, -cv), cv); gg.w = fminf(fmaxf(gg.w, -cv), cv); }
            float4 mm = reinterpret_cast<float4*>(m)[i];
            float4 vv = reinterpret_cast<float4*>(v)[i];
            const uchar4 wm = reinterpret_cast<const uchar4*>(wd_mask)[i];
            float* P = &pp.x; const float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
            const unsigned char W[4] = {wm.x, wm.y, wm.z, wm.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float x = P[k];
                if constexpr (!GROUPED) { if (W[k]) x *= (1.0f - a.lr * a.wd); }    // decoupled weight decay (torch AdamW order)
                M[k] = a.beta1 * M[k] + (1.0f - a.beta1) * G[k];
                V[k] = a.beta2 * V[k] + (1.0f - a.beta2) * G[k] * G[k];
                const float denom = sqrtf(V[k]) / a.bc2_sqrt + a.eps;
                if constexpr (GROUPED) {
                    // the ungrouped update rounds the decayed weight on its own (a select stands between its product and the
                    // subtraction) and then takes ONE fma; times 1.0f for an un-decayed group is exact.  The fma is spelled out: left to
                    // contraction, x * f - s * q could fuse the other product.
                    const float2 t = tab[W[k]];
                    x *= t.x;
                    P[k] = __builtin_fmaf(-t.y, M[k] / denom, x);
                } else {
                    P[k] = x - step_size * (M[k] / denom);
                }
            }
            reinterpret_cast<float4*>(p)[i] = pp;
            if (p16) { u32x2 o; o[0] = pack_bf2(pp.x, pp.y); o[1] = pack_bf2(pp.z, pp.w); reinterpret_cast<u32x2*>(p16)[i] = o; }
            reinterpret_cast<float4*>(m)[i] = mm;
            reinterpret_cast<float4*>(v)[i] = vv;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e < a.n_ema) {
                float4 ee = reinterpret_cast<float4*>(a.ema[e])[i];
                const float d = a.decay[e];
                ee.x = d * ee.x + (1.0f - d) * pp.x; ee.y = d * ee.y + (1.0f - d) * pp.y;
                ee.z = d * ee.z + (1.0f - d) * pp.z; ee.w = d * ee.w + (1.0f - d) * pp.w;
                reinterpret_cast<float4*>(a.ema[e])[i] = ee;
                if constexpr (E16) {
                    if (a.ema16[e]) { u32x2 o; o[0] = pack_bf2(ee.x, ee.y); o[1] = pack_bf2(ee.z, ee.w); reinterpret_cast<u32x2*>(a.ema16[e])[i] = o; }
                }
            }
        }
    }
}

// sum of squares of a flat fp32 slab in two deterministic passes: 1024 per-workgroup partials (fp64 inside a workgroup's tree),
// then one workgroup adds them in order.  16 bytes per lane, every load of a thread's sweep independent.
__global__ void __launch_bounds__(256)
k_sumsq_partial(const float* __restrict__ x, int64_t n, double* __restrict__ partial) {
    __shared__ double red[4];
    const int64_t nv = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        s0 = fmaf(v.x, v.x, s0); s1 = fmaf(v.y, v.y, s1); s2 = fmaf(v.z, v.z, s2); s3 = fmaf(v.w, v.w, s3);
    }
    double s = (double)s0 + (double)s1 + (double)s2 + (double)s3;
    if (blockIdx.x == 0 && threadIdx.x == 0) for (int64_t i = nv << 2; i < n; ++i) s += (double)x[i] * (double)x[i];     // (n % 4 tail)
    wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ void __launch_bounds__(256)
k_sumsq_final(const double* __restrict__ partial, int count, float* __restrict__ out) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < count; i += 256) s += partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) out[0] = (float)red[0];
}

extern "C" size_t ap_sumsq_workspace(void) { return (size_t)1024 * sizeof(double); }

extern "C" int ap_sumsq_f32(const float* x, int64_t n, float* out, void* workspace, size_t ws_bytes, ap_stream_t stream) {
    if (!x || !out || !workspace) return AP_ERR_NULL;
    if (n <= 0 || ws_bytes < ap_sumsq_workspace() || ((uintptr_t)x & 15)) return AP_ERR_SHAPE;
    int64_t grid = (n / 4 + 255) / 256;
    if (grid > 1024) grid = 1024;
    if (grid < 1) grid = 1;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_sumsq_partial, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, n, static_cast<double*>(workspace));
    hipLaunchKernelGGL(k_sumsq_final, dim3(1), dim3(256), 0, (hipStream_t)stream, static_cast<const double*>(workspace), (int)grid, out);
    return ap_check_launch();
}

// the argument checks and the launch all entry points share.  `guard` selects the guarded instantiations, `ema16` (an array of 4) the ones
// that emit bf16 copies of EMA slabs, `group_tab` (n_groups already checked) the ones that read wd_mask as group numbers
static int adamw_ema_launch(float* p, const float* g, float* m, float* v, const unsigned char* wd_mask, int64_t n,
                            float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                            const float* gnorm_sq, float max_norm, float clip_value, const float* step_scalars_dev,
                            float* const* ema, const float* ema_decay, int n_ema, ap_bf16* p_bf16, const ap_guard_state* guard, ap_stream_t stream,
                            ap_bf16* const* ema16 = nullptr, const float* group_tab = nullptr, int n_groups = 0) {
    using Kernel = void (*)(float*, const float*, float*, float*, const unsigned char*, int64_t, AdamArgs, bf16_t*);
    static const Kernel kernels[8] = {                  // [guard | e16 << 1 | grouped << 2]
        k_adamw_ema<false, false, false>, k_adamw_ema<true, false, false>, k_adamw_ema<false, true, false>, k_adamw_ema<true, true, false>,
        k_adamw_ema<false, false, true>,  k_adamw_ema<true, false, true>,  k_adamw_ema<false, true, true>,  k_adamw_ema<true, true, true>};
    // a refused bf16 copy comes before a null slab, the entry points' order of checks; slab_ema_args below makes the same check again per
    // copy (it is ap_lamb_ema_step's one) and can no longer fail on it here
    for (int e = 0; ema16 && e < 4; ++e) if (ema16_refused(ema16[e], e, n_ema)) return AP_ERR_SHAPE;
    if (!p || !g || !m || !v || !wd_mask) return AP_ERR_NULL;
    if (n <= 0 || (n & 3) || n_ema < 0 || n_ema > 4 || step < 1) return AP_ERR_SHAPE;
    if (gnorm_sq && !(max_norm > 0.f)) return AP_ERR_SHAPE;
    AdamArgs a;
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.wd = weight_decay; a.gscale = grad_scale;
    a.gnorm_sq = gnorm_sq; a.max_norm = max_norm; a.clip_value = clip_value > 0.f ? clip_value : 0.f; a.step_dev = step_scalars_dev;
    adam_bias_corrections(beta1, beta2, step, a.bc1, a.bc2_sqrt);
    a.n_ema = n_ema;
    if (const int rc = slab_ema_args(ema, ema_decay, n_ema, ema16, 0, a.ema, a.decay, a.ema16)) return rc;
    a.guard = guard;
    a.group_tab = reinterpret_cast<const AdamGroupEntry*>(group_tab);
    a.n_groups = n_groups;
    // (four null entries: nothing to emit, the launch is the one without the pointers)
    const bool e16 = a.ema16[0] || a.ema16[1] || a.ema16[2] || a.ema16[3];
    int64_t grid = (n / 4 + 255) / 256;
    if (grid > 256 * 16) grid = 256 * 16;
    (void)hipGetLastError();
    hipLaunchKernelGGL(kernels[(guard ? 1 : 0) | (e16 ? 2 : 0) | (group_tab ? 4 : 0)], dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream,
                       p, g, m, v, wd_mask, n, a, reinterpret_cast<bf16_t*>(p_bf16));
    return ap_check_launch();
}

extern "C" int ap_adamw_ema_step(float* p, const float* g, float* m, float* v, const unsigned char* wd_mask, int64_t n,
                                 float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                                 const float* gnorm_sq, float max_norm, float clip_value, const float* step_scalars_dev,
                                 float* const* ema, const float* ema_decay, int n_ema, ap_bf16* p_bf16, ap_stream_t stream) {
    return adamw_ema_launch(p, g, m, v, wd_mask, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, gnorm_sq, max_norm, clip_value,
                            step_scalars_dev, ema, ema_decay, n_ema, p_bf16, nullptr, stream);
}

// the bias corrections of the guarded step are the ones ap_grad_health wrote for t = applied: `step` is only checked (>= 1), and of
// step_scalars_dev only the learning rate is used
extern "C" int ap_adamw_ema_step_guarded(float* p, const float* g, float* m, float* v, const unsigned char* wd_mask, int64_t n,
                                         float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                                         const float* gnorm_sq, float max_norm, float clip_value, const float* step_scalars_dev,
                                         float* const* ema, const float* ema_decay, int n_ema, ap_bf16* p_bf16, const ap_guard_state* guard,
                                         ap_stream_t stream) {
    if (!guard) return AP_ERR_NULL;
    return adamw_ema_launch(p, g, m, v, wd_mask, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, gnorm_sq, max_norm, clip_value,
                            step_scalars_dev, ema, ema_decay, n_ema, p_bf16, guard, stream);
}

// the step that also emits bf16 copies of EMA slabs (a forward pass reads bf16 weights: an EMA copy becomes a network to compute with,
// the reference's ModelEmaV2 modules of main_prog.py:1030-1033, without a cast pass).  ema_bf16: HOST array of 4 device pointers, entry e
// the bf16 slab of EMA copy e (same offsets, 8-byte aligned) or null for "not this copy"; entries at e >= n_ema must be null.
// guard_or_null selects the guarded step.  Everything is checked before anything is launched.
extern "C" int ap_adamw_ema_step_ema16(float* p, const float* g, float* m, float* v, const unsigned char* wd_mask, int64_t n,
                                       float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                                       const float* gnorm_sq, float max_norm, float clip_value, const float* step_scalars_dev,
                                       float* const* ema, const float* ema_decay, int n_ema, ap_bf16* p_bf16, ap_bf16* const* ema_bf16,
                                       const ap_guard_state* guard_or_null, ap_stream_t stream) {
    if (!ema_bf16) return AP_ERR_NULL;
    if (n_ema < 0 || n_ema > 4) return AP_ERR_SHAPE;
    return adamw_ema_launch(p, g, m, v, wd_mask, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, gnorm_sq, max_norm, clip_value,
                            step_scalars_dev, ema, ema_decay, n_ema, p_bf16, guard_or_null, stream, ema_bf16);
}

// the step with one learning rate and one weight decay per parameter group (include/autoprog_hip.h): group_id[n] in the place of wd_mask,
// group_tab_dev[n_groups] of {lr, weight_decay}.  ema_bf16 is nullable here; the checks of ap_adamw_ema_step_ema16 apply to a given one.
// A byte >= n_groups is the caller's error (the kernel reads its own 256-entry LDS table, nothing outside it).  Everything is checked
// before anything is launched.
extern "C" int ap_adamw_ema_step_groups(float* p, const float* g, float* m, float* v, const unsigned char* group_id, int64_t n,
                                        float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                                        const float* gnorm_sq, float max_norm, float clip_value, const float* step_scalars_dev,
                                        float* const* ema, const float* ema_decay, int n_ema, ap_bf16* p_bf16, ap_bf16* const* ema_bf16,
                                        const ap_guard_state* guard_or_null, const float* group_tab_dev, int n_groups, ap_stream_t stream) {
    if (!group_id || !group_tab_dev) return AP_ERR_NULL;
    if (n_groups < 1 || n_groups > ADAM_MAX_GROUPS || ((uintptr_t)group_tab_dev & 7)) return AP_ERR_SHAPE;
    if (n_ema < 0 || n_ema > 4) return AP_ERR_SHAPE;
    return adamw_ema_launch(p, g, m, v, group_id, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, gnorm_sq, max_norm, clip_value,
                            step_scalars_dev, ema, ema_decay, n_ema, p_bf16, guard_or_null, stream, ema_bf16, group_tab_dev, n_groups);
}

// ---- gradient health (ap_grad_health): per parameter tensor the sum of squares of the finite elements (fp64) and the number of
// non-finite ones, in one pass over the gradient slab, and the skip decision of the guarded step.  The slab is cut into chunks of
// GH_CHUNK elements; a workgroup owns a contiguous run of them (all runs equally long), finds the segment its first chunk starts in by
// one binary search and from there only steps forward.  A chunk that lies inside one segment -- nearly all of them -- is 8 independent
// 16-byte loads per lane and one workgroup reduction.  A chunk that meets segment bounds hands its segments to its four waves in turn,
// each a strided sweep and a wave reduction.  The partial of (chunk c, segment s) goes to slot c + s of the workspace: c and s both
// only grow along the slab, so the slot is unique, and n_chunks + n_seg slots hold every pair.  k_grad_health_final adds a segment's
// slots in chunk order (one wave per segment, fixed tree): no floating-point atomics, the same bits every run.  x * x is exact in fp64,
// so only the order of the additions separates the result from a serial fp64 loop.  The step's total is an INTEGER: the workgroups of
// the second kernel add theirs with integer atomics and the one that draws the last ticket commits the step.
constexpr int GH_CHUNK = 8192;          // 256 lanes x 8 float4
constexpr int GH_MAX_GRID = 2048;       // 8 workgroups on each of 256 CUs

__global__ void __launch_bounds__(256)
k_grad_health(const float* __restrict__ g, int64_t n, const int64_t* __restrict__ seg_off, int n_seg, int64_t n_chunks, int per_wg,
              double* __restrict__ part_s, int* __restrict__ part_c, int* __restrict__ ticket) {
    __shared__ double red_s[4];
    __shared__ int red_c[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) { ticket[0] = 0; ticket[1] = 0; }  // (the second kernel's total and ticket counter)
    const int64_t first = (int64_t)blockIdx.x * per_wg;
    const int64_t last = (first + per_wg < n_chunks) ? first + per_wg : n_chunks;
    int lo = 0, hi = n_seg - 1;                                                  // the last segment that starts at or before the run
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (seg_off[mid] <= first * GH_CHUNK) lo = mid; else hi = mid - 1; }
    int s0 = lo;
    for (int64_t c = first; c < last; ++c) {
        const int64_t c0 = c * GH_CHUNK;
        const int64_t c1 = (c0 + GH_CHUNK < n) ? c0 + GH_CHUNK : n;
        while (s0 + 1 < n_seg && seg_off[s0 + 1] <= c0) ++s0;                    // ... at or before this chunk
        if (seg_off[s0 + 1] >= c1) {                                             // the whole chunk lies in segment s0
            const int len = (int)(c1 - c0), nv = len >> 2;                       // (c0 is a multiple of 4, the slab 16-byte aligned)
            const float4* gv = reinterpret_cast<const float4*>(g + c0);
            float4 x[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { const int i = threadIdx.x + 256 * k; x[k] = (i < nv) ? gv[i] : make_float4(0.f, 0.f, 0.f, 0.f); }
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            int cnt = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) { sq_add_finite(x[k].x, a0, cnt); sq_add_finite(x[k].y, a1, cnt); sq_add_finite(x[k].z, a2, cnt); sq_add_finite(x[k].w, a3, cnt); }
            double s = (a0 + a1) + (a2 + a3);
            if ((int)threadIdx.x < (len & 3)) sq_add_finite(g[c0 + (nv << 2) + threadIdx.x], s, cnt);      // (the slab's n % 4 tail)
            wave_sum(s, cnt);
            if (lane == 0) { red_s[wave] = s; red_c[wave] = cnt; }
            __syncthreads();
            if (threadIdx.x == 0) {
                part_s[c + s0] = ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
                part_c[c + s0] = red_c[0] + red_c[1] + red_c[2] + red_c[3];
            }
            __syncthreads();
        } else {
            for (int s = s0 + wave; s < n_seg; s += 4) {
                const int64_t b = seg_off[s];
                if (b >= c1) break;
                const int64_t e = seg_off[s + 1];
                const int64_t from = b > c0 ? b : c0, to = e < c1 ? e : c1;      // (clamped to the chunk: a malformed table reads nothing outside the slab)
                if (to <= from) continue;
                double acc = 0.0;
                int cnt = 0;
#pragma unroll 4
                for (int64_t i = from + lane; i < to; i += 64) sq_add_finite(g[i], acc, cnt);
                wave_sum(acc, cnt);
                if (lane == 0) { part_s[c + s] = acc; part_c[c + s] = cnt; }
            }
        }
    }
}

// wave w of the grid adds the slots of segment w in chunk order; a workgroup then adds its count to the step's total and draws a ticket,
// and the workgroup with the last ticket -- every other one's total is in by then -- commits the step
__global__ void __launch_bounds__(256)
k_grad_health_final(const double* __restrict__ part_s, const int* __restrict__ part_c, const int64_t* __restrict__ seg_off, int n_seg,
                    int64_t n_chunks, double* __restrict__ seg_sumsq, int* __restrict__ seg_nonfinite, ap_guard_state* __restrict__ st,
                    float beta1, float beta2, int* __restrict__ ticket) {
    __shared__ int tot[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.x * 4 + wave;
    int cnt = 0;
    if (s < n_seg) {
        const int64_t b = seg_off[s], e = seg_off[s + 1];
        double acc = 0.0;
        if (e > b) {
            int64_t cl = b / GH_CHUNK, ch = (e - 1) / GH_CHUNK;
            if (cl < 0) cl = 0;
            if (ch > n_chunks - 1) ch = n_chunks - 1;
            for (int64_t c = cl + lane; c <= ch; c += 64) { acc += part_s[c + s]; cnt += part_c[c + s]; }
        }
        wave_sum(acc, cnt);
        if (lane == 0) { seg_sumsq[s] = acc; seg_nonfinite[s] = cnt; }
    }
    if (lane == 0) tot[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&ticket[0], tot[0] + tot[1] + tot[2] + tot[3]);
        __threadfence();
        if (atomicAdd(&ticket[1], 1) == (int)gridDim.x - 1) {
            __threadfence();
            const int total = atomicAdd(&ticket[0], 0);
            int applied = st->applied;
            if (total == 0) { applied += 1; st->applied = applied; st->consecutive = 0; }
            else { st->skipped += 1; st->consecutive += 1; }
            st->nonfinite = total;
            // the expressions of ap_adamw_ema_step for t = applied (a skipped step's values are not used; t >= 1 keeps them finite)
            const double t = (double)(applied > 0 ? applied : 1);
            st->bc1 = (float)(1.0 - pow((double)beta1, t));
            st->bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, t));
        }
    }
}

static int64_t gh_chunks(int64_t n) { return (n + GH_CHUNK - 1) / GH_CHUNK; }

// workspace: n_chunks + n_seg fp64 slots, as many int32 slots, two int32 counters
extern "C" size_t ap_grad_health_workspace(int64_t n, int n_seg) {
    if (n <= 0 || n_seg <= 0) return 0;
    const size_t slots = (size_t)gh_chunks(n) + (size_t)n_seg;
    return (slots * (sizeof(double) + sizeof(int)) + 2 * sizeof(int) + 15) & ~(size_t)15;
}

extern "C" int ap_grad_health(const float* g, int64_t n, const int64_t* seg_off, int n_seg, double* seg_sumsq, int* seg_nonfinite,
                              ap_guard_state* state, float beta1, float beta2, void* workspace, size_t ws_bytes, ap_stream_t stream) {
    if (!g || !seg_off || !seg_sumsq || !seg_nonfinite || !state || !workspace) return AP_ERR_NULL;
    if (n <= 0 || n_seg <= 0 || ws_bytes < ap_grad_health_workspace(n, n_seg) || ((uintptr_t)g & 15) || ((uintptr_t)workspace & 7)) return AP_ERR_SHAPE;
    const int64_t chunks = gh_chunks(n);
    if (chunks > (int64_t)GH_MAX_GRID * 0x7fffffff / 2) return AP_ERR_SHAPE;
    const size_t slots = (size_t)chunks + (size_t)n_seg;
    double* part_s = static_cast<double*>(workspace);
    int* part_c = reinterpret_cast<int*>(part_s + slots);
    int* ticket = part_c + slots;
    const int per_wg = (int)((chunks + GH_MAX_GRID - 1) / GH_MAX_GRID);         // equally long runs: no workgroup does one chunk more than the rest
    const int64_t grid = (chunks + per_wg - 1) / per_wg;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_grad_health, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, g, n, seg_off, n_seg, chunks, per_wg, part_s, part_c, ticket);
    hipLaunchKernelGGL(k_grad_health_final, dim3((unsigned)((n_seg + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const double*)part_s, (const int*)part_c,
                       seg_off, n_seg, chunks, seg_sumsq, seg_nonfinite, state, beta1, beta2, ticket);
    return ap_check_launch();
}

// ---- batched transpose of many bf16 matrices living in one slab (the [K, ld(N)] weight copies used by
// the input-gradient GEMMs): one launch instead of one per Linear.  desc[i] = {src_off, dst_off, rows, cols,
// ld_dst, first_tile}; tiles are 32x32, a workgroup finds its matrix by binary search over first_tile.
struct TrDesc { long long src_off, dst_off; int rows, cols, ld_dst, first_tile; };

__global__ void __launch_bounds__(256)
k_batched_transpose(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, const TrDesc* __restrict__ desc, int count) {
    __shared__ bf16_t tile[32][34];
    int lo = 0, hi = count - 1;
    const int t = blockIdx.x;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (desc[mid].first_tile <= t) lo = mid; else hi = mid - 1; }
    const TrDesc d = desc[lo];
    const int tiles_c = (d.cols + 31) / 32;
    const int lt = t - d.first_tile;
    const int r0 = (lt / tiles_c) * 32, c0 = (lt % tiles_c) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    bf16_t v[4];                                  // all four loads of the thread before the first LDS store
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int r = r0 + ty + 8 * u, c = c0 + tx;
        v[u] = (r < d.rows && c < d.cols) ? src[d.src_off + (long long)r * d.cols + c] : (bf16_t)0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) tile[ty + 8 * u][tx] = v[u];
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, r = r0 + tx;
        if (c < d.cols && r < d.ld_dst) dst[d.dst_off + (long long)c * d.ld_dst + r] = tile[tx][i];
    }
}

extern "C" int ap_batched_transpose_bf16(const ap_bf16* src, ap_bf16* dst, const void* desc_dev, int count, int total_tiles, ap_stream_t stream) {
    if (!src || !dst || !desc_dev) return AP_ERR_NULL;
    if (count <= 0 || total_tiles <= 0) return AP_ERR_SHAPE;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_batched_transpose, dim3(total_tiles), dim3(256), 0, (hipStream_t)stream, src, dst, (const TrDesc*)desc_dev, count);
    return ap_check_launch();
}
