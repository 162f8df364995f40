// Fused LAMB + up to 4 EMA updates over the flat fp32 slabs of FlatAdamWEma, with one trust ratio per parameter tensor: ap_lamb_ema_step
// (the rule and its stated deviations: include/autoprog_hip.h; tests/_lamb_ref.py pins it in fp64).
//
// Layout: a READ-ONLY first pass and an applying pass that recomputes.  With four EMA copies and the bf16 weight slab, per parameter:
//   pass 1  k_lamb_norms   reads p, g, m, v (16 B) and the group byte (1 B)                                     17 B
//   pass 2  k_lamb_trust   reads two fp64 partials per chunk, writes three fp32 per tensor                       ~0 B
//   pass 3  k_lamb_apply   reads p, g, m, v, the group byte, 4 EMA (33 B); writes p, m, v, p16, 4 EMA (30 B)     63 B
// 80 B in all against the 63 B of the grouped AdamW launch on the same slabs; every emitted ema16 copy adds 2 B to both.  The ratio 1.27
// is a count of bytes, not a time.  Measured on VOLO-D1's slab (profiles/lamb.txt): the call takes 1.42 times the AdamW launch -- pass 1
// runs at the copy's rate (88 us for its 17 B), pass 3 takes 367 us where the AdamW launch moves the same 63 B in 336 us.  What separates
// the two has not been found: pass 3 holds 122 registers (4 waves per SIMD) and every chunk starts with a dependent load of its record.
// Storing m' and v' in pass 1 would save nothing (8 B written there, 0 B fewer read in pass 3) and would break the guard's and the
// reader's view that pass 1 changes no state.  g is read-only in every pass.
//
// Work division.  The host cuts every tensor into chunks of at most LAMB_CH consecutive elements (ap_lamb_chunk(), a multiple of 4) and
// hands over the table {start, length, tensor} once.  A workgroup takes chunks blockIdx.x, blockIdx.x + gridDim.x, ...; tensors start on
// any residue mod 4 (odd lengths sit back to back), so a chunk is up to 3 head scalars, a body of 16-byte accesses and up to 3 tail
// scalars.  A chunk never crosses a tensor, so nothing a lane computes depends on another tensor's values.
//
// Norms.  Pass 1 forms u with lamb_u -- the ONE function pass 3 forms it with, compiled with contraction off (Makefile) so that both
// inlined copies are the same instructions: the norm is of the values that are applied -- and adds the exact squares of p and u in fp64
// (the square of an fp32 is exact in fp64): per lane in sweep order, a butterfly over the wave, the four waves in order.  Pass 2 adds a
// tensor's partials in ascending chunk order, forms phi in fp64 and rounds it to fp32 once.  No floating-point atomics: two launches
// write the same bits, and a workspace full of NaN changes nothing (every partial is written before it is read).
//
// Guard.  With a guard record that says non-finite, passes 1 and 2 return at once (wn, un, phi keep the last applied step's values) and
// pass 3 reads neither g, m nor v and writes neither p, m, v nor p16; the EMA copies take their lerp towards the unchanged p.
//
// Table entries are clamped into the slab: a malformed table reads and writes nothing outside [0, n) of any slab.
#include "common.h"
#include "slab_math.h"

constexpr int LAMB_CH = 4096;               // 256 lanes x 4 float4
constexpr int LAMB_MAX_GRID = 2048;         // 8 workgroups on each of 256 CUs
constexpr int LAMB_MAX_GROUPS = 256;        // one byte per element

struct LambChunk { int64_t start; int32_t len; int32_t tensor; };

struct LambArgs {
    float beta1, omb1, beta2, omb2, eps, bc1, bc2_sqrt;   // omb = 1 - beta in fp32; bc1 = 1-beta1^t, bc2_sqrt = sqrt(1-beta2^t) (host values)
    float gscale, max_norm, clip_value;
    const float* gnorm_sq;                                 // device scalar of ap_sumsq_f32, or nullptr
    const float* step_dev;                                 // device {lr (not read), bc1, bc2_sqrt} (graph replay), or nullptr
    const ap_guard_state* guard;                           // or nullptr
    const float* group_tab;                                // device {lr_eff, wd} per group
    int n_groups;
    const LambChunk* chunks;
    int n_chunks;
    const int* tensor_first;                               // [n_tensors + 1]: the first chunk of every tensor, ascending
    int n_tensors;
    int always_adapt, trust_clip;
    int n_ema;
    float decay[4];
    float* ema[4];
    bf16_t* ema16[4];                                      // nullptr: that copy is not emitted
    float* trust;                                          // [3][n_tensors]: wn, un, phi
    double* partial;                                       // [n_chunks][2]: sum p^2, sum u^2
    int64_t n;
};

// what every element of a launch shares
struct LambK { float beta1, omb1, beta2, omb2, eps, bc1, bc2_sqrt, gs, cv; };

__device__ __forceinline__ LambK lamb_consts(const LambArgs& a) {
    LambK k;
    k.beta1 = a.beta1; k.omb1 = a.omb1; k.beta2 = a.beta2; k.omb2 = a.omb2; k.eps = a.eps; k.bc1 = a.bc1; k.bc2_sqrt = a.bc2_sqrt;
    // (volatile: hipcc otherwise selects between the ADDRESS of the kernel argument and the device pointer and reads through scratch)
    if (a.step_dev) { const volatile float* s = a.step_dev; k.bc1 = s[1]; k.bc2_sqrt = s[2]; }
    if (a.guard) { const volatile float* s = &a.guard->bc1; k.bc1 = s[0]; k.bc2_sqrt = s[1]; }
    // the AdamW kernel's gradient: the pending mean, times clip_grad_norm_'s coefficient on the MEAN gradient; then clip_grad_value_
    k.gs = clip_gscale(a.gscale, a.gnorm_sq, a.max_norm);
    k.cv = a.clip_value;
    return k;
}

// THE update direction of one element: the moments m', v' and u = r / bc1 + wd * p.  Every operation below is one rounding (the file is
// compiled with -ffp-contract=off; the three fused multiply-adds are spelled out):
//   gh  1 (gs * g; a clamp is exact)         m'  2 (omb1 * gh, fma)          v'  3 (gh * gh, omb2 *, fma)
//   den 3 (sqrt, / bc2_sqrt, + eps)          r   1                           u   2 (r / bc1, fma with wd * p)
__device__ __forceinline__ float lamb_u(float p, float g, float m, float v, float wd, const LambK& k, float& m_new, float& v_new) {
    float gh = g * k.gs;
    if (k.cv > 0.f) gh = fminf(fmaxf(gh, -k.cv), k.cv);
    m_new = __builtin_fmaf(k.beta1, m, k.omb1 * gh);
    v_new = __builtin_fmaf(k.beta2, v, k.omb2 * (gh * gh));
    const float denom = sqrtf(v_new) / k.bc2_sqrt + k.eps;
    const float r = m_new / denom;
    return __builtin_fmaf(wd, p, r / k.bc1);
}

// how chunk c splits: `head` scalars up to the first 16-byte boundary, nv float4, `tail` scalars; everything clamped into the slab
struct LambGeo { int64_t start; int head, nv, tail, tensor; };
__device__ __forceinline__ LambGeo lamb_geo(const LambArgs& a, int c) {
    const LambChunk ch = a.chunks[c];
    LambGeo q;
    q.start = ch.start < 0 ? 0 : (ch.start > a.n ? a.n : ch.start);
    int64_t len = ch.len < 0 ? 0 : (ch.len > LAMB_CH ? LAMB_CH : ch.len);
    if (len > a.n - q.start) len = a.n - q.start;
    // (slab_split's arithmetic, restated: called through the function, hipcc gives k_lamb_norms two more SGPRs and k_lamb_apply another
    // schedule -- profiles/optim_core_refactor.txt)
    q.head = (int)((4 - (q.start & 3)) & 3);
    if (q.head > len) q.head = (int)len;
    q.nv = (int)((len - q.head) >> 2);
    q.tail = (int)(len - q.head - ((int64_t)q.nv << 2));
    q.tensor = ch.tensor < 0 ? 0 : (ch.tensor >= a.n_tensors ? a.n_tensors - 1 : ch.tensor);
    return q;
}
// the element thread `tid` takes of a chunk's head and tail scalars (one each for tid < head + tail), or -1
__device__ __forceinline__ int64_t lamb_scalar_index(const LambGeo& q, int tid) {
    if (tid < q.head) return q.start + tid;
    if (tid - q.head < q.tail) return q.start + q.head + ((int64_t)q.nv << 2) + (tid - q.head);
    return -1;
}

// {lr_eff, wd} of every group in LDS; the entries past n_groups are zeros, so a stray group byte reads nothing unwritten
__device__ __forceinline__ void lamb_load_groups(const LambArgs& a, float2* s_tab) {
    for (int gi = threadIdx.x; gi < LAMB_MAX_GROUPS; gi += blockDim.x)
        s_tab[gi] = gi < a.n_groups ? make_float2(a.group_tab[2 * gi], a.group_tab[2 * gi + 1]) : make_float2(0.f, 0.f);
    __syncthreads();
}

// ---- pass 1: two fp64 partials per chunk.  Reads only.
__global__ void __launch_bounds__(256)
k_lamb_norms(const float* __restrict__ p, const float* __restrict__ g, const float* __restrict__ m, const float* __restrict__ v,
             const unsigned char* __restrict__ group_id, LambArgs a) {
    __shared__ float2 s_tab[LAMB_MAX_GROUPS];
    __shared__ double red_p[4], red_u[4];
    if (a.guard && a.guard->nonfinite != 0) return;                                // (uniform over the grid: a skipped step measures nothing)
    const LambK k = lamb_consts(a);
    lamb_load_groups(a, s_tab);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
        const LambGeo q = lamb_geo(a, c);
        const int64_t b0 = q.start + q.head;                                       // (a multiple of 4, or the body is empty)
        double sp = 0.0, su = 0.0;
        for (int i = tid; i < q.nv; i += 256) {
            const float4 pp = reinterpret_cast<const float4*>(p + b0)[i];
            const float4 gg = reinterpret_cast<const float4*>(g + b0)[i];
            const float4 mm = reinterpret_cast<const float4*>(m + b0)[i];
            const float4 vv = reinterpret_cast<const float4*>(v + b0)[i];
            const uchar4 wm = reinterpret_cast<const uchar4*>(group_id + b0)[i];
            const float P[4] = {pp.x, pp.y, pp.z, pp.w}, G[4] = {gg.x, gg.y, gg.z, gg.w}, M[4] = {mm.x, mm.y, mm.z, mm.w}, V[4] = {vv.x, vv.y, vv.z, vv.w};
            const unsigned char W[4] = {wm.x, wm.y, wm.z, wm.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float mn, vn;                                                      // (pass 1 stores no moments)
                const float u = lamb_u(P[e], G[e], M[e], V[e], s_tab[W[e]].y, k, mn, vn);
                sq_add(P[e], sp);
                sq_add(u, su);
            }
        }
        const int64_t j = lamb_scalar_index(q, tid);
        if (j >= 0) {
            float mn, vn;
            const float u = lamb_u(p[j], g[j], m[j], v[j], s_tab[group_id[j]].y, k, mn, vn);
            sq_add(p[j], sp);
            sq_add(u, su);
        }
        wave_sum(sp, su);
        if (lane == 0) { red_p[wave] = sp; red_u[wave] = su; }
        __syncthreads();
        if (tid == 0) {
            a.partial[2 * (int64_t)c] = ((red_p[0] + red_p[1]) + red_p[2]) + red_p[3];
            a.partial[2 * (int64_t)c + 1] = ((red_u[0] + red_u[1]) + red_u[2]) + red_u[3];
        }
        __syncthreads();                                                           // (the next chunk writes red_* again)
    }
}

// ---- pass 2: one wave per tensor adds its chunks' partials in ascending chunk order (64 at a time through one coalesced load, then
// lane by lane) and forms the trust ratio.  Every lane holds the same sums.
__global__ void __launch_bounds__(256)
k_lamb_trust(const unsigned char* __restrict__ group_id, LambArgs a) {
    if (a.guard && a.guard->nonfinite != 0) return;
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= a.n_tensors) return;
    int c0 = a.tensor_first[t], c1 = a.tensor_first[t + 1];
    c0 = c0 < 0 ? 0 : (c0 > a.n_chunks ? a.n_chunks : c0);
    c1 = c1 < c0 ? c0 : (c1 > a.n_chunks ? a.n_chunks : c1);
    double sp = 0.0, su = 0.0;
    for (int base = c0; base < c1; base += 64) {
        const int idx = base + lane;
        const int ld = idx < c1 ? idx : c1 - 1;
        const double x = a.partial[2 * (int64_t)ld], y = a.partial[2 * (int64_t)ld + 1];
        const int cnt = c1 - base < 64 ? c1 - base : 64;
        for (int j = 0; j < cnt; ++j) { sp += __shfl(x, j, 64); su += __shfl(y, j, 64); }
    }
    float wd = 0.f;
    if (c1 > c0) {                                                                 // the tensor's group: the one of its first element
        const LambGeo q = lamb_geo(a, c0);
        if (q.start < a.n) { const int gi = group_id[q.start]; if (gi < a.n_groups) wd = a.group_tab[2 * gi + 1]; }
    }
    const double wn = sqrt(sp), un = sqrt(su);
    const bool adapt = a.always_adapt || wd != 0.f;
    double phi = (adapt && wn > 0.0 && un > 0.0) ? wn / un : 1.0;
    if (a.trust_clip) phi = fmin(phi, 1.0);
    if (lane == 0) {
        a.trust[t] = (float)wn;
        a.trust[a.n_tensors + t] = (float)un;
        a.trust[2 * (int64_t)a.n_tensors + t] = (float)phi;
    }
}

// one element of pass 3: p' = p - (lr_eff * phi) * u (2 roundings: the product, the fma), then the EMA lerps towards p'
__device__ __forceinline__ void lamb_ema_elem(float pnew, int64_t j, const LambArgs& a) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (e < a.n_ema) {
            const float d = a.decay[e];
            const float ee = __builtin_fmaf(d, a.ema[e][j], (1.0f - d) * pnew);
            a.ema[e][j] = ee;
            if (a.ema16[e]) a.ema16[e][j] = f2bf(ee);
        }
    }
}

// ---- pass 3: the update, the EMA copies and the bf16 stores
__global__ void __launch_bounds__(256)
k_lamb_apply(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
             const unsigned char* __restrict__ group_id, bf16_t* __restrict__ p16, LambArgs a) {
    __shared__ float2 s_tab[LAMB_MAX_GROUPS];
    const bool skip = a.guard && a.guard->nonfinite != 0;
    const LambK k = lamb_consts(a);
    lamb_load_groups(a, s_tab);
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
        const LambGeo q = lamb_geo(a, c);
        const int64_t b0 = q.start + q.head;
        const float phi = skip ? 0.f : a.trust[2 * (int64_t)a.n_tensors + q.tensor];
        for (int i = tid; i < q.nv; i += 256) {
            float4 pp = reinterpret_cast<const float4*>(p + b0)[i];
            if (!skip) {
                const float4 gg = reinterpret_cast<const float4*>(g + b0)[i];
                float4 mm = reinterpret_cast<const float4*>(m + b0)[i];
                float4 vv = reinterpret_cast<const float4*>(v + b0)[i];
                const uchar4 wm = reinterpret_cast<const uchar4*>(group_id + b0)[i];
                float* P = &pp.x; const float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
                const unsigned char W[4] = {wm.x, wm.y, wm.z, wm.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float2 t = s_tab[W[e]];
                    float mn, vn;
                    const float u = lamb_u(P[e], G[e], M[e], V[e], t.y, k, mn, vn);
                    P[e] = __builtin_fmaf(-(t.x * phi), u, P[e]);
                    M[e] = mn;
                    V[e] = vn;
                }
                reinterpret_cast<float4*>(p + b0)[i] = pp;
                if (p16) { u32x2 o; o[0] = pack_bf2(pp.x, pp.y); o[1] = pack_bf2(pp.z, pp.w); reinterpret_cast<u32x2*>(p16 + b0)[i] = o; }
                reinterpret_cast<float4*>(m + b0)[i] = mm;
                reinterpret_cast<float4*>(v + b0)[i] = vv;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e < a.n_ema) {
                    float4 ee = reinterpret_cast<const float4*>(a.ema[e] + b0)[i];
                    const float d = a.decay[e], omd = 1.0f - d;
                    ee.x = __builtin_fmaf(d, ee.x, omd * pp.x); ee.y = __builtin_fmaf(d, ee.y, omd * pp.y);
                    ee.z = __builtin_fmaf(d, ee.z, omd * pp.z); ee.w = __builtin_fmaf(d, ee.w, omd * pp.w);
                    reinterpret_cast<float4*>(a.ema[e] + b0)[i] = ee;
                    if (a.ema16[e]) { u32x2 o; o[0] = pack_bf2(ee.x, ee.y); o[1] = pack_bf2(ee.z, ee.w); reinterpret_cast<u32x2*>(a.ema16[e] + b0)[i] = o; }
                }
            }
        }
        const int64_t j = lamb_scalar_index(q, tid);
        if (j >= 0) {
            float pn = p[j];
            if (!skip) {
                const float2 t = s_tab[group_id[j]];
                float mn, vn;
                const float u = lamb_u(pn, g[j], m[j], v[j], t.y, k, mn, vn);
                pn = __builtin_fmaf(-(t.x * phi), u, pn);
                p[j] = pn;
                if (p16) p16[j] = f2bf(pn);
                m[j] = mn;
                v[j] = vn;
            }
            lamb_ema_elem(pn, j, a);
        }
    }
}

extern "C" int ap_lamb_chunk(void) { return LAMB_CH; }

// two fp64 partials per chunk
extern "C" size_t ap_lamb_workspace(int n_chunks) { return n_chunks > 0 ? (size_t)n_chunks * 2 * sizeof(double) : 0; }

extern "C" int ap_lamb_ema_step(float* p, const float* g, float* m, float* v, const uint8_t* group_id, int64_t n,
                                float beta1, float beta2, float eps, int step, float grad_scale,
                                const float* gnorm_sq, float max_norm, float clip_value, const float* step_scalars_dev,
                                float* const* ema, const float* ema_decay, int n_ema, ap_bf16* p_bf16, ap_bf16* const* ema_bf16,
                                const ap_guard_state* guard_or_null, const float* group_tab_dev, int n_groups,
                                const void* chunk_tab_dev, int n_chunks, const int32_t* tensor_first_dev, int n_tensors,
                                int always_adapt, int trust_clip, float* trust_out, void* workspace, size_t ws_bytes,
                                int grid_cap, int passes, ap_stream_t stream) {
    if (!p || !g || !m || !v || !group_id || !group_tab_dev || !chunk_tab_dev || !tensor_first_dev || !trust_out || !workspace) return AP_ERR_NULL;
    if (n <= 0 || n_ema < 0 || n_ema > 4 || step < 1 || n_groups < 1 || n_groups > LAMB_MAX_GROUPS || n_chunks < 1 || n_tensors < 1) return AP_ERR_SHAPE;
    if (n_ema > 0 && (!ema || !ema_decay)) return AP_ERR_NULL;
    if (gnorm_sq && !(max_norm > 0.f)) return AP_ERR_SHAPE;
    if (grid_cap < 0 || passes < 0 || passes > 7 || ws_bytes < ap_lamb_workspace(n_chunks)) return AP_ERR_SHAPE;
    if (((uintptr_t)p & 15) || ((uintptr_t)g & 15) || ((uintptr_t)m & 15) || ((uintptr_t)v & 15) || ((uintptr_t)group_id & 3) || ((uintptr_t)p_bf16 & 7) ||
        ((uintptr_t)group_tab_dev & 7) || ((uintptr_t)chunk_tab_dev & 15) || ((uintptr_t)tensor_first_dev & 3) || ((uintptr_t)trust_out & 3) ||
        ((uintptr_t)workspace & 7))
        return AP_ERR_SHAPE;
    LambArgs a;
    a.beta1 = beta1; a.omb1 = 1.0f - beta1; a.beta2 = beta2; a.omb2 = 1.0f - beta2; a.eps = eps;
    adam_bias_corrections(beta1, beta2, step, a.bc1, a.bc2_sqrt);                   // (ap_adamw_ema_step's)
    a.gscale = grad_scale; a.max_norm = max_norm; a.clip_value = clip_value > 0.f ? clip_value : 0.f;
    a.gnorm_sq = gnorm_sq; a.step_dev = step_scalars_dev; a.guard = guard_or_null;
    a.group_tab = group_tab_dev; a.n_groups = n_groups;
    a.chunks = static_cast<const LambChunk*>(chunk_tab_dev); a.n_chunks = n_chunks;
    a.tensor_first = tensor_first_dev; a.n_tensors = n_tensors;
    a.always_adapt = always_adapt != 0; a.trust_clip = trust_clip != 0;
    a.n_ema = n_ema;
    if (const int rc = slab_ema_args(ema, ema_decay, n_ema, ema_bf16, 15, a.ema, a.decay, a.ema16)) return rc;     // (an EMA slab off 16 bytes is refused here)
    a.trust = trust_out; a.partial = static_cast<double*>(workspace); a.n = n;
    const int cap = grid_cap > 0 ? grid_cap : LAMB_MAX_GRID;
    const unsigned grid = (unsigned)(n_chunks < cap ? n_chunks : cap);
    const int which = passes ? passes : 7;                                          // (bit 0: the norms, bit 1: the trust ratios, bit 2: the update)
    hipStream_t s = (hipStream_t)stream;
    bf16_t* p16 = reinterpret_cast<bf16_t*>(p_bf16);
    (void)hipGetLastError();
    if (which & 1) hipLaunchKernelGGL(k_lamb_norms, dim3(grid), dim3(256), 0, s, (const float*)p, g, (const float*)m, (const float*)v, group_id, a);
    if (which & 2) hipLaunchKernelGGL(k_lamb_trust, dim3((unsigned)((n_tensors + 3) / 4)), dim3(256), 0, s, group_id, a);
    if (which & 4) hipLaunchKernelGGL(k_lamb_apply, dim3(grid), dim3(256), 0, s, p, g, m, v, group_id, p16, a);
    return ap_check_launch();
}
