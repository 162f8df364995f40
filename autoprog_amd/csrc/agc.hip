// Adaptive gradient clipping (AGC) on the flat gradient slab: ap_agc_clip (the rule: include/autoprog_hip.h; reference: the trainer's
// `--clip-mode agc`, main_prog.py:129-132, 1019-1027 -> timm's adaptive_clip_grad / unitwise_norm).  One pass over the slab, no
// workspace (a one-wave launch in front zeroes the two tallies when the caller asks for them).
//
// The slab is cut into UNITS by a device table (one output row of a Linear, one output channel of a conv, one whole 1-D tensor).  A
// workgroup takes four consecutive units at a time, one wave each:
//   short unit (<= AGC_SHORT_MAX elements)  the wave loads the unit's g ONCE into registers (up to AGC_K float4 per lane) and p for the
//                                           norm only, reduces both sums of squares over the wave, and -- when the unit clips -- multiplies
//                                           the registers and stores them.  An unclipped unit is never stored.
//   long unit                               the four waves of the workgroup that owns it walk it together: one walk for the two sums,
//                                           a second one over g when it clips.  A unit is never split across workgroups.
// A unit may start at any offset mod 4 (tensors of odd length sit back to back): up to 3 head elements and up to 3 tail elements go as
// scalars, everything between as 16-byte accesses (both slabs are 16-byte aligned at the same offsets).
// Sums are of exact squares in fp64 (sq_add, sq_add_finite, wave_sum and the split: slab_math.h), added in a fixed order: per lane in
// sweep order, a butterfly over the wave, the four waves in order.  No floating-point atomics: two launches write the same bits.  The
// two tallies are integers.
//
// Loads in flight.  The pass is bound by memory latency, not by arithmetic, so every load of a unit is issued before the first one is
// used.  Two forms that read naturally defeat that with hipcc; together they ran at 82 us where this file runs at 59 us (VOLO-D1's
// slab, profiles/agc.txt):
//   `(i < nv) ? v[i] : 0`   becomes a per-lane branch around the load; the first use (the conversion to fp64) is sunk into the branch
//                           and an s_waitcnt vmcnt(0) with it: every load waits for itself.  The short path reads through buffer
//                           descriptors, whose bounds check returns zeros past the end; the long walk (agc_ld4 / agc_ld1) loads from
//                           an address clamped into the unit in EVERY lane and drops the value with a select.
//   five scalar loads of table entries, each clamped before the next address is formed, cost five round trips in a row.  The table
//                           goes through one vector load per wave and readlane (agc_ask_group / agc_take_group).
#include "common.h"
#include "slab_math.h"

constexpr int AGC_K = 8;                            // float4 per lane a short unit keeps in registers
constexpr int AGC_SHORT_MAX = 64 * 4 * AGC_K;       // 2048: at most 512 aligned float4 (64 lanes x AGC_K) whatever the head and tail
constexpr int AGC_MAX_GRID = 4096;                  // workgroups; each sweep of the grid covers 4 x this many units
constexpr int AGC_P_CHUNK = 4;                      // float4 of p per lane a short unit has in flight at a time
constexpr int AGC_LONG_UNROLL = 4;                  // float4 of g and of p a thread of the long walk has in flight

// the rule, from the two sums of squares: -> the factor to multiply the unit by, `clipped` set when it is to be applied.  A unit with a
// non-finite gradient element is left alone (factor 1).
__device__ __forceinline__ float agc_factor(double sg, double sp, int bad, float clip_factor, float eps, float grad_scale, bool& clipped) {
    clipped = false;
    if (bad) return 1.0f;
    const double gn = (double)grad_scale * sqrt(sg);                               // the norm of the MEAN gradient
    const double max_norm = fmax(sqrt(sp), (double)eps) * (double)clip_factor;
    if (gn < max_norm) return 1.0f;
    clipped = true;
    return (float)(max_norm / fmax(gn, 1e-6));
}

__device__ __forceinline__ float4 agc_scale4(float4 v, float f) { v.x *= f; v.y *= f; v.z *= f; v.w *= f; return v; }

// float4 i of a body of nv > 0 float4, zeros for i >= nv: the address is clamped into the body, the load is made by every lane
__device__ __forceinline__ float4 agc_ld4(const float4* __restrict__ v, int64_t i, int64_t nv) {
    const float4 r = v[i < nv ? i : nv - 1];
    return i < nv ? r : make_float4(0.f, 0.f, 0.f, 0.f);
}
// element i of a slab, or 0 where the lane has none (`mine`): the address is clamped to `last`, an element of the same unit
__device__ __forceinline__ float agc_ld1(const float* __restrict__ v, int64_t i, int64_t last, bool mine) {
    const float r = v[i < last ? i : last];
    return mine ? r : 0.f;
}

// Short units are read through buffer descriptors (hardware bounds check: a lane past the end gets zeros, without a branch and without
// an address of its own): one over the unit for its head and tail scalars, one over its aligned body for the float4.  Descriptors are
// built from wave-uniform values only.
constexpr unsigned AGC_RSRC_FLAGS = 0x00020000u;
constexpr unsigned AGC_OOB = 0x7ffffff0u;               // a byte offset past any unit: the load returns 0
template <class R> __device__ __forceinline__ float4 agc_buf4(R rsrc, unsigned byte_off) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, byte_off, 0, 0);
    return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
}
template <class R> __device__ __forceinline__ float agc_buf1(R rsrc, unsigned byte_off) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, byte_off, 0, 0));
}

// one short unit [b, e), e > b, by one wave; KS = the float4 per lane its body takes at most.  -> the factor
template <int KS>
__device__ __forceinline__ float agc_short_unit(float* __restrict__ g, const float* __restrict__ p, int64_t b, int64_t e, int lane,
                                                float clip_factor, float eps, float grad_scale, int& n_clip, int& n_bad) {
    int head, tail;
    int64_t nv64;
    slab_split(b, e - b, head, nv64, tail);
    const int nv = (int)nv64, len = (int)(e - b);
    float* g_body = g + b + head;                                                  // (b + head is a multiple of 4, or the body is empty)
    const auto g_unit = __builtin_amdgcn_make_buffer_rsrc(g + b, 0, len * 4, AGC_RSRC_FLAGS);
    const auto g_vec = __builtin_amdgcn_make_buffer_rsrc(g_body, 0, nv * 16, AGC_RSRC_FLAGS);
    const auto p_unit = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p) + b, 0, len * 4, AGC_RSRC_FLAGS);
    const auto p_vec = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p) + b + head, 0, nv * 16, AGC_RSRC_FLAGS);
    const unsigned off_h = lane < head ? (unsigned)lane * 4u : AGC_OOB;
    const unsigned off_t = lane < tail ? (unsigned)(head + (nv << 2) + lane) * 4u : AGC_OOB;
    constexpr int YS = KS < AGC_P_CHUNK ? KS : AGC_P_CHUNK;
    float4 x[KS];
#pragma unroll
    for (int k = 0; k < KS; ++k) x[k] = agc_buf4(g_vec, (unsigned)lane * 16u + 1024u * k);
    const float xh = agc_buf1(g_unit, off_h), xt = agc_buf1(g_unit, off_t);
    const float yh = agc_buf1(p_unit, off_h), yt = agc_buf1(p_unit, off_t);
    // p is read for the norm only, AGC_P_CHUNK float4 per lane at a time: its registers go to g, which stays.  (All of p at once beside
    // all of g is 64 registers of data and costs a wave per SIMD; a unit of up to 1024 elements still has everything in flight.)
    double g0 = 0.0, g1 = 0.0, p0 = 0.0, p1 = 0.0;
    int bad = 0;
#pragma unroll
    for (int h = 0; h < KS; h += YS) {
        float4 y[YS];
#pragma unroll
        for (int k = 0; k < YS; ++k) y[k] = agc_buf4(p_vec, (unsigned)lane * 16u + 1024u * (h + k));
#pragma unroll
        for (int k = 0; k < YS; ++k) { sq_add(y[k].x, p0); sq_add(y[k].y, p1); sq_add(y[k].z, p0); sq_add(y[k].w, p1); }
    }
#pragma unroll
    for (int k = 0; k < KS; ++k) { sq_add_finite(x[k].x, g0, bad); sq_add_finite(x[k].y, g1, bad); sq_add_finite(x[k].z, g0, bad); sq_add_finite(x[k].w, g1, bad); }
    double sg = g0 + g1, sp = p0 + p1;
    sq_add_finite(xh, sg, bad); sq_add_finite(xt, sg, bad);
    sq_add(yh, sp); sq_add(yt, sp);
    wave_sum(sg, sp, bad);
    bool clipped;
    const float f = agc_factor(sg, sp, bad, clip_factor, eps, grad_scale, clipped);
    if (clipped) {                                                                 // (wave-uniform: every lane holds the same sums)
#pragma unroll
        for (int k = 0; k < KS; ++k) { const int i = lane + 64 * k; if (i < nv) reinterpret_cast<float4*>(g_body)[i] = agc_scale4(x[k], f); }
        if (lane < head) g[b + lane] = xh * f;
        if (lane < tail) g_body[(nv << 2) + lane] = xt * f;
    }
    n_clip += clipped ? 1 : 0;
    n_bad += bad ? 1 : 0;
    return f;
}

// the table entries of the four units base .. base + 3: five bounds and four skip bytes.  agc_ask_group issues ONE load of each kind per
// wave -- lane j holds bound min(j, 4) and skip byte j & 3 -- and agc_take_group, called an iteration later, spreads them over the wave
// with readlane: the table costs one memory round trip per group, and that one runs beside the previous group's work.  Bounds are
// clamped into the slab and made ascending: a malformed table reads and writes nothing outside g[0, n) and p[0, n).  A unit past the
// table's end comes out empty.
struct AgcGroup { int64_t off[5]; unsigned skip[4]; };
struct AgcAsked { int64_t off; unsigned skip; };
__device__ __forceinline__ AgcAsked agc_ask_group(const int64_t* __restrict__ unit_off, const unsigned char* __restrict__ unit_skip, int64_t base,
                                                  int n_units, int lane) {
    const int64_t io = base + (lane < 4 ? lane : 4), is = base + (lane & 3);
    AgcAsked a;
    a.off = unit_off[io < n_units ? io : n_units];
    a.skip = unit_skip[is < n_units ? is : n_units - 1];
    return a;
}
__device__ __forceinline__ void agc_take_group(const AgcAsked& a, int64_t n, AgcGroup& gr) {
    const int lo = (int)(a.off & 0xffffffff), hi = (int)(a.off >> 32);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int64_t v = (int64_t)(((uint64_t)(unsigned)__builtin_amdgcn_readlane(hi, j) << 32) | (unsigned)__builtin_amdgcn_readlane(lo, j));
        gr.off[j] = v < 0 ? 0 : (v > n ? n : v);
    }
#pragma unroll
    for (int j = 1; j < 5; ++j) if (gr.off[j] < gr.off[j - 1]) gr.off[j] = gr.off[j - 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) gr.skip[j] = (unsigned)__builtin_amdgcn_readlane((int)a.skip, j);
}

// (four waves per SIMD, nothing in scratch)
__global__ void __launch_bounds__(256, 4)
k_agc_clip(float* __restrict__ g, const float* __restrict__ p, int64_t n, const int64_t* __restrict__ unit_off,
           const unsigned char* __restrict__ unit_skip, int n_units, float clip_factor, float eps, float grad_scale,
           float* __restrict__ unit_factor, int* __restrict__ counts) {
    __shared__ double red_g[4], red_p[4];
    __shared__ int red_c[4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int n_clip = 0, n_bad = 0;                                                     // this wave's tallies (lane 0 holds them)
    // groups of four units, swept from the END of the table: the reducer lays the slab in reversed parameter order, so the one long unit
    // of a VOLO or DeiT that is not a head -- pos_embed -- sits at its very end; its workgroup starts first and the rest runs beside it
    const int64_t n_groups = ((int64_t)n_units + 3) >> 2;
    AgcAsked asked = {0, 0};
    if ((int64_t)blockIdx.x < n_groups) asked = agc_ask_group(unit_off, unit_skip, (n_groups - 1 - blockIdx.x) * 4, n_units, lane);
    for (int64_t q = blockIdx.x; q < n_groups; q += gridDim.x) {
        const int64_t base = (n_groups - 1 - q) * 4;
        AgcGroup cur;
        agc_take_group(asked, n, cur);
        // the next group's table entries are asked for now and first read an iteration later: their latency runs beside this group's
        if (q + gridDim.x < n_groups) asked = agc_ask_group(unit_off, unit_skip, (n_groups - 1 - q - gridDim.x) * 4, n_units, lane);
        // ---- this wave's unit, when it is short
        const int64_t u = base + wave;
        if (u < n_units) {
            const int64_t b = wave == 0 ? cur.off[0] : wave == 1 ? cur.off[1] : wave == 2 ? cur.off[2] : cur.off[3];
            const int64_t e = wave == 0 ? cur.off[1] : wave == 1 ? cur.off[2] : wave == 2 ? cur.off[3] : cur.off[4];
            const bool skip = (wave == 0 ? cur.skip[0] : wave == 1 ? cur.skip[1] : wave == 2 ? cur.skip[2] : cur.skip[3]) != 0;
            if (skip || e - b <= AGC_SHORT_MAX) {
                float f = 1.0f;
                if (!skip && e > b) {
                    int head, tail;
                    int64_t nv;
                    slab_split(b, e - b, head, nv, tail);                          // (wave-uniform: the body's length picks the code)
                    if (nv <= 128) f = agc_short_unit<2>(g, p, b, e, lane, clip_factor, eps, grad_scale, n_clip, n_bad);
                    else f = agc_short_unit<AGC_K>(g, p, b, e, lane, clip_factor, eps, grad_scale, n_clip, n_bad);
                }
                if (unit_factor && lane == 0) unit_factor[u] = f;
            }
        }
        // ---- the long units among these four: the whole workgroup, one after the other (every wave holds the same table entries, so
        // the branches and barriers below are uniform over the workgroup)
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            const int64_t uj = base + j;
            const int64_t b = j == 0 ? cur.off[0] : j == 1 ? cur.off[1] : j == 2 ? cur.off[2] : cur.off[3];
            const int64_t e = j == 0 ? cur.off[1] : j == 1 ? cur.off[2] : j == 2 ? cur.off[3] : cur.off[4];    // (a unit past the table's end is empty)
            if (e - b <= AGC_SHORT_MAX || (j == 0 ? cur.skip[0] : j == 1 ? cur.skip[1] : j == 2 ? cur.skip[2] : cur.skip[3]) != 0) continue;
            int head, tail;
            int64_t nv;
            slab_split(b, e - b, head, nv, tail);                                  // (nv > 0)
            float* g_body = g + b + head;
            const float* p_body = p + b + head;
            const float4* gv = reinterpret_cast<const float4*>(g_body);
            const float4* pv = reinterpret_cast<const float4*>(p_body);
            const int tid = threadIdx.x;
            const float xh = agc_ld1(g, b + tid, e - 1, tid < head), xt = agc_ld1(g_body, (nv << 2) + tid, (e - 1) - (b + head), tid < tail);
            const float yh = agc_ld1(p, b + tid, e - 1, tid < head), yt = agc_ld1(p_body, (nv << 2) + tid, (e - 1) - (b + head), tid < tail);
            double g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0, p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
            int bad = 0;
            for (int64_t i0 = tid; i0 < nv; i0 += 256 * AGC_LONG_UNROLL) {
                float4 x[AGC_LONG_UNROLL], y[AGC_LONG_UNROLL];
#pragma unroll
                for (int k = 0; k < AGC_LONG_UNROLL; ++k) x[k] = agc_ld4(gv, i0 + 256 * k, nv);
#pragma unroll
                for (int k = 0; k < AGC_LONG_UNROLL; ++k) y[k] = agc_ld4(pv, i0 + 256 * k, nv);
#pragma unroll
                for (int k = 0; k < AGC_LONG_UNROLL; ++k) {
                    sq_add_finite(x[k].x, g0, bad); sq_add_finite(x[k].y, g1, bad); sq_add_finite(x[k].z, g2, bad); sq_add_finite(x[k].w, g3, bad);
                    sq_add(y[k].x, p0); sq_add(y[k].y, p1); sq_add(y[k].z, p2); sq_add(y[k].w, p3);
                }
            }
            double sg = (g0 + g1) + (g2 + g3), sp = (p0 + p1) + (p2 + p3);
            sq_add_finite(xh, sg, bad); sq_add_finite(xt, sg, bad);
            sq_add(yh, sp); sq_add(yt, sp);
            wave_sum(sg, sp, bad);
            if (lane == 0) { red_g[wave] = sg; red_p[wave] = sp; red_c[wave] = bad; }
            __syncthreads();
            sg = ((red_g[0] + red_g[1]) + red_g[2]) + red_g[3];
            sp = ((red_p[0] + red_p[1]) + red_p[2]) + red_p[3];
            bad = red_c[0] + red_c[1] + red_c[2] + red_c[3];
            bool clipped;
            const float f = agc_factor(sg, sp, bad, clip_factor, eps, grad_scale, clipped);
            if (clipped) {
                for (int64_t i0 = tid; i0 < nv; i0 += 256 * AGC_LONG_UNROLL) {
                    float4 x[AGC_LONG_UNROLL];
#pragma unroll
                    for (int k = 0; k < AGC_LONG_UNROLL; ++k) x[k] = agc_ld4(gv, i0 + 256 * k, nv);
#pragma unroll
                    for (int k = 0; k < AGC_LONG_UNROLL; ++k) { const int64_t i = i0 + 256 * k; if (i < nv) reinterpret_cast<float4*>(g_body)[i] = agc_scale4(x[k], f); }
                }
                if (tid < head) g[b + tid] = xh * f;
                if (tid < tail) g_body[(nv << 2) + tid] = xt * f;
            }
            if (tid == 0) {
                if (unit_factor) unit_factor[uj] = f;
                n_clip += clipped ? 1 : 0;
                n_bad += bad ? 1 : 0;
            }
            __syncthreads();                                                       // (the next long unit writes red_* again)
        }
    }
    if (counts && lane == 0) {
        if (n_clip) atomicAdd(&counts[0], n_clip);
        if (n_bad) atomicAdd(&counts[1], n_bad);
    }
}

// the two tallies start at zero: a kernel node like every other one of a captured step
__global__ void k_agc_zero_counts(int* __restrict__ counts) { if (threadIdx.x < 2) counts[threadIdx.x] = 0; }

extern "C" int ap_agc_short_max(void) { return AGC_SHORT_MAX; }

extern "C" int ap_agc_clip(float* g, const float* p, int64_t n, const int64_t* unit_off, const uint8_t* unit_skip, int n_units,
                           float clip_factor, float eps, float grad_scale, float* unit_factor_or_null, int32_t* counts_or_null,
                           ap_stream_t stream) {
    if (!g || !p || !unit_off || !unit_skip) return AP_ERR_NULL;
    if (n <= 0 || n_units <= 0) return AP_ERR_SHAPE;
    if (((uintptr_t)g & 15) || ((uintptr_t)p & 15) || ((uintptr_t)unit_off & 7) || ((uintptr_t)unit_factor_or_null & 3) || ((uintptr_t)counts_or_null & 3))
        return AP_ERR_SHAPE;
    if (!(clip_factor > 0.f && clip_factor <= 3.0e38f) || !(eps >= 0.f && eps <= 3.0e38f) || !(grad_scale > 0.f && grad_scale <= 3.0e38f)) return AP_ERR_SHAPE;
    int64_t grid = ((int64_t)n_units + 3) / 4;
    if (grid > AGC_MAX_GRID) grid = AGC_MAX_GRID;
    (void)hipGetLastError();
    if (counts_or_null) hipLaunchKernelGGL(k_agc_zero_counts, dim3(1), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<int*>(counts_or_null));
    hipLaunchKernelGGL(k_agc_clip, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, g, p, n, unit_off, unit_skip, n_units, clip_factor, eps,
                       grad_scale, unit_factor_or_null, reinterpret_cast<int*>(counts_or_null));
    return ap_check_launch();
}
