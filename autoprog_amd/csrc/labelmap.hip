// ap_label_map_crop: stored top-k label maps -> the (class, score) pairs of a SparseTokenLabelTarget, ROI-aligned to each image's crop box
// and flipped with it, in ONE launch (include/autoprog_hip.h has the rule).  The reference's loader does this on the CPU before tlt's
// create_token_label_target (main_prog.py:994-1004): it densifies the stored NFNet-F6 maps and calls roi_align(aligned=False,
// sampling_ratio=-1) on them.  Here the box is drawn on the device side of the loader (data.DeviceRandomResizedCrop), so the maps are cut
// where the box is known, and nothing is densified: a bin's candidates are the (class, weight * score) of the few map pixels it touches.
//
// A bin is one row of the target: the class slot (a 1 x 1 pooling of the box) or one of the P x P token slots.  Its work is
//   1. the footprint: the map pixels its samples touch, per axis from the first and the last sample position
//   2. one candidate per (k, pixel) of the footprint: the class and  wy[y] * wx[x] * score,  the separable form of the sample loop
//   3. equal classes merged, each sum formed in candidate order
//   4. the K largest sums > 0 (equal sums: ascending class), and the sum of the rest into `dropped`
// Two bin sizes, two bodies.  A token bin touches a handful of pixels: up to 128 candidates are held two per lane by ONE wave, merged by
// passing every candidate round the wave once (a sum is formed by the first lane of its class, in candidate order), four bins per
// workgroup.  The class slot touches the whole box, up to 4096 candidates: the workgroup keeps them in LDS, sorts (class, candidate)
// keys, and sums each run of a class in a fixed order (per 16-key chunk, then the chunks of a run in order).  A token bin with a larger
// footprint (P = 1, a box that covers the map at a small P) takes the workgroup body too: the choice is made in the kernel from the
// record, the launch geometry never depends on it.  No atomics, every sum in a fixed order: bit-reproducible.
//
// Sample positions and the per-axis weights are fp64, the reference's expression operation for operation (built with -ffp-contract=off,
// csrc/Makefile), so a sample falls between the same two pixels as in the fp64 restatement (tests/_labelmap_ref.py) and a weight carries
// one fp32 rounding; products and sums are fp32.  Everything indexed is clamped: the footprint lies inside the map and holds at most
// Hm * Wm * Kin <= 4096 candidates whatever the record says, and a pixel's weight visits at most 16 samples.
#include "common.h"

#if defined(__FAST_MATH__)
#error "labelmap.hip must be built with -ffp-contract=off and without fast-math (csrc/Makefile)"
#endif

#define LM_THREADS 256
#define LM_MAXCAND 4096            // candidates of one bin in LDS
#define LM_WAVE_CAND 128           // candidates one wave holds: two per lane
#define LM_WAVE_SIDE 32            // ... on a footprint of at most 32 pixels per axis (the axis weights live in the wave's lanes)
#define LM_TOK_PER_BLOCK 4         // token bins per workgroup, one per wave
#define LM_NO_CLASS 0xfffffu       // class field of the key of a candidate without a class

typedef unsigned long long lm_u64;

struct LmAxis { double b1, bin, gd; int g, n; };       // box start, bin extent, samples per bin (fp64 and int), map extent
struct LmBin { LmAxis ay, ax; int ph, pw, ylo, ny, xlo, nx, slot; };

// (int)v clamped into [lo, hi]; a NaN gives lo
__device__ __forceinline__ int lm_d2i(double v, int lo, int hi) { return (int)fmin(fmax(v, (double)lo), (double)hi); }

__device__ __forceinline__ LmAxis lm_axis(float a1, float a2, int pn, int n) {
    LmAxis A;
    A.b1 = (double)a1;
    const double roi = fmax((double)a2 - (double)a1, 1.0);
    A.bin = roi / (double)pn;
    A.gd = fmin(fmax(ceil(roi / (double)pn), 1.0), 1073741824.0);
    A.g = (int)A.gd;
    A.n = n;
    return A;
}
// position of sample i of bin p:  x1 + pw * bin_w + (ix + 0.5) * bin_w / gw
__device__ __forceinline__ double lm_pos(const LmAxis& A, int p, int i) { return A.b1 + (double)p * A.bin + ((double)i + 0.5) * A.bin / A.gd; }

// the pixels bin p's samples touch (positions are monotone in i): [lo, hi] inside the map
__device__ __forceinline__ void lm_span(const LmAxis& A, int p, int& lo, int& n) {
    const double first = lm_pos(A, p, 0), last = lm_pos(A, p, A.g - 1);
    lo = lm_d2i(floor(fmax(first, 0.0)), 0, A.n - 1);
    n = lm_d2i(floor(fmax(last, 0.0)) + 1.0, lo, A.n - 1) - lo + 1;
}

// weight of map pixel x in bin p: (sum over the bin's samples of the pixel's share) / g.  Only samples within one pixel of x have a share;
// they are found from the sample pitch (> 0.5 wherever a bin has more than one sample) with a sample of slack on either side.
__device__ double lm_weight(const LmAxis& A, int p, int x) {
    const double start = A.b1 + (double)p * A.bin, pitch = A.bin / A.gd;
    const int i0 = lm_d2i(floor(((double)x - 1.0 - start) / pitch - 0.5) - 1.0, 0, A.g - 1);
    const int i1 = min(lm_d2i(ceil(((double)x + 1.0 - start) / pitch - 0.5) + 1.0, 0, A.g - 1), i0 + 15);
    double w = 0.0;
    for (int i = i0; i <= i1; ++i) {
        double s = lm_pos(A, p, i);
        if (s < -1.0 || s > (double)A.n) continue;
        s = fmax(s, 0.0);
        int lo = lm_d2i(s, 0, A.n - 1), hi;
        if (lo >= A.n - 1) { lo = hi = A.n - 1; s = (double)lo; } else hi = lo + 1;
        const double l = s - (double)lo, h = 1.0 - l;
        w += (lo == x ? h : 0.0) + (hi == x ? l : 0.0);
    }
    return w / A.gd;
}

// bin 0: the class slot; bin 1 + ph * P + pw: a token bin
__device__ __forceinline__ LmBin lm_bin(const ap_label_map_crop_args& A, const float* rec, int bin) {
    LmBin G;
    const int P = A.P, flip = rec[4] >= 0.5f ? 1 : 0;
    const int pn = bin == 0 ? 1 : P, t = max(bin - 1, 0);
    G.ph = t / P; G.pw = t - G.ph * P;
    G.slot = bin == 0 ? 1 : 2 + G.ph * P + (flip ? P - 1 - G.pw : G.pw);
    G.ax = lm_axis(rec[0], rec[2], pn, A.Wm);
    G.ay = lm_axis(rec[1], rec[3], pn, A.Hm);
    lm_span(G.ax, G.pw, G.xlo, G.nx);
    lm_span(G.ay, G.ph, G.ylo, G.ny);
    return G;
}

// candidate (k, y, x) of image b: its class (-1: none, outside [0, C)) and score
__device__ __forceinline__ void lm_load(const ap_label_map_crop_args& A, int b, int k, int y, int x, int& cls, float& s) {
    const int64_t off = ((int64_t)k * A.Hm + y) * A.Wm + x;
    const int64_t so = (int64_t)b * A.score_stride + off, co = (int64_t)b * A.class_stride + off;
    const bool half = A.score_dtype == AP_LM_F16;
    s = half ? (float)reinterpret_cast<const _Float16*>(A.scores)[so] : reinterpret_cast<const float*>(A.scores)[so];
    if (A.class_dtype == AP_LM_CLASS_I32) cls = reinterpret_cast<const int*>(A.classes)[co];
    else {
        const float cf = half ? (float)reinterpret_cast<const _Float16*>(A.classes)[co] : reinterpret_cast<const float*>(A.classes)[co];
        cls = (cf > -1.f && cf < 65537.f) ? (int)cf : -1;                    // truncation; a NaN has no class
    }
    if (cls < 0 || cls >= A.C) cls = -1;
}

// a sum > 0 and its class as one integer: the unsigned order is descending sum, then ascending class; 0: nothing
__device__ __forceinline__ lm_u64 lm_key(float sum, unsigned cls) { return ((lm_u64)__float_as_uint(sum) << 32) | (0xffffffffu - cls); }

__device__ __forceinline__ lm_u64 lm_wave_max(lm_u64 k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned hi = (unsigned)__shfl_xor((int)(k >> 32), o, 64), lo = (unsigned)__shfl_xor((int)(unsigned)k, o, 64);
        const lm_u64 t = ((lm_u64)hi << 32) | lo;
        k = t > k ? t : k;
    }
    return k;
}

// the K largest of the group's keys into the row (thread j stores round j), the rest summed into *dropped: NW waves, CPL keys per thread.
// Keys of a bin are distinct (one per class), so a round removes exactly its winner.  Sums: per thread in index order, one xor tree per
// wave, the waves in order.
template <int NW, int CPL>
__device__ __forceinline__ void lm_select(lm_u64 (&key)[CPL], int K, int tid, int* __restrict__ idx_row, float* __restrict__ val_row,
                                          float* __restrict__ dropped, lm_u64* red, float* redf) {
    const int lane = tid & 63, wave = tid >> 6;
    for (int j = 0; j < K; ++j) {
        lm_u64 t = 0;
#pragma unroll
        for (int e = 0; e < CPL; ++e) t = key[e] > t ? key[e] : t;
        t = lm_wave_max(t);
        if (NW > 1) {
            if (lane == 0) red[(j & 1) * 4 + wave] = t;
            __syncthreads();
            t = red[(j & 1) * 4];
#pragma unroll
            for (int w = 1; w < NW; ++w) t = red[(j & 1) * 4 + w] > t ? red[(j & 1) * 4 + w] : t;
        }
#pragma unroll
        for (int e = 0; e < CPL; ++e) key[e] = key[e] == t ? 0 : key[e];
        if (tid == j) {
            idx_row[j] = t ? (int)(0xffffffffu - (unsigned)t) : -1;
            val_row[j] = t ? __uint_as_float((unsigned)(t >> 32)) : 0.f;
        }
    }
    if (dropped) {
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < CPL; ++e) d += __uint_as_float((unsigned)(key[e] >> 32));
        d = group_sum<64>(d);
        if (NW > 1) {
            if (lane == 0) redf[wave] = d;
            __syncthreads();
            d = redf[0];
#pragma unroll
            for (int w = 1; w < NW; ++w) d += redf[w];
        }
        if (tid == 0) *dropped = d;
    }
}

// ---------------------------------------------------------------------------------------------------------------- one wave, <= 128 candidates
// Candidate j = k * npix + (y - ylo) * nx + (x - xlo) lives in lane j & 63, register j >> 6.
__device__ __forceinline__ void lm_bin_wave(const ap_label_map_crop_args& A, int b, const LmBin& G, int lane, int* __restrict__ idx_row,
                                            float* __restrict__ val_row, float* __restrict__ dropped) {
    float aw = 0.f;                                   // lanes 0 .. nx-1: wx of their column; lanes 32 .. 32+ny-1: wy of their row
    if (lane < G.nx) aw = (float)lm_weight(G.ax, G.pw, G.xlo + lane);
    else if (lane >= LM_WAVE_SIDE && lane - LM_WAVE_SIDE < G.ny) aw = (float)lm_weight(G.ay, G.ph, G.ylo + lane - LM_WAVE_SIDE);
    const int npix = G.nx * G.ny, n = npix * A.Kin;
    int cls[2];
    float v[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int j = lane + 64 * m, jj = min(j, n - 1);
        const int k = jj / npix, p = jj - k * npix, py = p / G.nx, px = p - py * G.nx;
        const float w = __shfl(aw, LM_WAVE_SIDE + py, 64) * __shfl(aw, px, 64);
        cls[m] = -1; v[m] = 0.f;
        if (j < n) {
            float s;
            lm_load(A, b, k, G.ylo + py, G.xlo + px, cls[m], s);
            v[m] = cls[m] >= 0 ? w * s : 0.f;
        }
    }
    float sum[2] = {0.f, 0.f};
    bool lead[2] = {cls[0] >= 0, cls[1] >= 0};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int cnt = min(n - 64 * h, 64);
        for (int i = 0; i < cnt; ++i) {               // (uniform trip count and source lane)
            const int ci = __shfl(cls[h], i, 64);
            const float vi = __shfl(v[h], i, 64);
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                if (ci == cls[m]) {
                    sum[m] += vi;
                    if (i + 64 * h < lane + 64 * m) lead[m] = false;
                }
            }
        }
    }
    lm_u64 key[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) key[m] = (lead[m] && sum[m] > 0.f) ? lm_key(sum[m], (unsigned)cls[m]) : 0;
    lm_select<1, 2>(key, A.K, lane, idx_row, val_row, dropped, nullptr, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------- the workgroup, <= 4096 candidates
struct LmShared {
    __attribute__((aligned(16))) unsigned keys[LM_MAXCAND + 8];   // first the axis weights (nx + ny <= 4097 floats), then the sort keys
    float vals[LM_MAXCAND];                                        // weight * score by candidate
    float carry[LM_THREADS];                                       // per chunk: the sum of its leading keys that continue the run before it
    int flags[LM_THREADS];                                         // bit 0: the chunk starts inside a run, bit 1: it lies inside that run entirely
    lm_u64 red[8];
    float redf[4];
    int big[LM_TOK_PER_BLOCK];
};

__device__ void lm_bin_block(const ap_label_map_crop_args& A, int b, const LmBin& G, int tid, int* __restrict__ idx_row,
                             float* __restrict__ val_row, float* __restrict__ dropped, LmShared& S) {
    const int npix = G.nx * G.ny, n = min(npix * A.Kin, LM_MAXCAND);          // (== npix * Kin: the footprint lies inside the map)
    int N2 = 64;
    while (N2 < n) N2 <<= 1;
    __syncthreads();                                                          // (the bin before this one is done with the arrays)
    float* wtab = reinterpret_cast<float*>(S.keys);
    for (int t = tid; t < G.nx + G.ny; t += LM_THREADS)
        wtab[t] = t < G.nx ? (float)lm_weight(G.ax, G.pw, G.xlo + t) : (float)lm_weight(G.ay, G.ph, G.ylo + t - G.nx);
    __syncthreads();
    int cl[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int j = tid + LM_THREADS * e;
        cl[e] = -1;
        if (j < n) {
            const int k = j / npix, p = j - k * npix, py = p / G.nx, px = p - py * G.nx;
            float s;
            lm_load(A, b, k, G.ylo + py, G.xlo + px, cl[e], s);
            S.vals[j] = cl[e] >= 0 ? (wtab[G.nx + py] * wtab[px]) * s : 0.f;
        }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int j = tid + LM_THREADS * e;
        if (j < N2) S.keys[j] = cl[e] >= 0 ? ((unsigned)cl[e] << 12) | (unsigned)j : 0xffffffffu;
    }
    // bitonic sort of keys[0 .. N2): ascending (class, candidate), the keys without a class last
    for (int k = 2; k <= N2; k <<= 1) {
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
            __syncthreads();
            for (int i = tid; i < (N2 >> 1); i += LM_THREADS) {
                const int a = ((i & ~(jj - 1)) << 1) | (i & (jj - 1)), c = a | jj;
                const unsigned x = S.keys[a], y = S.keys[c];
                if ((x > y) == ((a & k) == 0)) { S.keys[a] = y; S.keys[c] = x; }
            }
        }
    }
    __syncthreads();
    // thread t owns the sorted keys 16 t .. 16 t + 15
    const int nch = N2 >> 4;
    const bool live = tid < nch;
    unsigned c[16];
    float v[16];
    unsigned prev = 0xffffffffu;                                              // class of the key before the chunk; matches nothing for chunk 0
    bool full = false;
    if (live) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const u32x4 w = *reinterpret_cast<const u32x4*>(&S.keys[16 * tid + 4 * q]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                c[4 * q + r] = w[r] >> 12;
                v[4 * q + r] = w[r] == 0xffffffffu ? 0.f : S.vals[w[r] & (LM_MAXCAND - 1)];
            }
        }
        if (tid > 0) prev = S.keys[16 * tid - 1] >> 12;
        bool still = true;
        float lead = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            still = still && c[e] == prev;
            lead += still ? v[e] : 0.f;
        }
        full = still;
        S.carry[tid] = lead;
        S.flags[tid] = (c[0] == prev ? 1 : 0) | (full ? 2 : 0);
    }
    __syncthreads();
    lm_u64 key[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) key[e] = 0;
    if (live && !full) {
        float acc = 0.f;                                                      // what the later chunks add to the run this chunk ends in, in chunk order
        for (int t2 = tid + 1; t2 < nch; ++t2) {
            const int f = S.flags[t2];
            if (!(f & 1)) break;
            acc += S.carry[t2];
            if (!(f & 2)) break;
        }
#pragma unroll
        for (int e = 15; e >= 0; --e) {                                        // a run's sum lands on its first key
            acc += v[e];
            if (c[e] != (e ? c[e - 1] : prev)) {
                key[e] = (c[e] != LM_NO_CLASS && acc > 0.f) ? lm_key(acc, c[e]) : 0;
                acc = 0.f;
            }
        }
    }
    lm_select<4, 16>(key, A.K, tid, idx_row, val_row, dropped, S.red, S.redf);
}

__global__ void __launch_bounds__(LM_THREADS)
k_label_map_crop(ap_label_map_crop_args A, int tok_blocks) {
    __shared__ LmShared S;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int PP = A.P * A.P, slots = 2 + PP;
    int b, first, nb;                                                          // the workgroup's bins: first .. first + nb - 1 of image b
    if ((int)blockIdx.x < A.B) { b = blockIdx.x; first = 0; nb = 1; }
    else {
        const int r = (int)blockIdx.x - A.B;
        b = r / tok_blocks;
        const int tb = r - b * tok_blocks;
        first = 1 + tb * LM_TOK_PER_BLOCK;
        nb = min(LM_TOK_PER_BLOCK, PP - tb * LM_TOK_PER_BLOCK);
    }
    const float* rec = A.boxes + (int64_t)b * 8;
    const int64_t row0 = (int64_t)b * slots;
    if (first == 0 && tid < A.K) {                                             // slot 0: the ground truth
        A.idx[row0 * A.K + tid] = tid == 0 ? (int)A.labels[b] : -1;
        A.val[row0 * A.K + tid] = tid == 0 ? 1.f : 0.f;
    }
    bool big = false;
    if (wave < nb) {
        const LmBin G = lm_bin(A, rec, first + wave);
        if (G.nx <= LM_WAVE_SIDE && G.ny <= LM_WAVE_SIDE && G.nx * G.ny * A.Kin <= LM_WAVE_CAND)
            lm_bin_wave(A, b, G, lane, A.idx + (row0 + G.slot) * A.K, A.val + (row0 + G.slot) * A.K,
                        A.dropped ? A.dropped + (int64_t)b * (1 + PP) + G.slot - 1 : nullptr);
        else big = true;
    }
    if (lane == 0 && wave < LM_TOK_PER_BLOCK) S.big[wave] = big;
    __syncthreads();
    for (int w = 0; w < nb; ++w) {
        if (!S.big[w]) continue;                                               // (uniform over the workgroup)
        const LmBin G = lm_bin(A, rec, first + w);
        lm_bin_block(A, b, G, tid, A.idx + (row0 + G.slot) * A.K, A.val + (row0 + G.slot) * A.K,
                     A.dropped ? A.dropped + (int64_t)b * (1 + PP) + G.slot - 1 : nullptr, S);
    }
}

extern "C" int ap_label_map_crop(const ap_label_map_crop_args* args, ap_stream_t stream) {
    if (!args) return AP_ERR_NULL;
    const ap_label_map_crop_args& a = *args;
    if (a.B < 0 || a.K < 1 || a.K > 8 || a.Kin < 1 || a.Kin > 8 || a.P < 1 || (int64_t)a.P * a.P > 0x40000000 || a.Hm < 1 || a.Wm < 1 || a.C < 1 || a.C > 65536) return AP_ERR_SHAPE;
    if ((a.score_dtype != AP_LM_F16 && a.score_dtype != AP_LM_F32) || (a.class_dtype != AP_LM_CLASS_FLOAT && a.class_dtype != AP_LM_CLASS_I32))
        return AP_ERR_SHAPE;
    if ((int64_t)a.Hm * a.Wm * a.Kin > LM_MAXCAND) return AP_ERR_UNSUPPORTED;
    if (a.B == 0) return AP_OK;
    if (!a.scores || !a.classes || !a.labels || !a.boxes || !a.idx || !a.val) return AP_ERR_NULL;
    if (a.boxes_host) {
        for (int64_t i = 0; i < a.B; ++i) {
            const float* q = a.boxes_host + i * 8;
            for (int w = 0; w < 8; ++w) if (!(q[w] - q[w] == 0.f)) return AP_ERR_SHAPE;           // inf or NaN
            if (q[2] < q[0] || q[3] < q[1] || (q[4] != 0.f && q[4] != 1.f)) return AP_ERR_SHAPE;
        }
    }
    const int64_t tok_blocks = ((int64_t)a.P * a.P + LM_TOK_PER_BLOCK - 1) / LM_TOK_PER_BLOCK;
    const int64_t blocks = (int64_t)a.B * (1 + tok_blocks);
    if (blocks > 0x7fffffff) return AP_ERR_SHAPE;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_label_map_crop, dim3((unsigned)blocks), dim3(LM_THREADS), 0, (hipStream_t)stream, a, (int)tok_blocks);
    return ap_check_launch();
}
