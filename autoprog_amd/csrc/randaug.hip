// ap_randaug_u8: timm's RandAugment ops on a uint8 batch, byte for byte what Pillow makes of an RGB image (include/autoprog_hip.h states
// every pixel rule).  The step of the reference's loader between the random-resized crop (csrc/resample.hip) and the preparation
// (csrc/input_prep.hip): timm's rand_augment_transform, which the reference re-creates with its loader and worker processes at every stage
// change and inside every search to move the magnitude (main_prog.py:651-656, 1443-1518).
//
// Every image carries n_layers records, applied in order: ONE LAUNCH PER LAYER, each reading the bytes the launch before it wrote (the
// kernel boundary makes them visible), ping-pong between `scratch` and `out` so that the last layer lands in `out`.  A launch is a grid of
// (row bands, B) workgroups of RA_THREADS lanes; a workgroup reads its image's record (uniform: no divergence inside a workgroup) and
//   LUT ops    builds one 256-entry table per channel in LDS and maps its band through it, a dword at a time where the addresses allow.
//              AutoContrast, Equalize and Contrast need statistics of the WHOLE image: every band of such an image first walks all of it
//              (<= 150 KB at S = 224, L2-resident) into LDS histograms with LDS atomics -- integer counts, so every band builds the same table;
//   Color      one lane per pixel: the grey value, then the blend per channel;
//   Sharpness  one lane per pixel and channel: Pillow's 3 x 3 SMOOTH in float32, border pixels copied, then the blend;
//   Affine     one lane per pixel, a wave on 8 x 8 pixels: the source position in float64, Pillow's bilinear / bicubic sample of the three
//              channels, the fill colour outside.  A bicubic sample is 48 byte loads and ~250 fp64 operations per pixel: this is the op
//              that sets the launch's time.
// An unknown op code copies, a filter code other than AP_RESAMPLE_BICUBIC is bilinear, every source index is clamped into the image and
// the position test refuses NaN: whatever a record says, nothing is read or written out of bounds.
//
// Built with -ffp-contract=off and without fast-math (csrc/Makefile): no fused multiply-add in the float32 blends or the float64 samples.
#include "common.h"

#if defined(__FAST_MATH__)
#error "randaug.hip must be built with -ffp-contract=off and without fast-math (csrc/Makefile)"
#endif

#ifndef RA_THREADS
#define RA_THREADS 256
#endif
// bands: at least RA_MIN_ROWS rows each, and about RA_WG_PER_CU workgroups per compute unit over the batch.  By measurement
// (profiles/device_randaug_bands.txt; -DRA_WG_PER_CU / -DRA_MIN_ROWS for an ablation build): at B = 128 bands of 16 rows are the fastest,
// or level with the fastest, for the natural op mix and for the all-bicubic batch at S = 224 (14 bands) and at S = 128 (8 bands).  More
// bands cost the ops that need whole-image statistics (every band walks the image), fewer leave compute units idle under the affine ops
#ifndef RA_WG_PER_CU
#define RA_WG_PER_CU 8
#endif
#ifndef RA_MIN_ROWS
#define RA_MIN_ROWS 16
#endif
#define RA_BATCH 4                  // 16-byte loads a lane has in flight while it counts an image
#define RA_MAX_S 16384              // 3 S S stays below 2^31: offsets inside one image are formed in int

static_assert(RA_THREADS % 64 == 0, "a wave takes whole 8 x 8 tiles");

typedef unsigned char u8_t;

// byte offset of (channel c, row y, column x) inside one image
template <int NHWC>
__device__ __forceinline__ int ra_at(int S, int c, int y, int x) { return NHWC ? (y * S + x) * 3 + c : (c * S + y) * S + x; }

// Pillow's Image.blend on uint8: float32, the difference in int, every operation rounded on its own
__device__ __forceinline__ int ra_blend(int d, int i, float f) {
    const float t = (float)d + f * (float)(i - d);
    if (f >= 0.0f && f <= 1.0f) return (int)t;
    return !(t > 0.0f) ? 0 : (t >= 255.0f ? 255 : (int)t);
}

__device__ __forceinline__ int ra_grey(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// counts of the bytes of src[0 .. len) into h[channel * 256 + value]; channel = cfix, or (byte index) % 3 where cfix < 0.  16-byte loads,
// RA_BATCH of them in flight per lane before the first count: a lane that waited for each dword in turn spent its time on load latency
__device__ __forceinline__ void ra_hist(const u8_t* src, int len, int cfix, unsigned* h, int tid) {
    const int head = min(len, (int)((16 - (reinterpret_cast<uintptr_t>(src) & 15)) & 15));
    for (int i = tid; i < head; i += RA_THREADS) atomicAdd(&h[(cfix >= 0 ? cfix : i % 3) * 256 + src[i]], 1u);
    const int nq = (len - head) >> 4;
    for (int k0 = tid; k0 < nq; k0 += RA_BATCH * RA_THREADS) {
        u32x4 v[RA_BATCH];
#pragma unroll
        for (int j = 0; j < RA_BATCH; ++j) v[j] = ld16(src + head + 16 * min(k0 + j * RA_THREADS, nq - 1));
#pragma unroll
        for (int j = 0; j < RA_BATCH; ++j) {
            if (k0 + j * RA_THREADS >= nq) break;
            const int i = head + 16 * (k0 + j * RA_THREADS);
            int c = cfix >= 0 ? cfix : i % 3;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                atomicAdd(&h[c * 256 + ((v[j][e >> 2] >> (8 * (e & 3))) & 255u)], 1u);
                if (cfix < 0) c = c == 2 ? 0 : c + 1;
            }
        }
    }
    for (int i = head + 16 * nq + tid; i < len; i += RA_THREADS) atomicAdd(&h[(cfix >= 0 ? cfix : i % 3) * 256 + src[i]], 1u);
}

// dst[i] = lut[channel][src[i]] over len bytes: dwords where src and dst share their alignment, bytes before, after and otherwise
__device__ __forceinline__ void ra_map(const u8_t* src, u8_t* dst, int len, int cfix, const u8_t* lut, int tid) {
    int head = min(len, (int)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3));
    if ((reinterpret_cast<uintptr_t>(src) & 3) != (reinterpret_cast<uintptr_t>(dst) & 3)) head = len;
    for (int i = tid; i < head; i += RA_THREADS) dst[i] = lut[(cfix >= 0 ? cfix : i % 3) * 256 + src[i]];
    const int nd = (len - head) >> 2;
    for (int k = tid; k < nd; k += RA_THREADS) {
        const int i = head + 4 * k;
        const unsigned w = *reinterpret_cast<const unsigned*>(src + i);
        int c = cfix >= 0 ? cfix : i % 3;
        unsigned o = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o |= (unsigned)lut[c * 256 + ((w >> (8 * j)) & 255u)] << (8 * j);
            if (cfix < 0) c = c == 2 ? 0 : c + 1;
        }
        *reinterpret_cast<unsigned*>(dst + i) = o;
    }
    for (int i = head + 4 * nd + tid; i < len; i += RA_THREADS) dst[i] = lut[(cfix >= 0 ? cfix : i % 3) * 256 + src[i]];
}

__device__ __forceinline__ double ra_cub(double v1, double v2, double v3, double v4, double d) {
    const double p2 = -v1 + v3, p3 = 2.0 * (v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4;
    return v2 + d * (p2 + d * (p3 + d * p4));
}

template <int NHWC>
__global__ void __launch_bounds__(RA_THREADS)
k_randaug_u8(const u8_t* __restrict__ src_all, u8_t* __restrict__ dst_all, const int* __restrict__ records, int n_layers, int layer, int S, int tr,
             int fill_r, int fill_g, int fill_b) {
    __shared__ unsigned hist[3 * 256];
    __shared__ __attribute__((aligned(4))) u8_t lut[3 * 256];
    __shared__ int stat[8];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int y0 = blockIdx.x * tr;
    const int rows = min(y0 + tr, S) - y0;
    if (rows <= 0) return;
    const int64_t img = (int64_t)b * 3 * S * S;
    const u8_t* src = src_all + img;
    u8_t* dst = dst_all + img;
    const int* rec = records + ((int64_t)b * n_layers + layer) * AP_RANDAUG_RECORD_WORDS;
    int op = rec[0];
    const int bicubic = rec[1] == AP_RESAMPLE_BICUBIC;
    const int iarg = rec[2];
    const float farg = __int_as_float(rec[3]);
    if (op < AP_RA_NONE || op > AP_RA_AFFINE) op = AP_RA_NONE;
    const int plane = S * S;

    // ------------------------------------------------------------------------------------------------ ops that are one table per channel
    if (op <= AP_RA_CONTRAST) {
        if (op == AP_RA_AUTOCONTRAST || op == AP_RA_EQUALIZE || op == AP_RA_CONTRAST) {
            for (int i = tid; i < 3 * 256; i += RA_THREADS) hist[i] = 0u;
            __syncthreads();
            if (op == AP_RA_CONTRAST) {                              // the histogram of the grey value, in channel 0's bins
                for (int p0 = tid; p0 < plane; p0 += RA_BATCH * RA_THREADS) {
                    int L[RA_BATCH];
#pragma unroll
                    for (int j = 0; j < RA_BATCH; ++j) {             // (the loads of RA_BATCH pixels before the first count)
                        const int p = min(p0 + j * RA_THREADS, plane - 1);
                        const int y = p / S, x = p - y * S;
                        L[j] = ra_grey(src[ra_at<NHWC>(S, 0, y, x)], src[ra_at<NHWC>(S, 1, y, x)], src[ra_at<NHWC>(S, 2, y, x)]);
                    }
#pragma unroll
                    for (int j = 0; j < RA_BATCH; ++j) if (p0 + j * RA_THREADS < plane) atomicAdd(&hist[L[j]], 1u);
                }
            } else if (NHWC) ra_hist(src, 3 * plane, -1, hist, tid);
            else for (int c = 0; c < 3; ++c) ra_hist(src + c * plane, plane, c, hist, tid);
            __syncthreads();
            // per channel (Contrast: once), one lane: integer statistics of the counts
            if (tid < 3) {
                const unsigned* h = hist + tid * 256;
                if (op == AP_RA_CONTRAST) {
                    if (tid == 0) {
                        int64_t sum = 0;
                        for (int i = 0; i < 256; ++i) sum += (int64_t)i * h[i];
                        stat[0] = (int)((double)sum / (double)plane + 0.5);
                    }
                } else {
                    int lo = 256, hi = -1, nonempty = 0;
                    for (int i = 0; i < 256; ++i) if (h[i]) { if (lo > i) lo = i; hi = i; ++nonempty; }
                    stat[2 * tid] = lo; stat[2 * tid + 1] = hi;
                    if (op == AP_RA_EQUALIZE) {                      // the table needs a running sum: this lane writes all of it
                        const int step = nonempty <= 1 ? 0 : (int)(((unsigned)plane - h[hi]) / 255u);
                        int64_t n = step / 2;
                        for (int i = 0; i < 256; ++i) {
                            lut[tid * 256 + i] = (u8_t)(step == 0 ? i : (int)min((int64_t)255, n / step));
                            n += h[i];
                        }
                    }
                }
            }
            __syncthreads();
        }
        if (op != AP_RA_EQUALIZE) {
            for (int e = tid; e < 3 * 256; e += RA_THREADS) {
                const int c = e >> 8, i = e & 255;
                int v = i;
                switch (op) {
                case AP_RA_INVERT: v = 255 - i; break;
                case AP_RA_SOLARIZE: v = i < iarg ? i : 255 - i; break;
                case AP_RA_SOLARIZE_ADD: v = i < 128 ? min(255, i + max(iarg, 0)) : i; break;
                case AP_RA_POSTERIZE: v = i & ~((1 << (8 - min(max(iarg, 0), 8))) - 1); break;
                case AP_RA_BRIGHTNESS: v = ra_blend(0, i, farg); break;
                case AP_RA_CONTRAST: v = ra_blend(stat[0], i, farg); break;
                case AP_RA_AUTOCONTRAST: {
                    const int lo = stat[2 * c], hi = stat[2 * c + 1];
                    if (hi > lo) {
                        const double scale = 255.0 / (double)(hi - lo);
                        const double offset = -(double)lo * scale;
                        const double t = (double)i * scale + offset;     // |t| <= 255 * 255: the conversion is in range
                        v = min(max((int)t, 0), 255);
                    }
                } break;
                default: break;
                }
                lut[e] = (u8_t)v;
            }
            __syncthreads();
        }
        if (NHWC) ra_map(src + y0 * S * 3, dst + y0 * S * 3, rows * S * 3, -1, lut, tid);
        else for (int c = 0; c < 3; ++c) ra_map(src + c * plane + y0 * S, dst + c * plane + y0 * S, rows * S, c, lut, tid);
        return;
    }

    // ------------------------------------------------------------------------------------------------ Color: blend with the pixel's grey
    if (op == AP_RA_COLOR) {
        for (int p = tid; p < rows * S; p += RA_THREADS) {
            const int y = y0 + p / S, x = p % S;
            const int o0 = ra_at<NHWC>(S, 0, y, x), o1 = ra_at<NHWC>(S, 1, y, x), o2 = ra_at<NHWC>(S, 2, y, x);
            const int r = src[o0], g = src[o1], bl = src[o2];
            const int L = ra_grey(r, g, bl);
            dst[o0] = (u8_t)ra_blend(L, r, farg); dst[o1] = (u8_t)ra_blend(L, g, farg); dst[o2] = (u8_t)ra_blend(L, bl, farg);
        }
        return;
    }

    // ------------------------------------------------------------------------------------------------ Sharpness: blend with SMOOTH
    if (op == AP_RA_SHARPNESS) {
        const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
        const int dx = NHWC ? 3 : 1;
        for (int e = tid; e < rows * S * 3; e += RA_THREADS) {
            int c, y, x;                                            // consecutive lanes on consecutive bytes of the layout
            if (NHWC) { c = e % 3; const int p = e / 3; y = y0 + p / S; x = p % S; }
            else { c = e / (rows * S); const int p = e - c * rows * S; y = y0 + p / S; x = p % S; }
            const int o = ra_at<NHWC>(S, c, y, x);
            const int v = src[o];
            int sm = v;
            if (x > 0 && x < S - 1 && y > 0 && y < S - 1) {
                const u8_t* up = src + ra_at<NHWC>(S, c, y - 1, x);
                const u8_t* mid = src + o;
                const u8_t* down = src + ra_at<NHWC>(S, c, y + 1, x);
                float ss = 0.5f;
                ss += ((float)down[-dx] * k1 + (float)down[0] * k1) + (float)down[dx] * k1;
                ss += ((float)mid[-dx] * k1 + (float)mid[0] * k5) + (float)mid[dx] * k1;
                ss += ((float)up[-dx] * k1 + (float)up[0] * k1) + (float)up[dx] * k1;
                sm = !(ss > 0.0f) ? 0 : (ss >= 255.0f ? 255 : (int)ss);
            }
            dst[o] = (u8_t)ra_blend(sm, v, farg);
        }
        return;
    }

    // ------------------------------------------------------------------------------------------------ Affine, float64
    double m[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) m[i] = __hiloint2double(rec[5 + 2 * i], rec[4 + 2 * i]);
    const int fill[3] = {fill_r, fill_g, fill_b};
    const double Sd = (double)S;
    // a wave takes 8 x 8 output pixels, not 64 of one row: under a rotation its 64 source positions then lie in a compact patch, a
    // dozen cache lines per load where a row's run of 64 crosses thirty
    const int tpr = (S + 7) >> 3;
    const int ntile = tpr * ((rows + 7) >> 3);
    for (int p = tid; p < ntile * 64; p += RA_THREADS) {
        const int t = p >> 6, l = p & 63;
        const int ty = t / tpr, tx = t - ty * tpr;
        const int y = y0 + ty * 8 + (l >> 3), x = tx * 8 + (l & 7);
        if (y >= y0 + rows || x >= S) continue;
        const double xc = (double)x + 0.5, yc = (double)y + 0.5;
        double xin = m[0] * xc + m[1] * yc + m[2];
        double yin = m[3] * xc + m[4] * yc + m[5];
        int res[3] = {fill[0], fill[1], fill[2]};
        if (xin >= 0.0 && xin < Sd && yin >= 0.0 && yin < Sd) {     // (false for NaN; inside, every conversion below is in range)
            xin -= 0.5; yin -= 0.5;
            const int X = (int)floor(xin), Y = (int)floor(yin);
            const double dx = xin - (double)X, dy = yin - (double)Y;
            if (!bicubic) {
                const int x0 = min(max(X, 0), S - 1), x1 = min(max(X + 1, 0), S - 1);
                const int r0 = min(max(Y, 0), S - 1);
                const bool has1 = Y + 1 >= 0 && Y + 1 < S;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double a = (double)src[ra_at<NHWC>(S, c, r0, x0)], bb = (double)src[ra_at<NHWC>(S, c, r0, x1)];
                    const double v1 = a + (bb - a) * dx;
                    double v2 = v1;
                    if (has1) {
                        a = (double)src[ra_at<NHWC>(S, c, Y + 1, x0)]; bb = (double)src[ra_at<NHWC>(S, c, Y + 1, x1)];
                        v2 = a + (bb - a) * dx;
                    }
                    const double v = v1 + (v2 - v1) * dy;
                    res[c] = min(max((int)v, 0), 255);               // (v lies between its four samples: the clamp never acts)
                }
            } else {
                int xs[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) xs[j] = min(max(X - 1 + j, 0), S - 1);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double rv[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int yy = Y - 1 + j;
                        if (j == 0 || (yy >= 0 && yy < S)) {
                            const int r = j == 0 ? min(max(yy, 0), S - 1) : yy;
                            rv[j] = ra_cub((double)src[ra_at<NHWC>(S, c, r, xs[0])], (double)src[ra_at<NHWC>(S, c, r, xs[1])],
                                           (double)src[ra_at<NHWC>(S, c, r, xs[2])], (double)src[ra_at<NHWC>(S, c, r, xs[3])], dx);
                        } else rv[j] = rv[j - 1];
                    }
                    const double v = ra_cub(rv[0], rv[1], rv[2], rv[3], dy);
                    res[c] = !(v > 0.0) ? 0 : (v >= 255.0 ? 255 : (int)v);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[ra_at<NHWC>(S, c, y, x)] = (u8_t)res[c];
    }
}

extern "C" int ap_randaug_u8(const ap_randaug_args* args, ap_stream_t stream) {
    if (!args) return AP_ERR_NULL;
    const ap_randaug_args& a = *args;
    if (a.B < 0 || a.S <= 0 || a.S > RA_MAX_S || a.n_layers < 1 || a.n_layers > AP_RANDAUG_MAX_LAYERS) return AP_ERR_SHAPE;
    if (a.layout != AP_PREP_NCHW && a.layout != AP_PREP_NHWC) return AP_ERR_SHAPE;
    if (a.B == 0) return AP_OK;
    if (a.B > 65535) return AP_ERR_SHAPE;                           // (one image per workgroup row of the grid's y axis)
    if (!a.u8 || !a.out || !a.records || (a.n_layers > 1 && !a.scratch)) return AP_ERR_NULL;
    if (a.out == a.u8 || (a.n_layers > 1 && (a.scratch == a.u8 || a.scratch == a.out))) return AP_ERR_SHAPE;
    if (a.records_host) {
        for (int64_t i = 0; i < (int64_t)a.B * a.n_layers; ++i) {
            const int* q = a.records_host + i * AP_RANDAUG_RECORD_WORDS;
            if (q[0] < AP_RA_NONE || q[0] > AP_RA_AFFINE) return AP_ERR_SHAPE;
            if (q[0] == AP_RA_AFFINE && q[1] != AP_RESAMPLE_BILINEAR && q[1] != AP_RESAMPLE_BICUBIC) return AP_ERR_SHAPE;
        }
    }
    const int64_t want = ceil_div64((int64_t)RA_WG_PER_CU * ap_cu_count(), a.B);
    int tr = (int)ceil_div64(a.S, want < 1 ? 1 : want);
    if (tr < RA_MIN_ROWS) tr = RA_MIN_ROWS;
    tr = (tr + 7) / 8 * 8;                                          // whole 8 x 8 tiles of the affine ops
    const unsigned bands = (unsigned)ceil_div64(a.S, tr);
    (void)hipGetLastError();
    for (int layer = 0; layer < a.n_layers; ++layer) {
        // the last layer writes `out`, the one before it `scratch`, and so on backwards; the first reads the input
        const unsigned char* src = layer == 0 ? a.u8 : (((a.n_layers - layer) & 1) ? a.scratch : a.out);
        unsigned char* dst = ((a.n_layers - 1 - layer) & 1) ? a.scratch : a.out;
        if (a.layout == AP_PREP_NCHW)
            hipLaunchKernelGGL(k_randaug_u8<0>, dim3(bands, (unsigned)a.B), dim3(RA_THREADS), 0, (hipStream_t)stream, src, dst, a.records, a.n_layers,
                               layer, a.S, tr, (int)a.fill[0], (int)a.fill[1], (int)a.fill[2]);
        else
            hipLaunchKernelGGL(k_randaug_u8<1>, dim3(bands, (unsigned)a.B), dim3(RA_THREADS), 0, (hipStream_t)stream, src, dst, a.records, a.n_layers,
                               layer, a.S, tr, (int)a.fill[0], (int)a.fill[1], (int)a.fill[2]);
    }
    return ap_check_launch();
}
