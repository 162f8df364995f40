// ap_crop_resample_u8: per-image crop box + ANTIALIASED bilinear / bicubic resize + horizontal flip of a uint8 batch in ONE launch, byte
// for byte what Pillow's Image.crop(box).resize((S, S), BILINEAR | BICUBIC) gives on an RGB image (include/autoprog_hip.h states the rule).
// This is the resample of the reference's loader (timm's RandomResizedCropAndInterpolation, `--train-interpolation random`,
// main_prog.py:211, :632-658; validation: bicubic, models/volo.py:35-44), which ap_crop_resize_u8 (csrc/crop.hip) replaced by a two-tap
// sample: Pillow widens the filter's support by the reduction factor, so a 512-px canvas brought to r = 128 averages 16 x 16 (bicubic)
// source pixels per output pixel where the two-tap sample reads 2 x 2.
//
// Pillow's 8-bit resize is two separable passes in integers on 22-bit fixed-point coefficients, the horizontal pass rounded to uint8 before
// the vertical one reads it; the coefficients are float64, every operation rounded on its own.  A workgroup owns `tr` output rows of one
// image and
//   A  builds both coefficient tables in LDS: all S horizontal windows and its own rows' vertical ones, one lane per window walking its
//      taps in order in fp64 (the order of the sum that normalises them matters);
//   B  stages box rows ymin(first row) .. ymax(last row) - 1 over the box's column span in LDS with 16-byte loads (u8_box.h, shared
//      with k_crop_resize_u8);
//   C  runs the horizontal pass into an LDS intermediate of rows x 3 x S uint8 in the OUTPUT's layout, already flipped: one lane per
//      (row, output column) does the three channels with one read of each coefficient;
//   D  runs the vertical pass four bytes of an intermediate row at a time (one dword read per tap) and stores dwords, bytes where the
//      address is not 4-byte aligned and at a row's tail.
// Tiles of one image redo the horizontal pass on the rows their vertical supports share.  The record is clamped into the image and the
// filter code to {1, 2} first, every table length and row count to what the geometry reserved: whatever the record says, nothing is
// read or written out of bounds.
//
// Built with -ffp-contract=off and without fast-math (csrc/Makefile): no fused multiply-add, IEEE double division.
#include "u8_box.h"

#if defined(__FAST_MATH__)
#error "resample.hip must be built with -ffp-contract=off and without fast-math (csrc/Makefile)"
#endif

// Both by measurement (profiles/device_resample.txt; -DRS_THREADS / -DRS_LDS_LIMIT for an ablation build): 80 KB keeps two workgroups on a
// CU (160 KiB) and beats 64 KB (smaller tiles redo more horizontal rows) as well as 120 / 160 KB (one workgroup per CU); 512 threads
// at 80 KB are the fastest, or level with the fastest, on every row measured.  Past 64 KB a launch needs the per-device opt-in (common.h)
#ifndef RS_THREADS
#define RS_THREADS 512
#endif
#ifndef RS_LDS_LIMIT
#define RS_LDS_LIMIT (80 * 1024)
#endif
#define RS_BATCH 4                  // 16-byte loads a thread has in flight while staging
#define RS_MAX_TR 16

struct ResampleGeom {
    int tr;             // output rows per tile
    int tiles;          // tiles per image
    int maxrows;        // most box rows any tile of any box reads
    int pitch;          // LDS bytes of one staged row (a multiple of 16)
    int nseg;           // staged planes per image: 3 (NCHW) or 1 (NHWC)
    int ps;             // bytes between two pixels of a source row: 1 (NCHW) or 3 (NHWC)
    int ksh, ksv;       // most taps of a horizontal / vertical window (bicubic, the whole canvas)
    int Sp;             // S rounded up to a multiple of 4: an intermediate row is 3 Sp bytes
    int off_inter, off_hb, off_hk, off_vb, off_vk;      // LDS offsets (bytes, multiples of 16) behind the staged rows at 0
};

__host__ __device__ __forceinline__ double rs_filter(double x, int bicubic) {
    x = fabs(x);
    if (bicubic) {
        const double a = -0.5;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
        if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
        return 0.0;
    }
    return x < 1.0 ? 1.0 - x : 0.0;
}

// window o of an axis of extent n resampled to S: bounds[0] = first tap, bounds[1] = taps (1 .. ksize), K[0 .. taps) the coefficients
__device__ __forceinline__ void rs_window(int o, int n, int S, int bicubic, int ksize, int* bounds, int* K) {
    const double scale = (double)n / (double)S;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = (bicubic ? 2.0 : 1.0) * fs, ss = 1.0 / fs;
    const double center = ((double)o + 0.5) * scale;
    const int xmin = min(max((int)(center - support + 0.5), 0), n - 1);
    const int xmax = min((int)(center + support + 0.5), n);
    const int cnt = min(max(xmax - xmin, 1), ksize);              // (== xmax - xmin: ksize bounds it for every box, resample_geometry)
    double ww = 0.0;
    for (int i = 0; i < cnt; ++i) ww += rs_filter(((double)(i + xmin) - center + 0.5) * ss, bicubic);
    for (int i = 0; i < cnt; ++i) {
        double k = rs_filter(((double)(i + xmin) - center + 0.5) * ss, bicubic);      // (the same operations: the same value as above)
        if (ww != 0.0) k = k / ww;
        K[i] = (int)(k * 4194304.0 + (k < 0.0 ? -0.5 : 0.5));
    }
    bounds[0] = xmin; bounds[1] = cnt;
}

__device__ __forceinline__ unsigned rs_clip8(int acc) { return (unsigned)min(max(acc >> 22, 0), 255); }

template <int NHWC>
__global__ void __launch_bounds__(RS_THREADS)
k_crop_resample_u8(ap_crop_resample_args A, ResampleGeom G) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    unsigned char* stage = lds;
    unsigned char* inter = lds + G.off_inter;
    int* hb = reinterpret_cast<int*>(lds + G.off_hb);
    int* hk = reinterpret_cast<int*>(lds + G.off_hk);
    int* vb = reinterpret_cast<int*>(lds + G.off_vb);
    int* vk = reinterpret_cast<int*>(lds + G.off_vk);
    const int tid = threadIdx.x;
    const int b = blockIdx.x / G.tiles, tile = blockIdx.x % G.tiles;
    const int Hi = A.Hi, Wi = A.Wi, S = A.S;

    // ---- the record, clamped into the image, the filter into {1, 2}: nothing below can leave the image or the tables
    const int* rec = A.records + (int64_t)b * 8;
    const BoxRecord R = box_record(rec, Hi, Wi);
    const int h = R.h, w = R.w, flip = R.flip;
    const int bicubic = rec[5] == 2;

    const int oy_first = tile * G.tr;
    const int rows = min(oy_first + G.tr, S) - oy_first;

    // ---- A: the tables.  Items 0 .. S-1 are the horizontal windows, S .. S + rows - 1 this tile's vertical ones
    for (int it = tid; it < S + rows; it += RS_THREADS) {
        if (it < S) rs_window(it, w, S, bicubic, G.ksh, hb + 2 * it, hk + it * G.ksh);
        else rs_window(oy_first + it - S, h, S, bicubic, G.ksv, vb + 2 * (it - S), vk + (it - S) * G.ksv);
    }
    __syncthreads();
    const int y_lo = vb[0];                                       // (first taps and last taps both grow with the output row)
    const int nrows = min(max(vb[2 * (rows - 1)] + vb[2 * (rows - 1) + 1] - y_lo, 1), min(G.maxrows, h - y_lo));

    // ---- B: stage rows y_lo .. y_lo + nrows - 1 of the box
    box_stage<NHWC, RS_THREADS, RS_BATCH>(stage, A.u8, A.B, Hi, Wi, b, R.top + y_lo, R.left, w, nrows, G.maxrows, G.pitch, G.nseg, G.ps);
    __syncthreads();

    // ---- C: the horizontal pass, rounded to uint8.  Window o lands in column S - 1 - o of a flipped image
    const BoxStart M = box_start<NHWC>(Hi, Wi, b, R.top + y_lo, R.left, G.ps);
    const int ipitch = 3 * G.Sp;
    for (int it = tid; it < nrows * S; it += RS_THREADS) {
        const int r = it / S, o = it - r * S;
        const int xmin = hb[2 * o], cnt = hb[2 * o + 1];
        const int* K = hk + o * G.ksh;
        int src[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) src[c] = box_pixel<NHWC>(M, G.maxrows, G.pitch, c, r, xmin);
        int acc[3] = {1 << 21, 1 << 21, 1 << 21};
        for (int i = 0; i < cnt; ++i) {
            const int k = K[i];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += (int)stage[src[c] + i * G.ps] * k;
        }
        const int ox = flip ? S - 1 - o : o;
#pragma unroll
        for (int c = 0; c < 3; ++c) inter[r * ipitch + (NHWC ? ox * 3 + c : c * G.Sp + ox)] = (unsigned char)rs_clip8(acc[c]);
    }
    __syncthreads();

    // ---- D: the vertical pass on four consecutive bytes of an intermediate row: with S a multiple of 4 or not, dword d of a row is
    // channel d / (Sp / 4), columns 4 (d % (Sp / 4)) .. + 3 (NCHW) or bytes 4 d .. 4 d + 3 of the row's 3 S (NHWC)
    const int dpr = ipitch >> 2;
    for (int it = tid; it < rows * dpr; it += RS_THREADS) {
        const int ry = it / dpr, d = it - ry * dpr;
        const int r0 = vb[2 * ry] - y_lo, cnt = vb[2 * ry + 1];
        const int* K = vk + ry * G.ksv;
        int acc[4] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
        for (int i = 0; i < cnt; ++i) {
            const int r = min(max(r0 + i, 0), nrows - 1);
            const unsigned p = *reinterpret_cast<const unsigned*>(inter + r * ipitch + 4 * d);
            const int k = K[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += (int)((p >> (8 * j)) & 255u) * k;
        }
        const unsigned word = rs_clip8(acc[0]) | rs_clip8(acc[1]) << 8 | rs_clip8(acc[2]) << 16 | rs_clip8(acc[3]) << 24;
        const int oy = oy_first + ry;
        unsigned char* dstp;
        int nvalid;
        if (NHWC) {
            dstp = A.out + ((int64_t)b * S + oy) * S * 3 + 4 * d;
            nvalid = min(4, 3 * S - 4 * d);
        } else {
            const int qpr = G.Sp >> 2, c = d / qpr, q = d - c * qpr;
            dstp = A.out + ((((int64_t)b * 3 + c) * S + oy) * S + q * 4);
            nvalid = min(4, S - q * 4);
        }
        box_store4(dstp, word, nvalid);
    }
}

// most taps of a window of an axis of extent <= n brought to S under the widest filter: Pillow's ksize = ceil(support) * 2 + 1 with
// support = 2 max(n / S, 1); first tap >= center - support - 0.5 and last tap + 1 <= center + support + 0.5 keep every window below it
static int64_t rs_ksize(int n, int S) {
    const double scale = (double)n / (double)S;
    return (int64_t)ceil(2.0 * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}
static int64_t align16(int64_t v) { return (v + 15) / 16 * 16; }

// tile height and LDS bytes from Hi, Wi, S and the layout alone: the worst box is the whole image under bicubic.  Output rows o .. o + tr - 1
// of a box of height h read box rows from trunc(c(o) - support + 0.5) up to, not including, trunc(c(o + tr - 1) + support + 0.5) with
// c(o + tr - 1) - c(o) = (tr - 1) h / S: at most (tr - 1) h / S + 2 support + 1 rows, which grows with h; one more row covers the rounding
static int resample_geometry(const ap_crop_resample_args* a, ResampleGeom* g) {
    const int64_t pitch = box_row_geometry(a->layout, a->Wi, &g->nseg, &g->ps);
    const int64_t Sp = ((int64_t)a->S + 3) / 4 * 4;
    const int64_t ksh = rs_ksize(a->Wi, a->S), ksv = rs_ksize(a->Hi, a->S);
    const double scale = (double)a->Hi / (double)a->S, support = 2.0 * (scale < 1.0 ? 1.0 : scale);
    for (int tr = RS_MAX_TR; tr >= 1; --tr) {
        int64_t maxrows = (int64_t)ceil((tr - 1) * scale + 2.0 * support) + 2;
        if (maxrows > a->Hi) maxrows = a->Hi;
        const int64_t off_inter = pitch * maxrows * g->nseg;
        const int64_t off_hb = off_inter + align16(maxrows * 3 * Sp);
        const int64_t off_hk = off_hb + align16((int64_t)a->S * 8);
        const int64_t off_vb = off_hk + align16((int64_t)a->S * ksh * 4);
        const int64_t off_vk = off_vb + align16((int64_t)tr * 8);
        const int64_t lds = off_vk + align16((int64_t)tr * ksv * 4);
        if (lds <= RS_LDS_LIMIT) {
            g->tr = tr; g->tiles = (a->S + tr - 1) / tr; g->maxrows = (int)maxrows; g->pitch = (int)pitch;
            g->ksh = (int)ksh; g->ksv = (int)ksv; g->Sp = (int)Sp;
            g->off_inter = (int)off_inter; g->off_hb = (int)off_hb; g->off_hk = (int)off_hk; g->off_vb = (int)off_vb; g->off_vk = (int)off_vk;
            return (int)lds;
        }
    }
    return -1;
}

extern "C" int ap_crop_resample_u8(const ap_crop_resample_args* args, ap_stream_t stream) {
    bool empty;
    if (const int rc = box_check(args, true, &empty); rc != AP_OK || empty) return rc;
    const ap_crop_resample_args& a = *args;
    ResampleGeom g;
    const int lds = resample_geometry(&a, &g);
    if (lds < 0) return AP_ERR_UNSUPPORTED;                       // the tables and one output row's box rows do not fit the LDS budget
    const int64_t blocks = (int64_t)a.B * g.tiles;
    if (blocks > 0x7fffffff) return AP_ERR_SHAPE;
    (void)hipGetLastError();
    if (a.layout == AP_PREP_NCHW)
        AP_LAUNCH_LDS(k_crop_resample_u8<0>, dim3((unsigned)blocks), dim3(RS_THREADS), lds, (hipStream_t)stream, a, g);
    else
        AP_LAUNCH_LDS(k_crop_resample_u8<1>, dim3((unsigned)blocks), dim3(RS_THREADS), lds, (hipStream_t)stream, a, g);
    return ap_check_launch();
}
