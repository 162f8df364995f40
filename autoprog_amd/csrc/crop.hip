// ap_crop_resize_u8: per-image crop box + horizontal flip + bilinear resize of a uint8 batch in ONE launch (include/autoprog_hip.h).
// The reference realises its per-stage crop scale (`resize`, prog/progressive.py) by rebuilding its loader, worker processes included, at
// every stage change and inside every search: main_prog.py:651-653, 1513-1515 `create_stage_loader(args, current_r, current_aa,
// current_re, current_resize)`, the rebuilds at :711-712, :840-846.  Here the loader hands over one fixed-size decoded uint8 canvas per
// image, the boxes are drawn on the host (data.DeviceRandomResizedCrop) and this kernel lands each box at the stage's resolution: one
// resample where the reference does two (RandomResizedCrop to 224 on the CPU, F.interpolate to r on the GPU, main_prog.py:973-974).
// No antialiasing when a box is scaled down: that is what the reference's own 224 -> r F.interpolate does.
//
// A workgroup owns `tr` output rows of one image.  The source rows they read are staged in LDS as the bytes they are, with 16-byte loads,
// row by row and only over the box's column span, each row from its own 16-byte-aligned start.  A lane then produces four consecutive
// output pixels of a row in all three channels, the coordinates computed once: three dwords, one per channel plane (NCHW) or side by side
// (NHWC); byte stores where the address is not 4-byte aligned (odd S, an output view) and at a row's tail.  The record is clamped into
// the image first, so every source coordinate lies in [0, Hi-1] x [0, Wi-1] whatever the record says.
//
// Built with -ffp-contract=off (csrc/Makefile): every operation of the header's arithmetic is rounded on its own, which is the float32
// restatement of tests/_crop_ref.py operation for operation.
#include "common.h"

#if defined(__FAST_MATH__)
#error "crop.hip must be built with -ffp-contract=off and without fast-math (csrc/Makefile)"
#endif

#define CROP_THREADS 256
#define CROP_LDS_LIMIT (60 * 1024)
#define CROP_BATCH 4                // 16-byte loads a thread has in flight while staging

struct CropGeom {
    int tr;             // output rows per tile
    int tiles;          // tiles per image
    int maxrows;        // most source rows any tile of any box needs
    int pitch;          // LDS bytes of one staged row (a multiple of 16)
    int nseg;           // staged planes per image: 3 (NCHW) or 1 (NHWC)
    int ps;             // bytes between two pixels of a source row: 1 (NCHW) or 3 (NHWC)
};

// source coordinate of output index o inside a box of extent / S = scale (align_corners = False), every operation rounded
__host__ __device__ __forceinline__ float crop_src(int o, float scale) { return fmaxf(((float)o + 0.5f) * scale - 0.5f, 0.f); }

template <int NHWC>
__global__ void __launch_bounds__(CROP_THREADS)
k_crop_resize_u8(ap_crop_resize_args A, CropGeom G) {
    extern __shared__ __attribute__((aligned(16))) unsigned char stage[];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / G.tiles, tile = blockIdx.x % G.tiles;
    const int Hi = A.Hi, Wi = A.Wi, S = A.S;

    // ---- the record, clamped into the image: nothing below can leave it
    const int* rec = A.records + (int64_t)b * 8;
    const int h = min(max(rec[2], 1), Hi), w = min(max(rec[3], 1), Wi);
    const int top = min(max(rec[0], 0), Hi - h), left = min(max(rec[1], 0), Wi - w);
    const int flip = rec[4] & 1;
    const float sh = (float)h / (float)S, sw = (float)w / (float)S;

    // ---- the tile's output rows and the box rows they read
    const int oy_first = tile * G.tr;
    const int oy_last = min(oy_first + G.tr, S) - 1;
    const int y_lo = min((int)crop_src(oy_first, sh), h - 1);
    const int y_hl = min((int)crop_src(oy_last, sh), h - 1);
    const int y_hi = min(y_hl + 1, h - 1);
    const int nrows = min(y_hi - y_lo + 1, G.maxrows);           // (== y_hi - y_lo + 1: maxrows bounds it for every box, crop_geometry)

    // ---- stage rows y_lo .. y_lo + nrows - 1 of the box, columns left .. left + w - 1, per plane: chunk k of a row is the 16 bytes at
    // (the row's first byte & ~15) + 16 k.  CROP_BATCH loads are issued before the first one is stored; indices past the end repeat the
    // last chunk (loaded, not stored)
    const int64_t total = (int64_t)A.B * 3 * Hi * Wi;
    const int rowbytes = Wi * G.ps;
    const int cpr = min((w * G.ps + 30) >> 4, G.pitch >> 4);      // chunks per row: covers any misalignment of the row's start
    const int nchunk = G.nseg * nrows * cpr;
    const int64_t img0 = (int64_t)b * 3 * Hi * Wi;
    for (int base = tid; base < nchunk; base += CROP_BATCH * CROP_THREADS) {
        u32x4 v[CROP_BATCH];
        int64_t g[CROP_BATCH];
        int dst[CROP_BATCH];
#pragma unroll
        for (int j = 0; j < CROP_BATCH; ++j) {
            const int idx = min(base + j * CROP_THREADS, nchunk - 1);
            const int row = idx / cpr, k = idx - row * cpr;
            const int s = row / nrows, r = row - s * nrows;
            const int64_t g0 = img0 + ((int64_t)(NHWC ? 0 : s) * Hi + (top + y_lo + r)) * rowbytes + left * G.ps;
            g[j] = (g0 & ~(int64_t)15) + ((int64_t)k << 4);
            dst[j] = (s * G.maxrows + r) * G.pitch + (k << 4);
            v[j] = u32x4{0u, 0u, 0u, 0u};
            if (total >= 16) v[j] = ld16(A.u8 + (g[j] + 16 <= total ? g[j] : 0));      // (uniform: a batch below 16 bytes goes byte by byte)
        }
#pragma unroll
        for (int j = 0; j < CROP_BATCH; ++j) {
            if (base + j * CROP_THREADS >= nchunk) break;
            if (g[j] + 16 > total) {                                // the last chunk of the batch: byte by byte, nothing read past the end
                unsigned q[4] = {0u, 0u, 0u, 0u};
                for (int e = 0; e < 16; ++e) if (g[j] + e < total) q[e >> 2] |= (unsigned)A.u8[g[j] + e] << ((e & 3) * 8);
                v[j][0] = q[0]; v[j][1] = q[1]; v[j][2] = q[2]; v[j][3] = q[3];
            }
            st16(stage + dst[j], v[j]);
        }
    }
    __syncthreads();

    // ---- four consecutive output pixels of one row, all three channels, per lane and trip: the coordinates are computed once
    const int Q = (S + 3) >> 2;
    const int rows = oy_last - oy_first + 1;
    const int items = rows * Q;
    // where staged row r of plane s begins: its slot + ((first byte of plane s, row y_lo) + r rowbytes) & 15
    const int mis_img = (int)((img0 + (int64_t)(top + y_lo) * rowbytes + left * G.ps) & 15);
    const int mis_plane = NHWC ? 0 : (int)(((int64_t)Hi * rowbytes) & 15);
    const int64_t plane_out = NHWC ? 1 : (int64_t)S * S;                        // bytes between two channels of an output pixel
    for (int it = tid; it < items; it += CROP_THREADS) {
        const int ry = it / Q, q = it - ry * Q;
        const int oy = oy_first + ry;
        const float fy = crop_src(oy, sh);
        const int y0 = min((int)fy, h - 1), y1 = min(y0 + 1, h - 1);
        const float ly = fy - (float)y0, dy = 1.f - ly;
        const int r0 = min(max(y0 - y_lo, 0), nrows - 1), r1 = min(max(y1 - y_lo, 0), nrows - 1);
        int o0[3], o1[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (NHWC) {
                o0[c] = r0 * G.pitch + ((mis_img + r0 * rowbytes) & 15) + c;
                o1[c] = r1 * G.pitch + ((mis_img + r1 * rowbytes) & 15) + c;
            } else {
                o0[c] = (c * G.maxrows + r0) * G.pitch + ((mis_img + c * mis_plane + r0 * rowbytes) & 15);
                o1[c] = (c * G.maxrows + r1) * G.pitch + ((mis_img + c * mis_plane + r1 * rowbytes) & 15);
            }
        }
        // the lane's 12 output bytes as three dwords in the order they are stored: channel c's four pixels (NCHW: byte 4 c + j) or the four
        // pixels' channels side by side (NHWC: byte 3 j + c)
        unsigned word[3] = {0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ox = min(q * 4 + j, S - 1);
            const float fx = crop_src(flip ? S - 1 - ox : ox, sw);
            const int x0 = min((int)fx, w - 1), x1 = min(x0 + 1, w - 1);
            const float lx = fx - (float)x0, dx = 1.f - lx;
            const int a0 = x0 * G.ps, a1 = x1 * G.ps;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float p00 = (float)stage[o0[c] + a0], p01 = (float)stage[o0[c] + a1];
                const float p10 = (float)stage[o1[c] + a0], p11 = (float)stage[o1[c] + a1];
                const float v = dy * (dx * p00 + lx * p01) + ly * (dx * p10 + lx * p11);
                const int k = NHWC ? 3 * j + c : 4 * c + j;
                word[k >> 2] |= (unsigned)fminf(fmaxf(__builtin_rintf(v), 0.f), 255.f) << (8 * (k & 3));     // v_rndne_f32: half to even
            }
        }
        const int nvalid = min(4, S - q * 4);
        if (NHWC) {
            unsigned char* dstp = A.out + (((int64_t)b * S + oy) * S + q * 4) * 3;
            if (nvalid == 4 && !(reinterpret_cast<uintptr_t>(dstp) & 3)) {
                unsigned* d32 = reinterpret_cast<unsigned*>(dstp);
                d32[0] = word[0]; d32[1] = word[1]; d32[2] = word[2];
            } else {
#pragma unroll
                for (int k = 0; k < 12; ++k) if (k < 3 * nvalid) dstp[k] = (unsigned char)(word[k >> 2] >> (8 * (k & 3)));
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                unsigned char* dstp = A.out + ((((int64_t)b * 3 + c) * S + oy) * S + q * 4);
                if (nvalid == 4 && !(reinterpret_cast<uintptr_t>(dstp) & 3)) *reinterpret_cast<unsigned*>(dstp) = word[c];
                else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (j < nvalid) dstp[j] = (unsigned char)(word[c] >> (8 * j));
                }
            }
        }
    }
}

// tile height and LDS budget from Hi, Wi, S and the layout alone: the worst box is the whole image.  Output rows o .. o + tr - 1 of a box of
// height h read box rows floor(f(o)) .. floor(f(o + tr - 1)) + 1 with f(o + tr - 1) - f(o) = (tr - 1) h / S, and floor(a) - floor(b) <
// a - b + 1: at most ceil((tr - 1) h / S) + 2 rows, largest at h = Hi; one more row covers the rounding of the float expression.
static int crop_geometry(const ap_crop_resize_args* a, CropGeom* g) {
    g->nseg = a->layout == AP_PREP_NCHW ? 3 : 1;
    g->ps = a->layout == AP_PREP_NCHW ? 1 : 3;
    const int64_t pitch = ((int64_t)a->Wi * g->ps + 15 + 15) / 16 * 16;
    for (int tr = 16; tr >= 1; tr >>= 1) {
        int64_t maxrows = ((int64_t)(tr - 1) * a->Hi + a->S - 1) / a->S + 3;
        if (maxrows > a->Hi) maxrows = a->Hi;
        const int64_t lds = pitch * maxrows * g->nseg;
        if (lds <= CROP_LDS_LIMIT) {
            g->tr = tr; g->tiles = (a->S + tr - 1) / tr; g->maxrows = (int)maxrows; g->pitch = (int)pitch;
            return (int)lds;
        }
    }
    return -1;
}

extern "C" int ap_crop_resize_u8(const ap_crop_resize_args* args, ap_stream_t stream) {
    if (!args) return AP_ERR_NULL;
    const ap_crop_resize_args& a = *args;
    if (a.B < 0 || a.Hi <= 0 || a.Wi <= 0 || a.S <= 0) return AP_ERR_SHAPE;
    if (a.layout != AP_PREP_NCHW && a.layout != AP_PREP_NHWC) return AP_ERR_SHAPE;
    if (a.B == 0) return AP_OK;
    if (!a.u8 || !a.out || !a.records) return AP_ERR_NULL;
    if (reinterpret_cast<uintptr_t>(a.u8) & 15) return AP_ERR_SHAPE;
    if ((int64_t)a.B * 3 * a.Hi * a.Wi > ((int64_t)1 << 40)) return AP_ERR_SHAPE;
    if (a.records_host) {
        for (int64_t i = 0; i < a.B; ++i) {
            const int* q = a.records_host + i * 8;
            if (q[2] < 1 || q[3] < 1 || q[0] < 0 || q[1] < 0 || (int64_t)q[0] + q[2] > a.Hi || (int64_t)q[1] + q[3] > a.Wi) return AP_ERR_SHAPE;
            if (q[4] != 0 && q[4] != 1) return AP_ERR_SHAPE;
        }
    }
    CropGeom g;
    const int lds = crop_geometry(&a, &g);
    if (lds < 0) return AP_ERR_UNSUPPORTED;                       // one output row's source rows do not fit the LDS budget
    const int64_t blocks = (int64_t)a.B * g.tiles;
    if (blocks > 0x7fffffff) return AP_ERR_SHAPE;
    (void)hipGetLastError();
    if (a.layout == AP_PREP_NCHW)
        hipLaunchKernelGGL(k_crop_resize_u8<0>, dim3((unsigned)blocks), dim3(CROP_THREADS), lds, (hipStream_t)stream, a, g);
    else
        hipLaunchKernelGGL(k_crop_resize_u8<1>, dim3((unsigned)blocks), dim3(CROP_THREADS), lds, (hipStream_t)stream, a, g);
    return ap_check_launch();
}
