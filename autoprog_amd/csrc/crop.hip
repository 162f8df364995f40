// ap_crop_resize_u8: per-image crop box + horizontal flip + bilinear resize of a uint8 batch in ONE launch (include/autoprog_hip.h).
// The reference realises its per-stage crop scale (`resize`, prog/progressive.py) by rebuilding its loader, worker processes included, at
// every stage change and inside every search: main_prog.py:651-653, 1513-1515 `create_stage_loader(args, current_r, current_aa,
// current_re, current_resize)`, the rebuilds at :711-712, :840-846.  Here the loader hands over one fixed-size decoded uint8 canvas per
// image, the boxes are drawn on the host (data.DeviceRandomResizedCrop) and this kernel lands each box at the stage's resolution: one
// resample where the reference does two (RandomResizedCrop to 224 on the CPU, F.interpolate to r on the GPU, main_prog.py:973-974).
// No antialiasing when a box is scaled down: that is what the reference's own 224 -> r F.interpolate does.
//
// A workgroup owns `tr` output rows of one image.  The source rows they read are staged in LDS as the bytes they are, with 16-byte loads,
// row by row and only over the box's column span, each row from its own 16-byte-aligned start (u8_box.h, shared with resample.hip).  A
// lane then produces four consecutive output pixels of a row in all three channels, the coordinates computed once: three dwords, one per
// channel plane (NCHW) or side by side (NHWC); byte stores where the address is not 4-byte aligned (odd S, an output view) and at a
// row's tail.  The record is clamped into the image first, so every source coordinate lies in [0, Hi-1] x [0, Wi-1] whatever the record
// says.
//
// Built with -ffp-contract=off (csrc/Makefile): every operation of the header's arithmetic is rounded on its own, which is the float32
// restatement of tests/_crop_ref.py operation for operation.
#include "u8_box.h"

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
    const BoxRecord R = box_record(A.records + (int64_t)b * 8, Hi, Wi);
    const int h = R.h, w = R.w, top = R.top, left = R.left, flip = R.flip;
    const float sh = (float)h / (float)S, sw = (float)w / (float)S;

    // ---- the tile's output rows and the box rows they read
    const int oy_first = tile * G.tr;
    const int oy_last = min(oy_first + G.tr, S) - 1;
    const int y_lo = min((int)crop_src(oy_first, sh), h - 1);
    const int y_hl = min((int)crop_src(oy_last, sh), h - 1);
    const int y_hi = min(y_hl + 1, h - 1);
    const int nrows = min(y_hi - y_lo + 1, G.maxrows);           // (== y_hi - y_lo + 1: maxrows bounds it for every box, crop_geometry)

    // ---- stage rows y_lo .. y_lo + nrows - 1 of the box
    box_stage<NHWC, CROP_THREADS, CROP_BATCH>(stage, A.u8, A.B, Hi, Wi, b, top + y_lo, left, w, nrows, G.maxrows, G.pitch, G.nseg, G.ps);
    __syncthreads();

    // ---- four consecutive output pixels of one row, all three channels, per lane and trip: the coordinates are computed once
    const int Q = (S + 3) >> 2;
    const int rows = oy_last - oy_first + 1;
    const int items = rows * Q;
    const BoxStart M = box_start<NHWC>(Hi, Wi, b, top + y_lo, left, G.ps);
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
            o0[c] = box_pixel<NHWC>(M, G.maxrows, G.pitch, c, r0, 0);
            o1[c] = box_pixel<NHWC>(M, G.maxrows, G.pitch, c, r1, 0);
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
            // (written out, not box_store4 of u8_box.h: through the helper the compiler tests `j < nvalid` once for the three channels and
            // issues four of the pixel loop's LDS reads later -- measured 0.1 - 0.4 us per launch slower, profiles/loader_core_refactor.txt)
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
    const int64_t pitch = box_row_geometry(a->layout, a->Wi, &g->nseg, &g->ps);
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
    bool empty;
    if (const int rc = box_check(args, false, &empty); rc != AP_OK || empty) return rc;
    const ap_crop_resize_args& a = *args;
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
