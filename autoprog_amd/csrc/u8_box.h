// What the two box kernels of the loader share (crop.hip: k_crop_resize_u8, resample.hip: k_crop_resample_u8): the clamped record, the
// staging of a box's rows in LDS, where a staged row begins, the host's argument checks and the row geometry; and the dword-or-bytes
// store, which only the second of them calls.
// A workgroup stages rows row0 .. row0 + nrows - 1 of image b over the box's column span as the bytes they are, per plane (three for
// NCHW, one for NHWC), each row in a slot of `pitch` bytes from its own 16-byte-aligned start.  The filters, the LDS budgets and the
// tile-height searches are the kernels' own.
#pragma once
#include "common.h"

// ---- the record: top, left, h, w, flip from words 0 .. 4, clamped into Hi x Wi, so that no coordinate formed from it leaves the image
struct BoxRecord { int top, left, h, w, flip; };
__device__ __forceinline__ BoxRecord box_record(const int* rec, int Hi, int Wi) {
    BoxRecord r;
    r.h = min(max(rec[2], 1), Hi); r.w = min(max(rec[3], 1), Wi);
    r.top = min(max(rec[0], 0), Hi - r.h); r.left = min(max(rec[1], 0), Wi - r.w);
    r.flip = rec[4] & 1;
    return r;
}

// ---- stage rows row0 .. row0 + nrows - 1 of image b, columns left .. left + w - 1, per plane: chunk k of a row is the 16 bytes at (the
// row's first byte & ~15) + 16 k and lands at (s maxrows + r) pitch + 16 k.  BATCH loads are issued before the first one is stored;
// indices past the end repeat the last chunk (loaded, not stored).  Nothing is read past the last byte of the batch.  No barrier.
template <int NHWC, int THREADS, int BATCH>
__device__ __forceinline__ void box_stage(unsigned char* stage, const unsigned char* u8, int B, int Hi, int Wi, int b, int row0, int left,
                                          int w, int nrows, int maxrows, int pitch, int nseg, int ps) {
    const int tid = threadIdx.x;
    const int64_t total = (int64_t)B * 3 * Hi * Wi;
    const int rowbytes = Wi * ps;
    const int cpr = min((w * ps + 30) >> 4, pitch >> 4);          // chunks per row: covers any misalignment of the row's start
    const int nchunk = nseg * nrows * cpr;
    const int64_t img0 = (int64_t)b * 3 * Hi * Wi;
    for (int base = tid; base < nchunk; base += BATCH * THREADS) {
        u32x4 v[BATCH];
        int64_t g[BATCH];
        int dst[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
            const int idx = min(base + j * THREADS, nchunk - 1);
            const int row = idx / cpr, k = idx - row * cpr;
            const int s = row / nrows, r = row - s * nrows;
            const int64_t g0 = img0 + ((int64_t)(NHWC ? 0 : s) * Hi + (row0 + r)) * rowbytes + left * ps;
            g[j] = (g0 & ~(int64_t)15) + ((int64_t)k << 4);
            dst[j] = (s * maxrows + r) * pitch + (k << 4);
            v[j] = u32x4{0u, 0u, 0u, 0u};
            if (total >= 16) v[j] = ld16(u8 + (g[j] + 16 <= total ? g[j] : 0));       // (uniform: a batch below 16 bytes goes byte by byte)
        }
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
            if (base + j * THREADS >= nchunk) break;
            if (g[j] + 16 > total) v[j] = ld16_clipped(u8, g[j], total);              // the last chunk of the batch
            st16(stage + dst[j], v[j]);
        }
    }
}

// ---- where a staged row begins: staged row r of plane s starts at its slot + ((first byte of plane s, row row0) + r rowbytes) & 15
struct BoxStart { int img, plane, rowbytes; };
template <int NHWC>
__device__ __forceinline__ BoxStart box_start(int Hi, int Wi, int b, int row0, int left, int ps) {
    BoxStart m;
    m.rowbytes = Wi * ps;
    m.img = (int)(((int64_t)b * 3 * Hi * Wi + (int64_t)row0 * m.rowbytes + left * ps) & 15);
    m.plane = NHWC ? 0 : (int)(((int64_t)Hi * m.rowbytes) & 15);
    return m;
}
// LDS offset of channel c of pixel x (column left + x) of staged row r
template <int NHWC>
__device__ __forceinline__ int box_pixel(const BoxStart& m, int maxrows, int pitch, int c, int r, int x) {
    return NHWC ? r * pitch + ((m.img + r * m.rowbytes) & 15) + x * 3 + c
                : (c * maxrows + r) * pitch + ((m.img + c * m.plane + r * m.rowbytes) & 15) + x;
}

// ---- four output bytes, of which the first nvalid exist: one dword where all four do and the address is 4-byte aligned, bytes otherwise
// (k_crop_resample_u8; k_crop_resize_u8 writes the same lines out for its three planes, crop.hip says why)
__device__ __forceinline__ void box_store4(unsigned char* dstp, unsigned word, int nvalid) {
    if (nvalid == 4 && !(reinterpret_cast<uintptr_t>(dstp) & 3)) *reinterpret_cast<unsigned*>(dstp) = word;
    else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (j < nvalid) dstp[j] = (unsigned char)(word >> (8 * j));
    }
}

// ---- the host's checks in front of the geometry (ARGS: ap_crop_resize_args / ap_crop_resample_args).  filter: word 5 of a host record
// must be AP_RESAMPLE_BILINEAR or AP_RESAMPLE_BICUBIC.  *empty: B == 0, nothing to launch (AP_OK, and the pointers are not looked at)
template <class ARGS>
static int box_check(const ARGS* args, bool filter, bool* empty) {
    *empty = false;
    if (!args) return AP_ERR_NULL;
    const ARGS& a = *args;
    if (a.B < 0 || a.Hi <= 0 || a.Wi <= 0 || a.S <= 0) return AP_ERR_SHAPE;
    if (a.layout != AP_PREP_NCHW && a.layout != AP_PREP_NHWC) return AP_ERR_SHAPE;
    if (a.B == 0) { *empty = true; return AP_OK; }
    if (!a.u8 || !a.out || !a.records) return AP_ERR_NULL;
    if (reinterpret_cast<uintptr_t>(a.u8) & 15) return AP_ERR_SHAPE;
    if ((int64_t)a.B * 3 * a.Hi * a.Wi > ((int64_t)1 << 40)) return AP_ERR_SHAPE;
    if (a.records_host) {
        for (int64_t i = 0; i < a.B; ++i) {
            const int* q = a.records_host + i * 8;
            if (q[2] < 1 || q[3] < 1 || q[0] < 0 || q[1] < 0 || (int64_t)q[0] + q[2] > a.Hi || (int64_t)q[1] + q[3] > a.Wi) return AP_ERR_SHAPE;
            if (q[4] != 0 && q[4] != 1) return AP_ERR_SHAPE;
            if (filter && q[5] != AP_RESAMPLE_BILINEAR && q[5] != AP_RESAMPLE_BICUBIC) return AP_ERR_SHAPE;
        }
    }
    return AP_OK;
}

// ---- what the layout and Wi decide of a geometry: the staged planes, the pixel stride, and -> the LDS bytes of one staged row (the
// box's widest span plus any misalignment of its start and the round-up of its end)
static inline int64_t box_row_geometry(int layout, int Wi, int* nseg, int* ps) {
    *nseg = layout == AP_PREP_NCHW ? 3 : 1;
    *ps = layout == AP_PREP_NCHW ? 1 : 3;
    return ((int64_t)Wi * *ps + 15 + 15) / 16 * 16;
}
