// ap_input_prep: a loader's uint8 batch -> the stem's bf16 input in ONE launch (include/autoprog_hip.h): normalise (table lookup),
// Mixup / CutMix with image B-1-b, RandomErasing, bilinear resize, layout change.  19 MB in (38 MB when mixing) and 51 MB out at
// B = 128 / 224 px, where the composition in torch writes and re-reads a 77 MB fp32 batch several times.
//
// A workgroup owns `tp` pairs of output rows of one image.  The source rows those need -- and the partner image's when the tile
// mixes -- are staged in LDS as the uint8 they are, with 16-byte loads; the 3 x 256 normalisation table sits beside them.  A lane
// computes one 2 x 2 block of output pixels (one 32-byte space-to-depth block: two 16-byte stores).  Box tests are per tile first:
// a tile that no erase box and no CutMix box touches never tests a tap.
//
// The blend is written with explicit fmaf and this file is built with -ffp-contract=off (csrc/Makefile; the library's
// -ffp-contract=fast disregards a contract(off) pragma): it restates, operation for operation, what hipcc made of
// k_resize_bilinear_s2d16 / k_resize_bilinear_nhwc (csrc/elementwise.hip, -ffp-contract=fast), which is NOT the same for the three
// channels: the compiler packed channel pairs into v_pk_fma_f32 and chose a different operand of each sum to fuse.  Per kernel
// (a = 1 - lx, d = 1 - ly; p00 p01 / p10 p11 the taps):
//     s2d16  c0: top = fma(lx, p01, a p00)  bot = fma(a, p10, lx p11)  out = fma(ly, bot, d top)
//            c1: top = fma(lx, p01, a p00)  bot = fma(a, p10, lx p11)  out = fma(d, top, ly bot)
//            c2: top = fma(a, p00, lx p01)  bot = fma(a, p10, lx p11)  out = fma(d, top, ly bot)
//     nhwc   c0, c1: as s2d16 c2 (the vectorised channel pair)         c2 (loop remainder): out = d top + ly bot, both products rounded
// and the source index is ONE rounding, fma(o + 0.5, scale, -0.5).  tests/test_gpu_input_prep.py holds the two paths to torch.equal.
#include "common.h"

#if defined(__FAST_MATH__)
#error "input_prep.hip must be built with -ffp-contract=off and without fast-math (csrc/Makefile)"
#endif

#define PREP_THREADS 256
#define PREP_TABLE_BYTES (3 * 256 * 4)
#define PREP_LDS_LIMIT (60 * 1024)

struct PrepGeom {
    int tp;             // output row pairs per tile
    int tiles;          // tiles per image
    int maxrows;        // most source rows any tile needs
    int segcap;         // bytes of one staged segment (a multiple of 16)
    int nseg;           // segments per image: 3 channel planes (NCHW) or 1 (NHWC)
    int rowbytes;       // bytes of one source row inside a segment
    float sh, sw;
};

// PyTorch's source index (area_pixel_compute_source_index, align_corners = False), one rounding
__host__ __device__ __forceinline__ float prep_src(int o, float scale) { return fmaxf(fmaf((float)o + 0.5f, scale, -0.5f), 0.f); }

// ---- Philox-4x32-10 (Salmon et al., SC'11) on the counter (x, y, b, 0), key = seed: four 32-bit words per source pixel
__device__ __forceinline__ void philox4(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned* r) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}
// three standard normals of pixel (b, y, x): Box-Muller on (r0, r1) -> channels 0, 1 and on (r2, r3) -> channel 2.
// u in (0, 1] from the top 24 bits, so the logarithm is finite (|z| <= 5.8); the angle goes to v_sin / v_cos in revolutions
__device__ __forceinline__ void pixel_noise(unsigned k0, unsigned k1, int b, int y, int x, float* z) {
    unsigned r[4];
    philox4((unsigned)x, (unsigned)y, (unsigned)b, 0u, k0, k1, r);
    const float u0 = (float)((r[0] >> 8) + 1u) * 5.9604644775390625e-8f, t0 = (float)(r[1] >> 8) * 5.9604644775390625e-8f;
    const float u1 = (float)((r[2] >> 8) + 1u) * 5.9604644775390625e-8f, t1 = (float)(r[3] >> 8) * 5.9604644775390625e-8f;
    const float m0 = sqrtf(-2.f * __logf(u0)), m1 = sqrtf(-2.f * __logf(u1));
    z[0] = m0 * __builtin_amdgcn_cosf(t0);
    z[1] = m0 * __builtin_amdgcn_sinf(t0);
    z[2] = m1 * __builtin_amdgcn_cosf(t1);
}

struct PrepTile {
    const unsigned char* lds;      // staged bytes
    const float* tab;              // [3][256] in LDS
    const int* box;                // [n_boxes][8] in LDS
    int off_a[3], off_b[3];        // LDS byte offset of (c, y_lo, x = 0): this image / its partner
    int rs, ps;                    // byte strides of a source row / pixel
    int y_lo, nrows;
    int mix;                       // 0 none, 1 mixup, 2 cutmix -- for THIS tile (cutmix: only when the box meets its rows)
    float lam, oml;
    int yl, yh, xl, xh;
    int erase;                     // this tile meets a box
    int n_boxes, erase_mode;
    unsigned k0, k1;
    int b;
};

// value of source pixel (y, x) after normalise -> mix -> erase, three channels
__device__ __forceinline__ void prep_tap(const PrepTile& t, int y, int x, float* v) {
    const int ry = min(max(y - t.y_lo, 0), t.nrows - 1);
    const int o = ry * t.rs + x * t.ps;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = t.tab[c * 256 + t.lds[t.off_a[c] + o]];
    if (t.mix) {
        float p[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = t.tab[c * 256 + t.lds[t.off_b[c] + o]];
        if (t.mix == 1) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = t.lam * v[c] + t.oml * p[c];          // three roundings, as x * lam + x.flip(0) * (1 - lam)
        } else if (y >= t.yl && y < t.yh && x >= t.xl && x < t.xh) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = p[c];
        }
    }
    if (t.erase) {
        for (int r = 0; r < t.n_boxes; ++r) {
            const int* q = t.box + r * 8;
            const int top = q[0], left = q[1], h = q[2], w = q[3];
            if (h > 0 && y >= top && y < top + h && x >= left && x < left + w) {
                if (t.erase_mode == AP_ERASE_PIXEL) pixel_noise(t.k0, t.k1, t.b, y, x, v);
                else if (t.erase_mode == AP_ERASE_RAND) { v[0] = __int_as_float(q[4]); v[1] = __int_as_float(q[5]); v[2] = __int_as_float(q[6]); }
                else { v[0] = 0.f; v[1] = 0.f; v[2] = 0.f; }
            }
        }
    }
}

// one output pixel: the blend of its four taps, in the operation order of the kernel whose layout it writes (head of this file)
template <int OUT_NHWC>
__device__ __forceinline__ void prep_pixel(const PrepTile& t, int y0, int y1, float ly, int x0, int x1, float lx, float* out) {
    float p00[3], p01[3], p10[3], p11[3];
    prep_tap(t, y0, x0, p00); prep_tap(t, y0, x1, p01); prep_tap(t, y1, x0, p10); prep_tap(t, y1, x1, p11);
    const float a = 1.f - lx, d = 1.f - ly;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float bot = fmaf(a, p10[c], lx * p11[c]);
        if (OUT_NHWC) {
            const float top = fmaf(a, p00[c], lx * p01[c]);
            out[c] = c < 2 ? fmaf(d, top, ly * bot) : d * top + ly * bot;
        } else {
            const float top = c < 2 ? fmaf(lx, p01[c], a * p00[c]) : fmaf(a, p00[c], lx * p01[c]);
            out[c] = c == 0 ? fmaf(ly, bot, d * top) : fmaf(d, top, ly * bot);
        }
    }
}

template <int OUT_NHWC>
__global__ void __launch_bounds__(PREP_THREADS)
k_input_prep(ap_input_prep_args A, PrepGeom G) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int sbox[AP_PREP_MAX_BOXES * 8];
    float* tab = reinterpret_cast<float*>(smem);
    unsigned char* stage = smem + PREP_TABLE_BYTES;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / G.tiles, tile = blockIdx.x % G.tiles;
    const int Hi = A.Hi, Wi = A.Wi, Ho = A.Ho, Wo = A.Wo;

    // ---- the tile's output rows and the source rows they read
    const int oy_first = tile * G.tp * 2;
    const int oy_last = min(oy_first + G.tp * 2, Ho) - 1;
    const int y_lo = min((int)prep_src(oy_first, G.sh), Hi - 1);
    const int y_hl = min((int)prep_src(oy_last, G.sh), Hi - 1);
    const int y_hi = y_hl + (y_hl < Hi - 1);
    const int nrows = min(y_hi - y_lo + 1, G.maxrows);          // (== y_hi - y_lo + 1: maxrows is the host's maximum of the same expression)

    // ---- per-step decisions, from device memory
    int mode = 0, yl = 0, yh = 0, xl = 0, xh = 0;
    float lam = 1.f, oml = 0.f;
    unsigned k0 = 0, k1 = 0;
    if (A.params) {
        if (A.mix_enabled) {
            mode = A.params[0]; lam = __int_as_float(A.params[1]); oml = __int_as_float(A.params[8]);
            yl = A.params[2]; yh = A.params[3]; xl = A.params[4]; xh = A.params[5];
        }
        k0 = (unsigned)A.params[6]; k1 = (unsigned)A.params[7];
    }
    if (mode == 2 && !(yl <= y_lo + nrows - 1 && yh > y_lo && xl < xh)) mode = 0;       // the CutMix box misses this tile's rows
    if (mode != 1 && mode != 2) mode = 0;
    const int pb = A.B - 1 - b;

    for (int i = tid; i < 3 * 256; i += PREP_THREADS) tab[i] = A.table[i];
    const int nrec = A.boxes ? min(A.n_boxes, AP_PREP_MAX_BOXES) : 0;
    for (int i = tid; i < nrec * 8; i += PREP_THREADS) sbox[i] = A.boxes[((int64_t)b * A.n_boxes) * 8 + i];

    // ---- stage the source rows: per segment one contiguous span of global bytes, copied from its 16-byte-aligned start
    PrepTile T;
    const int64_t total = (int64_t)A.B * 3 * Hi * Wi;
    const int span = nrows * G.rowbytes;
    const int cap16 = G.segcap >> 4;
#pragma unroll
    for (int img = 0; img < 2; ++img) {
        if (img && !mode) break;
        const int ib = img ? pb : b;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            if (s >= G.nseg) break;
            const int64_t g0 = A.in_layout == AP_PREP_NCHW ? (((int64_t)ib * 3 + s) * Hi + y_lo) * Wi : ((int64_t)ib * Hi + y_lo) * Wi * 3;
            const int64_t a0 = g0 & ~(int64_t)15;
            const int mis = (int)(g0 - a0);
            const int lbase = (img * G.nseg + s) * G.segcap;
            const int nchunk = min((mis + span + 15) >> 4, cap16);
            for (int k = tid; k < nchunk; k += PREP_THREADS)        // (nothing read past the end of the batch)
                st16(stage + lbase + (k << 4), ld16_clipped(A.u8, a0 + ((int64_t)k << 4), total));
            if (A.in_layout == AP_PREP_NCHW) { (img ? T.off_b : T.off_a)[s] = lbase + mis; }
            else {
#pragma unroll
                for (int c = 0; c < 3; ++c) (img ? T.off_b : T.off_a)[c] = lbase + mis + c;
            }
        }
    }
    if (!mode) { T.off_b[0] = T.off_a[0]; T.off_b[1] = T.off_a[1]; T.off_b[2] = T.off_a[2]; }
    __syncthreads();

    int erase = 0;
    for (int r = 0; r < nrec; ++r) {
        const int top = sbox[r * 8], h = sbox[r * 8 + 2];
        erase |= (h > 0 && top <= y_lo + nrows - 1 && top + h > y_lo);
    }
    T.lds = stage; T.tab = tab; T.box = sbox;
    T.rs = A.in_layout == AP_PREP_NCHW ? Wi : Wi * 3; T.ps = A.in_layout == AP_PREP_NCHW ? 1 : 3;
    T.y_lo = y_lo; T.nrows = nrows;
    T.mix = mode; T.lam = lam; T.oml = oml; T.yl = yl; T.yh = yh; T.xl = xl; T.xh = xh;
    T.erase = erase; T.n_boxes = nrec; T.erase_mode = A.erase_mode; T.k0 = k0; T.k1 = k1; T.b = b;

    // ---- one 2 x 2 block of output pixels per lane and trip
    const int Wp = (Wo + 1) >> 1;
    const int rp = (oy_last - oy_first + 2) >> 1;                 // row pairs of this tile (the last one of an odd Ho holds one row)
    for (int it = tid; it < rp * Wp; it += PREP_THREADS) {
        const int py = it / Wp, px = it - py * Wp;
        float o[2][2][3];
        int valid[2][2];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int oy = oy_first + py * 2 + dy;
            const float fy = prep_src(min(oy, Ho - 1), G.sh);
            const int y0 = min((int)fy, Hi - 1), y1 = y0 + (y0 < Hi - 1);
            const float ly = fy - (float)y0;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int ox = px * 2 + dx;
                valid[dy][dx] = oy < Ho && ox < Wo;
                const float fx = prep_src(min(ox, Wo - 1), G.sw);
                const int x0 = min((int)fx, Wi - 1), x1 = x0 + (x0 < Wi - 1);
                prep_pixel<OUT_NHWC>(T, y0, y1, ly, x0, x1, fx - (float)x0, o[dy][dx]);
            }
        }
        if (!OUT_NHWC) {
            // channel (dy * 2 + dx) * 3 + c of the block, 12..15 zero (Ho, Wo even: all four pixels exist)
            bf16_t* dst = A.out + ((((int64_t)b * (Ho >> 1) + ((oy_first >> 1) + py)) * (Wo >> 1) + px) << 4);
            u32x4 lo, hi;
            lo[0] = pack_bf2(o[0][0][0], o[0][0][1]); lo[1] = pack_bf2(o[0][0][2], o[0][1][0]);
            lo[2] = pack_bf2(o[0][1][1], o[0][1][2]); lo[3] = pack_bf2(o[1][0][0], o[1][0][1]);
            hi[0] = pack_bf2(o[1][0][2], o[1][1][0]); hi[1] = pack_bf2(o[1][1][1], o[1][1][2]); hi[2] = 0u; hi[3] = 0u;
            st16_nt(dst, lo);
            st16_nt(dst + 8, hi);
        } else {
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                if (!valid[dy][0]) continue;
                const int64_t e = (((int64_t)b * Ho + (oy_first + py * 2 + dy)) * Wo + px * 2) * 3;       // element offset of pixel (oy, 2 px)
                bf16_t* dst = A.out + e;
                if (valid[dy][1] && !(e & 1)) {                    // both pixels, 4-byte aligned: three dword stores
                    unsigned* d32 = reinterpret_cast<unsigned*>(dst);
                    d32[0] = pack_bf2(o[dy][0][0], o[dy][0][1]); d32[1] = pack_bf2(o[dy][0][2], o[dy][1][0]); d32[2] = pack_bf2(o[dy][1][1], o[dy][1][2]);
                } else {
#pragma unroll
                    for (int c = 0; c < 3; ++c) dst[c] = f2bf(o[dy][0][c]);
                    if (valid[dy][1]) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) dst[3 + c] = f2bf(o[dy][1][c]);
                    }
                }
            }
        }
    }
}

// tile height and LDS budget: the source rows of a tile come from the same float expression the kernel evaluates
static int prep_geometry(const ap_input_prep_args* a, PrepGeom* g) {
    g->sh = (float)a->Hi / (float)a->Ho;
    g->sw = (float)a->Wi / (float)a->Wo;
    g->nseg = a->in_layout == AP_PREP_NCHW ? 3 : 1;
    g->rowbytes = a->in_layout == AP_PREP_NCHW ? a->Wi : a->Wi * 3;
    const int Hp = (a->Ho + 1) / 2;
    for (int tp = 4; tp >= 1; tp >>= 1) {
        const int tiles = (Hp + tp - 1) / tp;
        int maxrows = 1;
        for (int t = 0; t < tiles; ++t) {
            const int first = t * tp * 2;
            const int last = (first + tp * 2 < a->Ho ? first + tp * 2 : a->Ho) - 1;
            int lo = (int)prep_src(first, g->sh), hl = (int)prep_src(last, g->sh);
            if (lo > a->Hi - 1) lo = a->Hi - 1;
            if (hl > a->Hi - 1) hl = a->Hi - 1;
            const int hi = hl + (hl < a->Hi - 1);
            if (hi - lo + 1 > maxrows) maxrows = hi - lo + 1;
        }
        const int64_t segcap = ((int64_t)maxrows * g->rowbytes + 15 + 15) / 16 * 16;
        const int64_t lds = PREP_TABLE_BYTES + segcap * g->nseg * (a->mix_enabled ? 2 : 1);
        if (lds <= PREP_LDS_LIMIT) {
            g->tp = tp; g->tiles = tiles; g->maxrows = maxrows; g->segcap = (int)segcap;
            return (int)lds;
        }
    }
    return -1;
}

extern "C" int ap_input_prep(const ap_input_prep_args* args, ap_stream_t stream) {
    if (!args) return AP_ERR_NULL;
    const ap_input_prep_args& a = *args;
    if (a.B < 0 || a.Hi <= 0 || a.Wi <= 0 || a.Ho <= 0 || a.Wo <= 0) return AP_ERR_SHAPE;
    if (a.in_layout != AP_PREP_NCHW && a.in_layout != AP_PREP_NHWC) return AP_ERR_SHAPE;
    if (a.out_layout != AP_PREP_S2D16 && a.out_layout != AP_PREP_OUT_NHWC) return AP_ERR_SHAPE;
    if (a.out_layout == AP_PREP_S2D16 && ((a.Ho & 1) || (a.Wo & 1))) return AP_ERR_SHAPE;
    if (a.n_boxes < 0 || a.n_boxes > AP_PREP_MAX_BOXES) return AP_ERR_SHAPE;
    if (a.erase_mode != AP_ERASE_CONST && a.erase_mode != AP_ERASE_RAND && a.erase_mode != AP_ERASE_PIXEL) return AP_ERR_SHAPE;
    if (a.boxes_host) {
        for (int64_t i = 0; i < (int64_t)a.B * a.n_boxes; ++i) {
            const int* q = a.boxes_host + i * 8;
            if (q[2] == 0) continue;
            if (q[2] < 0 || q[3] <= 0 || q[0] < 0 || q[1] < 0 || (int64_t)q[0] + q[2] > a.Hi || (int64_t)q[1] + q[3] > a.Wi) return AP_ERR_SHAPE;
        }
    }
    if (a.B == 0) return AP_OK;
    if (!a.u8 || !a.out || !a.table || (a.n_boxes > 0 && !a.boxes)) return AP_ERR_NULL;
    if (reinterpret_cast<uintptr_t>(a.u8) & 15) return AP_ERR_SHAPE;
    if ((int64_t)a.B * 3 * a.Hi * a.Wi > ((int64_t)1 << 40)) return AP_ERR_SHAPE;
    PrepGeom g;
    const int lds = prep_geometry(&a, &g);
    if (lds < 0) return AP_ERR_UNSUPPORTED;                       // one row pair's source rows do not fit the LDS budget
    const int64_t blocks = (int64_t)a.B * g.tiles;
    if (blocks > 0x7fffffff) return AP_ERR_SHAPE;
    (void)hipGetLastError();
    if (a.out_layout == AP_PREP_S2D16)
        hipLaunchKernelGGL(k_input_prep<0>, dim3((unsigned)blocks), dim3(PREP_THREADS), lds, (hipStream_t)stream, a, g);
    else
        hipLaunchKernelGGL(k_input_prep<1>, dim3((unsigned)blocks), dim3(PREP_THREADS), lds, (hipStream_t)stream, a, g);
    return ap_check_launch();
}
