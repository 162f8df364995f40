// fp8 weight gradients C[N1,N2] += alpha * dq_a * dq_b * A8[M,N1]^T . B8[M,N2] (BASELINE configs[4]: "e4m3 fwd / e5m2 grads"): A8 the
// output gradient as OCP e5m2 (or e4m3) bytes, B8 the layer input as e4m3 bytes, fp32 accumulation.
//
// Tile.  128 x 128 outputs per 256-thread workgroup (waves 2 x 2, 64 x 64 each = 4 x 4 MFMA tiles), one v_mfma_scale_f32_16x16x128_f8f6f4
// with unit scales per tile and 128-token K-step (the double-rate fp8 instruction; its format fields say e5m2 for A, e4m3 for B).  A K-step
// of both operands is 2 x [128 tok][128 B] = 32 KB of LDS, filled from registers that were loaded during the previous step's MFMAs.
// Tokens past M are loaded as zeros: any M works.
//
// Fragments.  Tokens are the SLOW axis of both operands, so fragments come from transposed reads: ds_read_b64_tr_b8 hands each lane
// of a 16-lane group one column of an 8 token x 16 column byte block (lane 2q + p supplies the address of token row q, columns
// 8p .. 8p + 7).  Lane group G reads tokens 32 G + 8 r + (0..7), r = 0..3, for A and B alike: whatever order the MFMA gives the 32
// bytes of a lane, both operands agree on the token behind every byte.  Inside a token row the 16-byte chunk c sits at position
// c ^ sw(t), sw(t) = ((t >> 1) & 3) | (((t >> 5) & 1) << 2): the 16 rows one half-wave reads land in 16 different 16-byte bank slots.
#pragma once
#include "common.h"

typedef int __attribute__((ext_vector_type(8))) tf_i32x8;
typedef int __attribute__((ext_vector_type(2))) tf_i32x2;

struct TfItem {            // one problem of a grouped launch
    const unsigned char* A; const unsigned char* B; float* C; float* slab; const float* dq_a; const float* dq_b;
    int lda, ldb, ldc, M, N1, N2, t2, ksteps, ksps, splits, start, tiles;
    float alpha;
    int a_fmt, shared_out;          // shared_out: another problem of the launch adds to the same C (atomics even when unsplit)
};

__device__ __forceinline__ int tf_sw(int t) { return ((t >> 1) & 3) | (((t >> 5) & 1) << 2); }

__device__ __forceinline__ tf_i32x2 tf_read_tr8(const unsigned char* p) {
    typedef __attribute__((address_space(3))) tf_i32x2 lds_i32x2;
    return __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2*)(p));
}

// it: the problem; tile, split: which 128 x 128 tile and which token range; smem: 32 KB
template <int AF>
__device__ __forceinline__ void tf_tile(const TfItem& it, int tile, int split, unsigned char* smem) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int i1 = tile / it.t2, i2 = tile - i1 * it.t2;
    const int n1_0 = i1 * 128, n2_0 = i2 * 128;
    const int k0 = split * it.ksps, k1 = min(it.ksteps, k0 + it.ksps);
    unsigned char* const sA = smem;
    unsigned char* const sB = smem + 16384;

    // staging: thread tid moves chunks c = tid + 256 j (j < 4) of each operand: token c >> 3, 16-byte chunk c & 7 of the tile's row
    u32x4 ra[4], rb[4];
    auto gload = [&](int ks) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = tid + 256 * j, t = c >> 3, ch = c & 7, tok = ks * 128 + t;
            if (tok < it.M) {
                ra[j] = ld16(it.A + (int64_t)tok * it.lda + n1_0 + ch * 16);
                rb[j] = ld16(it.B + (int64_t)tok * it.ldb + n2_0 + ch * 16);
            } else {
                ra[j] = (u32x4){0u, 0u, 0u, 0u};
                rb[j] = (u32x4){0u, 0u, 0u, 0u};
            }
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = tid + 256 * j, t = c >> 3, ch = c & 7;
            const int off = t * 128 + ((ch ^ tf_sw(t)) << 4);
            st16(sA + off, ra[j]);
            st16(sB + off, rb[j]);
        }
    };
    // fragment addresses: lane = 16 G + 2 q + p reads token row 32 G + 8 r + q, bytes 8 p .. 8 p + 7 of a 16-column chunk
    const int G = lane >> 4, q = (lane >> 1) & 7, p = lane & 1;
    const int sw = (q >> 1) | ((G & 1) << 2);           // tf_sw of every row this lane reads
    const int row0 = (32 * G + q) * 128 + 8 * p;

    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

    if (k0 < k1) gload(k0);
    for (int ks = k0; ks < k1; ++ks) {
        __syncthreads();                              // the previous step's fragment reads are done
        lstore();
        __syncthreads();
        if (ks + 1 < k1) gload(ks + 1);               // in flight under this step's MFMAs
        tf_i32x8 af[4], bfr[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int ca = (wr * 4 + t) ^ sw, cb = (wc * 4 + t) ^ sw;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const tf_i32x2 va = tf_read_tr8(sA + row0 + r * 1024 + (ca << 4));
                const tf_i32x2 vb = tf_read_tr8(sB + row0 + r * 1024 + (cb << 4));
                af[t][2 * r] = va[0]; af[t][2 * r + 1] = va[1];
                bfr[t][2 * r] = vb[0]; bfr[t][2 * r + 1] = vb[1];
            }
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                acc[a][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[a], bfr[b], acc[a][b], AF, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
    }

    // ---- partial tile -> C / slab: lane holds rows 4 (lane >> 4) + r, column lane & 15 of each 16 x 16 tile
    const float f = it.alpha * it.dq_a[0] * it.dq_b[0];
    const int fr = lane & 15, g4 = (lane >> 4) * 4;
    const int row_base = n1_0 + wr * 64 + g4, col_base = n2_0 + wc * 64 + fr;
    if (it.slab) {                                    // deterministic: this split's partial tile is stored, k_tn_reduce adds the splits in order
        float* const s = it.slab + (int64_t)split * it.N1 * it.N2;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) s[(int64_t)(row_base + a * 16 + r) * it.N2 + col_base + b * 16] = acc[a][b][r] * f;
        return;
    }
    float* const crow = it.C + (int64_t)row_base * it.ldc + col_base;
    if (it.splits == 1 && !it.shared_out) {           // the whole token axis: nobody else adds to this tile
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float* c = crow + (int64_t)(a * 16 + r) * it.ldc + b * 16;
                    *c = fmaf(acc[a][b][r], f, *c);
                }
        return;
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) atomicAdd(crow + (int64_t)(a * 16 + r) * it.ldc + b * 16, acc[a][b][r] * f);
}
