// Distillation loss of a student row against a teacher row (DeiT's DistillationLoss), forward + gradient in one pass over both rows:
//   soft (mode 0)   p_s = softmax(x_s / T), p_t = softmax(x_t / T):   row_loss = T^2 sum_c p_t (log p_t - log p_s),   dx_s = gscale T (p_s - p_t)
//   hard (mode 1)   c* = argmax_c x_t (equal logits: the smallest class):   row_loss = logsumexp(x_s) - x_s[c*],   dx_s = gscale (softmax(x_s) - [c == c*])
// HBM-bound by design: student 2 B + teacher 2 B in, gradient 2 B out per (row, class), nothing else.  Written for any row count M
// (M = B for the class/distillation token pair of a DeiT; B N rows of a per-token use later).
//
// Statistics in fp32 with the maximum subtracted ((x - max) is exact for bf16 operands): both maxima, then
//   S_s = sum exp((x_s - m_s) / T),  S_t = sum exp((x_t - m_t) / T),  W = sum e_t ((x_t - m_t) - (x_s - m_s))
// in ONE walk, and  KL = W / (T S_t) + log S_s - log S_t.  A teacher row that equals the student row gives W = 0 and S_s == S_t bit
// for bit: the loss is exactly zero, and the gradient e_s ks - e_t kt is zero up to the rounding residue of one product (the compiler may
// contract it into fma(e_s, ks, -(e_t kt))): at most 2^-24 of gscale T p_s, measured <= 1.2e-9 at gscale = 0.5.
// The hard label is the maximum of one integer key per column (the order code of the bf16 value, -0 read as +0, above 0xFFFF - column:
// the tie rule of csrc/topk.hip), clamped into [0, C) whatever the row held.
// Fixed reduction order (one DPP tree per wave, then the waves of a team in index order): bit-reproducible.  No atomics, no workspace,
// plain grids (one workgroup per row group), clamped unconditional loads.
//
// What selects a kernel is Cp = round_up(C, 8), the columns that are ever read -- NOT the leading dimensions: a padded operand takes
// the kernel, and so the reduction order and the bits, of the compact one.  Columns C .. Cp-1 reach registers (and LDS) but are
// replaced by a select before any use; columns Cp .. ld-1 are never read.  dstudent's columns C .. ld_s-1 are stored as zero bits.
//   Cp <= 1024           k_distill: both rows in one wave's registers (two 16-byte chunks per lane and operand), DS_SR rows per wave, all of
//                        their loads issued before the first reduction.
//   1024 < Cp            k_distill_wide: the rows are staged in LDS ONCE, the maxima (or the hard label) on the way; the sums and the gradient
//                        walk LDS.  The teams and the rules are those of row_wide.h; its staging walk is written out here for two rows
//                        walked together (through the shared template this kernel measured 3 - 7 % slower).  Two barriers per workgroup.
//     soft, 4 Cp <= DS_LDS_MAX (Cp <= 40 704)   both rows in LDS, 4 B per column: both operands are read from global memory exactly once
//                                               (21 848 columns: 87 KB, one workgroup per CU).
//     soft, wider                               the STUDENT row is staged (2 B per column, 128 KB at 65 536) and read from global memory once;
//                                               the TEACHER row is read from global memory in each of the three walks (maximum, sums,
//                                               gradient) -- the second and third from L2, a row is at most 128 KB.
//     hard                                      only the student row is staged at any width; the teacher row is read once, for its label.
#include "row_wide.h"

#define DS_SR 2                          // narrow kernel: rows per wave
#define DS_NARROW_MAXC 1024
#define DS_LDS_MAX (159 * 1024)          // dynamic LDS of a workgroup (160 KB less the reduction words and slack)
#define DS_NEG (-3.0e38f)
#define DS_LOG2E 1.44269504088896341f

// max of t and the keys of the chunk whose first column is c0; columns >= C give key 0 (below every valid key)
__device__ __forceinline__ unsigned ds_chunk_key(const u32x4& v, int c0, int C, unsigned t) {
    const unsigned cc = 0xffffu - (unsigned)c0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const unsigned o = rw_encode2(v[w]);
        t = max(t, c0 + 2 * w < C ? ((o << 16) | ((cc - 2 * w) & 0xffffu)) : 0u);
        t = max(t, c0 + 2 * w + 1 < C ? ((o & 0xffff0000u) | ((cc - 2 * w - 1) & 0xffffu)) : 0u);
    }
    return t;
}
// the 8 values of a chunk, columns >= C replaced (only the last chunk of a row takes the branch)
__device__ __forceinline__ void ds_vals8(const u32x4& v, int c0, int C, float* f) {
    unpack8(v, f);
    if (c0 + 8 > C) {
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = c0 + j < C ? f[j] : DS_NEG;
    }
}
__device__ __forceinline__ float ds_soft_loss(float Ss, float St, float W, float inv_temp, float temp) {
    return temp * temp * (W * inv_temp / St + (__logf(Ss) - __logf(St)));
}

// ---------------------------------------------------------------------------------------------------------------- Cp <= 1024
// One wave per row, DS_SR rows per wave: lane l owns chunks l and l + 64 of both operands.
template <int MODE>
__global__ void __launch_bounds__(256)
k_distill(const bf16_t* __restrict__ student, int ld_s, const bf16_t* __restrict__ teacher, int ld_t, int C, float inv_temp, float temp,
          float* __restrict__ row_loss, bf16_t* __restrict__ dstudent, float gscale, int64_t M) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * DS_SR;
    if (row0 >= M) return;                                        // (whole waves; no barrier in this kernel)
    const int nch = (C + 7) >> 3, nchs = ld_s >> 3;
    const float scale = inv_temp * DS_LOG2E;
    u32x4 rs[DS_SR][2], rt[DS_SR][2];
#pragma unroll
    for (int r = 0; r < DS_SR; ++r) {
        const int64_t row = min(row0 + r, M - 1);
        const u32x4* sg = reinterpret_cast<const u32x4*>(student + row * ld_s);
        const u32x4* tg = reinterpret_cast<const u32x4*>(teacher + row * ld_t);
#pragma unroll
        for (int i = 0; i < 2; ++i) {                             // clamped, unconditional; a repeated chunk is masked below
            rs[r][i] = sg[min(lane + 64 * i, nch - 1)];
            rt[r][i] = tg[min(lane + 64 * i, nch - 1)];
        }
    }
#pragma unroll
    for (int r = 0; r < DS_SR; ++r) {
        const int64_t row = row0 + r;
        if (row >= M) break;
        float a[16], b[16];
        float mxs = DS_NEG, mxt = DS_NEG;
        unsigned key = 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int q = lane + 64 * i, c0 = q < nch ? 8 * q : C;                    // a chunk beyond the row: every column masked
            ds_vals8(rs[r][i], c0, C, a + 8 * i);
            if (MODE == 0) ds_vals8(rt[r][i], c0, C, b + 8 * i);
            else key = ds_chunk_key(rt[r][i], c0, C, key);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) { mxs = fmaxf(mxs, a[e]); if (MODE == 0) mxt = fmaxf(mxt, b[e]); }
        mxs = rw_wave_max(mxs);
        float Ss = 0.f, St = 0.f, W = 0.f, ks, kt = 0.f, loss;
        int cstar = -1;
        if (MODE == 0) {
            mxt = rw_wave_max(mxt);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float ds = a[e] - mxs, dt = b[e] - mxt;
                a[e] = __builtin_amdgcn_exp2f(ds * scale);
                b[e] = __builtin_amdgcn_exp2f(dt * scale);
                Ss += a[e]; St += b[e];
                W += b[e] * (dt - ds);
            }
            Ss = rw_wave_sum(Ss); St = rw_wave_sum(St); W = rw_wave_sum(W);
            loss = ds_soft_loss(Ss, St, W, inv_temp, temp);
            ks = gscale * temp / Ss; kt = gscale * temp / St;
        } else {
            cstar = rw_key_class(rw_wave_maxu(key), C);
            float xstar = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int c = 8 * (lane + 64 * (e >> 3)) + (e & 7);
                xstar += c == cstar ? a[e] : 0.f;
                a[e] = __builtin_amdgcn_exp2f((a[e] - mxs) * DS_LOG2E);
                Ss += a[e];
            }
            Ss = rw_wave_sum(Ss); xstar = rw_wave_sum(xstar);
            loss = (mxs - xstar) + __logf(Ss);
            ks = gscale / Ss;
        }
        if (lane == 0) row_loss[row] = loss;
        bf16_t* dr = dstudent + row * ld_s;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int q = lane + 64 * i;
            if (q < nch) {
                float d[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = 8 * q + j;
                    const float g = MODE == 0 ? a[8 * i + j] * ks - b[8 * i + j] * kt : a[8 * i + j] * ks - (c == cstar ? gscale : 0.f);
                    d[j] = c < C ? g : 0.f;
                }
                st16_nt(dr + 8 * q, pack8(d));
            }
        }
        const u32x4 zero = {0u, 0u, 0u, 0u};
        for (int q = nch + lane; q < nchs; q += 64) st16_nt(dr + 8 * q, zero);        // columns Cp .. ld_s-1
    }
}

// ---------------------------------------------------------------------------------------------------------------- 1024 < Cp <= 65 536
// MODE 0: soft, both rows in LDS; 1: hard, the student row in LDS; 2: soft, the student row in LDS and the teacher row from global memory
template <int WPR, int MODE>
__global__ void __launch_bounds__(256)
k_distill_wide(const bf16_t* __restrict__ student, int ld_s, const bf16_t* __restrict__ teacher, int ld_t, int C, float inv_temp, float temp,
               float* __restrict__ row_loss, bf16_t* __restrict__ dstudent, float gscale, int64_t M) {
    extern __shared__ __attribute__((aligned(16))) u32x4 ds_rows[];             // [4 / WPR][Cp / 8] student, then (MODE 0) the same of the teacher
    __shared__ float red_ms[4], red_mt[4], red_a[4], red_b[4], red_c[4];
    __shared__ unsigned red_k[4];
    constexpr int T = 64 * WPR, RPB = 4 / WPR, U = 4;
    const RwTeam g = rw_team<WPR>(M);
    const int wave = g.wave, lane = g.lane, team = g.team, tt = g.tt;
    const bool live = g.live;
    const int64_t row = g.row;
    const int nch = (C + 7) >> 3, nchs = ld_s >> 3;
    const float scale = MODE == 1 ? DS_LOG2E : inv_temp * DS_LOG2E;
    u32x4* ls = ds_rows + (size_t)team * nch;
    u32x4* lt = MODE == 0 ? ds_rows + (size_t)(RPB + team) * nch : nullptr;      // the teacher's rows exist in LDS in MODE 0 only
    const u32x4* sg = reinterpret_cast<const u32x4*>(student + row * ld_s);
    const u32x4* tg = reinterpret_cast<const u32x4*>(teacher + row * ld_t);
    // ---- walk 1: global -> LDS, the maxima (or the hard label's key) on the way: rw_stage of row_wide.h written out for two rows (see there)
    float mxs = DS_NEG, mxt = DS_NEG;
    unsigned key = 0;
    {
        u32x4 cs[U], ct[U], ns[U], nt[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { cs[u] = sg[min(tt + T * u, nch - 1)]; ct[u] = tg[min(tt + T * u, nch - 1)]; }       // clamped, unconditional
        for (int base = 0; base < nch; base += U * T) {
            const bool more = base + U * T < nch;                                // team-uniform: one branch around the whole batch
            if (more) {
#pragma unroll
                for (int u = 0; u < U; ++u) { ns[u] = sg[min(base + U * T + tt + T * u, nch - 1)]; nt[u] = tg[min(base + U * T + tt + T * u, nch - 1)]; }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = base + tt + T * u;
                if (q < nch) {
                    float f[8];
                    ls[q] = cs[u];
                    ds_vals8(cs[u], 8 * q, C, f);
#pragma unroll
                    for (int j = 0; j < 8; ++j) mxs = fmaxf(mxs, f[j]);
                    if (MODE == 1) {
                        key = ds_chunk_key(ct[u], 8 * q, C, key);
                    } else {
                        if (MODE == 0) lt[q] = ct[u];
                        ds_vals8(ct[u], 8 * q, C, f);
#pragma unroll
                        for (int j = 0; j < 8; ++j) mxt = fmaxf(mxt, f[j]);
                    }
                }
            }
            if (more) {
#pragma unroll
                for (int u = 0; u < U; ++u) { cs[u] = ns[u]; ct[u] = nt[u]; }
            }
        }
    }
    mxs = rw_wave_max(mxs);
    if (MODE == 1) key = rw_wave_maxu(key); else mxt = rw_wave_max(mxt);
    if (lane == 0) { red_ms[wave] = mxs; red_mt[wave] = mxt; red_k[wave] = key; }
    __syncthreads();
    mxs = red_ms[team * WPR]; mxt = red_mt[team * WPR]; key = red_k[team * WPR];
#pragma unroll
    for (int w = 1; w < WPR; ++w) { mxs = fmaxf(mxs, red_ms[team * WPR + w]); mxt = fmaxf(mxt, red_mt[team * WPR + w]); key = max(key, red_k[team * WPR + w]); }
    const int cstar = MODE == 1 ? rw_key_class(key, C) : -1;
    // ---- walk 2: the sums
    float Ss = 0.f, St = 0.f, W = 0.f;
#pragma unroll 2
    for (int q = tt; q < nch; q += T) {
        float a[8], b[8];
        ds_vals8(ls[q], 8 * q, C, a);
        if (MODE == 1) {
#pragma unroll
            for (int j = 0; j < 8; ++j) Ss += __builtin_amdgcn_exp2f((a[j] - mxs) * scale);
        } else {
            ds_vals8(MODE == 0 ? lt[q] : tg[q], 8 * q, C, b);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float ds = a[j] - mxs, dt = b[j] - mxt;
                const float et = __builtin_amdgcn_exp2f(dt * scale);
                Ss += __builtin_amdgcn_exp2f(ds * scale);
                St += et;
                W += et * (dt - ds);
            }
        }
    }
    Ss = rw_wave_sum(Ss);
    if (MODE != 1) { St = rw_wave_sum(St); W = rw_wave_sum(W); }
    if (lane == 0) { red_a[wave] = Ss; red_b[wave] = St; red_c[wave] = W; }
    __syncthreads();
    Ss = red_a[team * WPR]; St = red_b[team * WPR]; W = red_c[team * WPR];
#pragma unroll
    for (int w = 1; w < WPR; ++w) { Ss += red_a[team * WPR + w]; St += red_b[team * WPR + w]; W += red_c[team * WPR + w]; }
    float ks, kt = 0.f, loss;
    if (MODE == 1) {
        const float xstar = bf2f(reinterpret_cast<const bf16_t*>(ls)[cstar]);    // (written before the first barrier)
        loss = (mxs - xstar) + __logf(Ss);
        ks = gscale / Ss;
    } else {
        loss = ds_soft_loss(Ss, St, W, inv_temp, temp);
        ks = gscale * temp / Ss; kt = gscale * temp / St;
    }
    if (live && tt == 0) row_loss[row] = loss;
    // ---- walk 3: the gradient, columns C .. ld_s-1 as zeros
    bf16_t* dr = dstudent + row * ld_s;
#pragma unroll 2
    for (int q = tt; q < nch; q += T) {
        float a[8], b[8], d[8];
        ds_vals8(ls[q], 8 * q, C, a);
        if (MODE != 1) ds_vals8(MODE == 0 ? lt[q] : tg[q], 8 * q, C, b);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = 8 * q + j;
            const float es = __builtin_amdgcn_exp2f((a[j] - mxs) * scale);
            const float g = MODE == 1 ? es * ks - (c == cstar ? gscale : 0.f) : es * ks - __builtin_amdgcn_exp2f((b[j] - mxt) * scale) * kt;
            d[j] = c < C ? g : 0.f;
        }
        if (live) st16_nt(dr + 8 * q, pack8(d));
    }
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (int q = nch + tt; q < nchs; q += T)
        if (live) st16_nt(dr + 8 * q, zero);
}

// a workgroup of the wide kernels takes up to DS_LDS_MAX bytes of dynamic LDS
template <int WPR, int MODE>
static int ds_launch_wide(const bf16_t* s, int ld_s, const bf16_t* t, int ld_t, int C, float inv_temp, float temp, float* row_loss, bf16_t* ds,
                          float gscale, int64_t M, size_t lds, unsigned blocks, hipStream_t stream) {
    if (const int rc = ap_allow_lds<k_distill_wide<WPR, MODE>>(DS_LDS_MAX); rc != AP_OK) return rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL((k_distill_wide<WPR, MODE>), dim3(blocks), dim3(256), lds, stream, s, ld_s, t, ld_t, C, inv_temp, temp, row_loss, ds, gscale, M);
    return ap_check_launch();
}

extern "C" int ap_distill_fwd_bwd(const ap_bf16* student, int ld_s, const ap_bf16* teacher, int ld_t, int C, int mode, float inv_temp,
                                  float* row_loss, ap_bf16* dstudent, float grad_scale, int64_t M, ap_stream_t stream) {
    if (M < 0 || C < 1 || ld_s < C || ld_t < C || (ld_s & 7) || (ld_t & 7) || (mode != 0 && mode != 1)) return AP_ERR_SHAPE;
    if (mode == 0 && (!(inv_temp > 0.f) || !(inv_temp < 3.0e38f))) return AP_ERR_SHAPE;
    if (ld_s > RW_MAXLD || ld_t > RW_MAXLD) return AP_ERR_UNSUPPORTED;
    if (M == 0) return AP_OK;
    if (!student || !teacher || !row_loss || !dstudent) return AP_ERR_NULL;
    if (((uintptr_t)student | (uintptr_t)teacher | (uintptr_t)dstudent) & 15) return AP_ERR_SHAPE;     // rows are moved in 16-byte chunks
    if (mode == 1) inv_temp = 1.0f;
    const float temp = 1.0f / inv_temp;
    const bf16_t* s = reinterpret_cast<const bf16_t*>(student);
    const bf16_t* t = reinterpret_cast<const bf16_t*>(teacher);
    bf16_t* ds = reinterpret_cast<bf16_t*>(dstudent);
    hipStream_t st = (hipStream_t)stream;
    const int Cp = (C + 7) & ~7;
    if (Cp <= DS_NARROW_MAXC) {
        const int64_t blocks = (M + 4 * DS_SR - 1) / (4 * DS_SR);
        if (blocks > 0x7fffffffLL) return AP_ERR_SHAPE;
        (void)hipGetLastError();
        if (mode == 0) hipLaunchKernelGGL(k_distill<0>, dim3((unsigned)blocks), dim3(256), 0, st, s, ld_s, t, ld_t, C, inv_temp, temp, row_loss, ds, grad_scale, M);
        else hipLaunchKernelGGL(k_distill<1>, dim3((unsigned)blocks), dim3(256), 0, st, s, ld_s, t, ld_t, C, inv_temp, temp, row_loss, ds, grad_scale, M);
        return ap_check_launch();
    }
    return rw_launch(Cp, M, [&](auto wpr, unsigned blocks) {
        constexpr int WPR = decltype(wpr)::value;
        const size_t rows = (size_t)(4 / WPR) * Cp * sizeof(bf16_t);              // the student rows of a workgroup
        if (mode == 1) return ds_launch_wide<WPR, 1>(s, ld_s, t, ld_t, C, inv_temp, temp, row_loss, ds, grad_scale, M, rows, blocks, st);
        if constexpr (WPR == 4) {                                                // (four rows of a one-wave team and their teachers are 64 KB at the most)
            if (2 * rows > DS_LDS_MAX) return ds_launch_wide<4, 2>(s, ld_s, t, ld_t, C, inv_temp, temp, row_loss, ds, grad_scale, M, rows, blocks, st);
        }
        return ds_launch_wide<WPR, 0>(s, ld_s, t, ld_t, C, inv_temp, temp, row_loss, ds, grad_scale, M, 2 * rows, blocks, st);
    });
}
