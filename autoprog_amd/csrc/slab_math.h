// What the flat-slab optimizer files (optim.hip, agc.hip, lamb.hip) share: the small rules each of them used to restate.  Everything here
// is inlined into the including file and compiled under THAT file's contraction flag (lamb.o: off; optim.o, agc.o: fast -- Makefile), so
// every kernel keeps the instructions it had.
#pragma once
#include "common.h"
#include <math.h>

// ---- device: sums of exact squares.  x * x of an fp32 is exact in fp64, so only the order of the additions is left to the caller.
__device__ __forceinline__ void sq_add(float x, double& s) { const double d = (double)x; s = fma(d, d, s); }
// ... of the finite elements only; a non-finite one (exponent all ones: +-inf, NaN) is counted instead
__device__ __forceinline__ void sq_add_finite(float x, double& s, int& bad) {
    const bool nf = (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
    const double d = nf ? 0.0 : (double)x;
    s = fma(d, d, s);
    bad += nf ? 1 : 0;
}

// the butterfly over a wave of any number of fp64 sums and int counts: a fixed tree, every lane ends with the wave's totals
template <class... T> __device__ __forceinline__ void wave_sum(T&... x) {
    for (int o = 32; o > 0; o >>= 1) ((x += __shfl_xor(x, o, 64)), ...);
}

// how a range of `len` elements that starts at element b of a 16-byte aligned slab splits: `head` scalars up to the first 16-byte
// boundary (b may sit on any residue mod 4: tensors of odd length lie back to back), nv float4, `tail` scalars
__device__ __forceinline__ void slab_split(int64_t b, int64_t len, int& head, int64_t& nv, int& tail) {
    head = (int)((4 - (b & 3)) & 3);
    if (head > len) head = (int)len;
    nv = (len - head) >> 2;
    tail = (int)(len - head - (nv << 2));
}

// the factor on a slab element that makes it the clipped MEAN gradient: the pending mean `gscale` (1/world: the slab holds the all-reduced
// SUM under a deferred mean), times torch.nn.utils.clip_grad_norm_'s coefficient min(1, max_norm / (||g|| + 1e-6)) with ||g|| the norm of
// the mean gradient, when gnorm_sq -- the device scalar of ap_sumsq_f32 over the UNSCALED slab -- is given
__device__ __forceinline__ float clip_gscale(float gscale, const float* gnorm_sq, float max_norm) {
    float gs = gscale;
    if (gnorm_sq) {
        const float total = sqrtf(gnorm_sq[0]) * gscale;
        gs *= fminf(1.0f, max_norm / (total + 1e-6f));
    }
    return gs;
}

// ---- host: Adam's bias corrections 1 - beta1^t and sqrt(1 - beta2^t), in double from the float arguments and rounded once:
// graph.StepScalars.set_adam forms the SAME two numbers on the host, so a step replayed from a graph -- which reads them from device
// memory -- is bit-identical to the eager step
static inline void adam_bias_corrections(float beta1, float beta2, int step, float& bc1, float& bc2_sqrt) {
    bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
}

// ---- host: the EMA slabs of a launch.  A bf16 copy is refused when it is given for a copy the launch does not have or off 8 bytes
static inline bool ema16_refused(const ap_bf16* q, int e, int n_ema) { return q && (e >= n_ema || ((uintptr_t)q & 7)); }
// the four EMA slabs, their decays and their bf16 copies (ema_bf16: nullable, like each of its entries) from an entry point's host
// arrays into a launch's arguments, checked copy by copy: a null slab is AP_ERR_NULL, one off `ema_align_mask` or a refused bf16 copy
// AP_ERR_SHAPE.  Entries at e >= n_ema come out null / 0.
static inline int slab_ema_args(float* const* ema, const float* ema_decay, int n_ema, ap_bf16* const* ema_bf16, uintptr_t ema_align_mask,
                                float* (&o_ema)[4], float (&o_decay)[4], bf16_t* (&o_ema16)[4]) {
    for (int e = 0; e < 4; ++e) {
        o_ema[e] = (e < n_ema) ? ema[e] : nullptr;
        o_decay[e] = (e < n_ema) ? ema_decay[e] : 0.f;
        o_ema16[e] = ema_bf16 ? reinterpret_cast<bf16_t*>(ema_bf16[e]) : nullptr;
        if (e < n_ema && !ema[e]) return AP_ERR_NULL;
        if (e < n_ema && ((uintptr_t)ema[e] & ema_align_mask)) return AP_ERR_SHAPE;
        if (ema_bf16 && ema16_refused(ema_bf16[e], e, n_ema)) return AP_ERR_SHAPE;
    }
    return AP_OK;
}
