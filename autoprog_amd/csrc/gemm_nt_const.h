// Constants that the NT kernels (gemm.hip, gemm8p.h, gemm_ws.h) and their host-side launch planner (nt_plan.h) share.  Plain C: no HIP,
// no planner, nothing else included.
#pragma once

// epilogue flavour bits of the persistent 8-phase kernel (gemm8p.h: g8_flavour() forms them on the device, nt_flavour() below on the host)
enum { G8_BIAS = 1, G8_GELU = 2, G8_DGELU = 4, G8_RS = 8, G8_RES = 16, G8_MUL = 32, G8_MUL8 = 64, G8_GTAB = 128, G8_Q8 = 256, G8_NOSIDE = 512 };
#define G8_LDS_BYTES 163840                    // all of the CU's LDS: two K-tile buffers + the epilogue staging region
// the 224-row instantiations of the 8-phase kernel (256 x 192 tiles only): the flavours of the N = 384 products of a transformer block --
// plain, row scale, bias (+ row scale) + residual.  Any other flavour runs on 256-row tiles.
#define G8_FLAVOURS_224 0, G8_RS, G8_BIAS | G8_RES, G8_BIAS | G8_RS | G8_RES
// the weight-stationary kernel (gemm_ws.h)
#define WS_K 192
#define WS_BN 192
#define WS_BM 64
#define WS_ROWB 384                               // bytes of an LDS row (192 bf16)
#define WS_LDS_W (WS_BN * WS_ROWB)                // 73728
#define WS_LDS_A (WS_BM * WS_ROWB)                // 24576: the two groups' 32-row halves
// EPI 0: bf16 staging + the 16 KB table; EPI 1: fp32 staging (the multiply by the stored derivative happens on the fp32 accumulator value,
// rounded once -- as in the 8-phase kernel)
#define WS_LDS_BYTES(EPI) (WS_LDS_A + ((EPI) != 1 ? WS_LDS_A + 16384 : 2 * WS_LDS_A))
#define SK_STRIDE 36        // skinny kernel: floats per LDS row of a wave's 64x32 partial tile (16-B aligned, spreads the banks)
