// Constants that the attention and outlook kernels (mhsa.hip, outlook.hip) and their host-side launch planner (attn_plan.h) share.  No HIP,
// no planner, nothing included.
#pragma once
#ifdef __HIPCC__
#define AP_CONST_FN __device__ __host__ __forceinline__
#else
#define AP_CONST_FN static inline
#endif

// mhsa.hip
#define FP_LOADERS 3            // loader waves of k_mhsa_fwd_p (of 16)
#define DS_STR 232              // k_mhsa_bwd_ds: dS^T row stride (bf16): 224 queries + 8 of padding (464 B: conflict-free transposed reads)
#define DS_LOADERS 3

// outlook.hip
#define OHD 32          // head dim handled by these kernels
#define OKK 9           // 3x3 slots
#define OPP 81
#define OGT 256         // threads per workgroup of k_outlook_gather, k_outlook_gather_mfma and k_outlook_dlogits
#define OPZ 288         // bf16 elements of a window's P / Z slot (9 x 32)
// chunk stride (in pixels) of the CHUNK-major patch image, padded so the four chunks of a pixel start 16 banks apart
AP_CONST_FN int pad_npix(int npix) { return npix + ((4 - (npix & 15)) & 15); }
// row stride (pixels) of the persistent kernels' LDS patch: the smallest value >= pw that is 3 (mod 4) -- see k_outlook_p
AP_CONST_FN int olk_pws(int pw) { return pw + ((3 - pw) & 3); }
