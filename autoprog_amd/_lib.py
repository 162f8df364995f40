"""ctypes binding of libautoprog_hip.so (the C ABI declared in include/autoprog_hip.h).

The library is the product: there is NO fallback.  Importing this module on a machine
without the built .so, or calling an op without a GPU tensor, raises immediately.
"""
import ctypes
import os

import torch  # noqa: F401  (must be loaded BEFORE the extension: both must share torch's HIP runtime)
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_int64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AP_LIB_PATH") or os.path.join(_HERE, "libautoprog_hip.so")      # AP_LIB_PATH: ablation builds (tools/abl_tn.sh)


class GemmEpilogue(Structure):
    _fields_ = [("bias", c_void_p), ("gelu", c_int), ("preact_out", c_void_p), ("dgelu_of", c_void_p),
                ("row_scale", c_void_p), ("rows_per_scale", c_int), ("residual", c_void_p), ("ldr", c_int), ("mul_by", c_void_p),
                ("mul_by8", c_void_p), ("q8_out", c_void_p), ("q8_scale", c_void_p), ("q8_amax", c_void_p)]


class MlpFusedArgs(Structure):
    """ap_mlp_fused_args (include/autoprog_hip.h)"""
    _fields_ = [("x", c_void_p), ("ldx", c_int), ("wa", c_void_p), ("ldwa", c_int), ("wb", c_void_p), ("ldwb", c_int), ("out", c_void_p), ("ldo", c_int),
                ("hidden_out", c_void_p), ("ldh", c_int), ("codes", c_void_p), ("bias1", c_void_p), ("bias2", c_void_p),
                ("row_scale_hidden", c_void_p), ("row_scale_out", c_void_p), ("rows_per_scale", c_int), ("residual", c_void_p), ("ldr", c_int),
                ("m", c_int), ("c", c_int), ("hidden", c_int), ("backward", c_int),
                ("ln_in", c_void_p), ("ld_ln", c_int), ("ln_out", c_void_p), ("ld_lno", c_int), ("ln_gamma", c_void_p), ("ln_beta", c_void_p),
                ("ln_eps", c_float), ("ln_mean", c_void_p), ("ln_rstd", c_void_p)]


class TnProblem(Structure):
    """ap_tn_problem (include/autoprog_hip.h)"""
    _fields_ = [("A", c_void_p), ("lda", c_int), ("B", c_void_p), ("ldb", c_int), ("C", c_void_p), ("ldc", c_int),
                ("M", c_int), ("N1", c_int), ("N2", c_int), ("alpha", c_float), ("colsum_A", c_void_p), ("colsum_weight", c_void_p), ("colsum_scale", c_float), ("b_patch", c_void_p), ("b_bn", c_void_p)]


class Tn8Problem(Structure):
    """ap_tn8_problem (include/autoprog_hip.h)"""
    _fields_ = [("A", c_void_p), ("lda", c_int), ("B", c_void_p), ("ldb", c_int), ("C", c_void_p), ("ldc", c_int),
                ("M", c_int), ("N1", c_int), ("N2", c_int), ("a_fmt", c_int), ("alpha", c_float), ("dq_a", c_void_p), ("dq_b", c_void_p)]


class BnInput(Structure):
    """ap_bn_input (include/autoprog_hip.h)"""
    _fields_ = [("mean", c_void_p), ("rstd", c_void_p), ("gamma", c_void_p), ("beta", c_void_p)]


class LnReduce(Structure):
    """ap_ln_reduce (include/autoprog_hip.h)"""
    _fields_ = [("partial", c_void_p), ("n_partial", c_int), ("C", c_int), ("dgamma", c_void_p), ("dbeta", c_void_p)]


class InputPrepArgs(Structure):
    """ap_input_prep_args (include/autoprog_hip.h)"""
    _fields_ = [("u8", c_void_p), ("in_layout", c_int), ("B", c_int), ("Hi", c_int), ("Wi", c_int),
                ("out", c_void_p), ("out_layout", c_int), ("Ho", c_int), ("Wo", c_int),
                ("table", c_void_p), ("params", c_void_p), ("mix_enabled", c_int), ("boxes", c_void_p), ("boxes_host", c_void_p),
                ("n_boxes", c_int), ("erase_mode", c_int)]


class CropResizeArgs(Structure):
    """ap_crop_resize_args (include/autoprog_hip.h)"""
    _fields_ = [("u8", c_void_p), ("layout", c_int), ("B", c_int), ("Hi", c_int), ("Wi", c_int),
                ("out", c_void_p), ("S", c_int), ("records", c_void_p), ("records_host", c_void_p)]


class CropResampleArgs(Structure):
    """ap_crop_resample_args (include/autoprog_hip.h)"""
    _fields_ = CropResizeArgs._fields_


class RandAugArgs(Structure):
    """ap_randaug_args (include/autoprog_hip.h)"""
    _fields_ = [("u8", c_void_p), ("layout", c_int), ("B", c_int), ("S", c_int), ("out", c_void_p), ("scratch", c_void_p),
                ("records", c_void_p), ("records_host", c_void_p), ("n_layers", c_int), ("fill", ctypes.c_ubyte * 3)]


class LabelMapCropArgs(Structure):
    """ap_label_map_crop_args (include/autoprog_hip.h)"""
    _fields_ = [("scores", c_void_p), ("score_dtype", c_int), ("score_stride", c_int64), ("classes", c_void_p), ("class_dtype", c_int),
                ("class_stride", c_int64), ("labels", c_void_p), ("boxes", c_void_p), ("boxes_host", c_void_p), ("idx", c_void_p),
                ("val", c_void_p), ("dropped", c_void_p), ("B", c_int), ("Kin", c_int), ("Hm", c_int), ("Wm", c_int), ("P", c_int),
                ("K", c_int), ("C", c_int)]


class PatchMap(Structure):
    """ap_patch_map (include/autoprog_hip.h)"""
    _fields_ = [("group", c_int), ("group_stride", c_int), ("row_stride", c_int), ("kseg", c_int), ("kseg_stride", c_int)]


TN_MAX_GROUP = 32          # AP_TN_MAX_GROUP
TN_MAX_GROUP_DET = 8       # the deterministic mode (workspace) takes 8
BF8_COLSUM_SPLITS = 64     # AP_BF8_COLSUM_SPLITS: rows of the deterministic column-sum workspace of ap_quantize_bf8
FP8_E4M3, FP8_E5M2 = 0, 1  # AP_FP8_E4M3 / AP_FP8_E5M2
LN_MAX_BATCH = 12          # AP_LN_MAX_BATCH
PREP_MAX_BOXES = 8         # AP_PREP_MAX_BOXES
_P, _I, _L, _F = c_void_p, c_int, c_int64, c_float
_SIGNATURES = {
    "ap_abi_version": (c_int, []),
    "ap_error_string": (c_char_p, [_I]),
    "ap_cast_f32_bf16": (_I, [_P, _P, _L, _P]),
    "ap_cast_bf16_f32": (_I, [_P, _P, _L, _P]),
    "ap_cast_transpose_f32_bf16": (_I, [_P, _P, _I, _I, _I, _P]),
    "ap_resize_bilinear_nhwc": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "ap_droppath_masks": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "ap_layernorm_fwd": (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _F, _P]),
    "ap_layernorm_fwd_fp8": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _F, _P]),
    "ap_layernorm_bwd_workspace": (ctypes.c_size_t, [_L, _I]),
    "ap_layernorm_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _P, ctypes.c_size_t, _P]),
    "ap_layernorm_bwd_partial_pool": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, ctypes.c_size_t, POINTER(c_int), _P]),
    "ap_gemm_nt": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, POINTER(GemmEpilogue), _P]),
    "ap_gemm_tn_acc": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _P]),
    "ap_gemm_tn_grouped_workspace": (ctypes.c_size_t, [_P, _I]),
    "ap_gemm_tn_acc_grouped": (_I, [_P, _I, _P, ctypes.c_size_t, _P]),
    "ap_gemm_tn_acc_grouped_ln": (_I, [_P, _I, _P, _I, _P, ctypes.c_size_t, _P]),
    "ap_colsum_acc": (_I, [_P, _I, _P, _I, _I, _P]),
    "ap_outlook_fwd": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _I, _F, _P]),
    "ap_outlook_bwd": (_I, [_P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P]),
    "ap_avgpool2_fwd": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "ap_avgpool2_bwd_acc": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "ap_mhsa_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _F, _P, _P]),
    "ap_mhsa_bwd_workspace": (ctypes.c_size_t, [_I, _I, _I, _I]),
    "ap_mhsa_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P, ctypes.c_size_t, _P]),
    "ap_class_attn_fwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P]),
    "ap_class_attn_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P]),
    "ap_mix_token_swap": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ap_soft_ce_fwd_bwd": (_I, [_P, _I, _P, _L, _L, _L, _I, _P, _P, _F, _L, _I, _F, _I, _P]),
    "ap_soft_ce_sparse_fwd_bwd": (_I, [_P, _I, _P, _P, _I, _L, _L, _I, _F, _P, _P, _F, _L, _I, _F, _I, _P]),
    "ap_loss_combine": (_I, [_P, _L, _F, _P, _L, _F, _P, _P]),
    "ap_row_scale": (_I, [_P, _P, _P, _L, _I, _I, _P]),
    "ap_add_bcast": (_I, [_P, _P, _P, _L, _L, _P]),
    "ap_sum_reps_acc": (_I, [_P, _L, _L, _I, _P]),
    "ap_resample_grid": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _I, _I, _P]),
    "ap_bn_relu_workspace": (ctypes.c_size_t, [_L, _I]),
    "ap_bn_relu_fwd": (_I, [_P, _P, _P, _P, _P, _I, _F, _F, _P, _P, _P, _L, _I, _P, ctypes.c_size_t, _P]),
    "ap_bn_relu_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _P, ctypes.c_size_t, _P]),
    "ap_sumsq_workspace": (ctypes.c_size_t, []),
    "ap_sumsq_f32": (_I, [_P, _L, _P, _P, ctypes.c_size_t, _P]),
    "ap_adamw_ema_step": (_I, [_P, _P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _I, _F, _P, _F, _F, _P, POINTER(c_void_p), POINTER(c_float), _I, _P, _P]),
    "ap_mix_token_swap_dev": (_I, [_P, _P, _I, _I, _I, _I, _P, _I, _P]),
    "ap_soft_ce_fwd_bwd_dev": (_I, [_P, _I, _P, _L, _L, _L, _I, _P, _P, _F, _L, _I, _F, _I, _P, _P]),
    "ap_soft_ce_sparse_fwd_bwd_dev": (_I, [_P, _I, _P, _P, _I, _L, _L, _I, _F, _P, _P, _F, _L, _I, _F, _I, _P, _P]),
    "ap_batched_transpose_bf16": (_I, [_P, _P, _P, _I, _I, _P]),
}
_SIGNATURES["ap_resize_bilinear_s2d16"] = (_I, [_P, _P, _I, _I, _I, _I, _I, _P])
_SIGNATURES["ap_conv7_pack"] = (_I, [_P, _P, _P])
_SIGNATURES["ap_conv7_s2d_stat_rows"] = (_I, [_I, _I, _I])
_SIGNATURES["ap_conv7_s2d"] = (_I, [_P, _P, _P, _I, _I, _I, _P, _P])
_SIGNATURES["ap_conv7_s2d_wgrad_workspace"] = (ctypes.c_size_t, [_I, _I, _I])
_SIGNATURES["ap_conv7_s2d_wgrad"] = (_I, [_P, _P, _P, _I, _I, _I, _P, ctypes.c_size_t, _P])
_SIGNATURES["ap_layernorm_bwd_partial"] = (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _I, _P, ctypes.c_size_t, POINTER(c_int), _P])
_SIGNATURES["ap_layernorm_bwd_reduce_batched"] = (_I, [_P, _I, _P])
_SIGNATURES["ap_quantize_fp8"] = (_I, [_P, _P, _L, _P, _P, _P])
_SIGNATURES["ap_quantize_fp8_multi"] = (_I, [_P, _I, _P, _P, _P])
_SIGNATURES["ap_quantize_bf8"] = (_I, [_P, _P, _L, _P, _P, _P, _I, _I, _P, _F, _P, _P])
_SIGNATURES["ap_gemm_tn8_grouped_workspace"] = (ctypes.c_size_t, [_P, _I])
_SIGNATURES["ap_gemm_tn8_acc_grouped"] = (_I, [_P, _I, _P, ctypes.c_size_t, _P])
_SIGNATURES["ap_gemm_tn8_acc_grouped_ln"] = (_I, [_P, _I, _P, _I, _P, ctypes.c_size_t, _P])
_SIGNATURES["ap_debug_poison_lds"] = (_I, [ctypes.c_uint, _P, _P])
_SIGNATURES["ap_conv3x3_c64_bn"] = (_I, [_P, POINTER(BnInput), _P, _P, _I, _I, _I, _P, _P])
_SIGNATURES["ap_conv3x3_c64_wgrad_bn"] = (_I, [_P, POINTER(BnInput), _P, _P, _I, _I, _I, _P, ctypes.c_size_t, _P])
_SIGNATURES["ap_conv3x3_c64_bwd_stats"] = (_I, [_P, _P, _P, _I, _I, _I, _P, POINTER(BnInput), _P, _P])
_SIGNATURES["ap_bn_relu_bwd_act"] = (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _P, ctypes.c_size_t, _P])
_SIGNATURES["ap_bn_relu_bwd_partials"] = (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _L, _I, _P, ctypes.c_size_t, _P])
_SIGNATURES["ap_mhsa_fwd_fp8"] = (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P, _P])
_SIGNATURES["ap_gemm_nt_fp8"] = (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _P, POINTER(GemmEpilogue), _P])
_SIGNATURES["ap_mhsa_fwd_emits_fp8"] = (_I, [_I, _I])                  # (N, hd): csrc/attn_plan.h's plan of the ap_mhsa_fwd_fp8 launch
_SIGNATURES["ap_gemm_nt_q8_ok"] = (_I, [_I, _I, _I, _I, _I])          # (M, N, K, ldc, fp8): csrc/nt_plan.h's plan of the canonical q8 launch
_SIGNATURES["ap_gemm_nt_patch"] = (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _P, POINTER(PatchMap), _I, _P])
_SIGNATURES["ap_gemm_nt_patch_bn"] = (_I, [_P, POINTER(BnInput), _P, _I, _P, _I, _I, _I, _I, _P, POINTER(PatchMap), _I, _P])
_SIGNATURES["ap_bn_relu_fwd_partials"] = (_I, [_P, _P, _I, _P, _P, _P, _P, _F, _F, _P, _P, _P, _L, _I, _P])
_SIGNATURES["ap_conv3x3_c64_stat_rows"] = (_I, [_I, _I, _I])
_SIGNATURES["ap_conv3x3_c64_pack"] = (_I, [_P, _P, _P, _P])
_SIGNATURES["ap_conv3x3_c64"] = (_I, [_P, _P, _P, _I, _I, _I, _P, _P])
_SIGNATURES["ap_conv3x3_c64_wgrad_workspace"] = (ctypes.c_size_t, [_I, _I, _I])
_SIGNATURES["ap_conv3x3_c64_wgrad"] = (_I, [_P, _P, _P, _I, _I, _I, _P, ctypes.c_size_t, _P])
_SIGNATURES["ap_conv7_s2d_ld"] = (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P])
_SIGNATURES["ap_conv7_s2d_wgrad_ld"] = (_I, [_P, _P, _I, _P, _I, _I, _I, _P, ctypes.c_size_t, _P])
_SIGNATURES["ap_conv3x3_c128_pack"] = (_I, [_P, _P, _P, _P])
_SIGNATURES["ap_conv3x3_c128_stat_rows"] = (_I, [_I, _I, _I])
_SIGNATURES["ap_conv3x3_c128"] = (_I, [_P, _P, _P, _I, _I, _I, _P, _P])
_SIGNATURES["ap_conv3x3_c128_wgrad_workspace"] = (ctypes.c_size_t, [_I, _I, _I])
_SIGNATURES["ap_conv3x3_c128_wgrad"] = (_I, [_P, _P, _P, _I, _I, _I, _P, ctypes.c_size_t, _P])
# ap_sum_reps_acc(x, out, n, reps, stream)
_SIGNATURES["ap_sum_reps_acc"] = (_I, [_P, _P, _L, _I, _P])

_SIGNATURES["ap_mlp_fused"] = (_I, [POINTER(MlpFusedArgs), _P])
_SIGNATURES["ap_mlp_fused_infer"] = (_I, [POINTER(MlpFusedArgs), _P])
_SIGNATURES["ap_classify_stats"] = (_I, [_P, _I, _I, _P, _P, _P, _L, _P])
_SIGNATURES["ap_input_prep"] = (_I, [POINTER(InputPrepArgs), _P])
_SIGNATURES["ap_calib_copy"] = (_I, [_P, _P, _L, _P])
_SIGNATURES["ap_calib_mfma"] = (_I, [_P, _P, _I, _P])
# non-finite gradient guard (csrc/optim.hip): ap_grad_health(g, n, seg_off, n_seg, seg_sumsq, seg_nonfinite, state, beta1, beta2, ws, ws_bytes, stream)
_SIGNATURES["ap_grad_health_workspace"] = (ctypes.c_size_t, [_L, _I])
_SIGNATURES["ap_grad_health"] = (_I, [_P, _L, _P, _I, _P, _P, _P, _F, _F, _P, ctypes.c_size_t, _P])
_SIGNATURES["ap_adamw_ema_step_guarded"] = (_I, _SIGNATURES["ap_adamw_ema_step"][1][:-1] + [_P, _P])
# the step that also emits bf16 copies of EMA slabs: (... p_bf16, ema_bf16[4] (host array, null = not this copy), guard_or_null, stream)
_SIGNATURES["ap_adamw_ema_step_ema16"] = (_I, _SIGNATURES["ap_adamw_ema_step"][1][:-1] + [POINTER(c_void_p), _P, _P])
# the step with per-group learning rates and decays: wd_mask's place holds group_id (uint8 per element), and in front of the stream
# (... p_bf16, ema_bf16[4] or null, guard_or_null, group_tab_dev (n_groups x {lr, weight_decay} fp32), n_groups, stream)
_SIGNATURES["ap_adamw_ema_step_groups"] = (_I, _SIGNATURES["ap_adamw_ema_step_ema16"][1][:-1] + [_P, _I, _P])
# row-wise softmax + top-K (csrc/topk.hip): ap_softmax_topk_rows(logits, ld, C, K, inv_temp, idx, val, o_sb, o_sn, rows_per_batch, M, stream)
_SIGNATURES["ap_softmax_topk_rows"] = (_I, [_P, _I, _I, _I, _F, _P, _P, _L, _L, _I, _L, _P])
# distillation loss (csrc/distill.hip): ap_distill_fwd_bwd(student, ld_s, teacher, ld_t, C, mode, inv_temp, row_loss, dstudent, grad_scale, M, stream)
_SIGNATURES["ap_distill_fwd_bwd"] = (_I, [_P, _I, _P, _I, _I, _I, _F, _P, _P, _F, _L, _P])
# class rows of TokenLabelGTCrossEntropy on the sparse target (csrc/softce.hip): ap_soft_ce_sparse_gt_fwd_bwd(logits, ldx, idx, val, K, p_sb, p_s0,
# p_s1, smoothing, row_loss, dlogits, grad_scale, B, C, mix_lam, mix_batches, mix_lam_dev, stream)
_SIGNATURES["ap_soft_ce_sparse_gt_fwd_bwd"] = (_I, [_P, _I, _P, _P, _I, _L, _L, _L, _F, _P, _P, _F, _L, _I, _F, _I, _P, _P])
# per-image crop box + flip + bilinear resize of a uint8 batch (csrc/crop.hip)
_SIGNATURES["ap_crop_resize_u8"] = (_I, [POINTER(CropResizeArgs), _P])
# the same with Pillow's antialiased bilinear / bicubic filters, byte for byte (csrc/resample.hip)
_SIGNATURES["ap_crop_resample_u8"] = (_I, [POINTER(CropResampleArgs), _P])
# RandAugment's ops on a uint8 batch, one launch per layer, byte for byte Pillow's (csrc/randaug.hip)
_SIGNATURES["ap_randaug_u8"] = (_I, [POINTER(RandAugArgs), _P])
# stored top-k label maps -> the pairs of a SparseTokenLabelTarget, ROI-aligned to each image's crop box (csrc/labelmap.hip)
_SIGNATURES["ap_label_map_crop"] = (_I, [POINTER(LabelMapCropArgs), _P])
# adaptive gradient clipping on the gradient slab (csrc/agc.hip): ap_agc_clip(g, p, n, unit_off, unit_skip, n_units, clip_factor, eps,
# grad_scale, unit_factor_or_null, counts_or_null, stream)
_SIGNATURES["ap_agc_clip"] = (_I, [_P, _P, _L, _P, _P, _I, _F, _F, _F, _P, _P, _P])
_SIGNATURES["ap_agc_short_max"] = (_I, [])
# fused LAMB + EMA step with per-tensor trust ratios (csrc/lamb.hip): ap_lamb_ema_step(p, g, m, v, group_id, n, beta1, beta2, eps, step,
# grad_scale, gnorm_sq, max_norm, clip_value, step_scalars_dev, ema[], ema_decay[], n_ema, p_bf16, ema_bf16[4] or null, guard_or_null,
# group_tab_dev, n_groups, chunk_tab_dev, n_chunks, tensor_first_dev, n_tensors, always_adapt, trust_clip, trust_out, workspace, ws_bytes,
# grid_cap, passes, stream)
_SIGNATURES["ap_lamb_chunk"] = (_I, [])
_SIGNATURES["ap_lamb_workspace"] = (ctypes.c_size_t, [_I])
_SIGNATURES["ap_lamb_ema_step"] = (_I, [_P, _P, _P, _P, _P, _L, _F, _F, _F, _I, _F, _P, _F, _F, _P, POINTER(c_void_p), POINTER(c_float), _I, _P,
                                        POINTER(c_void_p), _P, _P, _I, _P, _I, _P, _I, _I, _I, _P, _P, ctypes.c_size_t, _I, _I, _P])

EXPORTED_SYMBOLS = tuple(_SIGNATURES.keys())
EXPECTED_ABI = 7                     # ap_abi_version() of the library these ctypes Structures mirror (include/autoprog_hip.h)


class AutoProgHipError(RuntimeError):
    pass


def _load():
    if not os.path.isfile(LIB_PATH):
        raise AutoProgHipError(
            "libautoprog_hip.so is missing (%s). Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C autoprog_amd/csrc`; there is no CPU/PyTorch fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    lib.ap_abi_version.restype = ctypes.c_int
    got = lib.ap_abi_version()
    if got != EXPECTED_ABI:          # (a stale or ablation .so with every symbol but older structs would read garbage past their end)
        raise AutoProgHipError("%s has ABI version %d, these bindings were written for %d: rebuild it (make -C autoprog_amd/csrc)"
                               % (LIB_PATH, got, EXPECTED_ABI))
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the ABI lost a symbol
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def check(code, what):
    if code != 0:
        raise AutoProgHipError("%s failed: %s (code %d)" % (what, lib.ap_error_string(code).decode(), code))
