"""Tensor-level wrappers over the C ABI (include/autoprog_hip.h).

Every function takes/returns torch CUDA tensors, allocates outputs with torch (device memory
and streams are PyTorch plumbing), and enqueues the gfx950 kernel on the current stream.
There is no fallback path: a CPU tensor or a missing library raises.
"""
import ctypes
import math
import os
from collections import namedtuple

import torch

from . import _lib
from ._lib import CropResampleArgs, CropResizeArgs, GemmEpilogue, InputPrepArgs, LabelMapCropArgs, LnReduce, RandAugArgs, TnProblem, LN_MAX_BATCH, PREP_MAX_BOXES, TN_MAX_GROUP, TN_MAX_GROUP_DET, AutoProgHipError, check, lib

BF16 = torch.bfloat16


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """the current stream's handle.  torch.cuda.current_stream() builds a Stream object through five Python layers (9 us a call,
    ~4 ms of host time per training step at ~440 launches -- the launching thread was at 82 % of the GPU's step time); the raw
    accessor the torch compiler stack uses costs 0.3 us and follows torch.cuda.stream() contexts the same way."""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def _req_fail(t, dtype, name):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise AutoProgHipError("%s must be a CUDA tensor (the HIP path has no CPU fallback)" % name)
    if t.dtype != dtype:
        raise AutoProgHipError("%s must be %s, got %s" % (name, dtype, t.dtype))
    raise AutoProgHipError("%s must be contiguous" % name)


def _req(t, dtype, name):
    """every tensor that goes to the library: CUDA, the kernel's dtype, contiguous (one expression on the hot path: ~1900 calls per step)"""
    try:
        ok = t.dtype is dtype and t.is_cuda and t.is_contiguous()
    except AttributeError:
        ok = False
    if not ok:
        _req_fail(t, dtype, name)
    return t


def round_up(v, m):
    return (v + m - 1) // m * m


# ------------------------------------------------------------------------------- calibration probes (bench.py `calibration`)
def calib_copy(src, dst):
    """dst <- src, 16 bytes per lane (the float4 copy the HBM figure of MI355X_MICROARCH.md is quoted on)"""
    if not (src.is_cuda and dst.is_cuda and src.is_contiguous() and dst.is_contiguous()) or src.numel() * src.element_size() != dst.numel() * dst.element_size():
        raise AutoProgHipError("calib_copy: two contiguous CUDA tensors of equal size")
    check(lib.ap_calib_copy(src.data_ptr(), dst.data_ptr(), src.numel() * src.element_size(), _stream()), "ap_calib_copy")


def calib_mfma(seed, sink, iters):
    """register-only bf16 MFMA loop on every CU; -> FLOP of the launch"""
    _req(seed, BF16, "seed")
    _req(sink, torch.float32, "sink")
    if seed.numel() < 2048:
        raise AutoProgHipError("calib_mfma: seed holds at least 2048 bf16")
    check(lib.ap_calib_mfma(seed.data_ptr(), sink.data_ptr(), int(iters), _stream()), "ap_calib_mfma")
    return 256.0 * 4 * iters * 16 * 16384


# ------------------------------------------------------------------------------------ casts
def cast_bf16(src):
    _req(src, torch.float32, "src")
    dst = torch.empty(src.shape, dtype=BF16, device=src.device)
    check(lib.ap_cast_f32_bf16(src.data_ptr(), dst.data_ptr(), src.numel(), _stream()), "ap_cast_f32_bf16")
    return dst


def cast_f32(src):
    _req(src, BF16, "src")
    dst = torch.empty(src.shape, dtype=torch.float32, device=src.device)
    check(lib.ap_cast_bf16_f32(src.data_ptr(), dst.data_ptr(), src.numel(), _stream()), "ap_cast_bf16_f32")
    return dst


def cast_transpose_bf16(w):
    """fp32 [rows, cols] -> bf16 [cols, round_up(rows, 8)] (pad columns zero)."""
    _req(w, torch.float32, "w")
    rows, cols = w.shape
    ld = round_up(rows, 8)
    dst = torch.empty((cols, ld), dtype=BF16, device=w.device)
    check(lib.ap_cast_transpose_f32_bf16(w.data_ptr(), dst.data_ptr(), rows, cols, ld, _stream()), "ap_cast_transpose_f32_bf16")
    return dst


def resize_bilinear_nhwc(x, size):
    """fp32 NCHW batch -> bf16 NHWC batch bilinearly resized to (size, size) (F.interpolate(..., mode='bilinear', align_corners=False),
    main_prog.py:973); size equal to the input size is the plain layout change + cast"""
    _req(x, torch.float32, "x")
    B, C, Hi, Wi = x.shape
    y = torch.empty((B, size, size, C), dtype=BF16, device=x.device)
    check(lib.ap_resize_bilinear_nhwc(x.data_ptr(), y.data_ptr(), B, C, Hi, Wi, size, size, _stream()), "ap_resize_bilinear_nhwc")
    return y


def droppath_masks(uniform, keep, tokens=0):
    """uniform fp32 [sites,B], keep fp32 [sites] -> (factor [sites,B], mask [sites,B], token_mask bf16 [sites,row] or None): one launch"""
    _req(uniform, torch.float32, "uniform"); _req(keep, torch.float32, "keep")
    sites, B = uniform.shape
    factor = torch.empty_like(uniform)
    mask = torch.empty_like(uniform)
    row = round_up(B * tokens, 8) if tokens else 0
    tm = torch.empty((sites, row), dtype=BF16, device=uniform.device) if tokens else None
    check(lib.ap_droppath_masks(uniform.data_ptr(), keep.data_ptr(), factor.data_ptr(), mask.data_ptr(), tm.data_ptr() if tm is not None else None,
                                sites, B, int(tokens), row, _stream()), "ap_droppath_masks")
    return factor, mask, tm


# -------------------------------------------------------------------------------- layernorm
def layernorm_fwd(x, gamma, beta, eps, fp8=None):
    """-> (y, mean, rstd); fp8 = (scale, amax) device scalars: -> (y, mean, rstd, y8) with y8 = e4m3 bytes of y * scale[0] and
    amax[0] raised to max |y| (what quantize_fp8(y, scale, amax) returns, without its pass over y)"""
    _req(x, BF16, "x"); _req(gamma, torch.float32, "gamma"); _req(beta, torch.float32, "beta")
    C = x.shape[-1]
    rows = x.numel() // C
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    if fp8 is not None:
        scale, amax = fp8
        y8 = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
        check(lib.ap_layernorm_fwd_fp8(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), y8.data_ptr(), scale.data_ptr(),
                                       amax.data_ptr() if amax is not None else None, mean.data_ptr(), rstd.data_ptr(),
                                       rows, C, float(eps), _stream()), "ap_layernorm_fwd_fp8")
        return y, mean, rstd, y8
    check(lib.ap_layernorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                               rows, C, float(eps), _stream()), "ap_layernorm_fwd")
    return y, mean, rstd


_ln_ws = {}          # (rows, C) -> ap_layernorm_bwd_workspace bytes (a pure function of the shape: one foreign call per shape, not per launch)


# a deferred LayerNorm dgamma / dbeta reduction (what layernorm_bwd(..., defer=...) appends): `n_partial` partial rows of width C in the fp32
# workspace `partial`, summed into dgamma / dbeta by layernorm_bwd_reduce_batched or by the weight-gradient launch it rides in
LnRider = namedtuple("LnRider", "partial n_partial C dgamma dbeta")


def layernorm_bwd(dy, x, gamma, mean, rstd, dres, dgamma, dbeta, defer=None, pool=None):
    """dx = dres + dLN/dx ; dgamma/dbeta (fp32) are accumulated in place.  defer: a list -- the dgamma/dbeta reduction is not
    launched but appended to it (layernorm_bwd_reduce_batched reduces the LayerNorms of a block in one launch).
    pool = (dpooled [B,h,w,C], (B, H, W)) with defer: the LayerNorm output also fed a 2 x 2 ceil-mode average pool whose output gradient is
    dpooled -- its backward is applied to dy inside the kernel; -> None where that kernel does not apply (the caller falls back)"""
    _req(dy, BF16, "dy"); _req(x, BF16, "x")
    C = x.shape[-1]
    rows = x.numel() // C
    dx = torch.empty_like(x)
    ws_bytes = _ln_ws.get((rows, C))
    if ws_bytes is None:
        ws_bytes = _ln_ws[(rows, C)] = lib.ap_layernorm_bwd_workspace(rows, C)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device)
    if pool is not None:
        dp, (B_, H_, W_) = pool
        _req(dp, BF16, "dpooled")
        if defer is None or B_ * H_ * W_ != rows:
            raise AutoProgHipError("layernorm_bwd(pool=...) needs defer and a [B,H,W,C] token grid")
        n = ctypes.c_int(0)
        rc = lib.ap_layernorm_bwd_partial_pool(dy.data_ptr(), dp.data_ptr(), B_, H_, W_, x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                               dres.data_ptr() if dres is not None else None, dx.data_ptr(), C, ws.data_ptr(), ws_bytes, ctypes.byref(n), _stream())
        if rc == -2:                   # AP_ERR_UNSUPPORTED
            return None
        check(rc, "ap_layernorm_bwd_partial_pool")
        defer.append(LnRider(ws, n.value, C, dgamma, dbeta))
        return dx
    if defer is not None and rows > 0:
        n = ctypes.c_int(0)
        check(lib.ap_layernorm_bwd_partial(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                           dres.data_ptr() if dres is not None else None, dx.data_ptr(), rows, C, ws.data_ptr(), ws_bytes,
                                           ctypes.byref(n), _stream()), "ap_layernorm_bwd_partial")
        defer.append(LnRider(ws, n.value, C, dgamma, dbeta))
        return dx
    check(lib.ap_layernorm_bwd(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                               dres.data_ptr() if dres is not None else None, dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                               rows, C, ws.data_ptr(), ws_bytes, _stream()), "ap_layernorm_bwd")
    return dx


def _ln_reduce_array(items):
    """the ap_ln_reduce table of a launch that carries these deferred reductions"""
    arr = (LnReduce * len(items))()
    for q, (ws, n, C, dg, db) in zip(arr, items):
        q.partial, q.n_partial, q.C, q.dgamma, q.dbeta = ws.data_ptr(), n, C, dg.data_ptr(), db.data_ptr()
    return arr


def layernorm_bwd_reduce_batched(items):
    """items: the entries layernorm_bwd(..., defer=items) appended; one launch per LN_MAX_BATCH LayerNorms"""
    for i0 in range(0, len(items), LN_MAX_BATCH):
        chunk = items[i0:i0 + LN_MAX_BATCH]
        check(lib.ap_layernorm_bwd_reduce_batched(ctypes.cast(_ln_reduce_array(chunk), ctypes.c_void_p), len(chunk), _stream()), "ap_layernorm_bwd_reduce_batched")


# ------------------------------------------------------------------------------------- gemm
GELU_CODE_SCALE, GELU_CODE_ZERO = 202.0, 26.0       # the 8-bit derivative codes of gelu = 3 (include/autoprog_hip.h): gelu' = (code - 26) / 202


GELU_TABLE_FALLBACKS = 0       # gemm_nt(gelu="table") launches the library refused and that ran as mode 3 with a side buffer of their own


def _gelu_mode(gelu, preact_grad, preact_out):
    """ap_gemm_epilogue.gelu: 1 stores h, 2 gelu'(h) as bf16, 3 gelu'(h) as 8-bit codes (preact_out then is a uint8 tensor);
    gelu = "table": 4, the value of mode 3 and no side store (forward-only passes)"""
    if not gelu:
        return 0
    if isinstance(gelu, str):
        if gelu != "table" or preact_out is not None or preact_grad:
            raise AutoProgHipError('gemm_nt: gelu="table" is the forward-only mode: no preact_out, no preact_grad')
        return 4
    mode = 1 + int(preact_grad)
    if mode == 3 and (preact_out is None or preact_out.dtype != torch.uint8):
        raise AutoProgHipError("gemm_nt: preact_grad = 2 stores 8-bit codes: preact_out must be a uint8 tensor")
    if mode != 3 and preact_out is not None and preact_out.dtype != BF16:
        raise AutoProgHipError("gemm_nt: preact_out must be bf16 (uint8 only with preact_grad = 2)")
    return mode


def mlp_fused_ok(M, C, hidden):
    """does ap_mlp_fused take this MLP?  (csrc/mlp_fused.hip: C = 384, hidden = 3 C, whole 128-row blocks)"""
    return C == 384 and hidden == 3 * C and M % 128 == 0 and M > 0


def _mlp_fused_args(x, wa, wb, bias1, bias2, row_scale_hidden, row_scale_out, rows_per_scale, residual, ln):
    """what mlp_fused and mlp_fused_infer hand to the library alike: -> (MlpFusedArgs without side outputs and direction, out [M, C], the rows read:
    x, or ln[0]), or None where mlp_fused_ok refuses the shape"""
    from ._lib import MlpFusedArgs
    if ln is not None:
        x = _req(ln[0], BF16, "ln rows")
    _req(x, BF16, "x"); _req(wa, BF16, "wa"); _req(wb, BF16, "wb")
    M, C = x.shape
    H = wa.shape[0]
    if not mlp_fused_ok(M, C, H):
        return None
    out = torch.empty((M, C), dtype=BF16, device=x.device)
    a = MlpFusedArgs()
    a.x, a.ldx = x.data_ptr(), x.shape[1]
    a.wa, a.ldwa = wa.data_ptr(), wa.shape[1]
    a.wb, a.ldwb = wb.data_ptr(), wb.shape[1]
    a.out, a.ldo = out.data_ptr(), C
    a.hidden_out, a.ldh, a.codes = None, H, None
    a.bias1 = _req(bias1, torch.float32, "bias1").data_ptr() if bias1 is not None else None
    a.bias2 = _req(bias2, torch.float32, "bias2").data_ptr() if bias2 is not None else None
    a.row_scale_hidden = _req(row_scale_hidden, torch.float32, "row_scale_hidden").data_ptr() if row_scale_hidden is not None else None
    a.row_scale_out = _req(row_scale_out, torch.float32, "row_scale_out").data_ptr() if row_scale_out is not None else None
    a.rows_per_scale = int(rows_per_scale)
    if residual is not None:
        _req(residual, BF16, "residual")
        a.residual, a.ldr = residual.data_ptr(), residual.shape[1]
    a.m, a.c, a.hidden = M, C, H
    if ln is not None:
        a.x = None
        a.ln_in, a.ld_ln = x.data_ptr(), C
        a.ln_gamma, a.ln_beta = _req(ln[1], torch.float32, "ln gamma").data_ptr(), _req(ln[2], torch.float32, "ln beta").data_ptr()
        a.ln_eps = float(ln[3])
    return a, out, x


def mlp_fused_infer(x, wa, wb, bias1=None, bias2=None, row_scale_hidden=None, row_scale_out=None, rows_per_scale=1, residual=None, ln=None):
    """the forward of mlp_fused for a pass no backward follows (ap_mlp_fused_infer): -> out [M, C], bit-identical to mlp_fused(...)[0]; the hidden
    activation, the gelu' codes and LN(rows) / mean / rstd are neither allocated nor written.  ln = (rows, gamma, beta, eps) with x = None as in mlp_fused.
    -> None when the library does not take the launch"""
    args = _mlp_fused_args(x, wa, wb, bias1, bias2, row_scale_hidden, row_scale_out, rows_per_scale, residual, ln)
    if args is None:
        return None
    a, out, _ = args
    a.backward = 0
    code = lib.ap_mlp_fused_infer(ctypes.byref(a), _stream())
    if code == -2:                    # AP_ERR_UNSUPPORTED
        return None
    check(code, "ap_mlp_fused_infer")
    return out


def mlp_fused(x, wa, wb, backward=False, bias1=None, bias2=None, row_scale_hidden=None, row_scale_out=None, rows_per_scale=1,
              residual=None, codes=None, ln=None):
    """the MLP of a block in one launch (include/autoprog_hip.h ap_mlp_fused).
    forward : x [M, C], wa = fc1 weight [H, C], wb = fc2 weight [C, H] -> (out [M, C], a [M, H] = gelu(.) * row_scale_hidden, codes [M, H] uint8)
    backward: x = dL/dout, wa = fc2 weight^T copy [H, ld(C)], wb = fc1 weight^T copy [C, ld(H)], codes = the forward's -> (dL/dx [M, C], dL/dh [M, H], codes)
    ln = (rows [M, C], gamma, beta, eps) (forward; x = None): the LayerNorm in front of fc1 runs inside the launch, bit-identical to
    layernorm_fwd -> (out, a, codes, LN(rows), mean, rstd)
    -> None when the library does not take the launch (the caller issues the two ap_gemm_nt launches)"""
    args = _mlp_fused_args(x, wa, wb, bias1, bias2, row_scale_hidden, row_scale_out, rows_per_scale, residual, ln)
    if args is None:
        return None
    a, out, x = args
    M, C, H = a.m, a.c, a.hidden
    hid = torch.empty((M, H), dtype=BF16, device=x.device)
    if backward:
        _req(codes, torch.uint8, "codes")
    else:
        codes = torch.empty((M, H), dtype=torch.uint8, device=x.device)
    a.hidden_out, a.codes, a.backward = hid.data_ptr(), codes.data_ptr(), 1 if backward else 0
    if ln is not None:
        xn = torch.empty((M, C), dtype=BF16, device=x.device)
        mean = torch.empty(M, dtype=torch.float32, device=x.device)
        rstd = torch.empty(M, dtype=torch.float32, device=x.device)
        a.ln_out, a.ld_lno, a.ln_mean, a.ln_rstd = xn.data_ptr(), C, mean.data_ptr(), rstd.data_ptr()
    code = lib.ap_mlp_fused(ctypes.byref(a), _stream())
    if code == -2:                    # AP_ERR_UNSUPPORTED (e.g. the GELU table cannot be built inside a stream capture)
        return None
    check(code, "ap_mlp_fused")
    if ln is not None:
        return out, hid, codes, xn, mean, rstd
    return out, hid, codes


_q8_ok = {}         # (M, N, K, ldc, fp8) -> ap_gemm_nt_q8_ok (a pure function of the shape in one process: one foreign call per shape, not per launch)


def _gemm_nt_q8_ok(M, N, K, fp8):
    key = (M, N, K, round_up(N, 8), fp8)            # (the ldc of gemm_nt / gemm_nt_fp8 when they allocate `out`)
    ok = _q8_ok.get(key)
    if ok is None:
        ok = _q8_ok[key] = bool(lib.ap_gemm_nt_q8_ok(*key))
    return ok


def gemm_nt_emits_q8(M, N, K, mul_by):
    """can a bf16 gemm_nt launch of these dimensions write its output a second time as e4m3 (q8=)?  The mul_by8 flavours of the 8-phase
    kernel (the input gradient of fc2): the library's own launch plan answers (csrc/nt_plan.h)"""
    return mul_by is not None and mul_by.dtype == torch.uint8 and _gemm_nt_q8_ok(M, N, K, 0)


def gemm_nt(a, b, n=None, k=None, bias=None, gelu=False, preact_out=None, dgelu_of=None, row_scale=None,
            rows_per_scale=1, residual=None, out=None, ldc=None, preact_grad=False, mul_by=None, q8=None):
    """out[M, :n] = epilogue(a[M, :k] @ b[:n, :k]^T); a/b bf16 2-D (row stride = shape[1]).
    preact_grad: with gelu, preact_out receives gelu'(h) instead of h (True / 1: bf16; 2: 8-bit codes, preact_out uint8); its backward
    passes that tensor as mul_by (a uint8 tensor is taken as the codes).
    gelu = "table" (forward-only passes): out holds exactly what the preact_grad = 2 launch stores there and no side tensor exists; where the
    library has no such kernel for the launch (AP_ERR_UNSUPPORTED) it runs as that launch with a side buffer allocated and dropped here.
    q8 = (scale, amax) (gemm_nt_emits_q8 launches): -> (out, out8), out8 = the e4m3 bytes of out * scale[0], amax[0] raised to max |out|"""
    _req(a, BF16, "a"); _req(b, BF16, "b")
    M = a.shape[0]
    n = b.shape[0] if n is None else n
    k = a.shape[1] if k is None else k
    if out is None:
        ldc = round_up(n, 8) if ldc is None else ldc
        out = torch.empty((M, ldc), dtype=BF16, device=a.device)
    else:
        ldc = out.shape[1]
    if preact_out is not None and not gelu:
        raise AutoProgHipError("gemm_nt: preact_out is the GELU launches' side output (pass gelu=True)")
    if bias is None and not gelu and dgelu_of is None and mul_by is None and row_scale is None and residual is None:
        epi_ref = None                                            # plain product: the library takes a null epilogue
    else:
        epi = GemmEpilogue()
        epi.bias = bias.data_ptr() if bias is not None else None
        epi.gelu = _gelu_mode(gelu, preact_grad, preact_out)
        epi.preact_out = preact_out.data_ptr() if preact_out is not None else None
        epi.dgelu_of = dgelu_of.data_ptr() if dgelu_of is not None else None
        if mul_by is not None and mul_by.dtype == torch.uint8:
            if mul_by.shape[-1] != ldc or not mul_by.is_contiguous():
                raise AutoProgHipError("gemm_nt: the derivative codes must be contiguous [M, ldc] bytes")
            epi.mul_by, epi.mul_by8 = None, mul_by.data_ptr()
        else:
            epi.mul_by = mul_by.data_ptr() if mul_by is not None else None
        epi.row_scale = row_scale.data_ptr() if row_scale is not None else None
        epi.rows_per_scale = int(rows_per_scale)
        epi.residual = residual.data_ptr() if residual is not None else None
        epi.ldr = residual.shape[1] if residual is not None else 0
        epi_ref = ctypes.byref(epi)
    out8 = None
    if q8 is not None:
        if epi_ref is None:
            raise AutoProgHipError("gemm_nt: q8 exists for the mul_by (8-bit codes) launches only")
        out8 = torch.empty((M, ldc), dtype=torch.uint8, device=a.device)
        epi.q8_out, epi.q8_scale, epi.q8_amax = out8.data_ptr(), q8[0].data_ptr(), (q8[1].data_ptr() if q8[1] is not None else None)
    code = lib.ap_gemm_nt(a.data_ptr(), a.shape[1], b.data_ptr(), b.shape[1], out.data_ptr(), ldc, M, n, k, epi_ref, _stream())
    if code == -2 and epi_ref is not None and epi.gelu == 4:
        global GELU_TABLE_FALLBACKS
        GELU_TABLE_FALLBACKS += 1
        side = torch.empty((M, ldc), dtype=torch.uint8, device=a.device)
        epi.gelu, epi.preact_out = 3, side.data_ptr()
        code = lib.ap_gemm_nt(a.data_ptr(), a.shape[1], b.data_ptr(), b.shape[1], out.data_ptr(), ldc, M, n, k, epi_ref, _stream())
    check(code, "ap_gemm_nt")
    return out if q8 is None else (out, out8)


FP8_MAX = 448.0          # OCP e4m3


def quantize_fp8(x, scale, amax=None):
    """bf16 tensor (numel % 16 == 0) -> uint8 tensor of e4m3 bytes, y = sat(x * scale[0]); scale / amax: fp32 device scalars
    (amax[0] = max(amax[0], max|x|): the statistic the NEXT step's scale is derived from -- delayed scaling)"""
    _req(x, BF16, "x"); _req(scale, torch.float32, "scale")
    y = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    check(lib.ap_quantize_fp8(x.data_ptr(), y.data_ptr(), x.numel(), scale.data_ptr(), amax.data_ptr() if amax is not None else None,
                              _stream()), "ap_quantize_fp8")
    return y


def quantize_fp8_multi(table, njobs, scales, amax):
    """table: int64 [njobs, 4] device tensor of ap_fp8_job records (x pointer, y pointer, n, slot); one launch for all of them"""
    _req(table, torch.int64, "table"); _req(scales, torch.float32, "scales")
    check(lib.ap_quantize_fp8_multi(table.data_ptr(), int(njobs), scales.data_ptr(), amax.data_ptr() if amax is not None else None, _stream()),
          "ap_quantize_fp8_multi")


BF8_MAX = 57344.0        # OCP e5m2


def quantize_bf8(g, scale, amax=None, colsum=None, colsum_weight=None, colsum_scale=1.0):
    """bf16 output gradient g [rows, cols] -> uint8 tensor of e5m2 bytes, y = sat(g * scale[0]); amax[0] = max(amax[0], max|g|).
    colsum (fp32 [cols], optional): += colsum_scale * sum_r w[r] * g[r, :] of the UN-quantised g (the bias gradient, in the same pass),
    w = colsum_weight (bf16 per-row weights, e.g. the DropPath token mask; None = ones, colsum_scale then unused).  Under
    `deterministic` the row splits' sums are added in split order."""
    from ._lib import BF8_COLSUM_SPLITS
    _req(g, BF16, "g"); _req(scale, torch.float32, "scale")
    y = torch.empty(g.shape, dtype=torch.uint8, device=g.device)
    rows, cols = (g.shape[0], g.shape[1]) if g.dim() == 2 else (1, g.numel())
    ws = None
    if colsum is not None:
        _req(colsum, torch.float32, "colsum")
        if g.dim() != 2 or colsum.numel() < cols:
            raise AutoProgHipError("quantize_bf8: colsum needs a 2-D g and cols entries")
        if colsum_weight is not None:
            _req(colsum_weight, BF16, "colsum_weight")
            if colsum_weight.numel() < rows:
                raise AutoProgHipError("quantize_bf8: colsum_weight needs one entry per row")
        if deterministic:
            ws = torch.empty(BF8_COLSUM_SPLITS * cols, dtype=torch.float32, device=g.device)
    check(lib.ap_quantize_bf8(g.data_ptr(), y.data_ptr(), g.numel(), scale.data_ptr(), amax.data_ptr() if amax is not None else None,
                              colsum.data_ptr() if colsum is not None else None, rows, cols,
                              colsum_weight.data_ptr() if colsum_weight is not None else None, float(colsum_scale),
                              ws.data_ptr() if ws is not None else None, _stream()), "ap_quantize_bf8")
    return y


def gemm_tn8_ok(n1, n2):
    """widths the fp8 weight-gradient kernel takes (ap_gemm_tn8_acc_grouped): multiples of 128"""
    return n1 % 128 == 0 and n2 % 128 == 0 and n1 > 0 and n2 > 0


def _tiles_192(prob):
    """tiles a weight-gradient problem takes in the table of the 192 x 192-tile kernel (restates tn8_fits() in csrc/gemm.hip)"""
    n1 = prob.c.shape[0] if prob.n1 is None else prob.n1
    n2 = prob.c.shape[1] if prob.n2 is None else prob.n2
    if n1 % 192 or n2 % 192 or prob.a.shape[0] % 64 or prob.a.shape[0] < 4096 or prob.b_patch is not None:
        return 0                      # not a problem of the 192 x 192-tile kernel: rides along, costs no slot
    return (n1 // 192) * (n2 // 192)


class WgradProblem(namedtuple("WgradProblem", "a b c n1 n2 colsum colsum_weight colsum_scale alpha b_patch b_bn", defaults=(None, 1.0, 1.0, None, None))):
    """a bf16 weight-gradient problem: the fields as gemm_tn_acc_grouped describes them"""
    __slots__ = ()
    tiles_192 = _tiles_192


class Tn8Problem(namedtuple("Tn8Problem", "a b c n1 n2 dq_a dq_b alpha a_fmt", defaults=(1.0, 1))):
    """an fp8 weight-gradient problem for gemm_tn8_acc_grouped / gemm_tn_acc_grouped:
    c[:n1, :n2] += alpha * dq_a[0] * dq_b[0] * a^T b with a [M, n1] e5m2 bytes (a_fmt = FP8_E5M2; e4m3 with FP8_E4M3) and b
    [M, n2] e4m3 bytes; dq_* fp32 device scalars.  No column sum (quantize_bf8 forms the bias gradient), no patch addressing."""
    __slots__ = ()
    colsum = b_patch = None
    tiles_192 = _tiles_192


def gemm_tn8_acc_grouped(problems, ln=None):
    """ONE launch of the fp8 weight-gradient kernel for a list of Tn8Problem (at most TN_MAX_GROUP); ln: deferred LayerNorm reductions
    riding in the launch (at most LN_MAX_BATCH).  Deterministic mode as for gemm_tn_acc_grouped."""
    ln = list(ln) if ln else []
    if len(problems) > TN_MAX_GROUP or len(ln) > LN_MAX_BATCH:
        raise AutoProgHipError("gemm_tn8_acc_grouped: at most %d problems and %d LayerNorm reductions" % (TN_MAX_GROUP, LN_MAX_BATCH))
    arr = (_lib.Tn8Problem * len(problems))()
    for q, prob in zip(arr, problems):
        a8, b8, c, n1, n2, dq_a, dq_b = prob.a, prob.b, prob.c, prob.n1, prob.n2, prob.dq_a, prob.dq_b
        _req(a8, torch.uint8, "a8"); _req(b8, torch.uint8, "b8"); _req(c, torch.float32, "c")
        _req(dq_a, torch.float32, "dq_a"); _req(dq_b, torch.float32, "dq_b")
        if a8.shape[0] != b8.shape[0]:
            raise ValueError("gemm_tn8_acc_grouped: token counts differ")
        q.A, q.lda, q.B, q.ldb, q.C, q.ldc = a8.data_ptr(), a8.shape[1], b8.data_ptr(), b8.shape[1], c.data_ptr(), c.shape[1]
        q.M, q.N1, q.N2 = a8.shape[0], (c.shape[0] if n1 is None else n1), (c.shape[1] if n2 is None else n2)
        q.a_fmt, q.alpha, q.dq_a, q.dq_b = int(prob.a_fmt), float(prob.alpha), dq_a.data_ptr(), dq_b.data_ptr()
    ptr = ctypes.cast(arr, ctypes.c_void_p)
    ws, ws_bytes = None, 0
    if deterministic:
        ws_bytes = lib.ap_gemm_tn8_grouped_workspace(ptr, len(problems))
        ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=problems[0].a.device)
    check(lib.ap_gemm_tn8_acc_grouped_ln(ptr, len(problems), ctypes.cast(_ln_reduce_array(ln), ctypes.c_void_p) if ln else None, len(ln),
                                         ws.data_ptr() if ws is not None else None, ws_bytes, _stream()), "ap_gemm_tn8_acc_grouped_ln")


def poison_lds(pattern=0x7FC07FC0):
    """test aid: every CU's LDS filled with `pattern` (default: bf16 NaN pairs)"""
    scratch = torch.zeros(2, dtype=torch.int32, device="cuda")
    check(lib.ap_debug_poison_lds(int(pattern) & 0xFFFFFFFF, scratch.data_ptr(), _stream()), "ap_debug_poison_lds")
    return scratch


def quantize_fp8_now(x):
    """current scaling (one extra pass for the amax): -> (bytes, dequantisation factor as a device scalar)"""
    amax = x.abs().amax().float().clamp_min(1e-12).reshape(1)
    return quantize_fp8(x, (FP8_MAX / amax).contiguous()), (amax / FP8_MAX).contiguous()


def gemm_nt_fp8_emits(M, N, K):
    """can this launch also emit its GELU output as e4m3 (q8)?  -- the 8-phase kernel's launches: the library's own launch plan answers"""
    return _gemm_nt_q8_ok(M, N, K, 1)


def gemm_nt_fp8(a8, b8, dq_a, dq_b, n=None, bias=None, gelu=False, preact_out=None, residual=None, row_scale=None, rows_per_scale=1,
                preact_grad=False, q8=None):
    """out[M, :n] = epilogue(dq_a * dq_b * a8 @ b8[:n]^T): a8 [M,K], b8 [>=n,K] uint8 e4m3 bytes (K % 16 == 0), bf16 output;
    the epilogue arguments as for gemm_nt.  q8 = (scale, amax) with gelu: -> (out, out8), out8 the e4m3 bytes of out * scale[0]"""
    _req(a8, torch.uint8, "a8"); _req(b8, torch.uint8, "b8")
    M, K = a8.shape
    n = b8.shape[0] if n is None else n
    ldc = round_up(n, 8)
    out = torch.empty((M, ldc), dtype=BF16, device=a8.device)
    epi = GemmEpilogue()
    epi.bias = bias.data_ptr() if bias is not None else None
    epi.gelu = _gelu_mode(gelu, preact_grad, preact_out)
    epi.preact_out = preact_out.data_ptr() if preact_out is not None else None
    epi.dgelu_of = None
    epi.mul_by = None
    epi.row_scale = row_scale.data_ptr() if row_scale is not None else None
    epi.rows_per_scale = int(rows_per_scale)
    epi.residual = residual.data_ptr() if residual is not None else None
    epi.ldr = residual.shape[1] if residual is not None else 0
    out8 = None
    if q8 is not None:
        out8 = torch.empty((M, ldc), dtype=torch.uint8, device=a8.device)
        epi.q8_out, epi.q8_scale, epi.q8_amax = out8.data_ptr(), q8[0].data_ptr(), (q8[1].data_ptr() if q8[1] is not None else None)
    check(lib.ap_gemm_nt_fp8(a8.data_ptr(), K, b8.data_ptr(), b8.shape[1], out.data_ptr(), ldc, M, n, K, dq_a.data_ptr(), dq_b.data_ptr(),
                             ctypes.byref(epi), _stream()), "ap_gemm_nt_fp8")
    return out if q8 is None else (out, out8)


def gemm_tn_acc(a, b, c, n1=None, n2=None, colsum=None):
    """c[:n1, :n2] += a[:, :n1]^T @ b[:, :n2]   (c fp32, accumulated); optionally colsum[:n1] += a.sum(0)."""
    _req(a, BF16, "a"); _req(b, BF16, "b"); _req(c, torch.float32, "c")
    n1 = c.shape[0] if n1 is None else n1
    n2 = c.shape[1] if n2 is None else n2
    check(lib.ap_gemm_tn_acc(a.data_ptr(), a.shape[1], b.data_ptr(), b.shape[1], c.data_ptr(), c.shape[1], a.shape[0], n1, n2,
                             colsum.data_ptr() if colsum is not None else None, _stream()), "ap_gemm_tn_acc")
    return c


# AP_DETERMINISTIC=1 (or ops.deterministic = True): weight gradients through stored partial tiles + an ordered reduce instead of
# fp32 atomics -- bitwise reproducible steps (loss-curve pins, debugging) for a few percent of the backward time.
deterministic = os.environ.get("AP_DETERMINISTIC", "0") == "1"


def patch_map(H, W, C, k):
    """ap_patch_map of a k x k / stride k convolution on a contiguous NHWC [B,H,W,C] feature map (H, W multiples of k)"""
    from ._lib import PatchMap
    if H % k or W % k:
        raise AutoProgHipError("patch addressing needs H, W divisible by the patch size (got %dx%d / %d)" % (H, W, k))
    return PatchMap(W // k, k * W * C, k * C, k * C, W * C)


def gemm_nt_patch_fwd(x, wmat, bias, k, bn_in=None):
    """x [B,H,W,C] bf16 NHWC, wmat [N, k*k*C] bf16 (columns ordered (dy, dx, c)) -> [B*(H/k)*(W/k), round_up(N, 8)] bf16:
    the forward of a k x k / stride k convolution, its input read in place (no gathered patch matrix).
    bn_in = (mean, rstd, gamma, beta) (C = 64): x is a PRE-BatchNorm tensor and the kernel convolves relu(bn(x)), applied while it stages x"""
    _req(x, BF16, "x"); _req(wmat, BF16, "wmat")
    B, H, W, C = x.shape
    pm = patch_map(H, W, C, k)
    M, N, K = B * (H // k) * (W // k), wmat.shape[0], k * k * C
    ld = round_up(N, 8)
    out = torch.empty((M, ld), dtype=BF16, device=x.device)
    if bn_in is not None:
        if C != 64:
            raise AutoProgHipError("gemm_nt_patch_fwd(bn_in=...): 64-channel feature maps")
        b = _bn_input(bn_in)
        check(lib.ap_gemm_nt_patch_bn(x.data_ptr(), ctypes.byref(b), wmat.data_ptr(), wmat.shape[1], out.data_ptr(), ld, M, N, K,
                                      bias.data_ptr() if bias is not None else None, ctypes.byref(pm), 1, _stream()), "ap_gemm_nt_patch_bn")
        return out
    check(lib.ap_gemm_nt_patch(x.data_ptr(), wmat.data_ptr(), wmat.shape[1], out.data_ptr(), ld, M, N, K,
                               bias.data_ptr() if bias is not None else None, ctypes.byref(pm), 1, _stream()), "ap_gemm_nt_patch")
    return out


def gemm_nt_patch_dgrad(dy, wmat_t, shape, k):
    """dy [M, ld >= N] bf16, wmat_t [k*k*C, >= N] bf16 (the transposed weight matrix) -> dx [B,H,W,C] bf16 written in feature-map layout"""
    _req(dy, BF16, "dy"); _req(wmat_t, BF16, "wmat_t")
    B, H, W, C = shape
    pm = patch_map(H, W, C, k)
    M, Kc = B * (H // k) * (W // k), k * k * C
    dx = torch.empty(shape, dtype=BF16, device=dy.device)
    check(lib.ap_gemm_nt_patch(dy.data_ptr(), wmat_t.data_ptr(), wmat_t.shape[1], dx.data_ptr(), dy.shape[1], M, Kc, wmat_t.shape[1],
                               None, ctypes.byref(pm), 2, _stream()), "ap_gemm_nt_patch")
    return dx


def gemm_tn_acc_grouped(problems, ln=None):
    """problems: list of WgradProblem -- or bare (a, b, c, n1, n2, colsum[, colsum_weight, colsum_scale[, alpha[, b_patch[, b_bn]]]]) -- as for gemm_tn_acc (b_bn: the
    (mean, rstd, gamma, beta) of a BatchNorm whose relu(bn(.)) is applied to the patch-addressed b while it is staged); ONE launch for
    the whole list (chunks of 8).  colsum_weight: bf16 per-token weights of the column sum (DropPath keep mask), colsum_scale its factor;
    alpha: factor of the product (c += alpha * a^T b); b_patch: PatchMap -- b is then an NHWC feature map whose patches are the rows.
    ln: deferred LayerNorm reductions (the entries layernorm_bwd(..., defer=...) appended): LN_MAX_BATCH of them ride in the first launch."""
    ln = list(ln) if ln else []
    fp8 = [p for p in problems if isinstance(p, Tn8Problem)]
    if fp8:                           # the fp8 problems (functional.FP8_WGRAD) in launches of their own; the riders go with the first
        problems = [p for p in problems if not isinstance(p, Tn8Problem)]
        for i0 in range(0, len(fp8), TN_MAX_GROUP):
            gemm_tn8_acc_grouped(fp8[i0:i0 + TN_MAX_GROUP], ln=None if problems else ln[:LN_MAX_BATCH])
            if not problems:
                ln = ln[LN_MAX_BATCH:]
        if not problems:
            if ln:
                layernorm_bwd_reduce_batched(ln)
            return
    if len(ln) > LN_MAX_BATCH:
        layernorm_bwd_reduce_batched(ln[LN_MAX_BATCH:])
        ln = ln[:LN_MAX_BATCH]
    per = TN_MAX_GROUP_DET if deterministic else TN_MAX_GROUP
    for i0 in range(0, len(problems), per):
        chunk = [p if type(p) is WgradProblem else WgradProblem(*p) for p in problems[i0:i0 + per]]
        arr = (TnProblem * len(chunk))()
        keep = []
        for q, prob in zip(arr, chunk):
            a, b, c, n1, n2, colsum = prob.a, prob.b, prob.c, prob.n1, prob.n2, prob.colsum
            csw, css, bp = prob.colsum_weight, prob.colsum_scale, prob.b_patch
            q.alpha = float(prob.alpha)
            _req(a, BF16, "a"); _req(b, BF16, "b"); _req(c, torch.float32, "c")
            if bp is not None:            # b is a feature map read in place: no row stride, no token count to compare, a plain column sum
                keep.append(bp)
                q.b_patch = ctypes.addressof(bp)
                if prob.b_bn is not None:
                    bb = _bn_input(prob.b_bn)
                    keep.append(bb)
                    q.b_bn = ctypes.addressof(bb)
                csw, css = None, 1.0
            elif a.shape[0] != b.shape[0]:
                raise ValueError("gemm_tn_acc_grouped: token counts differ")
            q.A, q.lda, q.B, q.ldb, q.C, q.ldc = a.data_ptr(), a.shape[1], b.data_ptr(), (0 if bp is not None else b.shape[1]), c.data_ptr(), c.shape[1]
            q.M, q.N1, q.N2 = a.shape[0], (c.shape[0] if n1 is None else n1), (c.shape[1] if n2 is None else n2)
            q.colsum_A = colsum.data_ptr() if colsum is not None else None
            if csw is not None:
                _req(csw, BF16, "colsum_weight")
                if csw.numel() < round_up(a.shape[0], 8) or csw.data_ptr() % 16:
                    raise AutoProgHipError("colsum_weight needs ceil(M/8)*8 elements and 16-byte alignment")
            q.colsum_weight = csw.data_ptr() if csw is not None else None
            q.colsum_scale = float(css)
        ptr = ctypes.cast(arr, ctypes.c_void_p)
        ws, ws_bytes = None, 0
        if deterministic:
            ws_bytes = lib.ap_gemm_tn_grouped_workspace(ptr, len(chunk))
            ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=chunk[0].a.device)
        if ln:
            check(lib.ap_gemm_tn_acc_grouped_ln(ptr, len(chunk), ctypes.cast(_ln_reduce_array(ln), ctypes.c_void_p), len(ln), ws.data_ptr() if ws is not None else None,
                                                ws_bytes, _stream()), "ap_gemm_tn_acc_grouped_ln")
            ln = []
        else:
            check(lib.ap_gemm_tn_acc_grouped(ptr, len(chunk), ws.data_ptr() if ws is not None else None, ws_bytes, _stream()), "ap_gemm_tn_acc_grouped")


def colsum_acc(a, out, n=None):
    _req(a, BF16, "a"); _req(out, torch.float32, "out")
    n = out.numel() if n is None else n
    check(lib.ap_colsum_acc(a.data_ptr(), a.shape[1], out.data_ptr(), a.shape[0], n, _stream()), "ap_colsum_acc")
    return out


# ---------------------------------------------------------------------------------- outlook
def outlook_fwd(v, logits, heads, scale):
    _req(v, BF16, "v"); _req(logits, BF16, "logits")
    B, H, W, C = v.shape
    y = torch.empty_like(v)
    check(lib.ap_outlook_fwd(v.data_ptr(), logits.data_ptr(), logits.shape[-1], y.data_ptr(), B, H, W, heads, C // heads,
                             float(scale), _stream()), "ap_outlook_fwd")
    return y


def outlook_bwd(v, logits, dy, heads, scale):
    _req(v, BF16, "v"); _req(logits, BF16, "logits"); _req(dy, BF16, "dy")
    B, H, W, C = v.shape
    dv = torch.empty_like(v)
    dlogits = torch.empty_like(logits)
    check(lib.ap_outlook_bwd(v.data_ptr(), logits.data_ptr(), logits.shape[-1], dy.data_ptr(), dv.data_ptr(), dlogits.data_ptr(),
                             B, H, W, heads, C // heads, float(scale), _stream()), "ap_outlook_bwd")
    return dv, dlogits


def avgpool2_fwd(x):
    _req(x, BF16, "x")
    B, H, W, C = x.shape
    y = torch.empty((B, (H + 1) // 2, (W + 1) // 2, C), dtype=BF16, device=x.device)
    check(lib.ap_avgpool2_fwd(x.data_ptr(), y.data_ptr(), B, H, W, C, _stream()), "ap_avgpool2_fwd")
    return y


def avgpool2_bwd_acc(dpooled, dx):
    _req(dpooled, BF16, "dpooled"); _req(dx, BF16, "dx")
    B, H, W, C = dx.shape
    check(lib.ap_avgpool2_bwd_acc(dpooled.data_ptr(), dx.data_ptr(), B, H, W, C, _stream()), "ap_avgpool2_bwd_acc")
    return dx


# ------------------------------------------------------------------------------------- mhsa
_mhsa_fp8_ok = {}   # (N, hd) -> ap_mhsa_fwd_emits_fp8 (a pure function of the shape in one process: one foreign call per shape)


def mhsa_emits_fp8(N, hd):
    """does mhsa_fwd(fp8=...) have the e4m3 side output for this shape?  (the key/query-blocked kernel: mhsa_plan in csrc/attn_plan.h)"""
    ok = _mhsa_fp8_ok.get((N, hd))
    if ok is None:
        ok = _mhsa_fp8_ok[(N, hd)] = bool(lib.ap_mhsa_fwd_emits_fp8(N, hd))
    return ok


def mhsa_fwd(qkv, B, N, heads, scale, out_row_scale=None, fp8=None):
    """out_row_scale: fp32 [B] factors (0/1 DropPath keep mask) folded into the stored output (see include/autoprog_hip.h).
    fp8 = (scale, amax) device scalars: -> (out, lse, out8), out8 the e4m3 bytes of out * scale[0] (mhsa_emits_fp8 shapes only)"""
    _req(qkv, BF16, "qkv")
    C = qkv.shape[-1] // 3
    out = torch.empty((B * N, C), dtype=BF16, device=qkv.device)
    lse = torch.empty((B, heads, N), dtype=torch.float32, device=qkv.device)
    if fp8 is not None:
        out8 = torch.empty((B * N, C), dtype=torch.uint8, device=qkv.device)
        check(lib.ap_mhsa_fwd_fp8(qkv.data_ptr(), out.data_ptr(), out8.data_ptr(), fp8[0].data_ptr(), fp8[1].data_ptr() if fp8[1] is not None else None,
                                  lse.data_ptr(), B, N, heads, C // heads, float(scale),
                                  out_row_scale.data_ptr() if out_row_scale is not None else None, _stream()), "ap_mhsa_fwd_fp8")
        return out, lse, out8
    check(lib.ap_mhsa_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, N, heads, C // heads, float(scale),
                          out_row_scale.data_ptr() if out_row_scale is not None else None, _stream()), "ap_mhsa_fwd")
    return out, lse


def mhsa_bwd(qkv, out, dout, lse, B, N, heads, scale):
    _req(qkv, BF16, "qkv"); _req(out, BF16, "out"); _req(dout, BF16, "dout")
    C = qkv.shape[-1] // 3
    dqkv = torch.empty_like(qkv)
    ws_bytes = lib.ap_mhsa_bwd_workspace(B, N, heads, C // heads)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=qkv.device) if ws_bytes else None
    check(lib.ap_mhsa_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), B, N, heads, C // heads,
                          float(scale), ws.data_ptr() if ws is not None else None, ws_bytes, _stream()), "ap_mhsa_bwd")
    return dqkv


def class_attn_fwd(q, kv, B, N, heads, scale, kv_cls=None):
    """kv_cls given: split layout -- key 0 is kv_cls[b], keys 1..N-1 the N-1 rows of kv (see include/autoprog_hip.h)"""
    _req(q, BF16, "q"); _req(kv, BF16, "kv")
    C = q.shape[-1]
    out = torch.empty((B, C), dtype=BF16, device=q.device)
    probs = torch.empty((B, heads, N), dtype=torch.float32, device=q.device)
    check(lib.ap_class_attn_fwd(q.data_ptr(), kv.data_ptr(), kv_cls.data_ptr() if kv_cls is not None else None, out.data_ptr(), probs.data_ptr(),
                                B, N, heads, C // heads, float(scale), _stream()), "ap_class_attn_fwd")
    return out, probs


def class_attn_bwd(q, kv, probs, dout, B, N, heads, scale, kv_cls=None):
    """-> (dq, dkv) or, in the split layout, (dq, dkv_tokens, dkv_cls)"""
    _req(dout, BF16, "dout")
    dq = torch.empty_like(q)
    dkv = torch.empty_like(kv)
    dkv_cls = torch.empty_like(kv_cls) if kv_cls is not None else None
    C = q.shape[-1]
    check(lib.ap_class_attn_bwd(q.data_ptr(), kv.data_ptr(), kv_cls.data_ptr() if kv_cls is not None else None, probs.data_ptr(), dout.data_ptr(),
                                dq.data_ptr(), dkv.data_ptr(), dkv_cls.data_ptr() if dkv_cls is not None else None,
                                B, N, heads, C // heads, float(scale), _stream()), "ap_class_attn_bwd")
    return (dq, dkv) if kv_cls is None else (dq, dkv, dkv_cls)


# ------------------------------------------------------------------------------ misc fused
def mix_token_swap(x, r0, r1, c0, c1):
    _req(x, BF16, "x")
    B, H, W, C = x.shape
    y = torch.empty_like(x)
    check(lib.ap_mix_token_swap(x.data_ptr(), y.data_ptr(), B, H, W, C, int(r0), int(r1), int(c0), int(c1), _stream()), "ap_mix_token_swap")
    return y


def mix_token_swap_dev(x, box_ptr, scale):
    """the same with the box {r0, r1, c0, c1} read from device memory (int32[4] at box_ptr, times `scale`): graph.StepScalars"""
    _req(x, BF16, "x")
    B, H, W, C = x.shape
    y = torch.empty_like(x)
    check(lib.ap_mix_token_swap_dev(x.data_ptr(), y.data_ptr(), B, H, W, C, int(box_ptr), int(scale), _stream()), "ap_mix_token_swap_dev")
    return y


def loss_combine(a, wa, b=None, wb=0.0):
    """fp32 scalar tensor wa * sum(a) + wb * sum(b) (one launch)"""
    _req(a, torch.float32, "a")
    out = torch.empty((), dtype=torch.float32, device=a.device)
    check(lib.ap_loss_combine(a.data_ptr(), a.numel(), float(wa), b.data_ptr() if b is not None else None, b.numel() if b is not None else 0,
                              float(wb), out.data_ptr(), _stream()), "ap_loss_combine")
    return out


def classify_stats(logits, labels, n_classes=None):
    """logits bf16 [rows, ld] (n_classes valid columns, default ld), labels int64 [rows] -> (loss fp32 [rows], rank int32 [rows]):
    loss = logsumexp(z) - z[label]; rank = number of classes whose logit is STRICTLY greater than the label's (top-k correct iff 0 <= rank < k);
    a label outside [0, n_classes) gives loss 0, rank -1 (include/autoprog_hip.h ap_classify_stats)"""
    _req(logits, BF16, "logits"); _req(labels, torch.int64, "labels")
    if logits.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits.shape[0]:
        raise AutoProgHipError("classify_stats: logits [rows, ld] and labels [rows]")
    rows, ld = logits.shape
    n_classes = ld if n_classes is None else int(n_classes)
    loss = torch.empty(rows, dtype=torch.float32, device=logits.device)
    rank = torch.empty(rows, dtype=torch.int32, device=logits.device)
    check(lib.ap_classify_stats(logits.data_ptr(), ld, n_classes, labels.data_ptr(), loss.data_ptr(), rank.data_ptr(), rows, _stream()), "ap_classify_stats")
    return loss, rank


def softmax_topk(logits, C, K, inv_temp, idx_out, val_out, o_sb, o_sn, rows_per_batch):
    """row-wise softmax + top-K (include/autoprog_hip.h ap_softmax_topk_rows): logits bf16 [M, ld] with C valid columns (a padded view: unit
    column stride, ld = its row stride, ld % 8 == 0); row r = (b, n), b = r // rows_per_batch, writes its K (class, score) pairs in descending
    order -- equal logits by ascending class -- at idx_out / val_out (int32 / fp32, any shape) + b * o_sb + n * o_sn elements.  Nothing is
    allocated; the caller's strides must keep every pair inside the two outputs (checked here against their sizes)."""
    _req(idx_out, torch.int32, "idx_out"); _req(val_out, torch.float32, "val_out")
    ld = _padded_rows(logits, 0, "logits", "softmax_topk: logits bf16 [M, >= C] with unit column stride")
    M = logits.shape[0]
    C, K, rows_per_batch = int(C), int(K), int(rows_per_batch)
    if C > logits.shape[1]:
        raise AutoProgHipError("softmax_topk: C = %d valid columns of %d" % (C, logits.shape[1]))
    if M > 0 and rows_per_batch > 0 and K > 0:
        last = ((M - 1) // rows_per_batch) * int(o_sb) + min(M - 1, rows_per_batch - 1) * int(o_sn) + K
        if int(o_sb) < 0 or int(o_sn) < 0 or last > min(idx_out.numel(), val_out.numel()):
            raise AutoProgHipError("softmax_topk: the output strides reach element %d of %d" % (last, min(idx_out.numel(), val_out.numel())))
    check(lib.ap_softmax_topk_rows(logits.data_ptr(), ld, C, K, float(inv_temp), idx_out.data_ptr(), val_out.data_ptr(), int(o_sb), int(o_sn),
                                   rows_per_batch, M, _stream()), "ap_softmax_topk_rows")


def _soft_ce(entry, what, logits, C, target_args, grad_scale, mix_lam, mix_batches, mix_lam_ptr, pairs=None):
    """what the three soft-target CE wrappers share: the logits -- bf16, CONTIGUOUS [M, ldx], ldx read from the shape: a padded view is not
    taken here (functional.ce_rows copies it) --, the (idx, val) tensors of a sparse target, the two outputs, and lam.  target_args: what the
    entry point takes between ldx and row_loss.  mix_lam_ptr: device address of lam (overrides mix_lam: graph.StepScalars).
    -> (row_loss fp32 [M], dlogits bf16 like logits)"""
    _req(logits, BF16, "logits")
    if pairs is not None:
        idx, val = pairs
        if not (idx.is_cuda and idx.dtype == torch.int32 and val.is_cuda and val.dtype == torch.float32):
            raise AutoProgHipError("sparse targets: idx must be CUDA int32 and val CUDA fp32")
    M, ldx = logits.shape
    row_loss = torch.empty(M, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    check(entry(logits.data_ptr(), ldx, *target_args, row_loss.data_ptr(), dlogits.data_ptr(), float(grad_scale), M, C, float(mix_lam),
                int(mix_batches), int(mix_lam_ptr) if mix_lam_ptr else None, _stream()), what)
    return row_loss, dlogits


def soft_ce_fwd_bwd(logits, C, target, t_sb, t_sc, t_sn, rows_per_batch, grad_scale, mix_lam=1.0, mix_batches=0, mix_lam_ptr=None):
    """returns (row_loss fp32 [M], dlogits bf16 like logits); mix_batches = B: target of batch b is lam*t[b] + (1-lam)*t[B-1-b].
    mix_lam_ptr: device address of lam (overrides mix_lam: graph.StepScalars)"""
    if not (target.is_cuda and target.dtype == torch.float32):
        raise AutoProgHipError("target must be a CUDA fp32 tensor (any strides; pass them explicitly)")
    return _soft_ce(lib.ap_soft_ce_fwd_bwd_dev, "ap_soft_ce_fwd_bwd_dev", logits, C,
                    (target.data_ptr(), int(t_sb), int(t_sc), int(t_sn), int(rows_per_batch)), grad_scale, mix_lam, mix_batches, mix_lam_ptr)


def soft_ce_sparse_fwd_bwd(logits, C, idx, val, p_sb, p_sn, rows_per_batch, smoothing, grad_scale, mix_lam=1.0, mix_batches=0, mix_lam_ptr=None):
    """soft-target CE against top-K (class, score) pairs + label smoothing (the token-label target before it is densified);
    idx int32 / val fp32 with K = idx.shape[-1] pairs per row at b * p_sb + n * p_sn.  Returns (row_loss fp32 [M], dlogits bf16).
    mix_batches = B: the target of row (b, n) is mix_lam * t[b, n] + (1 - mix_lam) * t[B-1-b, n] (the mix-token class target)."""
    return _soft_ce(lib.ap_soft_ce_sparse_fwd_bwd_dev, "ap_soft_ce_sparse_fwd_bwd_dev", logits, C,
                    (idx.data_ptr(), val.data_ptr(), int(idx.shape[-1]), int(p_sb), int(p_sn), int(rows_per_batch), float(smoothing)),
                    grad_scale, mix_lam, mix_batches, mix_lam_ptr, pairs=(idx, val))


def soft_ce_sparse_gt_fwd_bwd(logits, C, idx, val, p_sb, p_s0, p_s1, smoothing, grad_scale, mix_lam=1.0, mix_batches=0, mix_lam_ptr=None):
    """the class rows of TokenLabelGTCrossEntropy on the sparse target (include/autoprog_hip.h ap_soft_ce_sparse_gt_fwd_bwd): logits bf16
    [B, ldx], one row per image; image b holds K = idx.shape[-1] <= 8 pairs of the ground-truth slot at b * p_sb + p_s0 and of the
    image-level slot at b * p_sb + p_s1 (elements of idx int32 / val fp32).  The two argmaxes, ratio = 0.9 - 0.4 * [they agree] and the
    blend ratio * slot 1 + (1 - ratio) * slot 0 are formed on the device, for the row's image and -- mix_batches = B -- for its partner
    B-1-b.  Returns (row_loss fp32 [B], dlogits bf16)."""
    B = logits.shape[0]
    K, p_sb, p_s0, p_s1 = int(idx.shape[-1]), int(p_sb), int(p_s0), int(p_s1)
    if B > 0 and (min(p_sb, p_s0, p_s1) < 0 or (B - 1) * p_sb + max(p_s0, p_s1) + K > min(idx.numel(), val.numel())):
        raise AutoProgHipError("soft_ce_sparse_gt_fwd_bwd: the slot offsets reach past the %d elements of the pair arrays" % min(idx.numel(), val.numel()))
    return _soft_ce(lib.ap_soft_ce_sparse_gt_fwd_bwd, "ap_soft_ce_sparse_gt_fwd_bwd", logits, C,
                    (idx.data_ptr(), val.data_ptr(), K, p_sb, p_s0, p_s1, float(smoothing)), grad_scale, mix_lam, mix_batches, mix_lam_ptr,
                    pairs=(idx, val))


def _padded_rows(t, C, name, shape_error=None):
    """a bf16 CUDA matrix [M, >= C] with unit column stride -> its leading dimension (a padded view is taken as it is; a row stride
    that is no multiple of 8 or below C, or a misaligned base, is the library's AP_ERR_SHAPE).  shape_error: the caller's own text for a
    matrix of another form."""
    if not (torch.is_tensor(t) and t.is_cuda):
        raise AutoProgHipError("%s must be a CUDA tensor (the HIP path has no CPU fallback)" % name)
    if t.dtype != BF16 or t.dim() != 2 or t.shape[1] < C or (t.shape[1] > 1 and t.stride(1) != 1):
        raise AutoProgHipError(shape_error or "%s must be bf16 [M, >= %d] with unit column stride" % (name, C))
    ld = t.stride(0)
    if t.shape[0] <= 1 and (ld < t.shape[1] or ld % 8):         # (the row stride of a single row means nothing)
        ld = t.shape[1]
    return ld


def padded_view_rows(x2d):
    """logits [M, C] for an entry point that takes a padded view (ap_softmax_topk_rows, the teacher of ap_distill_fwd_bwd; _padded_rows is
    their check): bf16 with unit column stride, a row stride that is a multiple of 8 and at least C, and a 16-byte-aligned base -- what
    functional.linear returns -- is passed as it is; anything else is copied into zero-padded rows and viewed [:, :C].  The soft-target CE
    wrappers do not take such views: functional.ce_rows is their rule, and the two differ on purpose."""
    M, C = x2d.shape
    if x2d.dtype == BF16 and x2d.stride(1) == 1 and x2d.stride(0) % 8 == 0 and x2d.stride(0) >= C and x2d.data_ptr() % 16 == 0:
        return x2d
    xp = torch.zeros((M, round_up(C, 8)), dtype=BF16, device=x2d.device)
    xp[:, :C] = x2d
    return xp[:, :C]


def distill_fwd_bwd(student, C, teacher, mode, inv_temp, grad_scale):
    """distillation loss of student rows against teacher rows (include/autoprog_hip.h ap_distill_fwd_bwd): student / teacher bf16 [M, >= C]
    with C valid columns (padded views: unit column stride, ld = the row stride, ld % 8 == 0).  mode 0 (soft): row_loss = T^2 KL(p_t || p_s)
    at T = 1 / inv_temp, dstudent = grad_scale * T * (p_s - p_t); mode 1 (hard): CE against the teacher's argmax (equal logits: the smallest
    class), dstudent = grad_scale * (softmax(x_s) - onehot).  -> (row_loss fp32 [M], dstudent bf16 [M, ld_s], columns C .. ld_s-1 zero)"""
    C = int(C)
    ld_s, ld_t = _padded_rows(student, C, "student"), _padded_rows(teacher, C, "teacher")
    M = student.shape[0]
    if teacher.shape[0] != M or teacher.device != student.device:
        raise AutoProgHipError("distill_fwd_bwd: student and teacher must have the same rows on one device")
    row_loss = torch.empty(M, dtype=torch.float32, device=student.device)
    dstudent = torch.empty((M, ld_s), dtype=BF16, device=student.device)
    check(lib.ap_distill_fwd_bwd(student.data_ptr(), ld_s, teacher.data_ptr(), ld_t, C, int(mode), float(inv_temp), row_loss.data_ptr(),
                                 dstudent.data_ptr(), float(grad_scale), M, _stream()), "ap_distill_fwd_bwd")
    return row_loss, dstudent


def row_scale(x, scale, rows_per_scale):
    _req(x, BF16, "x"); _req(scale, torch.float32, "scale")
    C = x.shape[-1]
    y = torch.empty_like(x)
    check(lib.ap_row_scale(x.data_ptr(), scale.data_ptr(), y.data_ptr(), x.numel() // C, C, int(rows_per_scale), _stream()), "ap_row_scale")
    return y


def add_bcast(a, b):
    _req(a, BF16, "a"); _req(b, BF16, "b")
    y = torch.empty_like(a)
    check(lib.ap_add_bcast(a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(), b.numel(), _stream()), "ap_add_bcast")
    return y


def resample_grid(x, wy, wx, out=None, accumulate=False):
    """x fp32 [hi, wi, C], wy fp32 [ho, hi], wx fp32 [wo, wi] -> out fp32 [ho, wo, C] (+)= the separable resampling (ap_resample_grid)"""
    _req(x, torch.float32, "x"); _req(wy, torch.float32, "wy"); _req(wx, torch.float32, "wx")
    hi, wi, C = x.shape
    ho, wo = wy.shape[0], wx.shape[0]
    if wy.shape[1] != hi or wx.shape[1] != wi:
        raise AutoProgHipError("resample_grid: tap matrices do not match the grid")
    if out is None:
        out = torch.empty((ho, wo, C), dtype=torch.float32, device=x.device)
    else:
        _req(out, torch.float32, "out")
        if out.numel() != ho * wo * C:
            raise AutoProgHipError("resample_grid: output shape")
    check(lib.ap_resample_grid(x.data_ptr(), hi, wi, wy.data_ptr(), wx.data_ptr(), out.data_ptr(), ho, wo, C, 1 if accumulate else 0, _stream()),
          "ap_resample_grid")
    return out


def sum_reps_acc(x, out, reps):
    _req(x, BF16, "x"); _req(out, torch.float32, "out")
    check(lib.ap_sum_reps_acc(x.data_ptr(), out.data_ptr(), out.numel(), int(reps), _stream()), "ap_sum_reps_acc")
    return out


# ---------------------------------------------------------------------------- stem BN + ReLU
def bn_relu_fwd(x, gamma, beta, running_mean, running_var, training, momentum, eps, partials=None, apply=True):
    """x: bf16 [..., C] NHWC rows.  returns (y, mean, rstd).  partials (training only): fp32 [rows,2,C] partial sums / sums of squares
    of x from the kernel that produced it (conv3x3_c64 want_stats) -- the statistics pass over x is skipped.  apply=False (with
    partials, or in eval mode): statistics only, y is None -- the consumer normalises while it loads (conv3x3_c64(bn_in=...))"""
    _req(x, BF16, "x")
    C = x.shape[-1]
    T = x.numel() // C
    if not apply and not training:
        return None, running_mean.float().contiguous(), torch.rsqrt(running_var.float() + eps).contiguous()
    if not apply and partials is None:
        raise AutoProgHipError("bn_relu_fwd(apply=False) needs the producer's partial statistics")
    y = torch.empty_like(x) if apply else None
    if training and partials is not None:
        _req(partials, torch.float32, "partials")
        mean = torch.empty(C, dtype=torch.float32, device=x.device)
        rstd = torch.empty(C, dtype=torch.float32, device=x.device)
        check(lib.ap_bn_relu_fwd_partials(x.data_ptr(), partials.data_ptr(), partials.shape[0], gamma.data_ptr(), beta.data_ptr(),
                                          running_mean.data_ptr() if running_mean is not None else None,
                                          running_var.data_ptr() if running_var is not None else None,
                                          float(momentum), float(eps), y.data_ptr() if y is not None else None, mean.data_ptr(), rstd.data_ptr(), T, C, _stream()),
              "ap_bn_relu_fwd_partials")
        return y, mean, rstd
    if training:
        mean = torch.empty(C, dtype=torch.float32, device=x.device)
        rstd = torch.empty(C, dtype=torch.float32, device=x.device)
    else:
        mean = running_mean.float().contiguous()
        rstd = torch.rsqrt(running_var.float() + eps).contiguous()
    ws_bytes = lib.ap_bn_relu_workspace(T, C)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device)
    check(lib.ap_bn_relu_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                             running_mean.data_ptr() if (training and running_mean is not None) else None,
                             running_var.data_ptr() if (training and running_var is not None) else None,
                             1 if training else 0, float(momentum), float(eps), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                             T, C, ws.data_ptr(), ws_bytes, _stream()), "ap_bn_relu_fwd")
    return y, mean, rstd


def bn_relu_bwd(dy, x, gamma, beta, mean, rstd, dgamma, dbeta, act_out=False):
    """act_out: -> (dx, relu(bn(x))) -- the activation a fused forward never stored, written by the pass that holds x anyway"""
    _req(dy, BF16, "dy"); _req(x, BF16, "x")
    C = x.shape[-1]
    T = x.numel() // C
    dx = torch.empty_like(x)
    ws_bytes = lib.ap_bn_relu_workspace(T, C)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device)
    if act_out:
        act = torch.empty_like(x)
        check(lib.ap_bn_relu_bwd_act(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                     dx.data_ptr(), act.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), T, C, ws.data_ptr(), ws_bytes, _stream()),
              "ap_bn_relu_bwd_act")
        return dx, act
    check(lib.ap_bn_relu_bwd(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                             dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), T, C, ws.data_ptr(), ws_bytes, _stream()), "ap_bn_relu_bwd")
    return dx


def bn_relu_bwd_partials(dy, x, gamma, beta, mean, rstd, partial, dgamma, dbeta):
    """bn_relu_bwd whose first pass ran inside the convolution that produced dy (conv3x3_c64_bwd_stats): finalize + dx only"""
    _req(dy, BF16, "dy"); _req(x, BF16, "x"); _req(partial, torch.float32, "partial")
    C = x.shape[-1]
    T = x.numel() // C
    dx = torch.empty_like(x)
    ws_bytes = lib.ap_bn_relu_workspace(T, C)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device)
    check(lib.ap_bn_relu_bwd_partials(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                      partial.data_ptr(), partial.shape[0], dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), T, C,
                                      ws.data_ptr(), ws_bytes, _stream()), "ap_bn_relu_bwd_partials")
    return dx


# ------------------------------------------------------------------------------------- stem 3x3 convolution (C = 64)
def conv3x3_pack(weight):
    """fp32 [64,64,3,3] (or [128,128,3,3]: the VOLO-D4 / D5 stem) -> (w_fwd, w_bwd) bf16 operand layouts of conv3x3_c64 / conv3x3_c128"""
    _req(weight, torch.float32, "weight")
    if tuple(weight.shape) == (128, 128, 3, 3):
        wf = torch.empty(9 * 128 * 128, dtype=BF16, device=weight.device)
        wb = torch.empty_like(wf)
        check(lib.ap_conv3x3_c128_pack(weight.contiguous().data_ptr(), wf.data_ptr(), wb.data_ptr(), _stream()), "ap_conv3x3_c128_pack")
        return wf, wb
    if tuple(weight.shape) != (64, 64, 3, 3):
        raise AutoProgHipError("the HIP 3x3 convolutions handle 64 -> 64 and 128 -> 128 channels (got %s)" % (tuple(weight.shape),))
    wf = torch.empty(9 * 64 * 64, dtype=BF16, device=weight.device)
    wb = torch.empty_like(wf)
    check(lib.ap_conv3x3_c64_pack(weight.contiguous().data_ptr(), wf.data_ptr(), wb.data_ptr(), _stream()), "ap_conv3x3_c64_pack")
    return wf, wb


def _bn_input(bn_in):
    from ._lib import BnInput
    mean, rstd, gamma, beta = bn_in
    for t, n in ((mean, "mean"), (rstd, "rstd"), (gamma, "gamma"), (beta, "beta")):
        _req(t, torch.float32, n)
    b = BnInput()
    b.mean, b.rstd, b.gamma, b.beta = mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr()
    return b


def conv3x3_c64(x, w_packed, want_stats=False, bn_in=None):
    """x [B,H,W,64] bf16 (NHWC, contiguous) -> conv3x3 / stride 1 / pad 1.  want_stats: also return the partial BatchNorm
    statistics of the output (fp32 [rows,2,64], for bn_relu_fwd(..., partials=)).  bn_in = (mean, rstd, gamma, beta): x is the
    PRE-BatchNorm output of the previous convolution and the kernel applies relu(bn(x)) while it stages its input"""
    _req(x, BF16, "x"); _req(w_packed, BF16, "w_packed")
    B, H, W, C = x.shape
    if C == 128:                       # csrc/conv128.hip: patch in LDS, weights streamed per (tap, 64-channel) slab
        if bn_in is not None:
            raise AutoProgHipError("conv3x3 at 128 channels: the BatchNorm input transform exists at 64 channels only")
        if w_packed.numel() != 9 * 128 * 128:
            raise AutoProgHipError("conv3x3 at 128 channels needs the operand of conv3x3_pack on a [128,128,3,3] weight")
        y = torch.empty_like(x)
        stats = torch.empty((lib.ap_conv3x3_c128_stat_rows(B, H, W), 2, 128), dtype=torch.float32, device=x.device) if want_stats else None
        check(lib.ap_conv3x3_c128(x.data_ptr(), w_packed.data_ptr(), y.data_ptr(), B, H, W, stats.data_ptr() if want_stats else None, _stream()),
              "ap_conv3x3_c128")
        return (y, stats) if want_stats else y
    if C != 64:
        raise AutoProgHipError("conv3x3_c64: 64 (or 128) channels (got %d)" % C)
    y = torch.empty_like(x)
    stats = torch.empty((lib.ap_conv3x3_c64_stat_rows(B, H, W), 2, 64), dtype=torch.float32, device=x.device) if want_stats else None
    if bn_in is not None:
        b = _bn_input(bn_in)
        check(lib.ap_conv3x3_c64_bn(x.data_ptr(), ctypes.byref(b), w_packed.data_ptr(), y.data_ptr(), B, H, W,
                                    stats.data_ptr() if want_stats else None, _stream()), "ap_conv3x3_c64_bn")
    else:
        check(lib.ap_conv3x3_c64(x.data_ptr(), w_packed.data_ptr(), y.data_ptr(), B, H, W,
                                 stats.data_ptr() if want_stats else None, _stream()), "ap_conv3x3_c64")
    return (y, stats) if want_stats else y


def conv3x3_c64_bwd_stats(dz, w_packed_bwd, z_below, bn_below):
    """the input-gradient convolution of a 64-wide stem layer, with the first pass of the BatchNorm + ReLU backward of the layer BELOW in
    its epilogue: -> (da, partial [rows,2,64]) for bn_relu_bwd_partials(da, z_below, ..., partial, ...).  bn_below = (mean, rstd, gamma, beta)"""
    _req(dz, BF16, "dz"); _req(w_packed_bwd, BF16, "w_packed_bwd"); _req(z_below, BF16, "z_below")
    B, H, W, C = dz.shape
    if C != 64 or tuple(z_below.shape) != tuple(dz.shape):
        raise AutoProgHipError("conv3x3_c64_bwd_stats: [B,H,W,64] maps of one shape (got %s, %s)" % (tuple(dz.shape), tuple(z_below.shape)))
    da = torch.empty_like(dz)
    stats = torch.empty((lib.ap_conv3x3_c64_stat_rows(B, H, W), 2, 64), dtype=torch.float32, device=dz.device)
    b = _bn_input(bn_below)
    check(lib.ap_conv3x3_c64_bwd_stats(dz.data_ptr(), w_packed_bwd.data_ptr(), da.data_ptr(), B, H, W, z_below.data_ptr(), ctypes.byref(b),
                                       stats.data_ptr(), _stream()), "ap_conv3x3_c64_bwd_stats")
    return da, stats


def conv3x3_c64_wgrad(x, dy, dw, bn_in=None):
    """dw (fp32 [64,64,3,3], contiguous) += weight gradient of conv3x3_c64 for input x and output gradient dy; bn_in as for conv3x3_c64
    (the layer's input was relu(bn(x)))"""
    _req(x, BF16, "x"); _req(dy, BF16, "dy"); _req(dw, torch.float32, "dw")
    B, H, W, C = x.shape
    if C == 128 and tuple(dy.shape) == tuple(x.shape) and tuple(dw.shape) == (128, 128, 3, 3) and bn_in is None:
        ws_bytes = lib.ap_conv3x3_c128_wgrad_workspace(B, H, W)
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device)
        check(lib.ap_conv3x3_c128_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), B, H, W, ws.data_ptr(), ws_bytes, _stream()), "ap_conv3x3_c128_wgrad")
        return dw
    if C != 64 or tuple(dy.shape) != tuple(x.shape) or tuple(dw.shape) != (64, 64, 3, 3):
        raise AutoProgHipError("conv3x3_c64_wgrad: shapes %s %s %s" % (tuple(x.shape), tuple(dy.shape), tuple(dw.shape)))
    ws_bytes = lib.ap_conv3x3_c64_wgrad_workspace(B, H, W)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device)
    if bn_in is not None:
        b = _bn_input(bn_in)
        check(lib.ap_conv3x3_c64_wgrad_bn(x.data_ptr(), ctypes.byref(b), dy.data_ptr(), dw.data_ptr(), B, H, W, ws.data_ptr(), ws_bytes, _stream()),
              "ap_conv3x3_c64_wgrad_bn")
        return dw
    check(lib.ap_conv3x3_c64_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), B, H, W, ws.data_ptr(), ws_bytes, _stream()), "ap_conv3x3_c64_wgrad")
    return dw


# ------------------------------------------------------------------------------------- a loader's uint8 batch -> the stem's input
def _u8_batch(what, u8, layout):
    """-> (B, H, W) of a uint8 batch in `layout`: [B,3,H,W] ("nchw") or [B,H,W,3] ("nhwc")"""
    _req(u8, torch.uint8, "u8")
    if layout not in ("nchw", "nhwc") or u8.dim() != 4 or u8.shape[1 if layout == "nchw" else 3] != 3:
        raise AutoProgHipError("%s: a uint8 [B,3,H,W] (nchw) or [B,H,W,3] (nhwc) batch, got %s as %s" % (what, tuple(u8.shape), layout))
    return (u8.shape[0],) + ((u8.shape[2], u8.shape[3]) if layout == "nchw" else (u8.shape[1], u8.shape[2]))


def _host_records(what, records, host, words, dtype, name="records"):
    """`records` (on the device) holds at least `words` words of dtype, and so does `host`, where given: a CPU, contiguous copy of the
    same dtype -> its address, or None"""
    _req(records, dtype, name)
    if records.numel() < words or (host is not None and (host.is_cuda or host.dtype != dtype or not host.is_contiguous() or host.numel() < words)):
        raise AutoProgHipError("%s: %s must hold %d %s words (and so must a CPU, contiguous host copy of that dtype)" % (what, name, words, dtype))
    return None if host is None else host.data_ptr()


PREP_PARAM_WORDS, PREP_BOX_WORDS = 16, 8          # the device block of ap_input_prep: 16 words of per-step parameters, then 8 per box record
_PREP_ERASE = {"const": 0, "rand": 1, "pixel": 2}


def input_prep(u8, size, out="s2d16", table=None, params=None, layout="nchw", mix=False, n_boxes=0, erase_mode="const", host_block=None):
    """uint8 [B,3,Hi,Wi] (layout "nchw", what timm's fast_collate yields) or [B,Hi,Wi,3] ("nhwc") -> bf16 [B,size/2,size/2,16] (out
    "s2d16", the layout of resize_bilinear_s2d16) or [B,size,size,3] ("nhwc", that of resize_bilinear_nhwc): normalise by `table`
    (fp32 [3,256] on the device), Mixup / CutMix with image B-1-b, RandomErasing and the bilinear resize in one launch
    (include/autoprog_hip.h, ap_input_prep).  `params`: int32 device tensor, PREP_PARAM_WORDS words of per-step parameters followed by
    B * n_boxes box records of PREP_BOX_WORDS words (data.DeviceBatchPrep fills it); None: no mix, no erase.  `mix` False ignores the
    block's mix mode.  `host_block`: a CPU copy of `params` whose records are checked against the image before the launch."""
    B, Hi, Wi = _u8_batch("input_prep", u8, layout)
    _req(table, torch.float32, "table")
    if out not in ("s2d16", "nhwc") or erase_mode not in _PREP_ERASE or tuple(table.shape) != (3, 256):
        raise AutoProgHipError("input_prep: out %r, erase_mode %r, table %s" % (out, erase_mode, tuple(table.shape)))
    a = InputPrepArgs()
    a.u8, a.in_layout, a.B, a.Hi, a.Wi = u8.data_ptr(), int(layout == "nhwc"), B, Hi, Wi
    a.out_layout, a.Ho, a.Wo = int(out == "nhwc"), size, size
    a.table = table.data_ptr()
    a.mix_enabled, a.n_boxes, a.erase_mode = int(bool(mix)), int(n_boxes), _PREP_ERASE[erase_mode]
    if params is not None:
        _req(params, torch.int32, "params")
        words = PREP_PARAM_WORDS + B * max(0, min(int(n_boxes), PREP_MAX_BOXES)) * PREP_BOX_WORDS
        if params.numel() < words or (host_block is not None and (host_block.is_cuda or host_block.dtype != torch.int32 or host_block.numel() < words)):
            raise AutoProgHipError("input_prep: the parameter block holds %d words, %d needed" % (params.numel(), words))
        a.params = params.data_ptr()
        if n_boxes:
            a.boxes = params.data_ptr() + 4 * PREP_PARAM_WORDS
            if host_block is not None:
                a.boxes_host = host_block.data_ptr() + 4 * PREP_PARAM_WORDS
    elif mix or n_boxes:
        raise AutoProgHipError("input_prep: mix / erase need the parameter block")
    y = torch.empty((B, size // 2, size // 2, 16) if out == "s2d16" else (B, size, size, 3), dtype=BF16, device=u8.device)
    a.out = y.data_ptr()
    check(lib.ap_input_prep(ctypes.byref(a), _stream()), "ap_input_prep")
    return y


# ------------------------------------------------------------------------------------- per-image crop + flip + resize of a uint8 batch
CROP_RECORD_WORDS = 8                             # a record of ap_crop_resize_u8: top, left, h, w, flip, three zero words


def _crop_launch(what, args_type, entry, u8, size, records, layout, out, host_records):
    (B, Hi, Wi), size = _u8_batch(what, u8, layout), int(size)
    if size < 1:
        raise AutoProgHipError("%s: size %d" % (what, size))
    host = _host_records(what, records, host_records, B * CROP_RECORD_WORDS, torch.int32)
    shape = (B, 3, size, size) if layout == "nchw" else (B, size, size, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=u8.device)
    elif tuple(_req(out, torch.uint8, "out").shape) != shape:
        raise AutoProgHipError("%s: out must be %s, got %s" % (what, shape, tuple(out.shape)))
    a = args_type()
    a.u8, a.layout, a.B, a.Hi, a.Wi = u8.data_ptr(), int(layout == "nhwc"), B, Hi, Wi
    a.out, a.S, a.records, a.records_host = out.data_ptr(), size, records.data_ptr(), host
    check(entry(ctypes.byref(a), _stream()), "ap_" + what)
    return out


def crop_resize_u8(u8, size, records, layout="nchw", out=None, host_records=None):
    """uint8 [B,3,Hi,Wi] (layout "nchw") or [B,Hi,Wi,3] ("nhwc") -> uint8 [B,3,size,size] / [B,size,size,3]: image b's box
    (records[b] = top, left, h, w, flip, 0, 0, 0; int32, on the device) resized bilinearly to size x size, flipped along the width where
    flip is 1, in one launch (include/autoprog_hip.h, ap_crop_resize_u8; no antialiasing).  `out`: a uint8 device tensor of the result's
    shape to write into (contiguous, any alignment); `host_records`: a CPU copy of `records` whose boxes are checked against the image
    before the launch."""
    return _crop_launch("crop_resize_u8", CropResizeArgs, lib.ap_crop_resize_u8, u8, size, records, layout, out, host_records)


RESAMPLE_BILINEAR, RESAMPLE_BICUBIC = 1, 2        # word 5 of a record of ap_crop_resample_u8 (AP_RESAMPLE_*)


def crop_resample_u8(u8, size, records, layout="nchw", out=None, host_records=None):
    """crop_resize_u8 with Pillow's antialiased filters: image b's box (records[b] = top, left, h, w, flip, filter, 0, 0; filter
    RESAMPLE_BILINEAR or RESAMPLE_BICUBIC, per image) comes out as Pillow's Image.crop(box).resize((size, size), filter) gives it, byte for
    byte, mirrored along the width afterwards where flip is 1, in one launch (include/autoprog_hip.h, ap_crop_resample_u8).  Arguments
    as crop_resize_u8's."""
    return _crop_launch("crop_resample_u8", CropResampleArgs, lib.ap_crop_resample_u8, u8, size, records, layout, out, host_records)


# ------------------------------------------------------------------------------------- RandAugment's ops on a uint8 batch
RANDAUG_RECORD_WORDS, RANDAUG_MAX_LAYERS = 16, 8  # AP_RANDAUG_RECORD_WORDS / AP_RANDAUG_MAX_LAYERS
(RA_NONE, RA_AUTOCONTRAST, RA_EQUALIZE, RA_INVERT, RA_SOLARIZE, RA_SOLARIZE_ADD, RA_POSTERIZE, RA_BRIGHTNESS, RA_CONTRAST, RA_COLOR,
 RA_SHARPNESS, RA_AFFINE) = range(12)             # word 0 of a record of ap_randaug_u8 (AP_RA_*)


def randaug_u8(u8, records, n_layers, fill, layout="nchw", out=None, scratch=None, host_records=None):
    """uint8 [B,3,S,S] (layout "nchw") or [B,S,S,3] ("nhwc") -> a new uint8 batch of the same shape: image b goes through its n_layers
    records (int32, on the device, [B, n_layers, RANDAUG_RECORD_WORDS]: op code RA_*, filter RESAMPLE_*, an int argument, a float32
    argument, six float64 affine coefficients) in order, each op byte for byte what Pillow makes of it, one launch per layer
    (include/autoprog_hip.h, ap_randaug_u8).  `fill`: the (R, G, B) bytes of pixels an affine op maps from outside the image.  The input is
    not modified.  `out` / `scratch`: uint8 device tensors of the input's shape to write into (scratch is only used with n_layers > 1;
    allocated when not given); `host_records`: a CPU copy of `records` whose op and filter codes are checked before the launch."""
    (B, S, W), n_layers = _u8_batch("randaug_u8", u8, layout), int(n_layers)
    if S != W:
        raise AutoProgHipError("randaug_u8: square images, got %s as %s" % (tuple(u8.shape), layout))
    fill = tuple(int(v) for v in fill)
    if not 1 <= n_layers <= RANDAUG_MAX_LAYERS or len(fill) != 3 or min(fill) < 0 or max(fill) > 255:
        raise AutoProgHipError("randaug_u8: n_layers 1..%d and three fill bytes, got %d and %s" % (RANDAUG_MAX_LAYERS, n_layers, fill))
    host = _host_records("randaug_u8", records, host_records, B * n_layers * RANDAUG_RECORD_WORDS, torch.int32)
    if out is None:
        out = torch.empty_like(u8)
    elif tuple(_req(out, torch.uint8, "out").shape) != tuple(u8.shape):
        raise AutoProgHipError("randaug_u8: out must be %s, got %s" % (tuple(u8.shape), tuple(out.shape)))
    a = RandAugArgs()
    if n_layers > 1:
        if scratch is None:
            scratch = torch.empty_like(u8)
        elif tuple(_req(scratch, torch.uint8, "scratch").shape) != tuple(u8.shape):
            raise AutoProgHipError("randaug_u8: scratch must be %s, got %s" % (tuple(u8.shape), tuple(scratch.shape)))
        a.scratch = scratch.data_ptr()
    a.u8, a.layout, a.B, a.S = u8.data_ptr(), int(layout == "nhwc"), B, S
    a.out, a.records, a.n_layers = out.data_ptr(), records.data_ptr(), n_layers
    a.fill[0], a.fill[1], a.fill[2] = fill
    a.records_host = host
    check(lib.ap_randaug_u8(ctypes.byref(a), _stream()), "ap_randaug_u8")
    return out


# ------------------------------------------------------------------------------------- token labels from stored top-k label maps
LABEL_MAP_BOX_WORDS = 8                           # a record of ap_label_map_crop: x1, y1, x2, y2, flip (fp32), three zero words
LABEL_MAP_MAX_K = 8                               # pairs kept per bin: the mix-token class row of the loss carries 2 K <= 16


def _label_map_view(t, name):
    """a [B,Kin,Hm,Wm] device tensor whose images are contiguous (any stride between images, e.g. one half of tlt's [B,2,Kin,Hm,Wm])"""
    if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 4):
        raise AutoProgHipError("label_map_crop: %s must be a [B,Kin,Hm,Wm] CUDA tensor (the HIP path has no CPU fallback)" % name)
    _, Kin, Hm, Wm = t.shape
    if t.shape[0] and tuple(t.stride()[1:]) != (Hm * Wm, Wm, 1):
        raise AutoProgHipError("label_map_crop: the [Kin,Hm,Wm] block of every image of %s must be contiguous" % name)
    return t


def label_map_crop(scores, classes, labels, boxes, P, K, C, out=None, dropped=None, host_records=None):
    """stored top-k label maps -> the arrays of a SparseTokenLabelTarget at the token grid P, in one launch (include/autoprog_hip.h,
    ap_label_map_crop): scores fp16 / fp32 [B,Kin,Hm,Wm], classes the same shape in the scores' dtype or int32 (both may be views with
    their own stride between images), labels int64 [B], boxes fp32 on the device, B records x1, y1, x2, y2 (map pixel units), flip, 0, 0, 0.
    Slot 0 of the result is (label, 1), slot 1 the box's pooled top-K, slots 2.. those of the P x P ROI-align bins, flipped with the image.
    `out`: (idx int32, val fp32), both [B, 2 + P P, K] and contiguous, to write into; `dropped`: fp32 [B, 1 + P P] that receives the
    score mass of the classes beyond K per bin; `host_records`: a CPU copy of `boxes`, validated before the launch.  -> (idx, val)"""
    _label_map_view(scores, "scores"); _label_map_view(classes, "classes")
    _req(labels, torch.int64, "labels")
    if scores.dtype not in (torch.float16, torch.float32) or classes.dtype not in (scores.dtype, torch.int32):
        raise AutoProgHipError("label_map_crop: fp16 or fp32 scores, classes in the same dtype or int32 (got %s, %s)" % (scores.dtype, classes.dtype))
    B, Kin, Hm, Wm = scores.shape
    P, K, C = int(P), int(K), int(C)
    if tuple(classes.shape) != (B, Kin, Hm, Wm) or labels.numel() != B or classes.device != scores.device:
        raise AutoProgHipError("label_map_crop: scores and classes [B,Kin,Hm,Wm] on one device, labels [B]")
    a = LabelMapCropArgs()
    a.boxes_host = _host_records("label_map_crop", boxes, host_records, B * LABEL_MAP_BOX_WORDS, torch.float32, "boxes")
    shape = (B, 2 + P * P, K)
    if out is None:
        out = (torch.empty(shape, dtype=torch.int32, device=scores.device), torch.empty(shape, dtype=torch.float32, device=scores.device))
    idx, val = out
    if tuple(_req(idx, torch.int32, "idx").shape) != shape or tuple(_req(val, torch.float32, "val").shape) != shape:
        raise AutoProgHipError("label_map_crop: out must be (int32, fp32) tensors of shape %s" % (shape,))
    a.scores, a.score_dtype, a.score_stride = scores.data_ptr(), int(scores.dtype == torch.float32), scores.stride(0) if B else 0
    a.classes, a.class_dtype, a.class_stride = classes.data_ptr(), int(classes.dtype == torch.int32), classes.stride(0) if B else 0
    a.labels, a.boxes, a.idx, a.val = labels.data_ptr(), boxes.data_ptr(), idx.data_ptr(), val.data_ptr()
    if dropped is not None:
        if tuple(_req(dropped, torch.float32, "dropped").shape) != (B, 1 + P * P):
            raise AutoProgHipError("label_map_crop: dropped must be fp32 [%d, %d]" % (B, 1 + P * P))
        a.dropped = dropped.data_ptr()
    a.B, a.Kin, a.Hm, a.Wm, a.P, a.K, a.C = B, Kin, Hm, Wm, P, K, C
    check(lib.ap_label_map_crop(ctypes.byref(a), _stream()), "ap_label_map_crop")
    return idx, val


# ------------------------------------------------------------------------------------- stem 7x7 / stride 2 convolution (3 -> 64)
def resize_bilinear_s2d16(x, size):
    """fp32 [B,3,Hi,Wi] -> bf16 [B,size/2,size/2,16]: bilinear resize (F.interpolate align_corners=False) in the space-to-depth
    layout conv7_s2d reads (size even)"""
    _req(x, torch.float32, "x")
    B, C, Hi, Wi = x.shape
    if C != 3 or size % 2:
        raise AutoProgHipError("resize_bilinear_s2d16: 3 channels and an even output size (got C=%d, size=%d)" % (C, size))
    y = torch.empty((B, size // 2, size // 2, 16), dtype=BF16, device=x.device)
    check(lib.ap_resize_bilinear_s2d16(x.data_ptr(), y.data_ptr(), B, Hi, Wi, size, size, _stream()), "ap_resize_bilinear_s2d16")
    return y


def conv7_pack(weight):
    """fp32 [64,3,7,7] -> packed operand; [128,3,7,7] (VOLO-D4 / D5 stem): the two 64-channel halves' operands, one behind the other"""
    _req(weight, torch.float32, "weight")
    if tuple(weight.shape) not in ((64, 3, 7, 7), (128, 3, 7, 7)):
        raise AutoProgHipError("conv7_s2d handles 3 -> 64 / 128 channels, 7x7 (got %s)" % (tuple(weight.shape),))
    halves = weight.shape[0] // 64
    w = weight.contiguous()
    wp = torch.empty(halves * 16 * 64 * 16, dtype=BF16, device=weight.device)
    for h in range(halves):
        check(lib.ap_conv7_pack(w.data_ptr() + h * 64 * 147 * 4, wp.data_ptr() + h * 16 * 64 * 16 * 2, _stream()), "ap_conv7_pack")
    return wp


def conv7_s2d(xs, w_packed, want_stats=False):
    """xs [B,H,W,16] bf16 (space-to-depth image) -> [B,H,W,64] bf16 = conv7x7 / stride 2 / pad 3 of the image"""
    _req(xs, BF16, "xs"); _req(w_packed, BF16, "w_packed")
    B, H, W, C = xs.shape
    if C != 16:
        raise AutoProgHipError("conv7_s2d: 16 space-to-depth channels (got %d)" % C)
    if w_packed.numel() == 2 * 16 * 64 * 16:          # 128 output channels: the kernel once per 64-channel half, pixel stride 128
        y = torch.empty((B, H, W, 128), dtype=BF16, device=xs.device)
        rows = lib.ap_conv7_s2d_stat_rows(B, H, W)
        st = [torch.empty((rows, 2, 64), dtype=torch.float32, device=xs.device) if want_stats else None for _ in range(2)]
        for h in range(2):
            check(lib.ap_conv7_s2d_ld(xs.data_ptr(), w_packed.data_ptr() + h * 16 * 64 * 16 * 2, y.data_ptr() + h * 64 * 2, 128, B, H, W,
                                      st[h].data_ptr() if want_stats else None, _stream()), "ap_conv7_s2d_ld")
        return (y, torch.cat(st, dim=2)) if want_stats else y
    y = torch.empty((B, H, W, 64), dtype=BF16, device=xs.device)
    stats = torch.empty((lib.ap_conv7_s2d_stat_rows(B, H, W), 2, 64), dtype=torch.float32, device=xs.device) if want_stats else None
    check(lib.ap_conv7_s2d(xs.data_ptr(), w_packed.data_ptr(), y.data_ptr(), B, H, W, stats.data_ptr() if want_stats else None, _stream()),
          "ap_conv7_s2d")
    return (y, stats) if want_stats else y


def conv7_s2d_wgrad(xs, dz, dw):
    """dw (fp32 [64,3,7,7]) += weight gradient of conv7_s2d"""
    _req(xs, BF16, "xs"); _req(dz, BF16, "dz"); _req(dw, torch.float32, "dw")
    B, H, W, _ = xs.shape
    if tuple(dz.shape) == (B, H, W, 128) and tuple(dw.shape) == (128, 3, 7, 7):
        ws_bytes = lib.ap_conv7_s2d_wgrad_workspace(B, H, W)
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=xs.device)
        for h in range(2):
            check(lib.ap_conv7_s2d_wgrad_ld(xs.data_ptr(), dz.data_ptr() + h * 64 * 2, 128, dw.data_ptr() + h * 64 * 147 * 4, B, H, W, ws.data_ptr(), ws_bytes,
                                            _stream()), "ap_conv7_s2d_wgrad_ld")
        return dw
    if tuple(dz.shape) != (B, H, W, 64) or tuple(dw.shape) != (64, 3, 7, 7):
        raise AutoProgHipError("conv7_s2d_wgrad: shapes %s %s %s" % (tuple(xs.shape), tuple(dz.shape), tuple(dw.shape)))
    ws_bytes = lib.ap_conv7_s2d_wgrad_workspace(B, H, W)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=xs.device)
    check(lib.ap_conv7_s2d_wgrad(xs.data_ptr(), dz.data_ptr(), dw.data_ptr(), B, H, W, ws.data_ptr(), ws_bytes, _stream()), "ap_conv7_s2d_wgrad")
    return dw


def sumsq(x, out=None, workspace=None):
    """sum of squares of a flat fp32 slab (ap_sumsq_f32) -> fp32 device scalar [1]; `out` / `workspace` (fp64, ap_sumsq_workspace bytes) are
    allocated when not given"""
    _req(x, torch.float32, "x")
    out = torch.empty(1, dtype=torch.float32, device=x.device) if out is None else _req(out, torch.float32, "out")
    ws = torch.empty(lib.ap_sumsq_workspace() // 8, dtype=torch.float64, device=x.device) if workspace is None else _req(workspace, torch.float64, "workspace")
    check(lib.ap_sumsq_f32(x.data_ptr(), x.numel(), out.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream()), "ap_sumsq_f32")
    return out


def grad_health_workspace(n, n_seg):
    """bytes of workspace ap_grad_health needs for a slab of n elements in n_seg segments"""
    return int(lib.ap_grad_health_workspace(int(n), int(n_seg)))


def grad_health(g, seg_off, seg_sumsq, seg_nonfinite, state, workspace, beta1=0.9, beta2=0.999):
    """ap_grad_health: one pass over the fp32 gradient slab `g` against the device table `seg_off` (int64 [n_seg + 1], ascending from 0 to
    g.numel()).  Writes seg_sumsq (fp64 [n_seg]: sum of x^2 over the finite elements of each segment), seg_nonfinite (int32 [n_seg]: the
    inf / NaN elements) and commits the step into `state` (int32 [8], ap_guard_state: nonfinite, applied, skipped, consecutive, then the
    two bias corrections as fp32).  Every buffer is the caller's (workspace: fp64, grad_health_workspace bytes): nothing is allocated."""
    _req(g, torch.float32, "g"); _req(seg_off, torch.int64, "seg_off"); _req(seg_sumsq, torch.float64, "seg_sumsq")
    _req(seg_nonfinite, torch.int32, "seg_nonfinite"); _req(state, torch.int32, "state"); _req(workspace, torch.float64, "workspace")
    n_seg = seg_off.numel() - 1
    if n_seg < 1 or seg_sumsq.numel() != n_seg or seg_nonfinite.numel() != n_seg or state.numel() != 8:
        raise AutoProgHipError("grad_health: a table of n_seg + 1 bounds, n_seg sums, n_seg counts and a state of 8 words")
    check(lib.ap_grad_health(g.data_ptr(), g.numel(), seg_off.data_ptr(), n_seg, seg_sumsq.data_ptr(), seg_nonfinite.data_ptr(), state.data_ptr(),
                             float(beta1), float(beta2), workspace.data_ptr(), workspace.numel() * 8, _stream()), "ap_grad_health")
    return seg_sumsq, seg_nonfinite


def agc_short_max():
    """the longest unit ap_agc_clip reads once, one wave per unit; a longer one takes a workgroup and a second walk"""
    return int(lib.ap_agc_short_max())


def agc_clip(g, p, unit_off, unit_skip, clip_factor, eps=1e-3, grad_scale=1.0, unit_factor=None, counts=None):
    """ap_agc_clip: adaptive gradient clipping of the fp32 gradient slab `g`, in place, against the parameters `p` (fp32, as long as g,
    only read) and the device unit table `unit_off` (int64 [n_units + 1], ascending from 0 to g.numel()) / `unit_skip` (uint8 [n_units],
    non-zero: leave the unit alone).  Per unit: gn = grad_scale * ||g||, bound = max(||p||, eps) * clip_factor, and where gn >= bound
    the unit is multiplied by bound / max(gn, 1e-6); a unit with a non-finite gradient element is left alone (the rule in full:
    include/autoprog_hip.h).  unit_factor (fp32 [n_units], optional) receives the factor applied, 1 for a unit left alone; counts (int32
    [2], optional) {clipped units, non-finite units}.  Every buffer is the caller's: nothing is allocated."""
    _req(g, torch.float32, "g"); _req(p, torch.float32, "p"); _req(unit_off, torch.int64, "unit_off"); _req(unit_skip, torch.uint8, "unit_skip")
    n_units = unit_off.numel() - 1
    if n_units < 1 or unit_skip.numel() != n_units or p.numel() != g.numel():
        raise AutoProgHipError("agc_clip: p as long as g, a table of n_units + 1 bounds and n_units skip bytes")
    if unit_factor is not None and _req(unit_factor, torch.float32, "unit_factor").numel() != n_units:
        raise AutoProgHipError("agc_clip: unit_factor holds one fp32 per unit")
    if counts is not None and _req(counts, torch.int32, "counts").numel() != 2:
        raise AutoProgHipError("agc_clip: counts holds two int32")
    check(lib.ap_agc_clip(g.data_ptr(), p.data_ptr(), g.numel(), unit_off.data_ptr(), unit_skip.data_ptr(), n_units, float(clip_factor), float(eps),
                          float(grad_scale), unit_factor.data_ptr() if unit_factor is not None else None,
                          counts.data_ptr() if counts is not None else None, _stream()), "ap_agc_clip")
    return g


def lamb_chunk():
    """the most elements one chunk of ap_lamb_ema_step's work table holds (a multiple of 4)"""
    return int(lib.ap_lamb_chunk())


def lamb_chunk_table(offsets, chunk=None):
    """the work table of ap_lamb_ema_step for tensors that sit back to back at `offsets` (one entry more than there are tensors, ascending
    from 0): every tensor cut into chunks of at most `chunk` (default lamb_chunk()) consecutive elements, none crossing a tensor, tensors
    and chunks ascending.  -> {"start": int64 [n_chunks], "len": int32 [n_chunks], "tensor": int32 [n_chunks], "first": int32 [n_tensors
    + 1] -- the first chunk of every tensor}, numpy arrays on the host.  An empty tensor has no chunk.  Needs no device."""
    import numpy as np
    ch = lamb_chunk() if chunk is None else int(chunk)
    if ch < 4 or ch % 4:
        raise ValueError("lamb_chunk_table: a chunk holds a positive multiple of 4 elements, not %d" % ch)
    off = np.asarray(offsets, dtype=np.int64)
    if off.ndim != 1 or off.size < 2 or off[0] != 0 or (np.diff(off) < 0).any():
        raise ValueError("lamb_chunk_table: offsets ascend from 0 and hold one entry more than there are tensors")
    per = (np.diff(off) + ch - 1) // ch
    first = np.concatenate([[0], np.cumsum(per)])
    tensor = np.repeat(np.arange(off.size - 1), per)
    within = np.arange(int(first[-1])) - first[tensor]
    start = off[tensor] + within * ch
    length = np.minimum(ch, off[tensor + 1] - start)
    return {"start": start.astype(np.int64), "len": length.astype(np.int32), "tensor": tensor.astype(np.int32), "first": first.astype(np.int32)}


def lamb_pack_chunks(table):
    """a lamb_chunk_table as the two HOST tensors the kernel's tables are copied from: the 16-byte {int64 start, int32 length, int32 tensor}
    records as uint8 [n_chunks * 16], and `first` as int32"""
    import numpy as np
    rec = np.zeros(table["start"].size, dtype=np.dtype([("start", "<i8"), ("len", "<i4"), ("tensor", "<i4")]))
    rec["start"], rec["len"], rec["tensor"] = table["start"], table["len"], table["tensor"]
    return torch.from_numpy(rec.view(np.uint8).copy()), torch.from_numpy(np.ascontiguousarray(table["first"], dtype=np.int32))


def lamb_ema_step(p, g, m, v, group_id, group_tab, chunks, first, trust, workspace, step, beta1=0.9, beta2=0.999, eps=1e-6, grad_scale=1.0,
                  gnorm_sq=None, max_norm=0.0, clip_value=0.0, scalars_ptr=None, ema=(), ema_decay=(), p16=None, ema16=None, guard=None,
                  always_adapt=False, trust_clip=False, grid_cap=0, passes=0):
    """ap_lamb_ema_step: one LAMB + EMA update of the fp32 slabs p, m, v from the gradient slab g (only read), one trust ratio per tensor
    (the rule in full: include/autoprog_hip.h).  group_id: uint8 per element; group_tab: fp32 [G, 2] of {lr * lr_scale, weight_decay};
    chunks / first: the device copies of lamb_pack_chunks(lamb_chunk_table(offsets)); trust: fp32 [3, n_tensors], receives wn, un, phi of
    an applied step; workspace: fp64 [2 * n_chunks], its contents do not matter.  ema / ema_decay: up to four fp32 slabs and their decays;
    p16: the bf16 weight slab or None; ema16: None or a list as long as `ema` of bf16 slabs / None; guard: the int32 [8] ap_guard_state
    record of ops.grad_health, or None.  scalars_ptr: the device address of {lr, 1 - beta1^t, sqrt(1 - beta2^t)} (graph.StepScalars.adam_ptr)
    in the place of `step`.  grid_cap: workgroups of the two sweeping launches (0: the default); passes: bit 0 the norms, bit 1 the trust
    ratios, bit 2 the update (0: all).  Every buffer is the caller's: nothing is allocated."""
    for t, name in ((p, "p"), (g, "g"), (m, "m"), (v, "v"), (group_tab, "group_tab"), (trust, "trust")):
        _req(t, torch.float32, name)
    _req(group_id, torch.uint8, "group_id"); _req(chunks, torch.uint8, "chunks"); _req(first, torch.int32, "first"); _req(workspace, torch.float64, "workspace")
    n, n_chunks, n_tensors = p.numel(), chunks.numel() // 16, first.numel() - 1
    if not (g.numel() >= n and m.numel() == n and v.numel() == n and group_id.numel() >= n):
        raise AutoProgHipError("lamb_ema_step: g, m, v and group_id as long as p")
    if n_chunks < 1 or chunks.numel() != 16 * n_chunks or n_tensors < 1 or trust.numel() != 3 * n_tensors or workspace.numel() < 2 * n_chunks:
        raise AutoProgHipError("lamb_ema_step: 16 bytes per chunk, n_tensors + 1 first chunks, trust [3, n_tensors], two fp64 of workspace per chunk")
    if group_tab.dim() != 2 or group_tab.shape[1] != 2:
        raise AutoProgHipError("lamb_ema_step: group_tab is [G, 2]")
    ema, ema_decay = list(ema), list(ema_decay)
    if len(ema) > 4 or len(ema) != len(ema_decay) or any(_req(e, torch.float32, "ema").numel() != n for e in ema):
        raise AutoProgHipError("lamb_ema_step: up to four EMA slabs as long as p, one decay each")
    ema_ptrs = (ctypes.c_void_p * 4)(*[e.data_ptr() for e in ema])
    decays = (ctypes.c_float * 4)(*ema_decay)
    e16 = None
    if ema16 is not None:
        if len(ema16) != len(ema) or any(e is not None and _req(e, BF16, "ema16").numel() != n for e in ema16):
            raise AutoProgHipError("lamb_ema_step: ema16 holds one bf16 slab as long as p, or None, per EMA copy")
        e16 = (ctypes.c_void_p * 4)(*[e.data_ptr() if e is not None else None for e in ema16])
    if p16 is not None and _req(p16, BF16, "p16").numel() != n:
        raise AutoProgHipError("lamb_ema_step: p16 as long as p")
    if guard is not None and _req(guard, torch.int32, "guard").numel() != 8:
        raise AutoProgHipError("lamb_ema_step: the guard record holds 8 words")
    check(lib.ap_lamb_ema_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), group_id.data_ptr(), n, float(beta1), float(beta2), float(eps),
                               int(step), float(grad_scale), gnorm_sq.data_ptr() if gnorm_sq is not None else None, float(max_norm), float(clip_value),
                               scalars_ptr, ema_ptrs, decays, len(ema), p16.data_ptr() if p16 is not None else None, e16,
                               guard.data_ptr() if guard is not None else None, group_tab.data_ptr(), group_tab.shape[0], chunks.data_ptr(), n_chunks,
                               first.data_ptr(), n_tensors, int(bool(always_adapt)), int(bool(trust_clip)), trust.data_ptr(), workspace.data_ptr(),
                               workspace.numel() * 8, int(grid_cap), int(passes), _stream()), "ap_lamb_ema_step")
    return trust
