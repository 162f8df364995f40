"""No result depends on uninitialised device memory.

The library allocates nothing itself: every output, side output and workspace a kernel receives is a torch.empty made in Python, and the ABI
builds on that openly ("Only the N logical columns are written ... padding may hold anything", include/autoprog_hip.h at ap_gemm_nt).  A
parity test runs on whatever the caching allocator hands back -- in a fresh process very often zeros -- so a kernel that reads a pad column,
a workspace slot or a side-output byte before anything wrote it passes every tolerance test and fails in the middle of a long run.

Here every case runs four times under tests/_poison_alloc.py: `zero`, `zero` again (the control: a case that is not reproducible proves
nothing), `nan` (0xFF bytes) and `huge` (0x7F bytes: finite, so it survives the max / min instructions that drop a NaN).  The DOCUMENTED
outputs -- the logical columns where the header leaves the padding unspecified, whole tensors where it promises zeros -- must be
bit-identical across the four runs and finite, and every allocation site of the wrappers a case declares in `covers` must have been hit.
tests/test_poison_alloc_host.py holds the table against the source: every empty-family call under autoprog_amd/ belongs to some case.

Part A is one table over the allocating wrappers of ops.py (kernel level, chained where the product chains them through a padded view);
part B builds whole training / validation / loader scenarios twice from the same seeds.  Everything runs with ops.deterministic = True.
Integer buffers are filled with 1, never with a bit pattern (a wild index would be a fault, not a finding): what each kernel does with its
integer buffers was read first -- ap_grad_health zeroes its ticket words itself and writes every (chunk, segment) slot its second kernel
reads (csrc/optim.hip), ap_softmax_topk_rows, ap_classify_stats and ap_label_map_crop only write their index outputs.
"""
import numpy as np
import pytest
import torch

from tests._poison_alloc import poisoned, repoison, site_hit, sites_of
from tests._tilecheck import nan_padded, round_up

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
FILL_RUNS = ("zero", "zero", "nan", "huge")
TOL_F32 = 3e-3            # (tests/test_gpu_localized.py) only where fp32 atomics remain by design; no case below needs it


# ---------------------------------------------------------------------------------------------------------------------- seeded inputs
def rnd(*shape, scale=1.0, seed=0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(BF16)


def frand(*shape, seed=0, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift


def urand(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def bytes_(*shape, seed=0):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def dev(t):
    return t.cuda().contiguous()


def padn(t, extra=8):
    """an operand whose leading dimension is widened by NaN columns (NaN guard rows around it), on the device: what a caller may pass"""
    t2 = t.reshape(-1, t.shape[-1])
    return nan_padded(t2, round_up(t2.shape[1], 8) + extra, device="cuda")


def padz(t, ld=None):
    """an operand padded with zeros: what the contract promises of gradient matrices"""
    ld = round_up(t.shape[1], 8) if ld is None else ld
    return dev(torch.nn.functional.pad(t, (0, ld - t.shape[1])))


def scalar(v):
    return torch.tensor([float(v)], dtype=torch.float32).cuda()


def zeros(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).cuda()


def bn_stats(x):
    xf = x.float().reshape(-1, x.shape[-1])
    return dev(xf.mean(0)), dev((xf.var(0, unbiased=False) + 1e-5).rsqrt())


# ---------------------------------------------------------------------------------------------------------------------- the cases of part A
class Case:
    def __init__(self, name, covers, run):
        self.name, self.covers, self.run = name, tuple(covers), run


def _casts(ops):
    w = dev(frand(37, 50, seed=1))
    img = dev(frand(1, 3, 37, 37, seed=2))
    return {"cast_bf16": ops.cast_bf16(w), "cast_f32": ops.cast_f32(dev(rnd(37, 50, seed=3))),
            "cast_transpose (pad zero)": ops.cast_transpose_bf16(w),                       # [50, 40]: columns 37..39 are promised zero
            "resize_nhwc": ops.resize_bilinear_nhwc(img, 20), "resize_s2d16 (channels 12..15 zero)": ops.resize_bilinear_s2d16(img, 20)}


def _droppath(ops):
    u, keep = dev(urand(5, 7, seed=1)), dev(torch.tensor([1.0, 0.9, 0.5, 0.97, 0.3]))
    f, m, tm = ops.droppath_masks(u, keep, 13)                                          # token rows of 96 for 91 tokens: zero padding promised
    f2, m2, _ = ops.droppath_masks(u, keep, 0)
    return {"factor": f, "mask": m, "token_mask (pad zero)": tm, "factor0": f2, "mask0": m2}


def _layernorm(ops):
    rows, C = 33, 64
    x, dy, dres = dev(rnd(rows, C, scale=2.5, shift=1.5, seed=1)), dev(rnd(rows, C, seed=2)), dev(rnd(rows, C, seed=3))
    g, b = dev(frand(C, seed=4, scale=0.3, shift=1.0)), dev(frand(C, seed=5, scale=0.2))
    y, mean, rstd = ops.layernorm_fwd(x, g, b, 1e-5)
    amax = zeros(1)
    y2, mean2, rstd2, y8 = ops.layernorm_fwd(x, g, b, 1e-5, fp8=(scalar(16.0), amax))
    dg, db, dg2, db2 = zeros(C), zeros(C), zeros(C), zeros(C)
    dx = ops.layernorm_bwd(dy, x, g, mean, rstd, dres, dg, db)
    items = []
    dx2 = ops.layernorm_bwd(dy, x, g, mean, rstd, None, dg2, db2, defer=items)
    ops.layernorm_bwd_reduce_batched(items)
    return {"y": y, "mean": mean, "rstd": rstd, "y (fp8 launch)": y2, "mean2": mean2, "rstd2": rstd2, "y8_e4m3": y8, "amax": amax,
            "dx": dx, "dgamma": dg, "dbeta": db, "dx (deferred)": dx2, "dgamma (deferred)": dg2, "dbeta (deferred)": db2}


def _mlp_fused(ops):
    """layernorm_fwd into the fused MLP, forward and backward; the LayerNorm-in-launch flavour; the forward-only entry"""
    m, C, H, rps = 128, 384, 1152, 64
    xin = dev(rnd(m, C, scale=2.5, shift=1.5, seed=1))
    w1, w2 = rnd(H, C, scale=C ** -0.5, seed=2), rnd(C, H, scale=H ** -0.5, seed=3)
    b1, b2 = dev(frand(H, seed=4, scale=0.3)), dev(frand(C, seed=5, scale=0.3))
    keep = dev(torch.tensor([0.0, 1.0]))
    rs = dev(torch.tensor([0.0, 1.25]))
    lg, lb = dev(frand(C, seed=8, scale=0.3, shift=1.0)), dev(frand(C, seed=9, scale=0.2))
    dy = dev(rnd(m, C, seed=7))
    kw = dict(bias1=b1, bias2=b2, row_scale_hidden=keep, row_scale_out=rs, rows_per_scale=rps, residual=xin)
    y, mean, rstd = ops.layernorm_fwd(xin, lg, lb, 1e-5)
    fwd = ops.mlp_fused(y, dev(w1), dev(w2), **kw)
    fln = ops.mlp_fused(None, dev(w1), dev(w2), ln=(xin, lg, lb, 1e-5), **kw)
    inf = ops.mlp_fused_infer(y, dev(w1), dev(w2), **kw)
    assert fwd is not None and fln is not None and inf is not None, "ap_mlp_fused refused a launch it is built for"
    bwd = ops.mlp_fused(dy, dev(w2.t()), dev(w1.t()), backward=True, row_scale_hidden=rs, rows_per_scale=rps, codes=fwd[2])
    assert bwd is not None
    return {"ln y": y, "out": fwd[0], "hidden": fwd[1], "codes": fwd[2], "out (ln)": fln[0], "hidden (ln)": fln[1], "codes (ln)": fln[2],
            "xn": fln[3], "mean": fln[4], "rstd": fln[5], "out (infer)": inf, "dx": bwd[0], "dh": bwd[1]}


def _gemm_flavours(ops, M, N, K, flavours, rps=64):
    """ap_gemm_nt at one shape: A with lda = K + 8 and W with ldb = K + 16 (NaN padding), the residual with ldr = N + 8, mul_by / mul_by8
    with the output's leading dimension (NaN / 0xA5 padding); every output allocated by the wrapper -> the logical columns"""
    a, w = padn(rnd(M, K, seed=1), 8), padn(rnd(N, K, scale=K ** -0.5, seed=2), 16)
    n8 = round_up(N, 8)
    bias = dev(frand(N, seed=3))
    groups = (M + rps - 1) // rps
    rs = (urand(groups, seed=5) > 0.2).float() / 0.8
    rs[0], rs[-1] = 0.0, 1.25
    out = {}
    for f in flavours:
        if f == "plain":
            out[f] = ops.gemm_nt(a, w, n=N, k=K)[:, :N]
        elif f == "bias_res_rs":
            res = nan_padded(rnd(M, N, seed=4), n8 + 8, device="cuda")
            out[f] = ops.gemm_nt(a, w, n=N, k=K, bias=bias, residual=res, row_scale=dev(rs), rows_per_scale=rps)[:, :N]
        elif f == "gelu8":
            codes = torch.empty(M, n8, dtype=torch.uint8, device="cuda")
            out[f] = ops.gemm_nt(a, w, n=N, k=K, bias=bias, gelu=True, preact_out=codes, preact_grad=2)[:, :N]
            out[f + " codes"] = codes[:, :N]
        elif f == "table":
            out[f] = ops.gemm_nt(a, w, n=N, k=K, bias=bias, gelu="table")[:, :N]
        elif f == "mulby":
            out[f] = ops.gemm_nt(a, w, n=N, k=K, mul_by=nan_padded(rnd(M, N, seed=6), n8, device="cuda"))[:, :N]
        elif f == "mul8":
            out[f] = ops.gemm_nt(a, w, n=N, k=K, mul_by=nan_padded(bytes_(M, N, seed=7), n8, device="cuda"))[:, :N]
        else:
            raise ValueError(f)
    return out


_ALL = ("plain", "bias_res_rs", "gelu8", "table", "mulby", "mul8")


def _gemm_q8_chain(ops):
    """the fp8 chain of an MLP at the smallest shape the 8-phase kernel takes: fc1 with 8-bit gelu' codes; fc2's input gradient through
    mul_by8 with its e4m3 copy (q8) into the fp8 input-gradient product; quantize_fp8 / quantize_bf8 into the fp8 forward product (with
    its own q8) and the fp8 weight gradient.  And the launch gelu = "table" cannot serve (M <= 256), which allocates its own side buffer."""
    M, C, H = 4160, 384, 1152
    assert ops.gemm_nt_emits_q8(M, H, C, torch.empty(0, dtype=torch.uint8)) and ops.gemm_nt_fp8_emits(M, H, C)
    x, dy = dev(rnd(M, C, seed=1)), dev(rnd(M, C, seed=2))
    w1, w2 = rnd(H, C, scale=C ** -0.5, seed=3), rnd(C, H, scale=H ** -0.5, seed=4)
    b1 = dev(frand(H, seed=5, scale=0.3))
    codes = torch.empty(M, H, dtype=torch.uint8, device="cuda")
    h = ops.gemm_nt(x, dev(w1), bias=b1, gelu=True, preact_out=codes, preact_grad=2)
    s_dh, a_dh = scalar(64.0), zeros(1)
    dh, dh8 = ops.gemm_nt(dy, dev(w2.t()), mul_by=codes, q8=(s_dh, a_dh))
    s_w, s_x, a_x = scalar(256.0), scalar(32.0), zeros(1)
    w1t8 = ops.quantize_fp8(dev(w1.t()), s_w)
    dx = ops.gemm_nt_fp8(dh8, w1t8, scalar(1 / 64.0), scalar(1 / 256.0))
    x8, w18 = ops.quantize_fp8(x, s_x, a_x), ops.quantize_fp8(dev(w1), s_w)
    codes2 = torch.empty(M, H, dtype=torch.uint8, device="cuda")
    s_h, a_h = scalar(32.0), zeros(1)
    h_fp8, h8 = ops.gemm_nt_fp8(x8, w18, scalar(1 / 32.0), scalar(1 / 256.0), bias=b1, gelu=True, preact_out=codes2, preact_grad=2, q8=(s_h, a_h))
    s_g, a_g, db = scalar(1024.0), zeros(1), zeros(H)
    g8 = ops.quantize_bf8(dh, s_g, a_g, colsum=db)
    dw = zeros(H, C)
    ops.gemm_tn8_acc_grouped([ops.Tn8Problem(g8, x8, dw, None, None, scalar(1 / 1024.0), scalar(1 / 32.0))])
    small = _gemm_flavours(ops, 130, 32, 32, ("table",), rps=16)
    return {"h": h, "codes": codes, "dh": dh, "dh8_e4m3": dh8, "amax dh": a_dh, "w1t8_e4m3": w1t8, "dx": dx[:, :C], "x8_e4m3": x8, "amax x": a_x,
            "h (fp8)": h_fp8, "h8_e4m3": h8, "amax h": a_h, "codes (fp8)": codes2, "g8": g8, "amax g": a_g, "db": db, "dw": dw,
            "table without a kernel": small["table"]}


def _wgrad_grouped(ops):
    """ap_gemm_tn_acc_grouped in its workspace mode: a tile-kernel problem next to ragged ones, operands with NaN padding, C and the column
    sum from a seeded non-zero base (the contract is +=)"""
    probs, out = [], {}
    for i, (M, N1, N2) in enumerate([(4160, 192, 384), (130, 200, 75), (77, 37, 96)]):
        a, b = padn(rnd(M, N1, seed=10 + i), 8), padn(rnd(M, N2, seed=40 + i), 16)
        c = torch.empty(N1, round_up(N2, 8), device="cuda")
        c[:, :N2] = frand(N1, N2, seed=70 + i).cuda()
        cs = dev(frand(N1, seed=90 + i))
        probs.append((a, b, c, N1, N2, cs))
        out["C%d" % i], out["colsum%d" % i] = c[:, :N2], cs
    ops.gemm_tn_acc_grouped(probs)
    return out


def _patch_gemm(ops):
    B, H, W, C, k, N = 2, 16, 16, 64, 4, 44
    x = dev(rnd(B, H, W, C, scale=1.5, shift=0.3, seed=1))
    wmat = rnd(N, k * k * C, scale=(k * k * C) ** -0.5, seed=2)
    bias = dev(frand(N, seed=3))
    mean, rstd = bn_stats(x)
    gamma, beta = dev(urand(C, seed=4) + 0.5), dev(frand(C, seed=5, scale=0.3))
    y = ops.gemm_nt_patch_fwd(x, dev(wmat), bias, k)
    ybn = ops.gemm_nt_patch_fwd(x, dev(wmat), bias, k, bn_in=(mean, rstd, gamma, beta))
    dy = padz(rnd(B * (H // k) * (W // k), N, seed=6))                                   # (a gradient matrix: zero padding by contract)
    dx = ops.gemm_nt_patch_dgrad(dy, padz(wmat.t().contiguous()), (B, H, W, C), k)
    return {"y": y[:, :N], "y (bn input)": ybn[:, :N], "dx": dx}


def _outlook_chain(ops):
    """ap_gemm_nt's logits (N = heads * 81 in round_up(N, 8) columns, the padding never written) into the outlook kernels"""
    out = {}
    for B, H, W, heads, K in [(3, 19, 19, 6, 192), (2, 7, 7, 2, 64), (1, 5, 9, 1, 64)]:
        C, h, w, N = heads * 32, (H + 1) // 2, (W + 1) // 2, heads * 81
        v, dy = dev(rnd(B, H, W, C, seed=1)), dev(rnd(B, H, W, C, seed=3))
        a, wt = padn(rnd(B * h * w, K, seed=4), 8), padn(rnd(N, K, scale=2.0 * K ** -0.5, seed=5), 16)
        logits = ops.gemm_nt(a, wt, n=N, k=K)
        y = ops.outlook_fwd(v, logits, heads, 32 ** -0.5)
        dv, dl = ops.outlook_bwd(v, logits, dy, heads, 32 ** -0.5)
        tag = " %dx%dx%dx%d" % (B, H, W, heads)
        out.update({"logits" + tag: logits[:, :N], "y" + tag: y, "dv" + tag: dv, "dlogits (pad zero)" + tag: dl})
    out["avgpool"] = ops.avgpool2_fwd(dev(rnd(1, 5, 9, 32, seed=6)))
    return out


def _mhsa(ops):
    out = {}
    for B, N, heads, hd in [(2, 25, 2, 32), (2, 50, 3, 48), (2, 257, 1, 32)]:
        C = heads * hd
        qkv, do = dev(rnd(B * N, 3 * C, seed=1)), dev(rnd(B * N, C, seed=2))
        keep = dev(torch.tensor([0.0, 1.25]))
        tag = " %dx%dx%dx%d" % (B, N, heads, hd)
        if ops.mhsa_emits_fp8(N, hd):
            amax = zeros(1)
            o, lse, o8 = ops.mhsa_fwd(qkv, B, N, heads, hd ** -0.5, out_row_scale=keep, fp8=(scalar(32.0), amax))
            out.update({"out8_e4m3" + tag: o8, "amax" + tag: amax, "out (fp8 launch)" + tag: o})
        o, lse = ops.mhsa_fwd(qkv, B, N, heads, hd ** -0.5)
        out.update({"out" + tag: o, "lse" + tag: lse, "dqkv" + tag: ops.mhsa_bwd(qkv, o, do, lse, B, N, heads, hd ** -0.5)})
    return out


def _class_attn(ops):
    B, N, heads, hd = 4, 17, 1, 32
    C = heads * hd
    q, kv, do = dev(rnd(B, C, seed=1)), dev(rnd(B * N, 2 * C, seed=2)), dev(rnd(B, C, seed=3))
    o, probs = ops.class_attn_fwd(q, kv, B, N, heads, hd ** -0.5)
    dq, dkv = ops.class_attn_bwd(q, kv, probs, do, B, N, heads, hd ** -0.5)
    kvt, kvc = dev(rnd(B * (N - 1), 2 * C, seed=4)), dev(rnd(B, 2 * C, seed=5))       # the split layout: key 0 of image b is kv_cls[b]
    o2, probs2 = ops.class_attn_fwd(q, kvt, B, N, heads, hd ** -0.5, kv_cls=kvc)
    dq2, dkv2, dkc2 = ops.class_attn_bwd(q, kvt, probs2, do, B, N, heads, hd ** -0.5, kv_cls=kvc)
    return {"out": o, "probs": probs, "dq": dq, "dkv": dkv, "out (split)": o2, "probs (split)": probs2, "dq (split)": dq2,
            "dkv (split)": dkv2, "dkv_cls": dkc2}


def _small(ops):
    x = dev(rnd(5, 12, 10, 32, seed=1))
    box = torch.tensor([1, 4, 2, 5], dtype=torch.int32).cuda()                          # {r0, r1, c0, c1} on the token-label grid, times 2
    xs = dev(rnd(6 * 49, 64, seed=2))
    sc = dev(torch.tensor([0.0, 1.25, 1.25, 0.0, 1.25, 1.25]))
    a, b = dev(rnd(4, 7, 7, 64, seed=3)), dev(rnd(1, 7, 7, 64, seed=4))
    out = {"swap": ops.mix_token_swap(x, 2, 8, 4, 10), "swap_dev": ops.mix_token_swap_dev(x, box.data_ptr(), 2),
           "loss_combine": ops.loss_combine(dev(frand(7, seed=5)), 0.5, dev(frand(3, seed=6)), 0.25),
           "row_scale": ops.row_scale(xs, sc, 49), "add_bcast": ops.add_bcast(a, b)}
    assert torch.equal(out["swap"], out["swap_dev"])
    slab = dev(frand(70001, seed=7))
    out["sumsq"] = ops.sumsq(slab)
    hi, wi, ho, wo, C = 5, 7, 9, 4, 6
    out["resample_grid"] = ops.resample_grid(dev(frand(hi, wi, C, seed=8)), dev(urand(ho, hi, seed=9)), dev(urand(wo, wi, seed=10)))
    return out


def _losses(ops):
    """the soft-target CE entry points (logits with NaN padding), ap_classify_stats, ap_distill_fwd_bwd, ap_softmax_topk_rows; and a
    10-class ap_gemm_nt (16 columns, 6 never written) into them by the product's two rules: functional.ce_rows, ops.padded_view_rows"""
    from autoprog_amd import functional as AF
    out = {}
    for B, N, C in [(2, 9, 20), (5, 1, 1000), (3, 1, 1027)]:                              # 1027 classes in 1032 columns: the narrowest wide row (> 1024)
        ld = round_up(C, 8)
        logits = nan_padded(rnd(B * N, C, scale=2.0, seed=B), ld, device="cuda")
        t = dev(urand(B, C, 2 + N, seed=11) * (urand(B, C, 2 + N, seed=12) < 0.05) + 0.1 / C)
        rl, dl = ops.soft_ce_fwd_bwd(logits, C, t[:, :, 2:], t.stride(0), t.stride(1), t.stride(2), N, 0.5 / (B * N), mix_lam=0.7, mix_batches=B)
        K = 5
        idx = torch.randint(0, C, (B, 2 + N, K), generator=torch.Generator().manual_seed(13)).to(torch.int32).cuda()
        val = dev(torch.softmax(frand(B, 2 + N, K, seed=14), -1) * 0.9)
        rl2, dl2 = ops.soft_ce_sparse_fwd_bwd(logits, C, idx[:, 2:], val[:, 2:], idx.stride(0), idx.stride(1), N, 0.1, 0.5 / (B * N))
        tag = " %dx%dx%d" % (B, N, C)
        out.update({"row_loss" + tag: rl, "dlogits (pad zero)" + tag: dl, "sparse row_loss" + tag: rl2, "sparse dlogits (pad zero)" + tag: dl2})
    # ---- the 10-class head: 16 rows = 2 images x 8 tokens
    B, N, C, K = 2, 8, 10, 64
    a, w = padn(rnd(B * N, K, seed=20), 8), padn(rnd(C, K, scale=2.0 * K ** -0.5, seed=21), 16)
    z = ops.gemm_nt(a, w, n=C, k=K)                                                      # [16, 16]: columns 10..15 hold whatever the allocator gave
    zt = ops.gemm_nt(padn(rnd(B * N, K, seed=22), 8), w, n=C, k=K)                       # a teacher's rows, the same way
    t = dev(torch.softmax(frand(B, C, N, seed=23), 1))
    rl, dl = ops.soft_ce_fwd_bwd(AF.ce_rows(z[:, :C]), C, t, t.stride(0), t.stride(1), t.stride(2), N, 1.0 / (B * N))
    view, tview = ops.padded_view_rows(z[:, :C]), ops.padded_view_rows(zt[:, :C])
    assert view.data_ptr() == z.data_ptr() and view.stride(0) == 16, "padded_view_rows copied what functional.linear would hand it"
    ki, kv = torch.empty(B, N, 3, dtype=torch.int32, device="cuda"), torch.empty(B, N, 3, dtype=torch.float32, device="cuda")
    ops.softmax_topk(view, C, 3, 1.0, ki, kv, N * 3, 3, N)
    labels = torch.tensor([3, 9, 0, -1, 10, 5, 5, 1] * 2, dtype=torch.int64).cuda()      # (-1 and 10: padding rows, nothing is read through them)
    loss, rank = ops.classify_stats(z, labels, C)
    out.update({"head logits": z[:, :C], "head row_loss": rl, "head dlogits (pad zero)": dl, "topk idx": ki, "topk val": kv,
                "classify loss": loss, "classify rank": rank})
    for mode in (0, 1):
        rl, ds = ops.distill_fwd_bwd(view, C, tview, mode, 1 / 3.0, 0.25)
        out.update({"distill row_loss %d" % mode: rl, "dstudent (pad zero) %d" % mode: ds})
    wide_s, wide_t = nan_padded(rnd(3, 1027, scale=2.0, seed=24), 1032, device="cuda"), nan_padded(rnd(3, 1027, scale=2.0, seed=25), 1040, device="cuda")
    rl, ds = ops.distill_fwd_bwd(wide_s[:, :1027], 1027, wide_t[:, :1027], 0, 0.5, 0.25)
    wi, wv = torch.empty(3, 4, dtype=torch.int32, device="cuda"), torch.empty(3, 4, dtype=torch.float32, device="cuda")
    ops.softmax_topk(wide_s[:, :1027], 1027, 4, 1.0, wi, wv, 4, 0, 1)
    out.update({"wide distill row_loss": rl, "wide dstudent (pad zero)": ds, "wide topk idx": wi, "wide topk val": wv})
    return out


def _stem3x3(ops, C):
    """the 3 x 3 stem convolutions at C channels with their BatchNorm + ReLU: forward with the partial statistics, BatchNorm from them,
    the fused input (C = 64), input gradient with the BatchNorm backward's first pass (C = 64), weight gradients"""
    B, H, W = 1, 7, 5
    x = dev(rnd(B, H, W, C, scale=1.5, shift=0.3, seed=1))
    dy = dev(rnd(B, H, W, C, seed=2))
    w = dev(frand(C, C, 3, 3, seed=3, scale=0.05))
    gamma, beta = dev(urand(C, seed=4) + 0.5), dev(frand(C, seed=5, scale=0.3))
    wf, wb = ops.conv3x3_pack(w)
    y, st = ops.conv3x3_c64(x, wf, True)
    y0 = ops.conv3x3_c64(x, wf)
    rm, rv = zeros(C), torch.ones(C).cuda()
    a, mean, rstd = ops.bn_relu_fwd(y, gamma, beta, rm, rv, True, 0.1, 1e-5, partials=st)
    dw = dev(frand(C, C, 3, 3, seed=6))
    ops.conv3x3_c64_wgrad(x, dy, dw)
    out = {"wf": wf, "wb": wb, "y": y, "stats": st, "y (no stats)": y0, "bn act": a, "bn mean": mean, "bn rstd": rstd, "running mean": rm,
           "running var": rv, "dx": ops.conv3x3_c64(dy, wb), "dw": dw}
    if C == 64:
        bn = (mean, rstd, gamma, beta)
        y2, st2 = ops.conv3x3_c64(y, wf, True, bn_in=bn)
        da, part = ops.conv3x3_c64_bwd_stats(dy, wb, y, bn)
        dg, db = zeros(C), zeros(C)
        dz = ops.bn_relu_bwd_partials(da, y, gamma, beta, mean, rstd, part, dg, db)
        dw2 = dev(frand(C, C, 3, 3, seed=7))
        ops.conv3x3_c64_wgrad(y, dy, dw2, bn_in=bn)
        out.update({"y (bn input)": y2, "stats (bn input)": st2, "da": da, "bwd partials": part, "dz": dz, "dgamma": dg, "dbeta": db, "dw (bn input)": dw2})
    return out


def _stem(ops):
    out = {"c%d %s" % (C, k): v for C in (64, 128) for k, v in _stem3x3(ops, C).items()}
    # ---- BatchNorm + ReLU on its own at (2, 5, 5, 8): the statistics pass, eval mode, statistics only, the backward with and without the activation
    x, dy = dev(rnd(2, 5, 5, 8, scale=1.5, shift=0.3, seed=11)), dev(rnd(2, 5, 5, 8, seed=12))
    gamma, beta = dev(urand(8, seed=13) + 0.5), dev(frand(8, seed=14, scale=0.3))
    rm, rv = zeros(8), torch.ones(8).cuda()
    y, mean, rstd = ops.bn_relu_fwd(x, gamma, beta, rm, rv, True, 0.1, 1e-5)
    ye, _, _ = ops.bn_relu_fwd(x, gamma, beta, rm, rv, False, 0.1, 1e-5)
    dg, db, dg2, db2 = zeros(8), zeros(8), zeros(8), zeros(8)
    dx = ops.bn_relu_bwd(dy, x, gamma, beta, mean, rstd, dg, db)
    dx2, act = ops.bn_relu_bwd(dy, x, gamma, beta, mean, rstd, dg2, db2, act_out=True)
    out.update({"bn y": y, "bn mean": mean, "bn rstd": rstd, "bn running mean": rm, "bn running var": rv, "bn y (eval)": ye, "bn dx": dx,
                "bn dgamma": dg, "bn dbeta": db, "bn dx (act)": dx2, "bn act": act, "bn dgamma (act)": dg2, "bn dbeta (act)": db2})
    # ---- the 7 x 7 / stride 2 stem at 64 and 128 output channels on an 18 x 18 space-to-depth map
    img = dev(frand(1, 3, 36, 36, seed=15))
    xs = ops.resize_bilinear_s2d16(img, 36)
    for Co in (64, 128):
        w = dev(frand(Co, 3, 7, 7, seed=16, scale=0.1))
        wp = ops.conv7_pack(w)
        y, st = ops.conv7_s2d(xs, wp, True)
        dz = dev(rnd(1, 18, 18, Co, seed=17))
        dw = dev(frand(Co, 3, 7, 7, seed=18))
        ops.conv7_s2d_wgrad(xs, dz, dw)
        out.update({"c7 %d packed" % Co: wp, "c7 %d y" % Co: y, "c7 %d stats" % Co: st, "c7 %d y (no stats)" % Co: ops.conv7_s2d(xs, wp), "c7 %d dw" % Co: dw})
    # statistics only (apply = False): the consumer normalises while it loads
    y, st = ops.conv7_s2d(xs, ops.conv7_pack(dev(frand(64, 3, 7, 7, seed=19, scale=0.1))), True)
    g64, b64 = dev(urand(64, seed=20) + 0.5), dev(frand(64, seed=21, scale=0.3))
    none, mean, rstd = ops.bn_relu_fwd(y, g64, b64, zeros(64), torch.ones(64).cuda(), True, 0.1, 1e-5, partials=st, apply=False)
    assert none is None
    out.update({"stats-only mean": mean, "stats-only rstd": rstd})
    return out


def _loader(ops):
    """the loader stages at kernel level and through their data objects: crop (two-tap and antialiased), RandAugment, the batch prep launch,
    token labels from stored maps; every record block travels through a PinnedRing"""
    from autoprog_amd import data as D
    B, Hc = 4, 40
    u8 = dev(bytes_(B, 3, Hc, Hc, seed=1))
    crop = D.DeviceRandomResizedCrop(seed=3)
    c1 = crop.crop(u8, 32)
    crop2 = D.DeviceRandomResizedCrop(seed=4, interpolation="random")
    c2 = crop2.crop(u8, 32)
    aug = D.DeviceRandAugment(seed=5)
    a1 = aug(c2).clone()
    host = aug.draw(B, 32)                                                                # the wrapper's own out / scratch
    a2 = ops.randaug_u8(c2, aug._ring.send(c2.device), aug.n_layers, aug.fill, host_records=host)
    prep = D.DeviceBatchPrep((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), cutmix_alpha=1.0, num_classes=10, re_prob=1.0, re_mode="pixel", seed=6)
    pb = prep.prep(a2)
    x16, x3 = pb.run(32, "s2d16"), pb.run(24, "nhwc")
    maps = torch.stack([urand(B, 6, 5, 5, seed=7) * 8, torch.randint(0, 10, (B, 6, 5, 5), generator=torch.Generator().manual_seed(8)).float()], 1).half()
    stored = D.StoredLabelMaps(torch.tensor([1, 9, 0, 4]), maps.cuda())
    lm = D.DeviceLabelMapCrop(k=4, num_classes=10)
    t = lm.target(stored, crop2, 32)
    recs = lm._ring.send(u8.device)
    idx, val = ops.label_map_crop(stored.scores, stored.classes, stored.labels, recs, 2, 4, 10)
    return {"crop": c1, "crop (antialiased)": c2, "randaug": a1, "randaug (own buffers)": a2, "prep s2d16": x16, "prep nhwc": x3,
            "label idx": t.idx, "label val": t.val, "label idx (own)": idx, "label val (own)": val}


O = "ops."
CASES = [
    Case("casts-and-resizes", [O + n for n in ("cast_bf16", "cast_f32", "cast_transpose_bf16", "resize_bilinear_nhwc", "resize_bilinear_s2d16")], _casts),
    Case("droppath-masks", [O + "droppath_masks"], _droppath),
    Case("layernorm-33x64", [O + "layernorm_fwd", O + "layernorm_bwd"], _layernorm),
    Case("layernorm-into-fused-mlp-128", [O + "_mlp_fused_args", O + "mlp_fused"], _mlp_fused),
    Case("gemm-few-rows-130x32x32", [], lambda ops: _gemm_flavours(ops, 130, 32, 32, _ALL, rps=16)),
    Case("gemm-few-rows-ragged-65x37x40", [], lambda ops: _gemm_flavours(ops, 65, 37, 40, _ALL, rps=16)),
    Case("gemm-few-rows-77x1000x384", [], lambda ops: _gemm_flavours(ops, 77, 1000, 384, ("plain", "bias_res_rs", "gelu8"), rps=16)),
    Case("gemm-8p-192-4100x384x384", [], lambda ops: _gemm_flavours(ops, 4100, 384, 384, _ALL)),
    Case("gemm-8p-224-row-tiles-4097x192x128", [], lambda ops: _gemm_flavours(ops, 4097, 192, 128, ("plain", "bias_res_rs"))),
    Case("gemm-weight-stationary-16384x576x192", [], lambda ops: _gemm_flavours(ops, 16384, 576, 192, ("gelu8", "table", "mul8"))),
    Case("gemm-fp8-chain-4160x384x1152", [O + n for n in ("gemm_nt", "quantize_fp8", "quantize_bf8", "gemm_nt_fp8", "gemm_tn8_acc_grouped")], _gemm_q8_chain),
    Case("wgrad-grouped-workspace", [O + "gemm_tn_acc_grouped"], _wgrad_grouped),
    Case("patch-gemm", [O + "gemm_nt_patch_fwd", O + "gemm_nt_patch_dgrad"], _patch_gemm),
    Case("gemm-into-outlook", [O + "outlook_fwd", O + "outlook_bwd", O + "avgpool2_fwd"], _outlook_chain),
    Case("attention", [O + "mhsa_fwd", O + "mhsa_bwd"], _mhsa),
    Case("class-attention-4x17x1x32", [O + "class_attn_fwd", O + "class_attn_bwd"], _class_attn),
    Case("small-kernels", [O + n for n in ("mix_token_swap", "mix_token_swap_dev", "loss_combine", "row_scale", "add_bcast", "sumsq", "resample_grid")], _small),
    Case("losses-and-the-10-class-head", [O + n for n in ("_soft_ce", "classify_stats", "distill_fwd_bwd")], _losses),
    Case("stem", [O + n for n in ("conv3x3_pack", "conv3x3_c64", "conv3x3_c64_bwd_stats", "conv3x3_c64_wgrad", "bn_relu_fwd", "bn_relu_bwd",
                                  "bn_relu_bwd_partials", "conv7_pack", "conv7_s2d", "conv7_s2d_wgrad")], _stem),
    Case("loader-stages", [O + n for n in ("input_prep", "_crop_launch", "randaug_u8", "label_map_crop")]
         + ["data.DeviceRandAugment.__call__", "data.DeviceLabelMapCrop.target", "ring.PinnedRing.send"], _loader),
]


# ---------------------------------------------------------------------------------------------------------------------- running a case
def _bits(t):
    t = t.detach().contiguous()
    if t.dtype.is_floating_point:
        t = t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t.cpu()


def snapshot(outputs):
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in outputs.items()}


def compare_runs(what, runs, covers):
    """runs: [(fill, {name: tensor}, Poison)] in the order of FILL_RUNS.  The control first, then identity, finiteness and the sites."""
    base = runs[0][1]
    for i, (fill, outs, p) in enumerate(runs[1:], 1):
        assert outs.keys() == base.keys()
        for k in base:
            same = torch.equal(_bits(base[k]), _bits(outs[k]))
            if i == 1:
                assert same, "%s: %r differs between two `zero` runs: the case is not reproducible and proves nothing (all that differ: %s)" % (
                    what, k, [n for n in base if not torch.equal(_bits(base[n]), _bits(outs[n]))])
            else:
                bad = int((_bits(base[k]) != _bits(outs[k])).sum()) if not same else 0
                assert same, "%s: %r under the %s fill differs from the zero fill in %d of %d elements: it reads memory nothing wrote" % (what, k, fill, bad, base[k].numel())
    for fill, outs, p in runs:
        for k, v in outs.items():
            if v.dtype.is_floating_point:
                assert bool(torch.isfinite(v.float() if v.dtype != torch.float64 else v).all()), "%s: %r holds non-finite elements under the %s fill" % (what, k, fill)
            elif k.split(" ")[0].endswith("_e4m3"):
                assert not bool(((v & 0x7F) == 0x7F).any()), "%s: %r holds e4m3 NaN bytes under the %s fill" % (what, k, fill)
        missed = [s for q in covers for s in sites_of(q) if not site_hit(p.sites, s)]
        assert not missed, "%s (%s fill): allocation sites never reached: %s" % (what, fill, missed)
    return len(base), sum(p.count for _, _, p in runs)


@pytest.fixture
def ops(monkeypatch):
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from autoprog_amd import ops as _ops
    monkeypatch.setattr(_ops, "deterministic", True)
    return _ops


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_wrapper_outputs_do_not_depend_on_the_allocator(ops, case):
    runs = []
    for fill in FILL_RUNS:
        with poisoned(fill) as p:
            outs = snapshot(case.run(ops))
        runs.append((fill, outs, p))
    n, fills = compare_runs(case.name, runs, case.covers)
    print("UNINIT %s | %d outputs | %d fills over four runs | %d product sites" % (case.name, n, fills, len(runs[-1][2].sites)))


# ====================================================================================================================== part B: chains
class Scenario:
    def __init__(self, name, covers, run):
        self.name, self.covers, self.run = name, tuple(covers), run


def _state(model, red, opt, losses):
    out = {"loss %d" % i: l.detach().float().reshape(1) for i, l in enumerate(losses)}
    out.update({"grad slab": red.flat, "p": opt.p, "m": opt.m, "v": opt.v})
    out.update({"ema %d" % i: e for i, e in enumerate(opt.ema)})
    out.update({"buffer " + n: b for n, b in model.named_buffers() if b.dtype.is_floating_point})
    for i, bs in enumerate(opt.ema_buffers):
        out.update({"ema %d buffer %d" % (i, j): b for j, b in enumerate(bs) if b.dtype.is_floating_point})
    return out


def _volo(classes=10, dpr=0.1, stem=64, variant="volo_h2_l3"):
    from autoprog_amd.models import create_model
    return create_model("model_variant", variant=variant, num_classes=classes, img_size=64, stem_hidden_dim=stem, drop_path_rate=dpr).cuda().train()


def _optim(model, **kw):
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.optim import FlatAdamWEma
    red = GradientBucketReducer(list(model.parameters()), world_size=1, defer_mean=True)
    red.install_sink(model)
    return red, FlatAdamWEma(model, red, lr=2e-3, weight_decay=0.05, ema_decays=[0.9, 0.99], **kw)


def _batch(classes=10, B=8, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, 64, 64, generator=g).cuda()
    target = torch.softmax(torch.randn(B, classes, 18, generator=g) * 2, dim=1).cuda()
    return x, target


def _repoison_scratch(opt):
    """the buffers the optimizer caches as scratch, poisoned again in front of the second step: _sumsq_ws ("the norm's workspace",
    optim.py, _clip_workspace) and _guard["ws"] ("the pass's workspace", _guard_workspace).  _agc_workspace holds a table, tallies and
    factors that agc_report() reads back -- outputs, zero-allocated: nothing there is scratch."""
    if getattr(opt, "_sumsq_ws", None) is not None:
        repoison(opt._sumsq_ws)
    if opt._guard is not None:
        repoison(opt._guard["ws"])


def _train(model, red, opt, loss_fn, x, target, steps=2, before_step=None, **step_kw):
    losses = []
    try:
        for s in range(steps):
            if s:
                _repoison_scratch(opt)
            red.zero_grad()
            loss = loss_fn(model(x), target)
            loss.backward()
            red.finish()
            if before_step is not None:
                before_step()
            opt.step(**step_kw)
            losses.append(loss)
        return _state(model, red, opt, losses)
    finally:
        red.remove()


def _s1_dense(classes=10, dpr=0.1, stem=64, variant="volo_h2_l3"):
    from autoprog_amd.loss import TokenLabelCrossEntropy
    model = _volo(classes, dpr, stem, variant)
    red, opt = _optim(model)
    x, target = _batch(classes)
    return _train(model, red, opt, TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=classes), x, target, clip_grad=1.0)


def _s1_with_a_gelu_linear():
    """scenario 1, and functional.linear(gelu=True) on its own -- the models' MLPs take the fused paths, so the side tensor LinearFn.forward
    allocates for a GELU launch is reached here, forward and backward: at 16 output columns (whole chunks) and at 10 in 16, where the
    backward multiplies the padding of dL/da by the side tensor's padding (found by this test: dx was NaN under the nan fill; the padding
    is zero-allocated since)"""
    from autoprog_amd import functional as AF
    out = _s1_dense()
    for N in (16, 10):
        x = dev(rnd(33, 64, seed=31)).requires_grad_(True)
        w, b = dev(frand(N, 64, seed=32, scale=0.125)).requires_grad_(True), dev(frand(N, seed=33, scale=0.3)).requires_grad_(True)
        y = AF.linear(x, w, b, gelu=True)
        y.backward(dev(rnd(33, N, seed=34)))
        out.update({"gelu linear %d y" % N: y, "gelu linear %d dx" % N: x.grad, "gelu linear %d dw" % N: w.grad, "gelu linear %d db" % N: b.grad})
    return out


def _s2_sparse_agc_guard_groups():
    from autoprog_amd.loss import TokenLabelCrossEntropy
    from autoprog_amd.loss.cross_entropy import SparseTokenLabelTarget
    from autoprog_amd.optim import layer_decay_param_groups
    classes, B = 10, 8
    model = _volo(classes)
    red, opt = _optim(model, param_groups=layer_decay_param_groups(model, 0.05, 0.75))
    x, _ = _batch(classes)
    g = torch.Generator().manual_seed(2)
    labels = torch.randint(0, classes, (B,), generator=g).cuda()
    t_cls = (torch.randn(B, classes, generator=g) * 2).to(BF16).cuda()
    t_aux = (torch.randn(B, 16, classes, generator=g) * 2).to(BF16).cuda()
    target = SparseTokenLabelTarget.from_logits(labels, t_cls, t_aux, 4)
    out = _train(model, red, opt, TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=classes), x, target,
                 before_step=lambda: opt.adaptive_clip_grad(0.05), skip_nonfinite=True)
    out.update({"target idx": target.idx, "target val": target.val, "guard state": opt._guard["state"], "guard out": opt._guard["out"], "agc out": opt._agc["out"]})
    return out


def _s3_stem128():
    return _s1_dense(classes=10, dpr=0.0, stem=128)


def _s4_fp8(monkeypatch):
    from autoprog_amd import functional as AF
    AF.reset_fp8_state()
    monkeypatch.setattr(AF, "FP8_LINEAR", True)
    # the 16-wide stem of that test runs on the vendor's convolutions, whose default weight-gradient kernels add with atomics: two `zero` runs
    # differed by 8e-6 in the gradient slab, with and without fp8; their deterministic mode makes the control hold
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    try:
        return _s1_dense(classes=16, dpr=0.0, stem=16)
    finally:
        AF.reset_fp8_state()


def _s5_distilled_deit():
    from autoprog_amd.loss import DistillationLoss, SoftTargetCrossEntropy
    from autoprog_amd.models import create_model
    from autoprog_amd.prog.teacher import TeacherLogits
    classes, B = 10, 6
    model = create_model("deit_tiny_distilled_patch16_224", num_classes=classes, img_size=64)
    model.blocks = torch.nn.ModuleList(list(model.blocks)[:2])
    model = model.cuda().train()
    red, opt = _optim(model)
    teacher = TeacherLogits(opt.ema_model(0), num_classes=classes)
    dl = DistillationLoss(SoftTargetCrossEntropy(), "soft", alpha=0.5, tau=3.0)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 3, 64, 64, generator=g).cuda()
    labels = torch.randint(0, classes, (B,), generator=g).cuda()
    losses, logits = [], []
    try:
        for s in range(2):
            target = teacher(x, labels, 64)
            logits.append(target.teacher_logits)
            red.zero_grad()
            loss = dl(model(x), target)
            loss.backward()
            red.finish()
            opt.step()
            losses.append(loss)
        out = _state(model, red, opt, losses)
        out.update({"teacher logits %d" % i: t for i, t in enumerate(logits)})
        return out
    finally:
        red.remove()


def _s6_validate():
    from autoprog_amd import ops as _ops
    from autoprog_amd.prog.validate import validate
    model = _volo(10, 0.1)
    x, _ = _batch(10)
    labels = torch.randint(0, 10, (2, 8), generator=torch.Generator().manual_seed(4)).cuda()
    m = validate(model, [(x, labels[0]), (x.flip(0), labels[1])])
    model.eval()
    with torch.no_grad():
        z = model(x)
        loss, rank = _ops.classify_stats(z.contiguous(), labels[0])
    return {"logits": z, "loss": loss, "rank": rank, "validate": torch.tensor([m["loss"], m["top1"], m["top5"]], dtype=torch.float64)}


def _s8_graphed():
    from autoprog_amd.graph import GraphedStep
    from autoprog_amd.loss import TokenLabelCrossEntropy
    model = _volo(10, 0.0)
    red, opt = _optim(model)
    x, target = _batch(10)
    try:
        gs = GraphedStep(model, TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=10), red, opt, x, target, clip_grad=1.0)
        gs.capture(warmup=2)
        losses = [gs.step().detach().clone() for _ in range(3)]
        return _state(model, red, opt, losses)
    finally:
        red.remove()


F_, P_ = "functional.", "optim.FlatAdamWEma."
SCENARIOS = [
    Scenario("volo-10-classes-dense-droppath-clip", [F_ + "LinearFn.forward", F_ + "_gelu_side_buffer", F_ + "PatchConvFn.forward", F_ + "PatchConvFn.backward",
                                                     P_ + "__init__", P_ + "_clip_workspace"], lambda mp: _s1_with_a_gelu_linear()),
    Scenario("volo-sparse-agc-guard-layer-decay", [P_ + "_guard_workspace", "loss.cross_entropy.SparseTokenLabelTarget.from_logits"], lambda mp: _s2_sparse_agc_guard_groups()),
    Scenario("volo-on-the-128-channel-stem", [F_ + "PatchConvFn.forward", F_ + "PatchConvFn.backward"], lambda mp: _s3_stem128()),
    Scenario("fp8-training-step", [], _s4_fp8),
    Scenario("distilled-deit-with-its-ema-teacher", [P_ + "ema_model"], lambda mp: _s5_distilled_deit()),
    Scenario("validate-and-classify-stats", [], lambda mp: _s6_validate()),
    Scenario("graphed-step-three-replays", [], lambda mp: _s8_graphed()),
]


@pytest.mark.parametrize("scenario", SCENARIOS, ids=[s.name for s in SCENARIOS])
def test_chains_do_not_depend_on_the_allocator(ops, monkeypatch, scenario):
    """each scenario built and run entirely under the fill, twice from the same seeds under `zero`, then under `nan` and `huge`: every
    loss, the gradient slab, p, m, v, every EMA slab and every floating buffer after two steps, bit for bit (the loader stages, scenario 7
    of the plan, are the `loader-stages` case of the table above: they need no model)"""
    runs = []
    for fill in FILL_RUNS:
        torch.manual_seed(0)
        np.random.seed(0)
        with poisoned(fill) as p:
            outs = snapshot(scenario.run(monkeypatch))
        runs.append((fill, outs, p))
    n, fills = compare_runs(scenario.name, runs, scenario.covers)
    print("UNINIT %s | %d tensors | %d fills over four runs | %d product sites" % (scenario.name, n, fills, len(runs[-1][2].sites)))
