"""Block-level parity on the GPU against golden vectors of the REAL reference modules
(tests/golden/blocks.*.npz, outlook_attn.npz): forward output, input gradient and every parameter
gradient of the HIP-backed modules.  Tolerance: 2e-2 rel-L2 per tensor (bf16 activations inside a
single block; the fixtures use O(1)-scale random weights)."""
import numpy as np
import pytest
import torch

from tests._golden import load, sub
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
TOL = 2.5e-2
STEM_KERNEL_TOL = 5e-3
BLOCK_KERNEL_TOL = 5e-3


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def run(mod, d, tag, tol=TOL, reshape_in=None):
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in sub(d, tag + ".w").items()}
    mod.load_state_dict(sd, strict=True)
    mod = mod.cuda().train()
    x = torch.from_numpy(d[tag + ".x"]).cuda().to(torch.bfloat16).requires_grad_(True)
    y = mod(x)
    assert rel(y, d[tag + ".y"]) < tol, ("y", rel(y, d[tag + ".y"]))
    y.backward(torch.from_numpy(d[tag + ".dy"]).cuda().to(torch.bfloat16).reshape(y.shape))
    assert rel(x.grad, d[tag + ".dx"]) < tol, ("dx", rel(x.grad, d[tag + ".dx"]))
    errs = {n: rel(p.grad, d[tag + ".g." + n]) for n, p in mod.named_parameters()}
    bad = {k: v for k, v in errs.items() if v > tol}
    assert not bad, bad


def test_blocks_vs_reference_golden():
    from autoprog_amd.models import volo as V
    d = load("blocks")
    C, H = 64, 2
    run(V.Mlp(C, C * 3), d, "mlp")
    run(V.Attention(C, H), d, "attention")
    run(V.Attention(C, H), d, "attention_n25")
    run(V.ClassAttention(C, H), d, "class_attention")
    run(V.ClassBlock(C, H, mlp_ratio=3.0), d, "class_block")
    run(V.Outlooker(C, 3, 1, stride=2, num_heads=H, mlp_ratio=3.0), d, "outlooker")
    run(V.Transformer(C, H, mlp_ratio=3.0), d, "transformer")
    run(V.Downsample(32, 64, 2), d, "downsample")


@pytest.mark.parametrize("tag,C", [("rect6x10", 64), ("odd5x9", 32), ("even16", 64)])   # head_dim 32 fixtures
def test_outlook_attention_module_vs_reference_golden(tag, C):
    from autoprog_amd.models import volo as V
    d = load("outlook_attn")
    heads = int(d[tag + ".heads"])
    run(V.OutlookAttention(C, heads, kernel_size=3, padding=1, stride=2), d, tag)


def test_patch_embed_stem_vs_reference_golden():
    """PatchEmbed (models/volo.py:342-380: conv7x7/s2 -> BN -> ReLU -> 2x(conv3x3 -> BN -> ReLU) -> conv4x4/s4) against the
    reference golden tests/golden/stem.npz: train-mode output, UPDATED BatchNorm running statistics, every parameter gradient,
    eval-mode output.  The three stem convolutions run in bf16 (MIOpen) between the HIP BatchNorm+ReLU kernels; tolerance 3e-2
    rel-L2 on outputs and running stats, 0.1 on the parameter gradients that pass through the BatchNorm backward (measured
    0.03-0.09 there: bf16 activations under heavy cancellation, see test_gpu_model.py::test_loss_curve_realistic_init)."""
    from autoprog_amd.models import volo as V
    d = load("stem")
    pe = V.PatchEmbed(stem_conv=True, stem_stride=2, patch_size=8, in_chans=3, hidden_dim=8, embed_dim=16)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in sub(d, "train.w").items()}
    for k in sd:                                   # the fixture stores the statistics AFTER the train step: start from the defaults
        if k.endswith("running_mean"):
            sd[k] = torch.zeros_like(sd[k])
        elif k.endswith("running_var"):
            sd[k] = torch.ones_like(sd[k])
        elif k.endswith("num_batches_tracked"):
            sd[k] = torch.zeros_like(sd[k])
    pe.load_state_dict(sd, strict=True)
    pe = pe.cuda().train()
    x = torch.from_numpy(d["train.x"]).cuda()
    y = pe(x)
    assert rel(y, d["train.y"]) < 3e-2, rel(y, d["train.y"])
    y.backward(torch.from_numpy(d["train.dy"]).cuda().to(y.dtype))
    for i in (1, 4, 7):
        bn = pe.conv[i]
        assert rel(bn.running_mean, d["train.w.conv.%d.running_mean" % i]) < 3e-2, i
        assert rel(bn.running_var, d["train.w.conv.%d.running_var" % i]) < 3e-2, i
        assert int(bn.num_batches_tracked) == 1
    errs = {n: rel(p.grad, d["train.g." + n]) for n, p in pe.named_parameters()}
    print("stem gradient errors:", {k: round(v, 4) for k, v in sorted(errs.items(), key=lambda kv: -kv[1])[:6]})
    bad = {k: v for k, v in errs.items() if v > (3e-2 if k.startswith("proj") else 0.1)}
    assert not bad, bad
    sd_eval = {k: torch.from_numpy(np.asarray(v)) for k, v in sub(d, "train.w").items()}      # the reference's post-step statistics
    pe.load_state_dict(sd_eval, strict=True)
    pe.eval()
    with torch.no_grad():
        ye = pe(x)
    assert rel(ye, d["eval.y"]) < 3e-2, rel(ye, d["eval.y"])


def _stem64_module(d, hip, width=64):
    from autoprog_amd.models import volo as V
    pe = V.PatchEmbed(stem_conv=True, stem_stride=2, patch_size=8, in_chans=3, hidden_dim=width, embed_dim=32)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in sub(d, "train.w").items()}
    for k in sd:                                   # the fixture stores the statistics AFTER the train step: start from the defaults
        if k.endswith("running_mean"):
            sd[k] = torch.zeros_like(sd[k])
        elif k.endswith("running_var"):
            sd[k] = torch.ones_like(sd[k])
        elif k.endswith("num_batches_tracked"):
            sd[k] = torch.zeros_like(sd[k])
    pe.load_state_dict(sd, strict=True)
    pe = pe.cuda().train()
    pe.hip_conv = hip
    return pe


def test_hip_stem64_vs_reference_golden(monkeypatch):
    """The 64-wide stem ON THE HIP CONVOLUTIONS (csrc/conv7.hip, csrc/conv.hip, the patch-addressed GEMM; models/volo.py:342-380)
    against reference-generated vectors (tests/golden/stem64.npz, tools/gen_golden.py::gen_stem64): train-mode output, updated
    running statistics, every parameter gradient, eval-mode output -- and against the CPU oracle on a second input.  Any call of
    torch's convolution (MIOpen) fails the HIP part of the test: the narrow `stem.npz` fixture above exercises that path, not the
    kernels.

    Bounds.  Outputs and statistics: 1.5e-2 (measured 6.6e-3).  Parameter gradients behind the three training-mode BatchNorms of
    this fixture (2 x 16 x 16 samples per channel) lose up to 13 % to bf16 ACTIVATIONS whatever computes the convolutions: the same
    module on MIOpen's bf16 convolutions measures 0.016 - 0.123 per tensor, on fp32 convolutions 0.0000 (tools/dbg_stem64.py).  The
    test therefore measures that independent bf16 implementation first and holds the HIP kernels to 1.3x ITS error per tensor
    (floor 1e-2): a wrong kernel is caught, the precision recipe is not re-litigated."""
    import torch.nn.functional as F
    d = load("stem64")
    x = torch.from_numpy(d["train.x"]).cuda()
    dy = torch.from_numpy(d["train.dy"]).cuda()
    pm = _stem64_module(d, hip=False)              # bf16 activations, MIOpen convolutions: the yardstick
    ym = pm(x)
    ym.backward(dy.to(ym.dtype))
    base = {n: rel(p.grad, d["train.g." + n]) for n, p in pm.named_parameters()}
    base_y = rel(ym, d["train.y"])

    pe = _stem64_module(d, hip=True)

    torch_conv2d = F.conv2d

    def no_miopen(inp, *a, **k):                   # (the CPU oracle below convolves with the same function)
        if inp.is_cuda:
            raise AssertionError("torch conv2d called on the GPU: the 64-wide stem must run on the HIP convolution kernels")
        return torch_conv2d(inp, *a, **k)
    monkeypatch.setattr(F, "conv2d", no_miopen)
    y = pe(x)
    e_y = rel(y, d["train.y"])
    y.backward(dy.to(y.dtype))
    for i in (1, 4, 7):
        bn = pe.conv[i]
        assert rel(bn.running_mean, d["train.w.conv.%d.running_mean" % i]) < 1.5e-2, i
        assert rel(bn.running_var, d["train.w.conv.%d.running_var" % i]) < 1.5e-2, i
        assert int(bn.num_batches_tracked) == 1
    errs = {n: rel(p.grad, d["train.g." + n]) for n, p in pe.named_parameters()}
    print("stem64 train output error hip %.4f (miopen bf16 %.4f); gradient errors hip / miopen bf16:" % (e_y, base_y),
          {k: (round(v, 4), round(base[k], 4)) for k, v in sorted(errs.items(), key=lambda kv: -kv[1])})
    assert e_y < 1.5e-2 and e_y < 1.3 * base_y + 1e-3, (e_y, base_y)
    bad = {k: (v, base[k]) for k, v in errs.items() if v > max(1e-2, 1.3 * base[k])}
    assert not bad, bad
    sd_eval = {k: torch.from_numpy(np.asarray(v)) for k, v in sub(d, "train.w").items()}      # the reference's post-step statistics
    pe.load_state_dict(sd_eval, strict=True)
    pe.eval()
    with torch.no_grad():
        ye = pe(x)
    assert rel(ye, d["eval.y"]) < 1.5e-2, rel(ye, d["eval.y"])
    # the CPU oracle on another input: odd batch and a feature map that does not divide the convolution tiles; forward output and the
    # input-side quantities that do not pass through a BatchNorm backward (proj) at 1.5e-2, the rest against the oracle at the
    # yardstick's level measured above
    pe.train()
    g = torch.Generator().manual_seed(5)
    x2 = torch.randn(3, 3, 48, 48, generator=g)
    p64 = {k: v.detach().double().cpu() for k, v in pe.state_dict().items()}
    for k in p64:
        if k.endswith("running_mean"):
            p64[k] = torch.zeros_like(p64[k])
        elif k.endswith("running_var"):
            p64[k] = torch.ones_like(p64[k])
        elif p64[k].dtype.is_floating_point:
            p64[k].requires_grad_(True)
    with torch.no_grad():
        for i in (1, 4, 7):
            pe.conv[i].reset_running_stats()
    pe.zero_grad()
    y2 = pe(x2.cuda())
    ref = R.patch_embed(x2.double(), p64, train=True, patch_size=8, pre="")
    dy2 = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    ref.backward(dy2)
    y2.backward(dy2.permute(0, 3, 1, 2).cuda().to(y2.dtype))
    assert rel(y2, ref.detach().permute(0, 3, 1, 2)) < 1.5e-2
    errs2 = {n: rel(p.grad, p64[n].grad) for n, p in pe.named_parameters()}
    print("stem64 vs oracle (3 x 48 x 48) gradient errors:", {k: round(v, 4) for k, v in sorted(errs2.items(), key=lambda kv: -kv[1])})
    bad = {k: v for k, v in errs2.items() if v > (1.5e-2 if k.startswith("proj") else 1.3 * max(base.values()))}
    assert not bad, bad


def test_hip_stem128_vs_reference_golden(monkeypatch):
    """VERDICT r4, missing 2 (row X1): the 128-wide stem of VOLO-D4 / D5 (models/volo.py:799-821, stem_hidden_dim = 128) on HIP kernels --
    conv7 as two 64-channel launches into the 128-channel tensor, csrc/conv128.hip (patch in LDS, weights streamed per (tap, 64-channel)
    slab) forward and input gradient, the 64-channel weight-gradient kernel on the four quadrants, the patch-addressed projection --
    against reference-generated vectors (tests/golden/stem128.*.npz, tools/gen_golden.py::gen_stem128).  Any torch convolution on the GPU
    fails the HIP part.  Bounds as test_hip_stem64_vs_reference_golden: the same module on MIOpen's bf16 convolutions is measured first
    (the cost of bf16 activations under three training-mode BatchNorms of 2 x 16 x 16 samples) and the HIP kernels are held to 1.3x ITS
    error per tensor (floor 1e-2)."""
    import torch.nn.functional as F
    d = load("stem128")
    x = torch.from_numpy(d["train.x"]).cuda()
    dy = torch.from_numpy(d["train.dy"]).cuda()
    pm = _stem64_module(d, hip=False, width=128)
    ym = pm(x)
    ym.backward(dy.to(ym.dtype))
    base = {n: rel(p.grad, d["train.g." + n]) for n, p in pm.named_parameters()}
    base_y = rel(ym, d["train.y"])
    pe = _stem64_module(d, hip=True, width=128)
    torch_conv2d = F.conv2d

    def no_miopen(inp, *a, **k):
        if inp.is_cuda:
            raise AssertionError("torch conv2d called on the GPU: the 128-wide stem must run on the HIP convolution kernels")
        return torch_conv2d(inp, *a, **k)
    monkeypatch.setattr(F, "conv2d", no_miopen)
    y = pe(x)
    e_y = rel(y, d["train.y"])
    y.backward(dy.to(y.dtype))
    for i in (1, 4, 7):
        bn = pe.conv[i]
        assert rel(bn.running_mean, d["train.w.conv.%d.running_mean" % i]) < 1.5e-2, i
        assert rel(bn.running_var, d["train.w.conv.%d.running_var" % i]) < 1.5e-2, i
        assert int(bn.num_batches_tracked) == 1
    errs = {n: rel(p.grad, d["train.g." + n]) for n, p in pe.named_parameters()}
    print("stem128 train output error hip %.4f (miopen bf16 %.4f); gradient errors hip / miopen bf16:" % (e_y, base_y),
          {k: (round(v, 4), round(base[k], 4)) for k, v in sorted(errs.items(), key=lambda kv: -kv[1])})
    assert e_y < 1.5e-2 and e_y < 1.3 * base_y + 1e-3, (e_y, base_y)
    bad = {k: (v, base[k]) for k, v in errs.items() if v > max(1e-2, 1.3 * base[k])}
    assert not bad, bad
    sd_eval = {k: torch.from_numpy(np.asarray(v)) for k, v in sub(d, "train.w").items()}
    pe.load_state_dict(sd_eval, strict=True)
    pe.eval()
    with torch.no_grad():
        ye = pe(x)
    assert rel(ye, d["eval.y"]) < 1.5e-2, rel(ye, d["eval.y"])


def test_transformer_block_kernels_vs_fp64_with_the_same_rounding_points():
    """The transformer block's KERNELS (LayerNorm, the NT / TN GEMMs with their epilogues, attention forward / backward) held to
    BLOCK_KERNEL_TOL against oracle/ref_cpu.py transformer_bf16_points: the reference block in fp64 with every tensor that
    functional.TransformerBlockFn keeps in bf16 rounded at the same place, forward and backward -- the 2.5e-2 of the golden tests above
    is what bf16 activations cost, this is what the kernels add.  Two cases: the reference fixture's block (2 x 4 x 4 x 64, generic GEMM
    kernels, one-workgroup attention) and a D1-shaped one (24 x 14 x 14 x 384, 12 heads: the 8-phase GEMMs, the persistent attention
    kernels, the weight-gradient tile kernel).  Measured on MI355X: the fixture's output is BIT-IDENTICAL to the rounding-matched oracle
    and its parameter gradients agree to 3e-7; the D1-shaped block: output 5.3e-4, parameter gradients 4.6e-4 - 2.5e-3 (LayerNorm-1
    weight), input gradient 1.7e-3 (the HIP one is a bf16 tensor, the oracle's leaf gradient is not rounded).  Bound 5e-3."""
    from autoprog_amd.models import volo as V
    d = load("blocks")
    cases = []
    blk = V.Transformer(64, 2, mlp_ratio=3.0)
    blk.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sub(d, "transformer.w").items()}, strict=True)
    cases.append(("fixture", blk, 2, torch.from_numpy(d["transformer.x"]), torch.from_numpy(d["transformer.dy"])))
    torch.manual_seed(21)
    big = V.Transformer(384, 12, mlp_ratio=3.0)
    with torch.no_grad():
        for n_, p_ in big.named_parameters():
            if p_.dim() == 1 and "norm" in n_ and n_.endswith("weight"):
                p_.uniform_(0.5, 1.5)
            elif p_.dim() == 1:
                p_.normal_(0, 0.1)
    g = torch.Generator().manual_seed(22)
    cases.append(("24x14x14x384", big, 12, torch.randn(24, 14, 14, 384, generator=g), torch.randn(24, 14, 14, 384, generator=g)))
    for tag, mod, heads, x, dy in cases:
        xb, dyb = x.to(torch.bfloat16), dy.to(torch.bfloat16)
        p64 = {k: v.detach().double().clone().requires_grad_(True) for k, v in mod.state_dict().items()}
        B, H, W, C = xb.shape
        x64 = xb.double().reshape(B, H * W, C).requires_grad_(True)
        ref = R.transformer_bf16_points(x64, p64, "", heads)
        ref.backward(dyb.double().reshape(B, H * W, C))
        mod = mod.cuda().train()
        xg = xb.cuda().requires_grad_(True)
        y = mod(xg)
        y.backward(dyb.cuda().reshape(y.shape))
        e_y = rel(y.reshape(B, H * W, C), ref.detach())
        e_x = rel(xg.grad.reshape(B, H * W, C), x64.grad)
        errs = {n: rel(p_.grad, p64[n].grad) for n, p_ in mod.named_parameters()}
        print("transformer block kernels vs rounding-matched fp64 (%s): y %.2e dx %.2e; parameter gradients" % (tag, e_y, e_x),
              {k: float("%.2e" % v) for k, v in sorted(errs.items(), key=lambda kv: -kv[1])})
        assert e_y < BLOCK_KERNEL_TOL and e_x < BLOCK_KERNEL_TOL, (tag, e_y, e_x)
        bad = {k: v for k, v in errs.items() if v > BLOCK_KERNEL_TOL}
        assert not bad, (tag, bad)


def test_transformer_block_with_the_fused_mlp_is_the_block_bit_for_bit(monkeypatch):
    """AP_FUSED_MLP (functional.FUSED_MLP; csrc/mlp_fused.hip, round 6): a D1-shaped transformer block (32 x 14 x 14 x 384 = 6272 rows, 12 heads,
    DropPath factors on both branches) with its MLP as one launch per direction, with and without the LayerNorm in front of it inside the
    forward launch (functional.FUSED_MLP_LN) -- output, input gradient and EVERY parameter gradient equal the unfused block's bit for bit
    (deterministic weight gradients), and the fused launches really ran."""
    from autoprog_amd import functional as AF, ops
    from autoprog_amd.models import volo as V
    monkeypatch.setattr(ops, "deterministic", True)
    calls = []
    real = ops.mlp_fused

    def counted(*a, **kw):
        out = real(*a, **kw)
        calls.append(out is not None)
        return out
    monkeypatch.setattr(ops, "mlp_fused", counted)
    torch.manual_seed(31)
    blk = V.Transformer(384, 12, mlp_ratio=3.0, drop_path=0.2).cuda().train()
    g = torch.Generator().manual_seed(32)
    x = torch.randn(32, 14, 14, 384, generator=g).to(torch.bfloat16).cuda()
    dy = torch.randn(32, 14, 14, 384, generator=g).to(torch.bfloat16).cuda()
    # the block below has 6272 rows: by default (functional.FUSED_MLP_MIN_ROWS = 18432: one 128-row block per CU does not pay on fewer) it keeps the two launches
    blk(x.clone().requires_grad_(True)).backward(dy)
    assert calls == [], calls
    monkeypatch.setattr(AF, "FUSED_MLP_MIN_ROWS", 0)
    outs = {}
    lns = []
    real_ln = ops.layernorm_fwd

    def counted_ln(*a, **kw):
        lns.append(1)
        return real_ln(*a, **kw)
    monkeypatch.setattr(ops, "layernorm_fwd", counted_ln)
    for fused in (False, True, "ln"):
        monkeypatch.setattr(AF, "FUSED_MLP", 1 if fused else 0)
        monkeypatch.setattr(AF, "FUSED_MLP_BWD", bool(fused))
        monkeypatch.setattr(AF, "FUSED_MLP_LN", fused == "ln")
        blk.zero_grad(set_to_none=True)
        torch.manual_seed(5)                      # the same DropPath draws
        xg = x.clone().requires_grad_(True)
        y = blk(xg)
        y.backward(dy)
        outs[fused] = (y.detach().clone(), xg.grad.clone(), {n: p_.grad.clone() for n, p_ in blk.named_parameters()})
    assert calls == [True, True, True, True], calls           # one forward and one backward launch per fused pass
    assert len(lns) == 2 + 2 + 1, lns                          # the LayerNorm in front of the MLP has no launch of its own in the last pass
    (y0, dx0, g0) = outs[False]
    for mode in (True, "ln"):
        (y1, dx1, g1) = outs[mode]
        assert torch.equal(y0, y1) and torch.equal(dx0, dx1), mode
        for n in g0:
            assert torch.equal(g0[n], g1[n]), (mode, n)


def test_outlooker_block_kernels_vs_fp64_with_the_same_rounding_points():
    """The outlooker block's kernels (LayerNorm, the v / logits / proj / MLP GEMMs, the 2 x 2 average pool and its backward, the outlook
    attention core forward and its fused backward) against oracle/ref_cpu.py outlooker_bf16_points: the reference block in fp64 with the
    rounding points of functional.OutlookerBlockFn -- among them the per-WINDOW rounding of the outlook products in front of the fold and
    the unrounded probabilities in dlogits (csrc/outlook.hip).  The reference fixture's block (2 x 8 x 8 x 64) and a D1-shaped one
    (8 x 28 x 28 x 192, 6 heads: persistent outlook kernels, 8-phase GEMMs).  Measured on MI355X: fixture output 3.6e-7, parameter gradients
    <= 2.8e-6; the D1-shaped block: output 2.5e-4, parameter gradients 2e-4 - 1.1e-3; input gradients 1.7e-3 (bf16 tensor against an
    unrounded leaf gradient).  Bound BLOCK_KERNEL_TOL = 5e-3."""
    from autoprog_amd.models import volo as V
    d = load("blocks")
    cases = []
    blk = V.Outlooker(64, kernel_size=3, padding=1, stride=2, num_heads=2, mlp_ratio=3.0)
    blk.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sub(d, "outlooker.w").items()}, strict=True)
    cases.append(("fixture", blk, 2, torch.from_numpy(d["outlooker.x"]), torch.from_numpy(d["outlooker.dy"])))
    torch.manual_seed(31)
    big = V.Outlooker(192, kernel_size=3, padding=1, stride=2, num_heads=6, mlp_ratio=3.0)
    with torch.no_grad():
        for n_, p_ in big.named_parameters():
            if p_.dim() == 1 and "norm" in n_ and n_.endswith("weight"):
                p_.uniform_(0.5, 1.5)
            elif p_.dim() == 1:
                p_.normal_(0, 0.1)
    g = torch.Generator().manual_seed(32)
    cases.append(("8x28x28x192", big, 6, torch.randn(8, 28, 28, 192, generator=g), torch.randn(8, 28, 28, 192, generator=g)))
    for tag, mod, heads, x, dy in cases:
        xb, dyb = x.to(torch.bfloat16), dy.to(torch.bfloat16).reshape(x.shape)
        p64 = {k: v.detach().double().clone().requires_grad_(True) for k, v in mod.state_dict().items()}
        x64 = xb.double().requires_grad_(True)
        ref = R.outlooker_bf16_points(x64, p64, "", heads)
        ref.backward(dyb.double())
        mod = mod.cuda().train()
        xg = xb.cuda().requires_grad_(True)
        y = mod(xg)
        y.backward(dyb.cuda())
        e_y, e_x = rel(y, ref.detach()), rel(xg.grad, x64.grad)
        errs = {n: rel(p_.grad, p64[n].grad) for n, p_ in mod.named_parameters()}
        print("outlooker block kernels vs rounding-matched fp64 (%s): y %.2e dx %.2e; parameter gradients" % (tag, e_y, e_x),
              {k: float("%.2e" % v) for k, v in sorted(errs.items(), key=lambda kv: -kv[1])})
        assert e_y < BLOCK_KERNEL_TOL and e_x < BLOCK_KERNEL_TOL, (tag, e_y, e_x)
        bad = {k: v for k, v in errs.items() if v > BLOCK_KERNEL_TOL}
        assert not bad, (tag, bad)


def test_class_block_kernels_vs_fp64_with_the_same_rounding_points():
    """The class block's kernels (split LayerNorm, kv / q / proj / MLP GEMMs incl. the skinny ones, class attention forward / backward)
    against oracle/ref_cpu.py class_block_bf16_points: the reference fixture's block and a D1-shaped one (32 x (1 + 196) x 384, 12 heads).
    Measured on MI355X: the fixture's class token is BIT-IDENTICAL, its parameter gradients agree to 3.4e-5; the D1-shaped block: class
    token 6.3e-4, parameter gradients 5.5e-4 - 2.0e-3.  Bound BLOCK_KERNEL_TOL = 5e-3."""
    from autoprog_amd.models import volo as V
    d = load("blocks")
    x0 = torch.from_numpy(d["class_block.x"])
    C0 = x0.shape[-1]
    blk = V.ClassBlock(C0, 2, mlp_ratio=3.0)
    blk.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sub(d, "class_block.w").items()}, strict=True)
    cases = [("fixture", blk, 2, x0, torch.from_numpy(d["class_block.dy"]))]
    torch.manual_seed(41)
    big = V.ClassBlock(384, 12, mlp_ratio=3.0)
    with torch.no_grad():
        for n_, p_ in big.named_parameters():
            if p_.dim() == 1 and "norm" in n_ and n_.endswith("weight"):
                p_.uniform_(0.5, 1.5)
            elif p_.dim() == 1:
                p_.normal_(0, 0.1)
    g = torch.Generator().manual_seed(42)
    cases.append(("32x197x384", big, 12, torch.randn(32, 197, 384, generator=g), torch.randn(32, 197, 384, generator=g)))
    for tag, mod, heads, x, dy in cases:
        xb, dyb = x.to(torch.bfloat16), dy.to(torch.bfloat16).reshape(x.shape)
        p64 = {k: v.detach().double().clone().requires_grad_(True) for k, v in mod.state_dict().items()}
        x64 = xb.double().requires_grad_(True)
        ref = R.class_block_bf16_points(x64, p64, "", heads)
        ref.backward(dyb.double())
        mod = mod.cuda().train()
        xg = xb.cuda().requires_grad_(True)
        y = mod(xg)
        y.backward(dyb.cuda())
        e_y, e_x = rel(y[:, :1], ref.detach()[:, :1]), rel(xg.grad, x64.grad)
        errs = {n: rel(p_.grad, p64[n].grad) for n, p_ in mod.named_parameters()}
        print("class block kernels vs rounding-matched fp64 (%s): class token %.2e dx %.2e; parameter gradients" % (tag, e_y, e_x),
              {k: float("%.2e" % v) for k, v in sorted(errs.items(), key=lambda kv: -kv[1])})
        assert e_y < BLOCK_KERNEL_TOL and e_x < BLOCK_KERNEL_TOL, (tag, e_y, e_x)
        bad = {k: v for k, v in errs.items() if v > BLOCK_KERNEL_TOL}
        assert not bad, (tag, bad)


def test_hip_stem64_kernels_vs_fp64_with_the_same_rounding_points():
    """The stem KERNELS held to 5e-3 (measured 2.6e-3 at worst), independently of what bf16 activations cost under three training-mode BatchNorms (the test above
    can only hold them to an independent bf16 implementation's error, up to 0.16 per tensor): the oracle's PatchEmbed in fp64 with every
    tensor that the HIP pipeline keeps in bf16 -- image, convolution outputs, activations, weight operands, and their gradients on the
    way back -- rounded to bf16 at the same place (oracle/ref_cpu.py patch_embed(bf16_points=True)).  What is left is the kernels'
    own arithmetic: fp32 accumulation order, fp32 BatchNorm statistics, roundings that flip on a near-tie.  Output, running statistics
    and EVERY parameter gradient of csrc/conv7.hip, csrc/conv.hip (forward, input gradient, weight gradient, BatchNorm applied in the
    staging), csrc/bnrelu.hip and the patch-addressed GEMMs, on the reference fixture's weights (2 x 32 x 32) and on an odd batch whose
    feature map does not divide the convolution tiles (3 x 80 x 80).  Measured on MI355X: output 7.3e-4 / 6.8e-4; gradients 2e-4 behind one
    BatchNorm backward, 9e-4 behind two, 1.9e-3 - 2.6e-3 behind all three (fixture: 512 samples per channel; 1.1e-3 - 1.4e-3 on the larger
    input) -- a rounding that falls the other way is a 4e-3 step on that element and travels on through the layers below it.  Bound:
    STEM_KERNEL_TOL = 5e-3
BLOCK_KERNEL_TOL = 5e-3 per tensor, 60x below what the bf16 recipe itself costs on this fixture."""
    d = load("stem64")
    cases = [("fixture", torch.from_numpy(d["train.x"]), torch.from_numpy(d["train.dy"]))]
    g = torch.Generator().manual_seed(17)
    cases.append(("3x80x80", torch.randn(3, 3, 80, 80, generator=g), None))
    for tag, x, dy in cases:
        pe = _stem64_module(d, hip=True)
        p64 = {}
        for k, v in pe.state_dict().items():
            p64[k] = v.detach().double().cpu()
            if p64[k].dtype.is_floating_point and "running" not in k:
                p64[k].requires_grad_(True)
        y = pe(x.cuda())
        ref = R.patch_embed(x.double(), p64, train=True, patch_size=8, pre="", bf16_points=True)       # [B, h, w, C]
        if dy is None:
            dy = torch.randn(ref.permute(0, 3, 1, 2).shape, generator=g)
        dyb = dy.to(torch.bfloat16)
        ref.backward(dyb.double().permute(0, 2, 3, 1))
        y.backward(dyb.cuda().to(y.dtype))
        e_y = rel(y, ref.detach().permute(0, 3, 1, 2))
        errs = {n: rel(p.grad, p64[n].grad) for n, p in pe.named_parameters()}
        print("stem64 kernels vs rounding-matched fp64 (%s): output %.2e; gradients" % (tag, e_y),
              {k: float("%.2e" % v) for k, v in sorted(errs.items(), key=lambda kv: -kv[1])})
        assert e_y < STEM_KERNEL_TOL, (tag, e_y)
        bad = {k: v for k, v in errs.items() if v > STEM_KERNEL_TOL}
        assert not bad, (tag, bad)
        # running statistics after one step (momentum 0.1, unbiased variance): from the oracle's rounded convolution outputs
        xr = x.to(torch.bfloat16).double()
        with torch.no_grad():
            for i, (s, pad) in zip((0, 3, 6), ((2, 3), (1, 1), (1, 1))):
                z = torch.nn.functional.conv2d(xr, p64["conv.%d.weight" % i].detach().to(torch.bfloat16).double(), None, stride=s, padding=pad)
                z = z.to(torch.bfloat16).double()
                n = z.numel() // z.shape[1]
                bn = pe.conv[i + 1]
                assert rel(bn.running_mean, 0.1 * z.mean((0, 2, 3))) < 2e-3, (tag, i)
                assert rel(bn.running_var, 0.9 + 0.1 * z.var((0, 2, 3), unbiased=True)) < 2e-3, (tag, i, n)
                xr = torch.relu(R.batchnorm_train(z, p64["conv.%d.weight" % (i + 1)].detach(), p64["conv.%d.bias" % (i + 1)].detach()))
                xr = xr.to(torch.bfloat16).double()


def test_stem64_fused_batchnorm_input_is_bit_identical_to_the_chain(monkeypatch):
    """functional.Stem64Fn (the 3x3 convolutions read the PRE-BatchNorm tensor of the layer before them and apply relu(bn(.)) while they
    stage it: csrc/conv.hip PRE_BN, forward and weight gradient) against the chain of per-layer nodes with materialised activations
    (AP_STEM_FUSE_BN=0): the same bits -- train output, every parameter gradient, running statistics, eval output -- on an odd batch and
    a feature map that does not divide the convolution tiles; and the two kernels on their own against apply-then-convolve."""
    from autoprog_amd import functional as AF, ops
    from autoprog_amd.models.volo import PatchEmbed
    torch.manual_seed(3)
    x = torch.randn(3, 3, 80, 80, device="cuda")
    res = {}
    for fuse in (False, True, "stats"):
        monkeypatch.setattr(AF, "STEM_FUSE_BN", bool(fuse))
        monkeypatch.setattr(AF, "STEM_FUSE_BN_BWD_STATS", fuse == "stats")     # (round 5) the BatchNorm-backward sums in the input-gradient convolutions
        torch.manual_seed(11)
        pe = PatchEmbed(stem_conv=True, stem_stride=2, patch_size=8, in_chans=3, hidden_dim=64, embed_dim=192).cuda().train()
        y = pe(x)
        torch.manual_seed(12)
        y.backward(torch.randn_like(y))
        out = {"y": y.detach().clone()}
        out.update({"g." + n: p.grad.detach().clone() for n, p in pe.named_parameters()})
        out.update({"b." + n: b.detach().clone() for n, b in pe.named_buffers()})
        pe.eval()
        with torch.no_grad():
            out["eval"] = pe(x).clone()
        res[fuse] = out
    assert set(res[True]) == set(res[False]) and len(res[True]) > 15
    for k in res[True]:
        assert torch.equal(res[True][k], res[False][k]), k
    assert float(res[True]["g.conv.3.weight"].abs().max()) > 0 and float(res[True]["b.conv.4.running_mean"].abs().max()) > 0
    # with the sums formed in the convolution epilogue: the forward is the same code; the gradients differ by the order of an fp32 summation
    for k in res[True]:
        if k.startswith("g."):
            assert float((res["stats"][k] - res[True][k]).norm() / res[True][k].norm()) < 2e-3, k      # (bf16 dz maps downstream of 1e-7 differences)
        else:
            assert torch.equal(res["stats"][k], res[True][k]), k
    # kernel level
    g = torch.Generator(device="cuda").manual_seed(5)
    z = torch.randn(2, 37, 21, 64, device="cuda", generator=g).to(torch.bfloat16)
    dy = torch.randn(2, 37, 21, 64, device="cuda", generator=g).to(torch.bfloat16)
    mean, rstd = torch.randn(64, device="cuda", generator=g) * 0.3, torch.rand(64, device="cuda", generator=g) + 0.5
    gam, bet = torch.randn(64, device="cuda", generator=g) * 0.3 + 1, torch.randn(64, device="cuda", generator=g) * 0.3
    w = torch.randn(64, 64, 3, 3, device="cuda", generator=g) * 0.05
    wf, wb = ops.conv3x3_pack(w)
    a = torch.relu((z.float() - mean) * (rstd * gam) + bet)            # same association as k_bn_relu_apply: x * (rstd * gamma) + (beta - mean * rstd * gamma)
    sc = rstd * gam
    a = torch.clamp_min(torch.addcmul(bet - mean * sc, z.float(), sc), 0).to(torch.bfloat16)
    y0, s0 = ops.conv3x3_c64(a, wf, True)
    y1, s1 = ops.conv3x3_c64(z, wf, True, bn_in=(mean, rstd, gam, bet))
    assert float((y1.float() - y0.float()).abs().max()) <= 2 ** -6 * float(y0.float().abs().max())     # (fma vs mul + add inside the transform: <= 1 bf16 ulp of an input)
    dw0, dw1 = torch.zeros(64, 64, 3, 3, device="cuda"), torch.zeros(64, 64, 3, 3, device="cuda")
    ops.conv3x3_c64_wgrad(a, dy, dw0)
    ops.conv3x3_c64_wgrad(z, dy, dw1, bn_in=(mean, rstd, gam, bet))
    assert float((dw1 - dw0).norm() / dw0.norm()) < 2e-3
