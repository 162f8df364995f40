"""fp8 weight gradients (BASELINE configs[4]: "e4m3 fwd / e5m2 grads", functional.FP8_WGRAD): the e5m2 quantiser with its fused bias
gradient (ap_quantize_bf8), the fp8 weight-gradient kernel (ap_gemm_tn8_acc_grouped) against fp64 products of the same dequantised bytes,
and the transformer block / D5-shape network / training loop under the mode."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("rows,cols", [(8, 16), (37, 768), (784, 2304), (4099, 3072)])
@pytest.mark.parametrize("weighted", [False, True])
def test_quantize_bf8_bytes_amax_and_bias_sums(rows, cols, weighted):
    """bytes equal torch's e5m2 cast of the saturated product, amax is exact, column sums of the bf16 input within 1e-5 of fp64"""
    from autoprog_amd import ops
    torch.manual_seed(rows + cols)
    g = (torch.randn(rows, cols, device="cuda") * 3).to(torch.bfloat16)
    g[0, 0] = 1e6                                             # saturates
    s = torch.tensor([0.37], device="cuda")
    amax = torch.zeros(1, device="cuda")
    colsum = torch.randn(cols, device="cuda")
    c0 = colsum.clone()
    w = (torch.rand(rows, device="cuda") > 0.3).to(torch.bfloat16) if weighted else None
    y = ops.quantize_bf8(g, s, amax, colsum=colsum, colsum_weight=w, colsum_scale=1.25)
    torch.cuda.synchronize()
    ref = (g.float() * s).clamp(-57344, 57344).to(torch.float8_e5m2)
    assert torch.equal(y, ref.view(torch.uint8))
    assert float(amax[0]) == float(g.float().abs().max())
    gd = g.double().cpu()
    want = c0.double().cpu() + ((w.double().cpu()[:, None] * gd).sum(0) * 1.25 if weighted else gd.sum(0))
    assert rel(colsum, want) < 1e-5
    # the plain form (no column sums) writes the same bytes
    y2 = ops.quantize_bf8(g, s)
    assert torch.equal(y2, y)


def test_quantize_bf8_deterministic_bias_sums(monkeypatch):
    from autoprog_amd import ops
    monkeypatch.setattr(ops, "deterministic", True)
    g = torch.randn(5000, 768, device="cuda").to(torch.bfloat16)
    outs = []
    for _ in range(2):
        c = torch.zeros(768, device="cuda")
        ops.quantize_bf8(g, torch.ones(1, device="cuda"), colsum=c)
        outs.append(c)
    assert torch.equal(outs[0], outs[1])
    assert rel(outs[0], g.double().sum(0)) < 1e-5


def _operands(M, n1, n2, seed):
    from autoprog_amd import ops
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = (torch.randn(M, n1, device="cuda", generator=g) * 1e-3).to(torch.bfloat16)
    b = torch.randn(M, n2, device="cuda", generator=g).to(torch.bfloat16)
    sa = (ops.BF8_MAX / a.float().abs().amax()).reshape(1)
    sb = (ops.FP8_MAX / b.float().abs().amax()).reshape(1)
    a8, b8 = ops.quantize_bf8(a, sa), ops.quantize_fp8(b, sb)
    return a, b, a8, b8, (1.0 / sa).contiguous(), (1.0 / sb).contiguous()


def _deq(a8, b8, dq_a, dq_b):
    return (a8.view(torch.float8_e5m2).double().cpu() * float(dq_a), b8.view(torch.float8_e4m3fn).double().cpu() * float(dq_b))


D5_PROBLEMS = [(2304, 768), (768, 768), (3072, 768), (768, 3072)]          # qkv, proj, fc1, fc2 (N1 = out, N2 = in)


@pytest.mark.parametrize("M", [784, 4096, 50176, 1000])
def test_gemm_tn8_grouped_d5_widths_vs_fp64(M):
    """the four D5 problems of a block in one launch: rel-L2 < 1e-4 against fp64 of the same dequantised bytes, < 8e-2 against the
    un-quantised product; alpha is honoured and the products are added to a non-zero C"""
    from autoprog_amd import ops
    probs, refs, exact = [], [], []
    for i, (n1, n2) in enumerate(D5_PROBLEMS):
        a, b, a8, b8, dqa, dqb = _operands(M, n1, n2, 10 * i + M)
        c = torch.randn(n1, n2, device="cuda")
        c0 = c.double().cpu()
        alpha = 0.75 if i == 1 else 1.0
        probs.append(ops.Tn8Problem(a8, b8, c, n1, n2, dqa, dqb, alpha=alpha))
        ad, bd = _deq(a8, b8, dqa, dqb)
        refs.append((c, c0, alpha * ad.t() @ bd, alpha * a.double().cpu().t() @ b.double().cpu()))
    ops.gemm_tn8_acc_grouped(probs)
    torch.cuda.synchronize()
    for c, c0, pq, pf in refs:
        got = c.double().cpu() - c0
        e_q, e_f = rel(got, pq), rel(got, pf)
        print("M %d %s: vs dequantised %.2e, vs bf16 operands %.3e" % (M, tuple(c.shape), e_q, e_f))
        assert e_q < 1e-4 and e_f < 8e-2


def test_gemm_tn8_e4m3_a_operand_and_tn_grouped_dispatch():
    """a_fmt = e4m3 on A, and a Tn8Problem handed to gemm_tn_acc_grouped next to a bf16 problem (the weight-gradient window's path)"""
    from autoprog_amd import ops
    from autoprog_amd._lib import FP8_E4M3
    M, n1, n2 = 4096, 768, 768
    a = torch.randn(M, n1, device="cuda").to(torch.bfloat16)
    b = torch.randn(M, n2, device="cuda").to(torch.bfloat16)
    a8, dqa = ops.quantize_fp8_now(a)
    b8, dqb = ops.quantize_fp8_now(b)
    c8 = torch.zeros(n1, n2, device="cuda")
    c16 = torch.zeros(n1, n2, device="cuda")
    ops.gemm_tn_acc_grouped([ops.Tn8Problem(a8, b8, c8, n1, n2, dqa, dqb, a_fmt=FP8_E4M3), (a, b, c16, n1, n2, None)])
    torch.cuda.synchronize()
    ad = a8.view(torch.float8_e4m3fn).double().cpu() * float(dqa)
    bd = b8.view(torch.float8_e4m3fn).double().cpu() * float(dqb)
    assert rel(c8, ad.t() @ bd) < 1e-4
    assert rel(c16, a.double().cpu().t() @ b.double().cpu()) < 1e-2


def test_gemm_tn8_deterministic_bitwise(monkeypatch):
    from autoprog_amd import ops
    monkeypatch.setattr(ops, "deterministic", True)
    outs = []
    ops_ = []
    for i, (n1, n2) in enumerate(D5_PROBLEMS):
        ops_.append(_operands(50176 + 64, n1, n2, i))
    for _ in range(2):
        cs = [torch.zeros(n1, n2, device="cuda") for (n1, n2) in D5_PROBLEMS]
        ops.gemm_tn8_acc_grouped([ops.Tn8Problem(o[2], o[3], c, c.shape[0], c.shape[1], o[4], o[5]) for o, c in zip(ops_, cs)])
        outs.append(cs)
    for c1, c2, o in zip(outs[0], outs[1], ops_):
        assert torch.equal(c1, c2)
        ad, bd = _deq(o[2], o[3], o[4], o[5])
        assert rel(c1, ad.t() @ bd) < 1e-4


def test_gemm_tn8_deterministic_token_splits(monkeypatch):
    """one 768 x 768 problem at M = 4096 under the deterministic mode: the launch cuts the tokens into several ranges whose partial tiles
    the ordered reduce adds -- bitwise equal over two runs, and equal to the fp64 product of the same bytes"""
    from autoprog_amd import ops
    from autoprog_amd._lib import Tn8Problem as _P
    monkeypatch.setattr(ops, "deterministic", True)
    a, b, a8, b8, dqa, dqb = _operands(4096, 768, 768, 5)
    c0 = torch.zeros(768, 768, device="cuda")
    q = _P(a8.data_ptr(), 768, b8.data_ptr(), 768, c0.data_ptr(), 768, 4096, 768, 768, 1, 1.0, dqa.data_ptr(), dqb.data_ptr())
    from autoprog_amd._lib import lib
    assert lib.ap_gemm_tn8_grouped_workspace(ctypes.byref(q), 1) > 4 * 768 * 768          # more than one token split
    outs = []
    for _ in range(2):
        c = torch.full((768, 768), 0.5, device="cuda")
        ops.gemm_tn8_acc_grouped([ops.Tn8Problem(a8, b8, c, 768, 768, dqa, dqb)])
        outs.append(c)
    assert torch.equal(outs[0], outs[1])
    ad, bd = _deq(a8, b8, dqa, dqb)
    assert rel(outs[0].double().cpu() - 0.5, ad.t() @ bd) < 1e-4


def test_gemm_tn8_unsupported_width():
    from autoprog_amd._lib import Tn8Problem, lib
    t = torch.zeros(256, 200, dtype=torch.uint8, device="cuda")
    c = torch.zeros(200, 200, device="cuda")
    dq = torch.ones(1, device="cuda")
    q = Tn8Problem(t.data_ptr(), 208, t.data_ptr(), 208, c.data_ptr(), 200, 256, 200, 200, 1, 1.0, dq.data_ptr(), dq.data_ptr())
    assert lib.ap_gemm_tn8_acc_grouped(ctypes.byref(q), 1, None, 0, None) == -2          # AP_ERR_UNSUPPORTED
    assert lib.ap_gemm_tn8_grouped_workspace(ctypes.byref(q), 1) == 0


def _block_run(monkeypatch, wgrad8, real8, real16, B=8, N=784, C=768, heads=16):
    from autoprog_amd import functional as AF, ops, wgrad
    from autoprog_amd.models.volo import Transformer
    AF.reset_fp8_state()
    monkeypatch.setattr(AF, "FP8_LINEAR", True)
    monkeypatch.setattr(AF, "FP8_WGRAD", wgrad8)
    torch.manual_seed(0)
    blk = Transformer(C, heads, mlp_ratio=4.0, qkv_bias=True).cuda().train()
    x = torch.randn(B, 28, 28, C, device="cuda").to(torch.bfloat16).requires_grad_(True)
    dy = torch.randn_like(x)
    keep = 0.8
    g = torch.Generator(device="cuda").manual_seed(3)
    k1 = (torch.rand(B, device="cuda", generator=g) < keep).float()
    k2 = (torch.rand(B, device="cuda", generator=g) < keep).float()
    k1[0], k2[1] = 0.0, 0.0
    tm1, tm2 = AF.token_mask(k1, N), AF.token_mask(k2, N)
    a, m = blk.attn, blk.mlp
    kinds = []
    monkeypatch.setattr(ops, "gemm_tn8_acc_grouped", lambda p, ln=None: (kinds.extend(["fp8"] * len(p)), real8(p, ln=ln))[1])

    def tn16(p, ln=None):
        kinds.extend("bf16" for q in p if not isinstance(q, ops.Tn8Problem))
        return real16(p, ln=ln)
    monkeypatch.setattr(ops, "gemm_tn_acc_grouped", tn16)
    y = AF.TransformerBlockFn.apply(x, k1 / keep, k2 / keep, blk.norm1.weight, blk.norm1.bias, a.qkv.weight, a.qkv.bias, a.proj.weight,
                                    a.proj.bias, blk.norm2.weight, blk.norm2.bias, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias,
                                    B, N, heads, blk.norm1.eps, k1, k2, tm1, tm2, 1.0 / keep)
    y.backward(dy)
    wgrad.flush_wgrad_window()
    torch.cuda.synchronize()
    AF.reset_fp8_state()
    return y.detach().clone(), x.grad.detach().clone(), {n: p.grad.detach().clone() for n, p in blk.named_parameters()}, kinds


def test_block_fp8_wgrad_vs_bf16_wgrad(monkeypatch):
    """one VOLO-D5 transformer block (C = 768, 784 tokens x 8 images, DropPath masks with dropped samples) under FP8_LINEAR, with and
    without FP8_WGRAD (AP_DETERMINISTIC=1): output and input gradient bit-identical; four fp8 weight-gradient problems and no bf16 one;
    weight gradients within 0.08 of the bf16-wgrad run (measured 0.055 - 0.060 per tensor: e5m2 keeps 2 mantissa bits), biases within 1e-2
    (measured 0: the bias sums are formed from the bf16 gradient); the LayerNorm parameter gradients only change their summation order"""
    from autoprog_amd import ops
    monkeypatch.setattr(ops, "deterministic", True)
    real = (ops.gemm_tn8_acc_grouped, ops.gemm_tn_acc_grouped)
    y0, dx0, g0, k0 = _block_run(monkeypatch, False, *real)
    y1, dx1, g1, k1 = _block_run(monkeypatch, True, *real)
    assert k0 == ["bf16"] * 4 and k1 == ["fp8"] * 4, (k0, k1)
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
    errs = {n: rel(g1[n], g0[n]) for n in g0}
    print("fp8 wgrad vs bf16 wgrad:", {k: round(v, 4) for k, v in errs.items()})
    for n, e in errs.items():
        if n.endswith(".bias"):
            assert e < 1e-2, (n, e)
        elif n.startswith("norm"):
            assert e < 1e-6, (n, e)
        else:
            assert e < 8e-2, (n, e)


def test_volo_d5_shapes_448_fp8_wgrad_vs_oracle(monkeypatch):
    """the D5-shape network of tests/test_gpu_model.py under FP8_LINEAR + FP8_WGRAD against the fp64 oracle, at the bounds of the fp8
    forward test: parameter gradients <= 0.12 per tensor (0.2 in the stem); the printed line gives the median and the worst tensor"""
    from autoprog_amd import functional as AF
    from tests.test_gpu_model import _d5_shapes_vs_oracle
    AF.reset_fp8_state()
    monkeypatch.setattr(AF, "FP8_LINEAR", True)
    monkeypatch.setattr(AF, "FP8_WGRAD", True)
    try:
        _d5_shapes_vs_oracle(out_tol=8e-2, loss_tol=1e-2, grad_tol=0.12, stem_tol=0.2, tag="fp8 forward + fp8 weight gradients")
    finally:
        AF.reset_fp8_state()


def test_fp8_wgrad_training_steps_on_a_small_volo(monkeypatch):
    """six optimizer steps of a small VOLO (widths 128 / 256: the transformer blocks take the fp8 weight gradients) under the mode:
    the loss stays finite and decreases"""
    from autoprog_amd import functional as AF, ops
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import TokenLabelCrossEntropy
    from autoprog_amd.models.volo import VOLO
    from autoprog_amd.optim import FlatAdamWEma
    AF.reset_fp8_state()
    monkeypatch.setattr(AF, "FP8_LINEAR", True)
    monkeypatch.setattr(AF, "FP8_WGRAD", True)
    n8 = []
    real8 = ops.gemm_tn8_acc_grouped
    monkeypatch.setattr(ops, "gemm_tn8_acc_grouped", lambda p, ln=None: (n8.append(len(p)), real8(p, ln=ln))[1])
    torch.manual_seed(0); np.random.seed(0)
    model = VOLO([1, 2, 0, 0], img_size=64, num_classes=16, embed_dims=[128, 256, 256, 256], num_heads=[4, 8, 8, 8],
                 mlp_ratios=[4, 4, 4, 4], downsamples=[True, False, False, False], outlook_attention=[True, False, False, False],
                 post_layers=["ca", "ca"], stem_hidden_dim=16).cuda().train()
    red = GradientBucketReducer(list(model.parameters()), world_size=1)
    red.install_sink(model)
    opt = FlatAdamWEma(model, red, lr=1e-3, weight_decay=0.05, ema_decays=[0.9])
    loss_fn = TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=16)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(8, 3, 64, 64, generator=g).cuda()
    target = torch.softmax(torch.randn(8, 16, 18, generator=g) * 2, dim=1).cuda()
    ls = []
    try:
        for _ in range(6):
            red.zero_grad()
            loss = loss_fn(model(x), target)
            loss.backward()
            red.finish()
            opt.step()
            ls.append(float(loss.detach()))
    finally:
        red.remove()
        AF.reset_fp8_state()
    print("fp8-wgrad losses", [round(v, 4) for v in ls], "fp8 problems per step", sum(n8) / 6)
    assert sum(n8) == 6 * 8                                   # two transformer blocks x four Linears per step
    assert all(np.isfinite(ls)) and ls[-1] < ls[0]


def test_graphed_step_replay_matches_the_eager_step(monkeypatch):
    """one GraphedStep replay under FP8_LINEAR + FP8_WGRAD and AP_DETERMINISTIC=1 (the e5m2 gradient sites roll inside the captured step;
    every dq is read from device memory) equals the eager step from the same state bit for bit: loss, weights, Adam moments"""
    from autoprog_amd import functional as AF, ops
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.graph import GraphedStep
    from autoprog_amd.loss import TokenLabelCrossEntropy
    from autoprog_amd.models.volo import VOLO
    from autoprog_amd.optim import FlatAdamWEma
    AF.reset_fp8_state()
    monkeypatch.setattr(ops, "deterministic", True)
    monkeypatch.setattr(AF, "FP8_LINEAR", True)
    monkeypatch.setattr(AF, "FP8_WGRAD", True)
    n8 = []
    real8 = ops.gemm_tn8_acc_grouped
    monkeypatch.setattr(ops, "gemm_tn8_acc_grouped", lambda p, ln=None: (n8.append(len(p)), real8(p, ln=ln))[1])
    torch.manual_seed(0); np.random.seed(0)
    model = VOLO([1, 2, 0, 0], img_size=64, num_classes=16, embed_dims=[128, 256, 256, 256], num_heads=[4, 8, 8, 8],
                 mlp_ratios=[4, 4, 4, 4], downsamples=[True, False, False, False], outlook_attention=[True, False, False, False],
                 post_layers=["ca", "ca"], stem_hidden_dim=64).cuda().train()
    red = GradientBucketReducer(list(model.parameters()), world_size=1, defer_mean=True)
    red.install_sink(model)
    opt = FlatAdamWEma(model, red, lr=1e-3, weight_decay=0.05, ema_decays=[0.9])
    loss_fn = TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=16)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(8, 3, 64, 64, generator=g).cuda()
    target = torch.softmax(torch.randn(8, 16, 18, generator=g) * 2, dim=1).cuda()
    sc = AF.fp8_scales
    try:
        gs = GraphedStep(model, loss_fn, red, opt, x, target)
        gs.capture(warmup=2)
        assert sum(n8) > 0 and sc.qmax is not None                    # fp8 weight gradients and e5m2 sites took part
        torch.cuda.synchronize()
        snap = [t.clone() for t in (opt.p, opt.m, opt.v, *opt.ema, *opt._buffers, sc.amax, sc.scale, sc.dq)]
        bufs = [b.detach().clone() for b in model.buffers()]
        step0 = opt.step_count
        np.random.seed(11); torch.manual_seed(5)
        loss_g = gs.step().clone()
        torch.cuda.synchronize()
        got = [opt.p.clone(), opt.m.clone(), opt.v.clone()]
        with torch.no_grad():
            for t, t0 in zip((opt.p, opt.m, opt.v, *opt.ema, *opt._buffers, sc.amax, sc.scale, sc.dq), snap):
                t.copy_(t0)
            for b, b0 in zip(model.buffers(), bufs):
                b.copy_(b0)
        opt.step_count = step0
        opt.resync()
        AF._WeightBank.generation += 1                                # the replayed step rolled the scales and re-quantised the weights
        gs.release()
        np.random.seed(11); torch.manual_seed(5)
        red.zero_grad()
        loss_e = loss_fn(model(x), target)
        loss_e.backward()
        red.finish()
        opt.step()
        torch.cuda.synchronize()
    finally:
        red.remove()
        AF.reset_fp8_state()
    print("graphed %.6f eager %.6f" % (float(loss_g), float(loss_e)))
    assert torch.equal(loss_g.float().reshape(-1), loss_e.detach().float().reshape(-1))
    for a, b in zip(got, (opt.p, opt.m, opt.v)):
        assert torch.equal(a, b)
