"""The forward-only path (functional.infer_mode): ap_mlp_fused_infer, ap_gemm_epilogue.gelu = 4 and the forward-only block bodies are
BIT-IDENTICAL to the training forward (torch.equal, no tolerance); ap_classify_stats against fp64 on the CPU; prog.validate against a
loop written the way the reference writes it; the driver's per-epoch validation."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, device="cuda", generator=g) * scale).to(BF16)


def _f32(*shape, scale=1.0, seed=0, shift=0.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, device="cuda", generator=g) * scale + shift


# ------------------------------------------------------------------------------------------------ 1. ap_mlp_fused_infer
def _mlp_operands(m, seed):
    C, H = 384, 1152
    x = _bf(m, C, scale=2.0, seed=seed)                       # |x| up to a few units; the pre-activations cover both sides of zero
    wa, wb = _bf(H, C, scale=0.05, seed=seed + 1), _bf(C, H, scale=0.03, seed=seed + 2)
    b1, b2 = _f32(H, scale=0.5, seed=seed + 3), _f32(C, scale=0.5, seed=seed + 4)
    res = _bf(m, C, seed=seed + 5)
    return x, wa, wb, b1, b2, res, (_f32(C, scale=0.2, seed=seed + 6, shift=1.0), _f32(C, scale=0.2, seed=seed + 7))


@pytest.mark.parametrize("m", [128, 3200, 25088])
@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("scaled", [False, True])
def test_mlp_fused_infer_bit_identical(m, ln, residual, scaled):
    from autoprog_amd import ops
    x, wa, wb, b1, b2, res, (gam, bet) = _mlp_operands(m, seed=m + 10 * ln + 100 * residual)
    rps = 64 if m % 64 == 0 else 1
    kw = dict(bias1=b1, bias2=b2, rows_per_scale=rps, residual=res if residual else None)
    if scaled:
        g = torch.Generator(device="cuda").manual_seed(9)
        keep = (torch.rand(m // rps, device="cuda", generator=g) > 0.25).float()
        kw.update(row_scale_hidden=keep, row_scale_out=keep / 0.75)
    lnk = dict(ln=(x, gam, bet, 1e-5)) if ln else {}
    ref = ops.mlp_fused(None if ln else x, wa, wb, **kw, **lnk)
    got = ops.mlp_fused_infer(None if ln else x, wa, wb, **kw, **lnk)
    assert ref is not None and got is not None
    torch.cuda.synchronize()
    assert torch.equal(got, ref[0])


@pytest.mark.parametrize("ln", [False, True])
def test_mlp_fused_infer_never_writes_side_outputs(ln):
    """a call with sentinel-filled side buffers leaves them untouched; the ops call passes them as null (the test above)"""
    from autoprog_amd import ops
    from autoprog_amd._lib import lib, MlpFusedArgs
    m, C, H = 256, 384, 1152
    x, wa, wb, b1, b2, res, (gam, bet) = _mlp_operands(m, seed=5)
    out = torch.empty(m, C, dtype=BF16, device="cuda")
    hid = torch.full((m, H), 0x5A, dtype=torch.uint8, device="cuda").repeat(1, 2)           # [m, 2 H] bytes = bf16 [m, H]
    codes = torch.full((m, H), 0x5A, dtype=torch.uint8, device="cuda")
    lno = torch.full((m, 2 * C), 0x5A, dtype=torch.uint8, device="cuda")
    mean, rstd = torch.full((m, 4), 0x5A, dtype=torch.uint8, device="cuda"), torch.full((m, 4), 0x5A, dtype=torch.uint8, device="cuda")
    a = MlpFusedArgs()
    a.x, a.ldx, a.wa, a.ldwa, a.wb, a.ldwb, a.out, a.ldo = x.data_ptr(), C, wa.data_ptr(), C, wb.data_ptr(), H, out.data_ptr(), C
    a.hidden_out, a.ldh, a.codes = hid.data_ptr(), H, codes.data_ptr()
    a.bias1, a.bias2, a.rows_per_scale, a.residual, a.ldr = b1.data_ptr(), b2.data_ptr(), 1, res.data_ptr(), C
    a.m, a.c, a.hidden, a.backward = m, C, H, 0
    if ln:
        a.x = None
        a.ln_in, a.ld_ln, a.ln_out, a.ld_lno = x.data_ptr(), C, lno.data_ptr(), C
        a.ln_gamma, a.ln_beta, a.ln_eps, a.ln_mean, a.ln_rstd = gam.data_ptr(), bet.data_ptr(), 1e-5, mean.data_ptr(), rstd.data_ptr()
    assert lib.ap_mlp_fused_infer(ctypes.byref(a), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    for t in (hid, codes, lno, mean, rstd):
        assert bool((t == 0x5A).all())
    ref = ops.mlp_fused(None if ln else x, wa, wb, bias1=b1, bias2=b2, residual=res, **(dict(ln=(x, gam, bet, 1e-5)) if ln else {}))
    assert torch.equal(out, ref[0])


def test_mlp_fused_infer_error_codes():
    """shapes the host refuses before any launch"""
    from autoprog_amd._lib import lib, MlpFusedArgs
    big = torch.zeros(128, 1152, dtype=BF16, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    P = big.data_ptr()

    def margs(**kw):
        a = MlpFusedArgs()
        a.x, a.ldx, a.wa, a.ldwa, a.wb, a.ldwb, a.out, a.ldo = P, 384, P, 384, P, 1152, P, 384
        a.ldh, a.rows_per_scale, a.m, a.c, a.hidden, a.backward = 1152, 1, 128, 384, 1152, 0
        for k_, v_ in kw.items():
            setattr(a, k_, v_)
        return ctypes.byref(a)
    assert lib.ap_mlp_fused_infer(None, st) == -4
    assert lib.ap_mlp_fused_infer(margs(out=None), st) == -4
    assert lib.ap_mlp_fused_infer(margs(m=100), st) == -2
    assert lib.ap_mlp_fused_infer(margs(c=192, hidden=576, ldx=192, ldwa=192, ldwb=576, ldo=192), st) == -2
    assert lib.ap_mlp_fused_infer(margs(backward=1), st) < 0
    assert lib.ap_mlp_fused_infer(margs(x=None, ln_in=P, ld_ln=384), st) == -4                     # LayerNorm without gamma / beta
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. gelu = 4 against gelu = 3
@pytest.mark.parametrize("M,N,K,rps", [(100352, 576, 192, 196), (8192, 1152, 384, 64), (12800, 1152, 384, 100), (25088, 1152, 384, 196),
                                       (12608, 3072, 768, 197), (15680, 1152, 384, 196), (64, 1152, 384, 1)])
@pytest.mark.parametrize("scaled", [False, True])
def test_gemm_gelu_table_mode_equals_mode3_out(M, N, K, rps, scaled):
    from autoprog_amd import ops
    a, w, b = _bf(M, K, scale=1.5, seed=M + N), _bf(N, K, scale=0.06, seed=K), _f32(N, scale=0.5, seed=3)
    kw = {}
    if scaled:
        g = torch.Generator(device="cuda").manual_seed(11)
        kw = dict(row_scale=(torch.rand(M // rps, device="cuda", generator=g) > 0.25).float(), rows_per_scale=rps)
    side = torch.empty(M, N, dtype=torch.uint8, device="cuda")
    ref = ops.gemm_nt(a, w, bias=b, gelu=True, preact_out=side, preact_grad=2, **kw)
    n0 = ops.GELU_TABLE_FALLBACKS
    got = ops.gemm_nt(a, w, bias=b, gelu="table", **kw)
    fell_back = ops.GELU_TABLE_FALLBACKS - n0
    torch.cuda.synchronize()
    # the skinny kernel (M <= 256) has no mode 4: ops ran mode 3 with a side buffer of its own; the model's un-fused shapes are served
    assert fell_back == (1 if M <= 256 else 0)
    assert torch.equal(got, ref)


def test_gemm_gelu_mode4_raw_abi():
    """mode 4 ignores preact_out (null here), and a launch outside its kernels answers AP_ERR_UNSUPPORTED, not a launch"""
    from autoprog_amd._lib import lib, GemmEpilogue
    a, w, b = _bf(8192, 384, seed=1), _bf(1152, 384, scale=0.05, seed=2), _f32(1152, seed=3)
    out = torch.empty(8192, 1152, dtype=BF16, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    e = GemmEpilogue()
    e.bias, e.gelu, e.preact_out, e.rows_per_scale = b.data_ptr(), 4, None, 1
    assert lib.ap_gemm_nt(a.data_ptr(), 384, w.data_ptr(), 384, out.data_ptr(), 1152, 8192, 1152, 384, ctypes.byref(e), st) == 0
    assert lib.ap_gemm_nt(a.data_ptr(), 384, w.data_ptr(), 384, out.data_ptr(), 1152, 64, 1152, 384, ctypes.byref(e), st) == -2
    e.gelu = 5
    assert lib.ap_gemm_nt(a.data_ptr(), 384, w.data_ptr(), 384, out.data_ptr(), 1152, 8192, 1152, 384, ctypes.byref(e), st) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. whole blocks
def _both_paths(monkeypatch, fn):
    """fn() under no_grad with the forward-only bodies, and with the training Functions (switch off)"""
    from autoprog_amd import functional as AF
    with torch.no_grad():
        monkeypatch.setattr(AF, "INFER", True)
        got = fn()
        monkeypatch.setattr(AF, "INFER", False)
        ref = fn()
    monkeypatch.setattr(AF, "INFER", True)
    torch.cuda.synchronize()
    return got, ref


@pytest.mark.parametrize("B,N,drop", [(128, 196, 0.0), (128, 64, 0.0), (128, 196, 0.2)])
def test_transformer_block_forward_only_equals_training_forward(monkeypatch, B, N, drop):
    from autoprog_amd.models.volo import Transformer
    torch.manual_seed(1)
    blk = Transformer(384, num_heads=12, mlp_ratio=3.0, drop_path=drop).cuda().train()
    for p in blk.parameters():
        if p.dim() == 1:
            torch.nn.init.normal_(p, std=0.3)
    x = _bf(B, N, 384, seed=N)

    def run():
        torch.manual_seed(7)                     # the DropPath masks of a train-mode forward: the same draws on both paths
        return blk(x)
    got, ref = _both_paths(monkeypatch, run)
    assert torch.equal(got, ref)
    torch.manual_seed(7)
    assert torch.equal(got, blk(x).detach())     # ... and the forward with autograd on


def test_outlooker_block_forward_only_equals_training_forward(monkeypatch):
    from autoprog_amd.models.volo import Outlooker
    torch.manual_seed(2)
    blk = Outlooker(192, kernel_size=3, padding=1, stride=2, num_heads=6, mlp_ratio=3.0).cuda().train()
    x = _bf(8, 56, 56, 192, seed=4)
    got, ref = _both_paths(monkeypatch, lambda: blk(x))
    assert torch.equal(got, ref)
    assert torch.equal(got, blk(x).detach())


def test_class_block_forward_only_equals_training_forward(monkeypatch):
    from autoprog_amd.models.volo import ClassBlock
    torch.manual_seed(3)
    blk = ClassBlock(384, num_heads=12, mlp_ratio=3.0).cuda().train()
    cls, tok = _bf(32, 384, seed=5), _bf(32, 196, 384, seed=6)
    got, ref = _both_paths(monkeypatch, lambda: blk.forward_split(cls, tok))
    assert torch.equal(got, ref)
    assert torch.equal(got, blk.forward_split(cls, tok).detach())


@pytest.mark.parametrize("mode,fuse_proj", [("train", True), ("eval", True), ("train", False)])
def test_stem_forward_only_equals_training_forward_with_its_running_statistics(monkeypatch, mode, fuse_proj):
    """the 64-wide stem under no_grad, forward-only body against the training Function from the same state_dict: the output and every buffer after
    the pass (a train-mode pass takes batch statistics and updates the running ones), on an odd batch and a map that does not divide the
    convolution tiles.  fuse_proj: the last BatchNorm + ReLU inside the patch projection (Stem64Fn apply_last = False), or applied by the stem"""
    from autoprog_amd import functional as AF
    from autoprog_amd.models.volo import PatchEmbed
    monkeypatch.setattr(AF, "STEM_FUSE_BN_PROJ", fuse_proj)
    torch.manual_seed(11)
    pe = PatchEmbed(stem_conv=True, stem_stride=2, patch_size=8, in_chans=3, hidden_dim=64, embed_dim=192).cuda()
    with torch.no_grad():
        for name, b in pe.named_buffers():                        # running statistics away from their initial 0 / 1: an eval pass reads them
            if name.endswith("running_mean"):
                b.normal_(std=0.2)
            elif name.endswith("running_var"):
                b.uniform_(0.5, 1.5)
    pe.train(mode == "train")
    state = {k: v.clone() for k, v in pe.state_dict().items()}
    x = torch.randn(3, 3, 80, 80, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))

    def run():
        pe.load_state_dict(state)
        return pe(x).clone(), {n: b.clone() for n, b in pe.named_buffers()}
    (y, bufs), (y_ref, bufs_ref) = _both_paths(monkeypatch, run)
    assert torch.equal(y, y_ref) and bool(torch.isfinite(y.float()).all())
    assert set(bufs) == set(bufs_ref) and len(bufs) == 9          # three BatchNorms: running_mean, running_var, num_batches_tracked
    for n in bufs:
        assert torch.equal(bufs[n], bufs_ref[n]), n
        assert torch.equal(bufs[n], state[n]) == (mode == "eval"), n      # train mode moved every one of them, eval none


# ------------------------------------------------------------------------------------------------ 4 / 5. whole models
def _outs(o):
    return [t for t in (o if isinstance(o, (tuple, list)) else [o]) if torch.is_tensor(t)]


def _model_three_ways(monkeypatch, model, x):
    """-> (no_grad + forward-only, no_grad + switch off, autograd on), same numpy / torch seeds before each"""
    from autoprog_amd import functional as AF
    res = []
    for infer, grad in ((True, False), (False, False), (True, True)):
        monkeypatch.setattr(AF, "INFER", infer)
        np.random.seed(5)
        torch.manual_seed(5)
        with torch.set_grad_enabled(grad):
            res.append([t.detach() for t in _outs(model(x))])
    monkeypatch.setattr(AF, "INFER", True)
    torch.cuda.synchronize()
    return res


def _assert_same(res):
    a, b, c = res
    assert len(a) == len(b) == len(c) and len(a) >= 1
    for t, u, v in zip(a, b, c):
        assert torch.equal(t, u) and torch.equal(t, v)


def test_volo_d1_eval_forward_only_equals_autograd_forward_and_takes_the_path(monkeypatch):
    from autoprog_amd import functional as AF, ops
    from autoprog_amd.models import create_model
    torch.manual_seed(0)
    model = create_model("volo_d1", num_classes=1000, img_size=224).cuda().eval()
    x = torch.randn(32, 3, 224, 224, device="cuda")
    _assert_same(_model_three_ways(monkeypatch, model, x))
    # 5. the path is really taken (batch 128: the transformer stages have 25088 rows, the fused MLP's ground)
    counts = {"infer": 0, "train": 0, "side": 0}

    def counting(name, fn):
        def wrapped(*a, **k):
            counts[name] += 1
            return fn(*a, **k)
        return wrapped
    monkeypatch.setattr(ops, "mlp_fused_infer", counting("infer", ops.mlp_fused_infer))
    monkeypatch.setattr(ops, "mlp_fused", counting("train", ops.mlp_fused))
    monkeypatch.setattr(AF, "_gelu_side_buffer", counting("side", AF._gelu_side_buffer))
    x = torch.randn(128, 3, 224, 224, device="cuda")
    with torch.no_grad():
        model(x)
    torch.cuda.synchronize()
    assert counts["infer"] >= 1 and counts["train"] == 0 and counts["side"] == 0, counts


def test_supernet_probe_forward_only_equals_autograd_forward(monkeypatch):
    """the search's probe: volo_h12_l18 in train() mode at (l, r) = (9, 128), mix-token on, DropPath 0"""
    from autoprog_amd.models import create_model
    torch.manual_seed(0)
    model = create_model("model_variant", variant="volo_h12_l18", num_classes=1000, img_size=224).cuda().train()
    model.set_sample_config(dict(layer_num=9, min_layer_num=9, max_layer_num=18, input_size=128, token_label_size=8))
    model.set_drop_path_rate(0.0)
    x = torch.randn(32, 3, 128, 128, device="cuda")
    _assert_same(_model_three_ways(monkeypatch, model, x))


def test_deit_tiny_forward_only_equals_autograd_forward(monkeypatch):
    from autoprog_amd.models import create_model
    torch.manual_seed(0)
    model = create_model("deit_tiny_patch16_224", num_classes=1000).cuda().eval()
    x = torch.randn(32, 3, 224, 224, device="cuda")
    _assert_same(_model_three_ways(monkeypatch, model, x))


# ------------------------------------------------------------------------------------------------ 6. peak memory
def test_forward_only_peak_memory_is_lower(monkeypatch):
    from autoprog_amd import functional as AF
    from autoprog_amd.models import create_model
    torch.manual_seed(0)
    model = create_model("volo_d1", num_classes=1000, img_size=224).cuda().eval()
    x = torch.randn(128, 3, 224, 224, device="cuda")
    peak = {}
    for infer in (False, True, False, True):          # (the first round also warms the allocator and the weight copies)
        monkeypatch.setattr(AF, "INFER", infer)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        with torch.no_grad():
            y = model(x)
        torch.cuda.synchronize()
        peak[infer] = torch.cuda.max_memory_allocated()
        del y
    monkeypatch.setattr(AF, "INFER", True)
    print("peak bytes of a no_grad forward, volo_d1 224 px batch 128: switch off %d, forward-only %d" % (peak[False], peak[True]))
    assert peak[True] < peak[False], peak


# ------------------------------------------------------------------------------------------------ 7 / 8. ap_classify_stats
def _distinct_rows(rows, C, ld, seed):
    """rows that are permutations of C DISTINCT bf16 values: the consecutive bit patterns from 0x3C00 upward"""
    g = torch.Generator().manual_seed(seed)
    vals = (torch.arange(C, dtype=torch.int32) + 0x3C00).to(torch.int16).view(BF16)
    z = torch.zeros(rows, ld, dtype=BF16)
    for r in range(rows):
        z[r, :C] = vals[torch.randperm(C, generator=g)]
    if ld > C:
        z[:, C:] = 100.0                            # columns beyond n_classes must not be read as classes
    return z, torch.randint(0, C, (rows,), generator=g)


@pytest.mark.parametrize("ld", [1000, 1008])
def test_classify_stats_rank_and_loss_without_ties(ld):
    from autoprog_amd import ops
    C, rows = 1000, 257
    z, lab = _distinct_rows(rows, C, ld, seed=ld)
    loss, rank = ops.classify_stats(z.cuda(), lab.cuda(), n_classes=C)
    loss, rank = loss.cpu(), rank.cpu()
    zc = z[:, :C]
    order = torch.topk(zc.float(), C, dim=1).indices                       # no ties: the order is unique
    pos = (order == lab[:, None]).int().argmax(1)
    assert torch.equal(rank.long(), pos.long())
    # timm.utils.accuracy restated: the label is among the first k of topk
    for k in (1, 5):
        correct = (order[:, :k] == lab[:, None]).any(1)
        assert torch.equal(rank < k, correct)
    want = torch.nn.functional.cross_entropy(zc.double(), lab, reduction="none")
    err = (loss.double() - want).abs()
    print("classify_stats loss: max |err| %.3e (bound 1e-5 * max(1, loss), loss up to %.3f)" % (float(err.max()), float(want.max())))
    assert bool((err <= 1e-5 * want.clamp(min=1.0)).all())


@pytest.mark.parametrize("C,ld", [(1000, 1000), (10, 16)])
def test_classify_stats_loss_random_logits(C, ld):
    from autoprog_amd import ops
    g = torch.Generator().manual_seed(C)
    z = torch.zeros(300, ld, dtype=BF16)
    z[:, :C] = (torch.randn(300, C, generator=g) * 4).to(BF16)
    lab = torch.randint(0, C, (300,), generator=g)
    loss, rank = ops.classify_stats(z.cuda(), lab.cuda(), n_classes=C)
    want = torch.nn.functional.cross_entropy(z[:, :C].double(), lab, reduction="none")
    err = (loss.cpu().double() - want).abs()
    print("classify_stats loss (randn * 4, C = %d): max |err| %.3e" % (C, float(err.max())))
    assert bool((err <= 1e-5 * want.clamp(min=1.0)).all())
    zl = z[:, :C].float().gather(1, lab[:, None])
    assert torch.equal(rank.cpu().long(), (z[:, :C].float() > zl).sum(1))


@pytest.mark.parametrize("C", [10, 1000])
def test_classify_stats_ties_padding_and_empty(C):
    from autoprog_amd import ops
    from autoprog_amd._lib import lib
    g = torch.Generator().manual_seed(3)
    z = (torch.randn(6, C, generator=g) * 2).to(BF16)
    lab = torch.tensor([1, 0, 2, -1, C, 3])
    z[0, 4] = z[0, 7] = z[0, 1]                      # the label's value three times
    z[1, :] = 0.75                                   # all equal
    loss, rank = ops.classify_stats(z.cuda(), lab.cuda())
    loss, rank = loss.cpu(), rank.cpu()
    zf = z.float()
    for r in (0, 1, 2, 5):
        assert int(rank[r]) == int((zf[r] > zf[r, lab[r]]).sum())
    assert int(rank[1]) == 0
    assert rank[3] == -1 and rank[4] == -1 and loss[3] == 0 and loss[4] == 0
    want = torch.nn.functional.cross_entropy(z[[0, 1, 2, 5]].double(), lab[[0, 1, 2, 5]], reduction="none")
    assert bool(((loss[[0, 1, 2, 5]].double() - want).abs() <= 1e-5 * want.clamp(min=1.0)).all())
    assert lib.ap_classify_stats(None, C, C, None, None, None, 0, torch.cuda.current_stream().cuda_stream) == 0      # no rows: no launch
    assert lib.ap_classify_stats(z.data_ptr(), C - 2, C, None, None, None, 6, None) == -1                           # ld < n_classes
    e_loss, e_rank = ops.classify_stats(torch.empty(0, C, dtype=BF16, device="cuda"), torch.empty(0, dtype=torch.int64, device="cuda"))
    assert e_loss.numel() == 0 and e_rank.numel() == 0


# ------------------------------------------------------------------------------------------------ 9 / 10. validate, the driver
def _tiny(ema_decays=(0.9, 0.99), img=64, variant="volo_h2_l6"):
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import FlatAdamWEma
    torch.manual_seed(0)
    model = create_model("model_variant", variant=variant, num_classes=16, img_size=img, stem_hidden_dim=16).cuda().train()
    red = GradientBucketReducer(list(model.parameters()), world_size=1, defer_mean=True)
    red.install_sink(model)
    opt = FlatAdamWEma(model, red, lr=1e-3, weight_decay=0.05, ema_decays=list(ema_decays))
    return model, red, opt


def _val_batches(seed=1, img=64):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, 3, img, img, generator=g).cuda(), torch.randint(0, 16, (n,), generator=g).cuda()) for n in (16, 16, 16, 16, 16, 7)]


def _reference_loop(model, batches):
    """the reference's validate, sample-weighted: eval(), no_grad, F.cross_entropy on output.float(), the strict-rank top-k rule"""
    was = model.training
    model.eval()
    tot, c1, c5, n = 0.0, 0, 0, 0
    with torch.no_grad():
        for x, lab in batches:
            out = model(x)
            out = out[0] if isinstance(out, (tuple, list)) else out
            z = out.float()
            tot += float(torch.nn.functional.cross_entropy(z.double(), lab, reduction="sum"))
            rank = (z > z.gather(1, lab[:, None])).sum(1)
            c1 += int((rank < 1).sum()); c5 += int((rank < 5).sum()); n += len(lab)
    model.train(was)
    return tot / n, 100.0 * c1 / n, 100.0 * c5 / n


def test_validate_matches_reference_loop_and_ema_copies_are_restored():
    from autoprog_amd.prog.validate import validate, validate_ema
    model, red, opt = _tiny()
    try:
        with torch.no_grad():                                      # EMA copies that differ from the model and from each other
            opt.ema[0].mul_(1.01)
            opt.ema[1].mul_(0.98)
        batches = _val_batches()
        want = _reference_loop(model, batches)
        assert model.training
        m = validate(model, batches)
        assert model.training and list(m) == ["loss", "top1", "top5"]
        assert abs(m["loss"] - want[0]) <= 1e-5 * abs(want[0])
        assert m["top1"] == want[1] and m["top5"] == want[2]
        p0, e0 = opt.p.clone(), [e.clone() for e in opt.ema]
        me = validate_ema(model, opt, batches)
        assert list(me) == ["%s_EMA_%s" % (k, d) for d in (0.9, 0.99) for k in ("loss", "top1", "top5")]
        assert torch.equal(opt.p, p0) and all(torch.equal(a, b) for a, b in zip(opt.ema, e0))
        for i, d in enumerate((0.9, 0.99)):
            with opt.ema_weights(i):
                w = _reference_loop(model, batches)
            assert abs(me["loss_EMA_%s" % d] - w[0]) <= 1e-5 * abs(w[0])
            assert me["top1_EMA_%s" % d] == w[1] and me["top5_EMA_%s" % d] == w[2]
        assert me["loss_EMA_0.9"] != m["loss"]
    finally:
        red.remove()


def test_driver_validates_after_each_training_epoch():
    from autoprog_amd.loss import TokenLabelCrossEntropy
    from autoprog_amd.prog.driver import AutoProgDriver
    keys = {}
    for with_val in (False, True):
        model, red, opt = _tiny(img=96)
        loss_fn = TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=16)
        g = torch.Generator().manual_seed(1)

        def get_batch(r):
            x = torch.randn(8, 3, 96, 96, generator=g).cuda()
            return x, torch.softmax(torch.randn(8, 16, 2 + (r // 16) ** 2, generator=g) * 2, dim=1).cuda()
        calls = []

        def get_val_batches():
            calls.append(1)
            return _val_batches(seed=2, img=96)[:2]
        drv = AutoProgDriver(model, loss_fn, opt, red, get_batch, r_list=[64, 96], l_list=[3, 6], dp_list=[0.0, 0.0], grow_epochs=[0, 1],
                             steps_per_epoch=2, auto_grow=False, **(dict(get_val_batches=get_val_batches) if with_val else {}))
        try:
            np.random.seed(3)
            hist = drv.run(2)
        finally:
            red.remove()
        assert [h["kind"] for h in hist] == ["train", "train"]
        keys[with_val] = [sorted(h) for h in hist]
        if with_val:
            assert len(calls) == 2 * 3                             # the model and two EMA copies, per epoch
            for h in hist:
                for sfx in ("", "_EMA_0.9", "_EMA_0.99"):
                    assert 0.0 <= h["top1" + sfx] <= h["top5" + sfx] <= 100.0 and h["loss" + sfx] > 0
            assert model.training
    assert keys[False] == [["dp", "epoch", "kind", "l", "loss", "r"]] * 2
    assert all(set(k) > set(keys[False][0]) for k in keys[True])
