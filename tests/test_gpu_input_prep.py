"""ap_input_prep and what is built on it (autoprog_amd/data.py): a loader's uint8 batch prepared on the device in one launch.

The reference arithmetic is torch on the CPU, written the way the reference's loader and loop write it: timm's PrefetchLoader
`(u8.float() - 255 mean) / (255 std)`, the mix with `x.flip(0)`, the box fill of RandomErasing, then main_prog.py:973
`F.interpolate(..., mode="bilinear", align_corners=False)`.

Bounds: a bf16 output is within ONE bf16 ulp of the fp32 reference, `max(err / (|ref| 2^-8 + 1e-6)) <= 1.01` -- the bound of
test_gpu_kernels.py::test_resize_bilinear; where no arithmetic separates the two (same size, no blend) the outputs are torch.equal; and
with no mix and no erase the launch is torch.equal to the existing resize kernels fed the normalised fp32 tensor."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SIZES = [(224, 224), (224, 192), (224, 160), (224, 128), (256, 224), (64, 96)]
B = 7                                   # odd: image 3 is its own partner
CASES = [(li, lo, hi, ho) for li in ("nchw", "nhwc") for lo in ("s2d16", "nhwc") for hi, ho in SIZES]
IDS = ["%s-%s-%d-%d" % c for c in CASES]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from autoprog_amd import ops as _ops
    return _ops


def dev(t):
    return t.cuda().contiguous()


def norm_consts():
    mean = torch.tensor([m * 255 for m in MEAN]).view(1, 3, 1, 1)
    std = torch.tensor([s * 255 for s in STD]).view(1, 3, 1, 1)
    return mean, std


def table():
    mean, std = norm_consts()
    return ((torch.arange(256, dtype=torch.float32).view(1, 256) - mean.view(3, 1)) / std.view(3, 1)).contiguous()


def batch_hw(n, h, w, seed=0):
    """uint8 NCHW [n,3,h,w]"""
    return torch.randint(0, 256, (n, 3, h, w), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed + h))


def batch(hi, seed=0):
    """uint8 NCHW, every byte value present"""
    return batch_hw(B, hi, hi, seed)


def normalised(u8):
    mean, std = norm_consts()
    return (u8.float() - mean) / std


def block(n_img, R=0, mode=0, lam=1.0, box=(0, 0, 0, 0), seed=0, recs=None):
    """the parameter block of ap_input_prep as a CPU int32 tensor; recs: {(image, slot): (top, left, h, w, v0, v1, v2)}"""
    a = np.zeros(16 + n_img * R * 8, dtype=np.int32)
    f, u = a.view(np.float32), a.view(np.uint32)
    a[0] = mode
    f[1] = lam
    a[2:6] = box
    u[6], u[7] = seed & 0xffffffff, (seed >> 32) & 0xffffffff
    f[8] = 1.0 - lam
    for (b, r), rec in (recs or {}).items():
        o = 16 + (b * R + r) * 8
        a[o:o + 4] = rec[:4]
        f[o + 4:o + 7] = rec[4:7] if len(rec) > 4 else 0.0
    return torch.from_numpy(a)


def reference(u8, ho, mode=0, lam=1.0, box=(0, 0, 0, 0), recs=None, R=0, const=False):
    """[B,3,ho,ho] fp32: collate-time mix -> normalise -> erase -> F.interpolate (the order of the reference's prefetcher path;
    normalising first and mixing after is the same arithmetic up to the uint8 rounding timm's FastCollateMixup adds)"""
    x = normalised(u8)
    if mode == 1:
        x = x * lam + x.flip(0) * (1.0 - lam)
    elif mode == 2:
        yl, yh, xl, xh = box
        x = x.clone()
        x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
    for b in range(u8.shape[0]):
        for r in range(R):
            rec = (recs or {}).get((b, r))
            if rec is None or rec[2] == 0:
                continue
            top, left, h, w = rec[:4]
            v = torch.zeros(3) if const else torch.tensor(rec[4:7], dtype=torch.float32)
            x[b, :, top:top + h, left:left + w] = v.view(3, 1, 1)
    return F.interpolate(x, size=(ho, ho), mode="bilinear", align_corners=False)


def to_nchw(y, lo):
    """the kernel's output as fp32-free bf16 [B,3,H,W] (CPU)"""
    y = y.cpu()
    if lo == "nhwc":
        return y.permute(0, 3, 1, 2)
    n, h2, w2, _ = y.shape
    assert float(y[..., 12:].float().abs().sum()) == 0.0          # channels 12..15 of every space-to-depth block
    return y[..., :12].reshape(n, h2, w2, 2, 2, 3).permute(0, 5, 1, 3, 2, 4).reshape(n, 3, h2 * 2, w2 * 2)


def ratio(y, ref):
    err = (y.float() - ref).abs()
    return float((err / (ref.abs() * 2 ** -8 + 1e-6)).max())


def run(ops, u8, li, lo, ho, blk=None, **kw):
    src = u8 if li == "nchw" else u8.permute(0, 2, 3, 1)
    return to_nchw(ops.input_prep(dev(src), ho, out=lo, table=dev(table()), params=None if blk is None else dev(blk), layout=li,
                                  host_block=blk, **kw), lo)


# ------------------------------------------------------------------------------------------ 1. plain
# every batch of SIZES is a multiple of 16 bytes.  One 5 x 7 image is 105: more than 16 and no multiple of it, so the last 16-byte chunk
# the staging reads crosses the end of the batch and goes byte by byte
PLAIN = [(li, lo, B, hi, hi, ho) for li, lo, hi, ho in CASES] + [(li, lo, 1, 5, 7, 6) for li in ("nchw", "nhwc") for lo in ("s2d16", "nhwc")]


@pytest.mark.parametrize("li,lo,n,hi,wi,ho", PLAIN, ids=IDS + ["%s-%s-5x7-6" % c[:2] for c in PLAIN[len(CASES):]])
def test_plain_is_the_existing_resize_on_the_normalised_tensor(ops, li, lo, n, hi, wi, ho):
    u8 = batch_hw(n, hi, wi)
    x = normalised(u8)                                          # on the CPU: no GPU division enters the comparison
    y = run(ops, u8, li, lo, ho)
    old = ops.resize_bilinear_s2d16(dev(x), ho) if lo == "s2d16" else ops.resize_bilinear_nhwc(dev(x), ho)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (n, 3, ho, ho)
    assert torch.equal(y, to_nchw(old, lo)), "a run fed uint8 and a run fed fp32 are not the same run"
    ref = F.interpolate(x, size=(ho, ho), mode="bilinear", align_corners=False)
    r = ratio(y, ref)
    print("plain %s %s %dx%d->%d: worst err / ulp %.4f" % (li, lo, hi, wi, ho, r))
    assert r <= 1.01
    if hi == wi == ho:
        assert torch.equal(y, ref.to(torch.bfloat16))


# ------------------------------------------------------------------------------------------ 2. mix
@pytest.mark.parametrize("li,lo,hi,ho", CASES, ids=IDS)
def test_mixup_and_cutmix(ops, li, lo, hi, ho):
    u8 = batch(hi, 1)
    plain = run(ops, u8, li, lo, ho)
    for lam in (0.3, 0.5, 1.0):
        y = run(ops, u8, li, lo, ho, block(B, mode=1, lam=lam), mix=True)
        r = ratio(y, reference(u8, ho, 1, lam))
        print("mixup lam %.1f %s %s %d->%d: %.4f" % (lam, li, lo, hi, ho, r))
        assert r <= 1.01
        if lam == 1.0:
            assert torch.equal(y, plain)
    q = hi // 4
    boxes = {"interior": (q, 3 * q, q + 3, 2 * q + 5), "clipped": (0, q + 1, hi - q, hi), "empty": (q, q, 5, 9), "whole": (0, hi, 0, hi)}
    for name, bx in boxes.items():
        y = run(ops, u8, li, lo, ho, block(B, mode=2, lam=0.5, box=bx), mix=True)
        ref = reference(u8, ho, 2, box=bx)
        r = ratio(y, ref)
        print("cutmix %s %s %s %d->%d: %.4f" % (name, li, lo, hi, ho, r))
        assert r <= 1.01
        if hi == ho:
            assert torch.equal(y, ref.to(torch.bfloat16))
        if name == "empty":
            assert torch.equal(y, plain)
        if name == "whole":
            assert torch.equal(y, plain.flip(0))
    # the mix mode in the block is ignored by a launch that was told not to mix
    assert torch.equal(run(ops, u8, li, lo, ho, block(B, mode=1, lam=0.3), mix=False), plain)


# ------------------------------------------------------------------------------------------ 3. erase, given values
def erase_records(hi):
    q = hi // 8
    return {(0, 0): (q, q, 3 * q, 2 * q, 0.5, -1.25, 2.0),                                        # one box
            (1, 0): (2 * q, q, 3 * q, 3 * q, -0.75, 0.25, 1.5), (1, 1): (3 * q, 2 * q, 4 * q, 2 * q, 1.0, -2.0, 0.125),   # two, overlapping: the later wins
            (2, 1): (0, 0, q, hi - 1, 0.3, 0.6, -0.9),                                           # touching two borders, first slot empty
            (4, 0): (hi - q, hi - 2 * q, q, 2 * q, -0.1, 0.2, 0.4), (4, 1): (q, q, 2, 2, 3.0, 3.0, 3.0),     # the far corner; two apart
            (6, 0): (q + 1, q + 3, 5 * q, 4 * q, 1.75, -0.5, 0.0)}                                # over the CutMix box below; 3 and 5: none


@pytest.mark.parametrize("li,lo,hi,ho", CASES, ids=IDS)
def test_erase_const_and_rand(ops, li, lo, hi, ho):
    u8 = batch(hi, 2)
    recs = erase_records(hi)
    q = hi // 8
    cut = (2 * q, 5 * q, q, 6 * q)
    for mode, bx in ((0, (0, 0, 0, 0)), (2, cut)):
        base = run(ops, u8, li, lo, ho, block(B, mode=mode, box=bx), mix=True)
        for em in ("const", "rand"):
            blk = block(B, R=2, mode=mode, box=bx, recs=recs)
            y = run(ops, u8, li, lo, ho, blk, mix=True, n_boxes=2, erase_mode=em)
            ref = reference(u8, ho, mode, box=bx, recs=recs, R=2, const=(em == "const"))
            r = ratio(y, ref)
            print("erase %s mix %d %s %s %d->%d: %.4f" % (em, mode, li, lo, hi, ho, r))
            assert r <= 1.01
            if hi == ho:
                assert torch.equal(y, ref.to(torch.bfloat16))
            for b in (3, 5):                                   # images without a box: what the launch gives without erasing
                assert torch.equal(y[b], base[b])
            assert not torch.equal(y[0], base[0])


# ------------------------------------------------------------------------------------------ 4. erase, per-pixel noise
@pytest.mark.parametrize("li,lo", [("nchw", "s2d16"), ("nhwc", "s2d16"), ("nchw", "nhwc"), ("nhwc", "nhwc")])
def test_erase_pixel_noise(ops, li, lo):
    """the bounds on the moments are > 6 standard errors at this sample size (1.4e5 pixels: 0.0027 for a mean or a correlation): they
    catch a broken generator -- a constant, a repeated stream, a channel copied to another -- not a slightly biased one"""
    hi = 224
    u8 = batch(hi, 3)
    recs = {(b, 0): (10 + 7 * b, 40 - 5 * b, 140, 140) for b in range(B)}
    plain = run(ops, u8, li, lo, hi)
    y = run(ops, u8, li, lo, hi, block(B, R=1, seed=1234, recs=recs), n_boxes=1, erase_mode="pixel")
    inside = torch.zeros(B, hi, hi, dtype=torch.bool)
    for (b, _), (t, l, h, w) in recs.items():
        inside[b, t:t + h, l:l + w] = True
    m3 = inside[:, None].expand(B, 3, hi, hi)
    assert torch.equal(y[~m3], plain[~m3])
    z = y.float().permute(1, 0, 2, 3)[:, inside]                # [3, pixels]
    assert z.shape[1] * 3 >= 100000 and bool(torch.isfinite(z).all())
    print("pixel noise %s %s: mean %.4f std %.4f" % (li, lo, float(z.mean()), float(z.std())))
    assert abs(float(z.mean())) < 0.02 and abs(float(z.std()) - 1.0) < 0.02
    c = torch.corrcoef(z)
    print("  channel correlations %.4f %.4f %.4f" % (float(c[0, 1]), float(c[0, 2]), float(c[1, 2])))
    assert max(abs(float(c[0, 1])), abs(float(c[0, 2])), abs(float(c[1, 2]))) < 0.02
    pair = inside[:, :, :-1] & inside[:, :, 1:]                 # horizontal neighbours, both erased
    yf = y.float()
    for ch in range(3):
        h = torch.corrcoef(torch.stack([yf[:, ch, :, :-1][pair], yf[:, ch, :, 1:][pair]]))[0, 1]
        print("  neighbour correlation, channel %d: %.4f" % (ch, float(h)))
        assert abs(float(h)) < 0.02
    again = run(ops, u8, li, lo, hi, block(B, R=1, seed=1234, recs=recs), n_boxes=1, erase_mode="pixel")
    other = run(ops, u8, li, lo, hi, block(B, R=1, seed=1235, recs=recs), n_boxes=1, erase_mode="pixel")
    assert torch.equal(again, y) and not torch.equal(other, y)
    assert torch.equal(other[~m3], plain[~m3])
    # through a resize: an output pixel whose four taps lie outside every box does not know that anything was erased
    for ho in (160, 96):
        plain_r = run(ops, u8, li, lo, ho)
        y_r = run(ops, u8, li, lo, ho, block(B, R=1, seed=1234, recs=recs), n_boxes=1, erase_mode="pixel")
        src = torch.clamp((torch.arange(ho, dtype=torch.float32) + 0.5) * (hi / ho) - 0.5, min=0)
        i0 = src.floor().long()
        i1 = torch.clamp(i0 + 1, max=hi - 1)
        touched = torch.zeros(B, ho, ho, dtype=torch.bool)
        for ya in (i0, i1):
            for xa in (i0, i1):
                touched |= inside[:, ya][:, :, xa]
        free = ~touched[:, None].expand(B, 3, ho, ho)
        assert bool(free.any()) and torch.equal(y_r[free], plain_r[free])
        assert bool(torch.isfinite(y_r.float()).all()) and not torch.equal(y_r, plain_r)


# ------------------------------------------------------------------------------------------ 5. error codes
def test_error_codes(ops):
    from autoprog_amd._lib import AutoProgHipError
    u8 = batch(64)
    with pytest.raises(AutoProgHipError, match="code -1"):      # AP_ERR_SHAPE: the space-to-depth layout holds 2 x 2 blocks
        ops.input_prep(dev(u8), 63, out="s2d16", table=dev(table()))
    assert tuple(ops.input_prep(dev(u8), 63, out="nhwc", table=dev(table())).shape) == (B, 63, 63, 3)
    with pytest.raises(AutoProgHipError, match="code -1"):      # nine boxes per image
        ops.input_prep(dev(u8), 64, table=dev(table()), params=dev(block(B, R=9)), n_boxes=9)
    for rec in ((60, 0, 5, 5), (0, 60, 5, 5), (-1, 0, 5, 5), (0, 0, 65, 1), (0, 0, -3, 4), (0, 0, 4, 0)):
        blk = block(B, R=1, recs={(6, 0): rec})
        with pytest.raises(AutoProgHipError, match="code -1"):  # a record that reaches outside the image
            ops.input_prep(dev(u8), 64, table=dev(table()), params=dev(blk), n_boxes=1, host_block=blk)
    blk = block(B, R=1, recs={(6, 0): (59, 59, 5, 5)})          # the last rows and columns: inside
    ops.input_prep(dev(u8), 64, table=dev(table()), params=dev(blk), n_boxes=1, host_block=blk)
    empty = ops.input_prep(torch.empty(0, 3, 64, 64, dtype=torch.uint8, device="cuda"), 64, table=dev(table()))       # AP_OK, no launch
    assert tuple(empty.shape) == (0, 32, 32, 16)
    torch.cuda.synchronize()


# =========================================================================================== model level
def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _step(model, loss_fn, x, target, seed):
    """one training step (forward, loss, backward) from the same state and the same host / device random streams"""
    np.random.seed(seed)
    torch.manual_seed(seed)
    model.zero_grad(set_to_none=True)
    out = model(x)
    loss = loss_fn(out, target)
    loss.backward()
    first = out[0] if isinstance(out, tuple) else out
    return loss.detach().clone(), first.detach().clone(), _grads(model)


def _same(a, b):
    (la, oa, ga), (lb, ob, gb) = a, b
    assert torch.equal(oa, ob) and torch.equal(la, lb), (float(la), float(lb))
    assert ga.keys() == gb.keys() and all(torch.equal(ga[k], gb[k]) for k in ga), [k for k in ga if not torch.equal(ga[k], gb[k])][:5]


@pytest.fixture
def deterministic():
    from autoprog_amd import ops as _ops
    old = _ops.deterministic
    _ops.deterministic = True
    yield
    _ops.deterministic = old


def _bn_state(model):
    return {k: v.clone() for k, v in model.state_dict().items()}


def test_volo_step_fed_uint8_is_the_step_fed_the_normalised_tensor(deterministic):
    """the configuration of __graft_entry__.smoke(): one training step fed prep(u8), mix and erase off, is bit for bit the step fed the
    normalised fp32 tensor -- at the model's own size and through the stage resize; with `const` erasing on (no resize) it is bit for bit
    the step fed the tensor prepared on the CPU"""
    from autoprog_amd.data import DeviceBatchPrep
    from autoprog_amd.loss import TokenLabelCrossEntropy
    from autoprog_amd.models import create_model
    torch.manual_seed(0)
    classes, n_img, r = 32, 4, 64
    model = create_model("model_variant", variant="volo_h4_l6", num_classes=classes, img_size=r, stem_hidden_dim=64).cuda().train()
    loss_fn = TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=classes)
    u8 = torch.randint(0, 256, (n_img, 3, r, r), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    state = _bn_state(model)
    for size in (r, 32):
        model.patch_embed.resize_to = None if size == r else size
        n = (size // 16) ** 2
        target = torch.softmax(torch.randn(n_img, classes, 2 + n, generator=torch.Generator().manual_seed(size)), dim=1).cuda()
        prep = DeviceBatchPrep(MEAN, STD, seed=1)
        a = _step(model, loss_fn, dev(normalised(u8)), target, 7)
        model.load_state_dict(state)                            # (the BatchNorm running statistics moved)
        b = _step(model, loss_fn, prep.prep(dev(u8)), target, 7)
        model.load_state_dict(state)
        _same(a, b)
    model.patch_embed.resize_to = None
    prep = DeviceBatchPrep(MEAN, STD, re_prob=1.0, re_mode="const", re_count=2, seed=2)
    batch_ = prep.prep(dev(u8))
    recs = {}
    for b_, top, left, h, w in prep.last["boxes"]:
        recs[(b_, sum(1 for k in recs if k[0] == b_))] = (top, left, h, w)
    assert len(recs) == 2 * n_img
    x_cpu = reference(u8, r, recs=recs, R=2, const=True)
    target = torch.softmax(torch.randn(n_img, classes, 2 + 16, generator=torch.Generator().manual_seed(3)), dim=1).cuda()
    a = _step(model, loss_fn, dev(x_cpu), target, 9)
    model.load_state_dict(state)
    b = _step(model, loss_fn, batch_, target, 9)
    _same(a, b)


def test_deit_step_fed_uint8(deterministic):
    """deit_tiny at depth 4 (BASELINE.json configs[0]): plain, the uint8 step is the fp32 step bit for bit; with CutMix and `const` erasing
    the logits equal those of the step fed the CPU-prepared tensor bit for bit (the prepared input is bit-exact), and the loss on
    (labels, lam) agrees with the loss on timm's dense mixup target within the bounds of the sparse-vs-dense loss test"""
    from autoprog_amd.data import DeviceBatchPrep, MIX_CUTMIX
    from autoprog_amd.loss import SoftTargetCrossEntropy
    from autoprog_amd.models import create_model
    torch.manual_seed(0)
    model = create_model("model_variant", variant="deit_h3_l4").cuda().train()
    n_img = 5
    u8 = torch.randint(0, 256, (n_img, 3, 224, 224), dtype=torch.uint8, generator=torch.Generator().manual_seed(6))
    labels = torch.tensor([3, 999, 17, 17, 250]).cuda()
    loss_fn = SoftTargetCrossEntropy()
    prep = DeviceBatchPrep(MEAN, STD, seed=1)
    batch_ = prep.prep(dev(u8))
    tgt = batch_.target(labels)
    assert tgt.lam == 1.0
    _same(_step(model, loss_fn, dev(normalised(u8)), tgt, 7), _step(model, loss_fn, batch_, tgt, 7))
    prep = DeviceBatchPrep(MEAN, STD, cutmix_alpha=1.0, re_prob=1.0, re_mode="const", seed=4)
    batch_ = prep.prep(dev(u8))
    d = prep.last
    assert d["mode"] == MIX_CUTMIX and 0.0 < d["lam"] < 1.0 and len(d["boxes"]) == n_img
    recs = {(b_, 0): (top, left, h, w) for b_, top, left, h, w in d["boxes"]}
    x_cpu = reference(u8, 224, 2, box=d["box"], recs=recs, R=1, const=True)
    tgt = batch_.target(labels)
    la, oa, ga = _step(model, loss_fn, dev(x_cpu), tgt.dense(1000), 8)
    lb, ob, gb = _step(model, loss_fn, batch_, tgt, 8)
    assert torch.equal(oa, ob)
    print("deit cutmix lam %.4f: loss dense %.7f sparse %.7f" % (d["lam"], float(la), float(lb)))
    assert abs(float(la) - float(lb)) <= 1e-6 * abs(float(la))
    worst = max(float((ga[k].float() - gb[k].float()).norm() / (ga[k].float().norm() + 1e-30)) for k in ga)
    print("  worst relative gradient difference %.3e" % worst)
    assert worst < 2e-3


@pytest.mark.parametrize("lam,labels", [(1.0, [1, 5, 9, 200, 999, 0]), (0.37, [1, 5, 9, 200, 999, 0]), (0.37, [4, 7, 33, 33, 7, 4])])
def test_soft_target_ce_on_labels_and_lam_equals_the_dense_target(lam, labels):
    """SoftTargetCrossEntropy on MixedLabelTarget (the sparse kernel: one pair per image, smoothing, batch mix) against the same module on
    timm's dense mixup target: loss to 1e-6 relative, logit gradient to 2e-3 in relative norm (the bounds of
    test_gpu_loss.py::test_sparse_token_label_ce_equals_dense_on_the_densified_target); the third case pairs equal labels"""
    from autoprog_amd.data import MixedLabelTarget
    from autoprog_amd.loss import SoftTargetCrossEntropy
    C = 1000
    x = (torch.randn(len(labels), C, generator=torch.Generator().manual_seed(3)) * 2).cuda().to(torch.bfloat16)
    tgt = MixedLabelTarget(torch.tensor(labels).cuda(), lam, smoothing=0.1, num_classes=C)
    dense = tgt.dense()
    assert float((dense.sum(1) - 1).abs().max()) < 1e-6
    outs = []
    for t in (dense, tgt):
        xi = x.clone().requires_grad_(True)
        loss = SoftTargetCrossEntropy()(xi, t)
        loss.backward()
        outs.append((float(loss.detach()), xi.grad.float().cpu()))
    (l0, g0), (l1, g1) = outs
    ref = float((-(dense.double().cpu() * torch.log_softmax(x.double().cpu(), -1)).sum(-1)).mean())
    print("lam %.2f: dense %.7f labels %.7f fp64 %.7f, gradient %.3e" % (lam, l0, l1, ref, float((g0 - g1).norm() / g0.norm())))
    assert abs(l0 - l1) <= 1e-6 * abs(l0), (l0, l1)
    assert float((g0 - g1).norm() / g0.norm()) < 2e-3
    assert abs(l1 - ref) < 2e-5 * abs(ref)


def _graph_setup():
    from autoprog_amd.data import DeviceBatchPrep
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import SoftTargetCrossEntropy
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import FlatAdamWEma
    torch.manual_seed(0)
    model = create_model("model_variant", variant="deit_h3_l2", num_classes=16, img_size=64).cuda().train()
    red = GradientBucketReducer(list(model.parameters()), world_size=1, defer_mean=True)
    red.install_sink(model)
    opt = FlatAdamWEma(model, red, lr=2e-3, weight_decay=0.05, ema_decays=[0.9])
    prep = DeviceBatchPrep(MEAN, STD, mixup_alpha=0.8, cutmix_alpha=1.0, re_prob=0.5, re_mode="pixel", num_classes=16, seed=21)
    g = torch.Generator().manual_seed(2)
    batches = [(torch.randint(0, 256, (6, 3, 64, 64), dtype=torch.uint8, generator=g).cuda(), torch.randint(0, 16, (6,), generator=g).cuda())
               for _ in range(3)]
    return model, red, opt, SoftTargetCrossEntropy(), prep, batches


def test_graphed_step_on_prepared_batches_is_the_eager_step(deterministic):
    """three replays with three different draws (Mixup or CutMix, lam, erase boxes, noise key -- all from the parameter block in device
    memory -- and three different uint8 batches) equal the three eager steps with the same seeds bit for bit: losses and parameters"""
    from autoprog_amd.graph import GraphedStep
    model, red, opt, loss_fn, prep, batches = _graph_setup()
    try:
        le, draws_e = [], []
        for u8, labels in batches:
            red.zero_grad()
            pb = prep.prep(u8)
            draws_e.append((prep.last["mode"], prep.last["lam"]))
            loss = loss_fn(model(pb), pb.target(labels))
            loss.backward()
            red.finish()
            opt.step()
            le.append(float(loss.detach()))
        pe = opt.p.clone()
    finally:
        red.remove()
    model, red, opt, loss_fn, prep, batches = _graph_setup()
    try:
        from autoprog_amd.data import DeviceBatchPrep
        scratch = DeviceBatchPrep(MEAN, STD, mixup_alpha=0.8, cutmix_alpha=1.0, re_prob=0.5, re_mode="pixel", num_classes=16, seed=99)
        pb0 = scratch.prep(batches[0][0])                       # the capture's own batch and draw: any
        gs = GraphedStep(model, loss_fn, red, opt, pb0, pb0.target(batches[0][1]))
        p0, m0, v0 = opt.p.clone(), opt.m.clone(), opt.v.clone()
        ema0 = [e.clone() for e in opt.ema]
        gs.capture(warmup=2)
        with torch.no_grad():
            opt.p.copy_(p0); opt.m.copy_(m0); opt.v.copy_(v0)
            for e, e0 in zip(opt.ema, ema0):
                e.copy_(e0)
        opt.step_count = 0
        opt.resync()
        lg, draws_g = [], []
        for u8, labels in batches:
            pb = prep.prep(u8)
            draws_g.append((prep.last["mode"], prep.last["lam"]))
            lg.append(float(gs.step(pb, pb.target(labels)).detach()))
        print("eager :", le, draws_e)
        print("graph :", lg, draws_g)
        assert draws_e == draws_g and len({d[0] for d in draws_e}) >= 2
        assert le == lg
        assert torch.equal(pe, opt.p)
    finally:
        red.remove()


def test_driver_sets_the_stage_erase_probability_and_prepares_uint8_batches():
    """a two-stage schedule (no search): batch_prep.re_prob is the stage's `re` entry from the first batch of each stage on, uint8 batches
    reach the patch embedding as PreparedBatch (resized to the stage's r there), and integer labels become (labels, lam) targets"""
    from autoprog_amd.data import DeviceBatchPrep, MixedLabelTarget, PreparedBatch
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import TokenLabelCrossEntropy
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import FlatAdamWEma
    from autoprog_amd.prog.driver import AutoProgDriver
    torch.manual_seed(0)
    model = create_model("model_variant", variant="volo_h2_l6", num_classes=16, img_size=96, stem_hidden_dim=64).cuda().train()
    red = GradientBucketReducer(list(model.parameters()), world_size=1, defer_mean=True)
    red.install_sink(model)
    opt = FlatAdamWEma(model, red, lr=1e-3, weight_decay=0.05, ema_decays=[0.9])
    prep = DeviceBatchPrep(MEAN, STD, re_prob=0.9, re_mode="pixel", num_classes=16, seed=5)
    loss_fn = TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=16)
    g = torch.Generator().manual_seed(1)
    seen = []

    def get_batch(r):
        seen.append(prep.re_prob)
        u8 = torch.randint(0, 256, (8, 3, 96, 96), dtype=torch.uint8, generator=g).cuda()
        return u8, torch.softmax(torch.randn(8, 16, 2 + (r // 16) ** 2, generator=g) * 2, dim=1).cuda()

    real_forward = model.patch_embed.forward
    kinds = []
    model.patch_embed.forward = lambda x: (kinds.append(type(x)), real_forward(x))[1]
    drv = AutoProgDriver(model, loss_fn, opt, red, get_batch, r_list=[64, 96], l_list=[3, 6], dp_list=[0.0, 0.0], grow_epochs=[0, 1],
                         steps_per_epoch=3, auto_grow=False, batch_prep=prep, re_list=[0.0, 0.25])
    try:
        np.random.seed(3)
        hist = drv.run(2)
    finally:
        red.remove()
    assert seen == [0.0] * 3 + [0.25] * 3 and prep.re_prob == 0.25
    assert len(kinds) == 6 and all(k is PreparedBatch for k in kinds)
    assert all(np.isfinite(h["loss"]) for h in hist)
    # integer labels beside a uint8 batch become the batch's (labels, lam) target; anything that is not uint8 passes untouched
    drv._raw_get_batch = lambda r: (torch.zeros(4, 3, 32, 32, dtype=torch.uint8).cuda(), torch.tensor([1, 2, 3, 4]).cuda())
    images, target = drv.get_batch(32)
    assert isinstance(images, PreparedBatch) and isinstance(target, MixedLabelTarget) and target.lam == 1.0
    x = torch.zeros(4, 3, 32, 32).cuda()
    drv._raw_get_batch = lambda r: (x, x)
    assert drv.get_batch(32)[0] is x
    with pytest.raises(ValueError):
        AutoProgDriver(model, loss_fn, opt, red, get_batch, r_list=[64, 96], l_list=[3, 6], dp_list=[0.0, 0.0], grow_epochs=[0, 1],
                       steps_per_epoch=3, re_list=[0.0, 0.25])
