"""DeiT's distillation loss from a teacher: ap_distill_fwd_bwd (csrc/distill.hip) through the C ABI -- compact and behind guard bands, per
16 x 8 tile against fp64 on the same bf16 operands --, the tie rule of the hard label, a teacher that equals the student, the argument
paths, then loss.DistillationLoss on a distilled DeiT against the oracle, on a CutMix batch and under the driver (eager steps).

Bounds are the ones the 1000-class and wide CE tests hold: row losses 1e-4 relative as one vector, gradients 1e-2 whole and 2e-2 per tile.
The fp64 reference is the formula of include/autoprog_hip.h written with torch on the CPU; the hard label comes from a stable descending
sort (argmax's order among equal values is unspecified).

The kernel is selected by round_up(C, 8), not by the leading dimensions, so the boundaries of the shapes below are csrc/softce.hip's own
(1024 / 1025, 4096 / 4104) and both runs of a case take the same kernel.  One departure: at C = 65 536 a leading dimension wider than the
row is refused (AP_ERR_UNSUPPORTED above 65 536), so the guarded run of that shape keeps ld = 65 536 for both operands -- NaN guard rows
around the operands and guard bands around both outputs, no padding columns."""
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as R
from tests._tilecheck import assert_tiled, nan_padded, rel, round_up
from tests.test_gpu_localized import TOL_BF16, P, case, dev, gbuf, gflat, ops, same_bits, stream  # noqa: F401  (ops, case: fixtures)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ======================================================================================================================== reference
def distill_ref(xs, xt, mode, T, gs):
    """fp64 (row losses, d(gs * sum of row losses) / d student) of bf16 operands [M, C]"""
    a, b = xs.double().requires_grad_(True), xt.double()
    if mode == 0:
        ls, lt = torch.log_softmax(a / T, -1), torch.log_softmax(b / T, -1)
        rows = T * T * (lt.exp() * (lt - ls)).sum(-1)
    else:
        cstar = torch.sort(b, dim=-1, descending=True, stable=True).indices[:, :1]
        rows = torch.logsumexp(a, -1) - a.gather(1, cstar)[:, 0]
    (rows.sum() * gs).backward()
    return rows.detach(), a.grad


_CASES = {}


class DistillCase:
    """independent seeded randn * 2 student and teacher logits rounded to bf16, and their fp64 results; built once per (M, C, mode, T)"""

    def __init__(self, M, C, mode, T):
        self.M, self.C, self.mode, self.T = M, C, mode, T
        gen = torch.Generator().manual_seed(M * 31 + C)
        self.xs = (torch.randn(M, C, generator=gen) * 2).to(BF16)
        self.xt = (torch.randn(M, C, generator=gen) * 2).to(BF16)
        self.gs = 0.5 / M
        self.rows_ref, self.grad_ref = distill_ref(self.xs, self.xt, mode, T, self.gs)

    @classmethod
    def get(cls, M, C, mode, T):
        key = (M, C, mode, T)
        if key not in _CASES:
            _CASES[key] = cls(M, C, mode, T)
        return _CASES[key]

    def check(self, case, loss, dl, what):
        e = rel(loss, self.rows_ref)
        rep = assert_tiled(dl[:, :self.C], self.grad_ref, TOL_BF16, "%s %s dstudent" % (case, what))
        print("DISTILL %s %s | row loss rel %.3e | dstudent whole %.3e worst tile %.3e" % (case, what, e, rep.whole, rep.worst))
        assert e < 1e-4, "%s %s: row losses off by %.3e" % (case, what, e)
        assert bool((dl[:, self.C:].view(torch.int16) == 0).all()), "%s %s: columns C .. ld_s-1 of dstudent are not all zero bits" % (case, what)


def launch(lib, xs, xt, mode, T, gs, guard):
    """-> (row_loss, dstudent [M, ld_s], guards).  guard: NaN-padded operands with ld_s = round_up(C, 8) + 8 and ld_t = round_up(C, 8) + 16
    (ld = C at 65 536 columns) and guard bands around both outputs; else compact, ld = round_up(C, 8), zero padding"""
    M, C = xs.shape
    c8 = round_up(C, 8)
    if guard:
        ld_s, ld_t = (c8 + 8, c8 + 16) if c8 + 16 <= 65536 else (c8, c8)
        s, t = nan_padded(xs, ld_s, device="cuda"), nan_padded(xt, ld_t, device="cuda")
        loss, g0 = gflat(M, what="row_loss")
        dl, g1 = gbuf(M, ld_s, ld_s, what="dstudent")
        guards = [g0, g1]
    else:
        ld_s = ld_t = c8
        s, t = dev(F.pad(xs, (0, c8 - C))), dev(F.pad(xt, (0, c8 - C)))
        loss, dl, guards = torch.empty(M, device="cuda"), torch.empty(M, ld_s, dtype=BF16, device="cuda"), []
    rc = lib.ap_distill_fwd_bwd(P(s), ld_s, P(t), ld_t, C, mode, 1.0 / T, P(loss), P(dl), gs, M, stream())
    assert rc == 0, "ap_distill_fwd_bwd at ld_s = %d, ld_t = %d: code %d" % (ld_s, ld_t, rc)
    torch.cuda.synchronize()
    return loss, dl, guards


# ======================================================================================================================== 1. the kernel
# (1, 8) .. (7, 1024): both rows in a wave's registers (37 rows: five workgroups, the last with five rows of eight and a wave with one row of
# two); (3, 1025) .. (5, 4096): LDS rows, one wave per row; (2, 4104) ..: four waves per row; soft mode stages both rows up to (1, 40704) and
# only the student's from (1, 40712) on -- there the teacher row, NaN-padded with its own leading dimension, is read from global memory in all three walks
SHAPES = [(1, 8), (5, 1000), (37, 1000), (7, 1024), (3, 1025), (37, 1100), (5, 4096), (2, 4104), (2, 21843), (1, 40704), (1, 40712), (1, 65536)]
# the last chunk of a row one chunk either side of a batch of the staging walk (256 chunks for a team of one wave, 1024 for a team of four)
SHAPES += [(3, 2040), (3, 2041), (3, 2049), (3, 8185), (3, 8193)]
MODES = [("soft", 0, 1.0), ("soft", 0, 3.0), ("hard", 1, 1.0)]


@pytest.mark.parametrize("name,mode,T", MODES, ids=["soft-T1", "soft-T3", "hard"])
@pytest.mark.parametrize("M,C", SHAPES)
def test_distill_kernel_localized(ops, case, M, C, name, mode, T):
    """compact and guarded runs bit-identical, guards untouched, row losses 1e-4 against fp64, every 16 x 8 tile of dstudent inside the bf16
    bound, columns C .. ld_s-1 zero bits"""
    from autoprog_amd._lib import lib
    c = DistillCase.get(M, C, mode, T)
    loss_c, dl_c, _ = launch(lib, c.xs, c.xt, mode, T, c.gs, False)
    loss_g, dl_g, guards = launch(lib, c.xs, c.xt, mode, T, c.gs, True)
    for g in guards:
        g.check(pad="untouched")
    assert torch.equal(loss_c, loss_g), "%s: row losses of the guarded run differ from the compact run" % case
    same_bits(case, "dstudent", dl_c[:, :C], dl_g[:, :C], c.grad_ref, TOL_BF16)
    c.check(case, loss_c, dl_c, "compact")
    c.check(case, loss_g, dl_g, "guarded")


# ======================================================================================================================== 2. ties
TIES = [(1000, [(8, 9), (100, 612), (0, 999), (511, 512)]),
        (1100, [(1023, 1024), (0, 1099), (40, 552)]),
        (4104, [(3, 4100), (0, 4103), (4095, 4096)])]


@pytest.mark.parametrize("C,pairs", TIES, ids=["C1000", "C1100", "C4104"])
def test_hard_label_ties_resolve_to_the_smaller_class(ops, case, C, pairs):
    """the teacher's maximum planted twice per row: adjacent columns of one 16-byte chunk, 512 apart, across 1023 / 1024, column 0 and C - 1,
    the first and the last staged chunk.  The row loss is lse - x_s[smaller column] and the -grad_scale step sits there; the student's logits
    at the two columns are 3 and -1, so the two choices cannot be confused.  One more row ties -0.0 with +0.0 as its maximum."""
    from autoprog_amd._lib import lib
    M, gs = len(pairs) + 1, 0.5
    gen = torch.Generator().manual_seed(C)
    xs = (torch.randn(M, C, generator=gen) * 2).to(BF16)
    xt = (torch.randn(M, C, generator=gen) * 2).to(BF16)
    cols = list(pairs) + [(5, C - 3)]
    for r, (c1, c2) in enumerate(pairs):
        xt[r, c1] = xt[r, c2] = 20.0
    xt[M - 1] = -xt[M - 1].abs() - 0.5                     # every logit negative, then +0.0 at the larger column and -0.0 at the smaller
    xt[M - 1, 5], xt[M - 1, C - 3] = -0.0, 0.0
    for r, (c1, c2) in enumerate(cols):
        xs[r, c1], xs[r, c2] = 3.0, -1.0
    rows_ref, grad_ref = distill_ref(xs, xt, 1, 1.0, gs)
    lse = torch.logsumexp(xs.double(), -1)
    for r, (c1, c2) in enumerate(cols):
        assert abs(float(rows_ref[r]) - (float(lse[r]) - 3.0)) < 1e-9          # the reference itself picked the smaller column
    for guard in (False, True):
        loss, dl, guards = launch(lib, xs, xt, 1, 1.0, gs, guard)
        for g in guards:
            g.check(pad="untouched")
        e = rel(loss, rows_ref)
        rep = assert_tiled(dl[:, :C], grad_ref, TOL_BF16, "%s dstudent" % case)
        print("DISTILL %s guard %s | row loss rel %.3e | dstudent whole %.3e worst tile %.3e" % (case, guard, e, rep.whole, rep.worst))
        assert e < 1e-4
        step = dl[:, :C].double().cpu() - gs * torch.softmax(xs.double(), -1)
        for r, (c1, c2) in enumerate(cols):
            assert abs(float(loss[r]) - (float(lse[r]) - 3.0)) < 1e-4 * abs(float(lse[r]) - 3.0), (r, c1, c2, float(loss[r]))
            assert abs(float(step[r, c1]) + gs) < 0.02 * gs and abs(float(step[r, c2])) < 0.02 * gs, (r, c1, c2, float(step[r, c1]), float(step[r, c2]))


# ======================================================================================================================== 3. self-teacher
@pytest.mark.parametrize("T", [1.0, 3.0])
@pytest.mark.parametrize("M,C", [(5, 1000), (3, 1025)])
def test_teacher_equal_to_student_gives_zero(ops, case, M, C, T):
    """fp64 gives zero loss and zero gradient: |row_loss| <= 1e-5 T^2 and |dstudent| <= 1e-5 T grad_scale (ten times the ~1e-6 relative
    accuracy of an fp32 softmax, whose terms are at most 1)"""
    from autoprog_amd._lib import lib
    xs = (torch.randn(M, C, generator=torch.Generator().manual_seed(C + M)) * 2).to(BF16)
    gs = 0.5
    loss, dl, guards = launch(lib, xs, xs.clone(), 0, T, gs, True)
    for g in guards:
        g.check(pad="untouched")
    worst_l, worst_g = float(loss.abs().max()), float(dl[:, :C].float().abs().max())
    print("DISTILL %s | max |row_loss| %.3e (bound %.1e) | max |dstudent| %.3e (bound %.1e)" % (case, worst_l, 1e-5 * T * T, worst_g, 1e-5 * T * gs))
    assert worst_l <= 1e-5 * T * T and worst_g <= 1e-5 * T * gs
    assert bool((dl[:, C:].view(torch.int16) == 0).all())


# ======================================================================================================================== 4. argument paths
def test_two_runs_are_bit_identical(ops):
    from autoprog_amd._lib import lib
    for (M, C, mode, T) in [(37, 1000, 0, 3.0), (37, 1100, 0, 1.0), (2, 21843, 0, 3.0), (2, 21843, 1, 1.0)]:
        c = DistillCase.get(M, C, mode, T)
        l0, d0, _ = launch(lib, c.xs, c.xt, mode, T, c.gs, False)
        l1, d1, _ = launch(lib, c.xs, c.xt, mode, T, c.gs, False)
        assert torch.equal(l0, l1) and torch.equal(d0.view(torch.int16), d1.view(torch.int16)), (M, C, mode)


def test_error_codes(ops):
    from autoprog_amd._lib import AutoProgHipError, lib
    SENT = 0x7FA5
    x = torch.zeros(4, 32, dtype=BF16, device="cuda")
    loss = torch.full((4,), -7.0, device="cuda")
    dl = torch.full((4, 32), SENT, dtype=torch.int16, device="cuda")

    def call(s=None, t=None, ld_s=32, ld_t=32, C=16, mode=0, inv_temp=1.0, M=4, lp=None, dp=None):
        return lib.ap_distill_fwd_bwd(P(x) if s is None else s, ld_s, P(x) if t is None else t, ld_t, C, mode, inv_temp,
                                      P(loss) if lp is None else lp, P(dl) if dp is None else dp, 1.0, M, stream())
    assert call(ld_s=12) == -1 and call(ld_t=12) == -1                                    # AP_ERR_SHAPE: ld % 8
    assert call(C=0) == -1 and call(ld_s=8) == -1 and call(ld_t=8) == -1                  # C outside 1 .. min(ld_s, ld_t)
    assert call(s=P(x) + 2) == -1 and call(t=P(x) + 2) == -1 and call(dp=P(dl) + 2) == -1  # 16-byte alignment of the three matrices
    assert call(inv_temp=0.0) == -1 and call(inv_temp=-1.0) == -1 and call(inv_temp=float("inf")) == -1 and call(inv_temp=float("nan")) == -1
    assert call(mode=2) == -1 and call(M=-1) == -1
    assert call(ld_s=65544) == -2 and call(ld_t=65544) == -2                              # AP_ERR_UNSUPPORTED
    assert call(s=0) == -4 and call(t=0) == -4 and call(lp=0) == -4 and call(dp=0) == -4  # AP_ERR_NULL
    assert call(M=0) == 0 and call(s=0, t=0, lp=0, dp=0, M=0) == 0                        # no rows: success without a launch
    torch.cuda.synchronize()
    assert bool((dl == SENT).all()) and bool((loss == -7.0).all()), "a refused call wrote something"
    assert call(mode=1, inv_temp=0.0) == 0                                                # hard mode ignores inv_temp
    torch.cuda.synchronize()
    assert bool((dl[:, 16:] == 0).all()) and abs(float(loss[0]) - float(np.log(16.0))) < 1e-5
    with pytest.raises(AutoProgHipError):
        ops.distill_fwd_bwd(x.cpu(), 16, x, 0, 1.0, 1.0)
    with pytest.raises(AutoProgHipError):
        ops.distill_fwd_bwd(x, 16, x.cpu(), 0, 1.0, 1.0)
    with pytest.raises(AutoProgHipError):
        ops.distill_fwd_bwd(x.float(), 16, x, 0, 1.0, 1.0)
    rows, d = ops.distill_fwd_bwd(x[:, :20], 20, x[:, :24], 1, 1.0, 0.25)                 # padded views pass as they are
    assert tuple(rows.shape) == (4,) and tuple(d.shape) == (4, 32)


# ======================================================================================================================== 5. on a network
def _loss_ref(y, yd, labels, teacher, kind, alpha, tau, soft_norm, smoothing):
    """fp64 DistillationLoss on the oracle's logits: base = smoothed CE of integer labels (or of a dense target given as `labels`)"""
    B, C = y.shape
    t = labels if labels.dim() == 2 else F.one_hot(labels, C).double() * (1.0 - smoothing) + smoothing / C
    base = R.soft_target_ce(y, t)
    if kind == "none":
        return base
    if kind == "soft":
        ls, lt = torch.log_softmax(yd / tau, -1), torch.log_softmax(teacher / tau, -1)
        distill = tau * tau * (lt.exp() * (lt - ls)).sum() / (B * C if soft_norm == "numel" else B)
    else:
        cstar = torch.sort(teacher, dim=-1, descending=True, stable=True).indices[:, 0]
        distill = F.cross_entropy(yd, cstar)
    return (1.0 - alpha) * base + alpha * distill


@pytest.fixture(scope="module")
def deit_pair(ops):
    """(student deit_tiny_distilled with 40 classes cut to two blocks, TeacherLogits over a one-block deit_tiny, images, labels)"""
    from autoprog_amd.models import create_model
    from autoprog_amd.prog.teacher import TeacherLogits
    torch.manual_seed(4)
    student = create_model("deit_tiny_distilled_patch16_224", num_classes=40).cuda().train()
    student.blocks = student.blocks[:2]
    teacher = create_model("deit_tiny_patch16_224", num_classes=40).cuda()
    teacher.blocks = teacher.blocks[:1]
    x = torch.randn(3, 3, 224, 224, device="cuda")
    labels = torch.tensor([3, 39, 17], device="cuda")
    return student, TeacherLogits(teacher, num_classes=40), x, labels


@pytest.mark.parametrize("kind,soft_norm", [("soft", "numel"), ("soft", "batchmean"), ("hard", "numel")])
def test_distillation_loss_on_a_distilled_deit(deit_pair, case, kind, soft_norm):
    """loss 2e-3 relative, every parameter gradient 6e-2 against the oracle (the bounds of test_deit_distilled_vs_oracle); the teacher's
    bf16 logits are taken from the device and fed to the fp64 formula"""
    from autoprog_amd.loss import DistillationLoss, DistillTarget, SoftTargetCrossEntropy
    student, teach, x, labels = deit_pair
    alpha, tau, smoothing = 0.5, 3.0, 0.1
    loss_fn = DistillationLoss(SoftTargetCrossEntropy(), kind, alpha=alpha, tau=tau, soft_norm=soft_norm, smoothing=smoothing)
    target = teach(x, labels, 224)
    assert isinstance(target, DistillTarget) and target.teacher_logits.dtype == BF16 and tuple(target.teacher_logits.shape) == (3, 40)
    assert not teach.teacher.training and not target.teacher_logits.requires_grad
    student.zero_grad(set_to_none=True)
    loss = loss_fn(student(x), target)
    loss.backward()
    p = {k: v.detach().double().cpu().requires_grad_(True) for k, v in student.state_dict().items()}
    yr, ydr = R.vit_forward(p, x.double().cpu(), depth=2, heads=3, distilled=True)
    lr = _loss_ref(yr, ydr, labels.cpu(), target.teacher_logits.double().cpu(), kind, alpha, tau, soft_norm, smoothing)
    lr.backward()
    errs = {n: rel(q.grad, p[n].grad) for n, q in student.named_parameters() if float(p[n].grad.norm()) > 1e-9}
    print("DISTILL %s | loss %.6f oracle %.6f | worst %.4f (%s) | head_dist.weight %.4f" % (case, float(loss.detach()), float(lr.detach()), max(errs.values()),
                                                                                           max(errs, key=errs.get), errs.get("head_dist.weight", -1.0)))
    assert abs(float(loss.detach()) - float(lr.detach())) < 2e-3 * abs(float(lr.detach()))
    assert {"dist_token", "pos_embed", "head_dist.weight", "head.weight"} <= set(errs)
    bad = {k: v for k, v in errs.items() if v > 6e-2}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]


def test_distillation_type_none_is_the_base_criterion(deit_pair):
    """"none": the base criterion on x_cls bit for bit, no gradient for head_dist; a single tensor as outputs is accepted"""
    from autoprog_amd.data import MixedLabelTarget
    from autoprog_amd.loss import DistillationLoss, SoftTargetCrossEntropy
    student, teach, x, labels = deit_pair
    target = teach(x, labels, 224)
    loss_fn = DistillationLoss(SoftTargetCrossEntropy(), "none", smoothing=0.1)
    student.zero_grad(set_to_none=True)
    y, yd = student(x)
    loss = loss_fn((y, yd), target)
    want = SoftTargetCrossEntropy()(y.detach(), MixedLabelTarget(labels, 1.0, 0.1, 40))
    assert torch.equal(loss.detach(), want)
    assert torch.equal(loss_fn(y.detach(), target), want)
    loss.backward()
    g = student.head_dist.weight.grad
    assert g is None or not bool(g.any())
    assert student.head.weight.grad is not None and bool(student.head.weight.grad.any())
    with pytest.raises(ValueError):
        DistillationLoss(SoftTargetCrossEntropy(), "hard")(y.detach(), target)


# ======================================================================================================================== 6. CutMix base
def _small_student(classes=16, depth=1, seed=0):
    from autoprog_amd.models.deit import DistilledVisionTransformer
    torch.manual_seed(seed)
    return DistilledVisionTransformer(img_size=64, patch_size=16, embed_dim=192, depth=depth, num_heads=3, mlp_ratio=4, qkv_bias=True,
                                   norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), num_classes=classes).cuda().train()


def _small_teacher(classes=16, seed=9):
    from autoprog_amd.models import create_model
    torch.manual_seed(seed)
    return create_model("model_variant", variant="deit_h3_l1", num_classes=classes, img_size=64).cuda()


@pytest.mark.parametrize("kind", ["soft", "hard"])
def test_distillation_loss_on_a_cutmix_batch(ops, case, kind):
    """a uint8 batch with CutMix forced, 64 px, one-block student and teacher with 16 classes: the DistillTarget's base is the batch's
    MixedLabelTarget, the teacher sees the mixed pixels, and the loss is within 2e-3 of the fp64 formula on the densified mixed target
    and the student's own logits"""
    from autoprog_amd.data import MIX_CUTMIX, DeviceBatchPrep, MixedLabelTarget
    from autoprog_amd.loss import DistillationLoss, SoftTargetCrossEntropy
    from autoprog_amd.prog.teacher import TeacherLogits
    student, teach = _small_student(), TeacherLogits(_small_teacher(), num_classes=16)
    prep = DeviceBatchPrep(MEAN, STD, cutmix_alpha=1.0, num_classes=16, seed=4)
    g = torch.Generator().manual_seed(6)
    pb = prep.prep(torch.randint(0, 256, (6, 3, 64, 64), dtype=torch.uint8, generator=g).cuda())
    assert prep.last["mode"] == MIX_CUTMIX and 0.0 < prep.last["lam"] < 1.0
    labels = torch.randint(0, 16, (6,), generator=g).cuda()
    target = teach(pb, labels, 64)
    assert isinstance(target.base, MixedLabelTarget) and target.base.lam == pb.lam
    with torch.no_grad():
        assert torch.equal(target.teacher_logits, teach.teacher(pb))                      # the same mixed pixels, the same logits
    loss_fn = DistillationLoss(SoftTargetCrossEntropy(), kind, alpha=0.5, tau=3.0)
    y, yd = student(pb)
    loss = float(loss_fn((y, yd), target).detach())
    ref = float(_loss_ref(y.detach().double().cpu(), yd.detach().double().cpu(), target.base.dense().double().cpu(), target.teacher_logits.double().cpu(),
                          kind, 0.5, 3.0, "numel", 0.1))
    print("DISTILL %s | lam %.4f | loss %.7f fp64 %.7f" % (case, pb.lam, loss, ref))
    assert abs(loss - ref) < 2e-3 * abs(ref)


# ======================================================================================================================== 7. the driver
def _step_setup(depth=1):
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import DistillationLoss, SoftTargetCrossEntropy
    from autoprog_amd.optim import FlatAdamWEma
    from autoprog_amd.prog.teacher import TeacherLogits
    student = _small_student(depth=depth)
    red = GradientBucketReducer(list(student.parameters()), world_size=1, defer_mean=True)
    red.install_sink(student)
    opt = FlatAdamWEma(student, red, lr=2e-3, weight_decay=0.05, ema_decays=[0.9])
    g = torch.Generator().manual_seed(2)
    batches = [(torch.randn(6, 3, 64, 64, generator=g).cuda(), torch.randint(0, 16, (6,), generator=g).cuda()) for _ in range(5)]
    return student, red, opt, DistillationLoss(SoftTargetCrossEntropy(), "soft", alpha=0.5, tau=3.0), TeacherLogits(_small_teacher(), num_classes=16), batches


def _driver_batches(seed=1):
    g = torch.Generator().manual_seed(seed)

    def get_batch(r):
        return torch.randn(6, 3, r, r, generator=g).cuda(), torch.randint(0, 16, (6,), generator=g).cuda()
    return get_batch


def test_driver_with_teacher_logits(ops, monkeypatch):
    """AutoProgDriver(teacher=TeacherLogits(...)) on an elastic four-block distilled DeiT, integer labels from get_batch, two epochs of three
    eager steps at one configuration, against a hand-written loop of the same six steps from the same state (teacher, loss, backward,
    optimizer; deterministic weight gradients): losses and weights bit for bit, and the driver's loss only ever sees DistillTargets.  With
    use_graphs the capture of a DistillTarget is refused."""
    from autoprog_amd import ops as _ops
    from autoprog_amd.graph import GraphedStep
    from autoprog_amd.loss import DistillTarget
    from autoprog_amd.prog.driver import AutoProgDriver
    monkeypatch.setattr(_ops, "deterministic", True)
    student, red, opt, dl, teach, _ = _step_setup(depth=4)
    try:
        get_batch, want = _driver_batches(), []
        student.set_sample_config(dict(layer_num=4, min_layer_num=4, max_layer_num=4))
        for _ in range(6):
            x, labels = get_batch(64)
            target = teach(x, labels, 64)
            red.zero_grad()
            loss = dl(student(x), target)
            loss.backward()
            red.finish()
            opt.step()
            want.append(float(loss.detach()))
        p_want = opt.p.clone()
    finally:
        red.remove()
    student, red, opt, dl, teach, _ = _step_setup(depth=4)
    seen, steps = [], []

    def loss_fn(outputs, target, _dl=dl):
        seen.append(type(target))
        loss = _dl(outputs, target)
        steps.append(loss.detach())
        return loss

    try:
        get_batch = _driver_batches()
        drv = AutoProgDriver(student, loss_fn, opt, red, get_batch, r_list=[64], l_list=[4], dp_list=[0.0], grow_epochs=[0], steps_per_epoch=3,
                             auto_grow=False, teacher=teach)
        hist = drv.run(2)
        losses = [float(s) for s in steps]
        print("DISTILL driver:", losses)
        print("DISTILL loop  :", want)
        assert len(losses) == 6 and all(np.isfinite(v) for v in losses) and len(set(losses)) == 6
        assert seen and all(t is DistillTarget for t in seen) and len(hist) == 2
        assert losses == want, (losses, want)
        assert torch.equal(opt.p, p_want)
        assert abs(hist[0]["loss"] - sum(want[:3]) / 3) < 1e-5 and abs(hist[1]["loss"] - sum(want[3:]) / 3) < 1e-5
        x, labels = get_batch(64)
        with pytest.raises(NotImplementedError):
            GraphedStep(student, dl, red, opt, x, teach(x, labels, 64))
    finally:
        red.remove()


# ======================================================================================================================== 8. module, 1100 classes
@pytest.mark.parametrize("kind,soft_norm", [("soft", "numel"), ("soft", "batchmean"), ("hard", "numel")])
def test_distillation_loss_module_at_1100_classes(ops, case, kind, soft_norm):
    """just past the narrow kernel, batch 5, random (x_cls, x_dist) and teacher logits, integer labels: loss 2e-5 relative and both logit
    gradients 6e-3 against fp64 (the bounds of the 21 843-class soft-target test)"""
    from autoprog_amd.loss import DistillationLoss, DistillTarget, SoftTargetCrossEntropy
    B, C, alpha, tau = 5, 1100, 0.5, 3.0
    g = torch.Generator().manual_seed(11)
    x_cls, x_dist, teacher = ((torch.randn(B, C, generator=g) * 2).to(BF16) for _ in range(3))
    labels = torch.tensor([0, 1023, 1024, C - 1, 7])
    a, b = x_cls.cuda().requires_grad_(True), x_dist.cuda().requires_grad_(True)
    loss = DistillationLoss(SoftTargetCrossEntropy(), kind, alpha=alpha, tau=tau, soft_norm=soft_norm)((a, b), DistillTarget(labels.cuda(), teacher.cuda()))
    loss.backward()
    ar, br = x_cls.double().requires_grad_(True), x_dist.double().requires_grad_(True)
    ref = _loss_ref(ar, br, labels, teacher.double(), kind, alpha, tau, soft_norm, 0.1)
    ref.backward()
    print("DISTILL %s | loss %.7f fp64 %.7f | grads cls %.3e dist %.3e" % (case, float(loss.detach()), float(ref.detach()), rel(a.grad, ar.grad), rel(b.grad, br.grad)))
    assert abs(float(loss.detach()) - float(ref.detach())) < 2e-5 * abs(float(ref.detach()))
    assert rel(a.grad, ar.grad) < 6e-3 and rel(b.grad, br.grad) < 6e-3
