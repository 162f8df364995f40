"""Host logic of DeiT's distillation loss without a GPU: what DistillationLoss, DistillTarget and TeacherLogits refuse before anything is
launched, "none" delegating to the base criterion, the graph's refusal of a DistillTarget, and the DropPath rates the driver sets on
a DeiT."""
import pytest
import torch


class _Stub(torch.nn.Module):
    """a base criterion that records what it was given"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, x, target):
        self.calls.append((x, target))
        return x.float().sum() * 0.0 + 4.25


def test_distillation_loss_constructor_refusals():
    from autoprog_amd.loss import DistillationLoss
    base = _Stub()
    for kw in (dict(distillation_type="kl"), dict(alpha=-0.1), dict(alpha=1.5), dict(tau=0.0), dict(tau=-1.0), dict(soft_norm="mean")):
        with pytest.raises(ValueError):
            DistillationLoss(base, **kw)
    loss = DistillationLoss(base)
    assert (loss.distillation_type, loss.alpha, loss.tau, loss.soft_norm, loss.smoothing) == ("hard", 0.5, 1.0, "numel", 0.1)
    for kw in (dict(alpha=0.0), dict(alpha=1.0), dict(distillation_type="soft", tau=3.0, soft_norm="batchmean"), dict(distillation_type="none")):
        DistillationLoss(base, **kw)


def test_distill_target_validates_shapes_and_casts_once():
    from autoprog_amd.data import MixedLabelTarget
    from autoprog_amd.loss import DistillTarget
    labels, logits = torch.tensor([1, 2, 3]), torch.randn(3, 10)
    t = DistillTarget(labels, logits)
    assert t.base is labels and t.teacher_logits.dtype == torch.bfloat16 and tuple(t.teacher_logits.shape) == (3, 10)
    assert torch.equal(t.teacher_logits, logits.to(torch.bfloat16)) and not t.teacher_logits.requires_grad
    bf = torch.zeros(3, 16, dtype=torch.bfloat16)[:, :10]               # a padded view is taken as it is
    assert DistillTarget(labels, bf).teacher_logits.data_ptr() == bf.data_ptr()
    mixed = MixedLabelTarget(labels, 0.4, 0.1, 10)
    assert DistillTarget(mixed, logits).base is mixed
    dense = torch.rand(3, 10)
    assert DistillTarget(dense, logits).base is dense
    for base, tl in ((labels, torch.randn(10)), (labels, torch.randn(4, 10)), (torch.tensor([1, 2]), logits), (dense[:, :9], logits),
                     (MixedLabelTarget(labels, 0.4, 0.1, 11), logits), (torch.rand(3), logits), ("labels", logits), (labels, None)):
        with pytest.raises(ValueError):
            DistillTarget(base, tl)


def test_none_delegates_to_the_base_criterion_and_soft_or_hard_need_the_pair():
    from autoprog_amd.loss import DistillationLoss, DistillTarget
    base = _Stub()
    labels = torch.tensor([1, 2, 3])
    target = DistillTarget(labels, torch.randn(3, 10))
    x_cls, x_dist = torch.randn(3, 10), torch.randn(3, 10, requires_grad=True)
    loss_fn = DistillationLoss(base, "none")
    out = loss_fn((x_cls, x_dist), target)
    assert float(out) == 4.25 and len(base.calls) == 1 and base.calls[0][0] is x_cls and base.calls[0][1] is labels
    assert float(loss_fn(x_cls, target)) == 4.25 and base.calls[1][0] is x_cls       # a single tensor as outputs
    assert x_dist.grad is None
    for kind in ("soft", "hard"):
        with pytest.raises(ValueError):
            DistillationLoss(base, kind)(x_cls, target)
    assert len(base.calls) == 2                                                       # refused before the base criterion ran
    with pytest.raises(ValueError):
        loss_fn((x_cls, x_dist), labels)                                              # not a DistillTarget
    with pytest.raises(ValueError):
        DistillationLoss(base, "soft")((x_cls, torch.randn(3, 12)), target)           # x_dist beside teacher logits of another width


def test_teacher_logits_refuses_a_class_count_mismatch():
    from autoprog_amd.prog.teacher import TeacherLogits
    from tests.test_token_label_teacher_host import _driver
    teacher = torch.nn.Linear(4, 4).train()
    teacher.num_classes = 24
    with pytest.raises(ValueError):
        TeacherLogits(teacher, num_classes=25)
    t = TeacherLogits(teacher, num_classes=24)
    assert t.num_classes == 24 and not teacher.training
    assert TeacherLogits(torch.nn.Linear(4, 4), num_classes=7).num_classes == 7       # any module: the count is then checked on its logits
    with pytest.raises(ValueError):
        TeacherLogits(torch.nn.Linear(4, 4), num_classes=7)(torch.zeros(2, 4), torch.zeros(2, dtype=torch.int64), 64)
    out = TeacherLogits(torch.nn.Linear(4, 7))(torch.zeros(2, 4), torch.tensor([1, 2]), 64)
    assert tuple(out.teacher_logits.shape) == (2, 7) and out.teacher_logits.dtype == torch.bfloat16 and out.base.tolist() == [1, 2]
    student = torch.nn.Linear(4, 4)
    student.num_classes = 25
    with pytest.raises(ValueError):                                                   # the driver's existing class-count check applies
        _driver(model=student, teacher=t)
    student.num_classes = 24
    assert _driver(model=student, teacher=t).teacher is t


def test_graph_refuses_a_distill_target():
    """a GraphedStep keeps no static copy of a DistillTarget yet: a clear refusal instead of a tensor method on the wrong object"""
    from autoprog_amd import graph
    from autoprog_amd.loss import DistillTarget
    with pytest.raises(NotImplementedError):
        graph._clone_target(DistillTarget(torch.tensor([1, 2, 3]), torch.randn(3, 10)))


def test_deit_set_drop_path_rate_follows_the_active_blocks():
    from autoprog_amd.models import create_model
    m = create_model("model_variant", variant="deit_h3_l4", num_classes=8, img_size=64)
    m.set_sample_config(dict(layer_num=4, min_layer_num=4, max_layer_num=4))
    m.set_drop_path_rate(0.3)
    assert [round(b.drop_prob, 6) for b in m.blocks] == [0.0, 0.1, 0.2, 0.3]
    m.set_drop_path_rate(0.0)
    assert all(b.drop_prob == 0.0 for b in m.blocks)
