"""DeiT's distillation objective (`DistillationLoss` of the published DeiT training code) on the HIP distillation kernel.

A distilled DeiT returns (x_cls, x_dist) in training mode.  The class-token logits take the base criterion against the labels, the
distillation-token logits take the teacher:

    soft   distill = kl_div(log_softmax(x_dist / T), log_softmax(teacher / T), reduction="sum", log_target=True) * T^2 / x_dist.numel()
    hard   distill = cross_entropy(x_dist, teacher.argmax(dim=1))
    loss   = (1 - alpha) * base + alpha * distill

The teacher's logits travel with the labels as a `DistillTarget` (prog.teacher.TeacherLogits builds one per batch), so the loss keeps
the `loss_fn(model(images), target)` call of every training loop here.  Eager steps only: graph.GraphedStep refuses a DistillTarget."""
import torch
import torch.nn as nn

from .. import functional as AF
from .cross_entropy import SoftTargetCrossEntropy


def _is_labels(t):
    return torch.is_tensor(t) and t.dim() == 1 and not t.dtype.is_floating_point


class DistillTarget:
    """what the base criterion takes -- integer labels [B], a data.MixedLabelTarget or a dense [B, C] tensor -- and the teacher's logits
    [B, C] of the same batch.  The logits are kept as bf16 on the base's device: anything else is cast once, here; a padded view (what
    functional.linear returns at a class count that is no multiple of 8) is taken as it is."""

    def __init__(self, base, teacher_logits):
        from ..data import MixedLabelTarget
        if not torch.is_tensor(teacher_logits) or teacher_logits.dim() != 2:
            raise ValueError("DistillTarget: teacher_logits must be [B, C]")
        B, C = teacher_logits.shape
        if isinstance(base, MixedLabelTarget):
            rows, dev = base.labels.shape[0], base.labels.device
            if base.num_classes != C:
                raise ValueError("DistillTarget: the mixed labels are of %d classes, the teacher's logits of %d" % (base.num_classes, C))
        elif _is_labels(base):
            rows, dev = base.shape[0], base.device
        elif torch.is_tensor(base) and base.dim() == 2 and base.dtype.is_floating_point:
            rows, dev = base.shape[0], base.device
            if base.shape[1] != C:
                raise ValueError("DistillTarget: a dense base target [B, %d] beside teacher logits [B, %d]" % (base.shape[1], C))
        else:
            raise ValueError("DistillTarget: base must be integer labels [B], a MixedLabelTarget or a dense [B, C] tensor")
        if rows != B:
            raise ValueError("DistillTarget: %d base rows beside %d teacher rows" % (rows, B))
        if teacher_logits.dtype != torch.bfloat16 or teacher_logits.device != dev:
            teacher_logits = teacher_logits.detach().to(device=dev, dtype=torch.bfloat16)
        self.base, self.teacher_logits = base, teacher_logits.detach()

    def base_for(self, criterion, smoothing, classes):
        """the base as `criterion` takes it: integer labels become the one-pair MixedLabelTarget (lam = 1, label smoothing) of the sparse CE
        kernel when the criterion is this library's SoftTargetCrossEntropy -- no dense [B, C] tensor is built.  Made at every call from the
        labels as they are then (a cast and a fill of B elements)."""
        from ..data import MixedLabelTarget
        if _is_labels(self.base) and isinstance(criterion, SoftTargetCrossEntropy):
            return MixedLabelTarget(self.base, 1.0, smoothing, classes)
        return self.base


class DistillationLoss(nn.Module):
    """forward((x_cls, x_dist), DistillTarget) -> (1 - alpha) * base_criterion(x_cls, target.base) + alpha * distill(x_dist, teacher).
    distillation_type: "none" | "soft" | "hard"; tau: the temperature of the soft form; soft_norm: "numel" divides the summed KL by B * C
    as the published code does, "batchmean" by B (what its comment says it meant); smoothing: the label smoothing of integer labels."""

    def __init__(self, base_criterion, distillation_type="hard", alpha=0.5, tau=1.0, soft_norm="numel", smoothing=0.1):
        super().__init__()
        if distillation_type not in ("none", "soft", "hard"):
            raise ValueError("DistillationLoss: distillation_type must be 'none', 'soft' or 'hard', got %r" % (distillation_type,))
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError("DistillationLoss: alpha must be in [0, 1], got %r" % (alpha,))
        if not float(tau) > 0.0:
            raise ValueError("DistillationLoss: tau must be positive, got %r" % (tau,))
        if soft_norm not in ("numel", "batchmean"):
            raise ValueError("DistillationLoss: soft_norm must be 'numel' or 'batchmean', got %r" % (soft_norm,))
        self.base_criterion = base_criterion
        self.distillation_type, self.alpha, self.tau = distillation_type, float(alpha), float(tau)
        self.soft_norm, self.smoothing = soft_norm, float(smoothing)

    def forward(self, outputs, target):
        if not isinstance(target, DistillTarget):
            raise ValueError("DistillationLoss: the target must be a DistillTarget (the base target and the teacher's logits)")
        pair = isinstance(outputs, (tuple, list))
        if pair and len(outputs) != 2:
            raise ValueError("DistillationLoss: outputs must be (x_cls, x_dist)")
        if not pair and self.distillation_type != "none":
            raise ValueError("DistillationLoss: %s distillation needs the pair (x_cls, x_dist) a distilled model returns in training mode"
                             % self.distillation_type)
        x_cls = outputs[0] if pair else outputs
        base = self.base_criterion(x_cls, target.base_for(self.base_criterion, self.smoothing, x_cls.shape[-1]))
        if self.distillation_type == "none":
            return base
        x_dist = outputs[1]
        B, C = x_dist.shape
        if tuple(target.teacher_logits.shape) != (B, C):
            raise ValueError("DistillationLoss: teacher logits %s beside x_dist %s" % (tuple(target.teacher_logits.shape), (B, C)))
        if self.distillation_type == "soft":
            weight = self.alpha / (B * C if self.soft_norm == "numel" else B)
            return AF.DistillCEFn.apply(x_dist.to(torch.bfloat16), target.teacher_logits, 0, 1.0 / self.tau, weight, base, 1.0 - self.alpha)
        return AF.DistillCEFn.apply(x_dist.to(torch.bfloat16), target.teacher_logits, 1, 1.0, self.alpha / B, base, 1.0 - self.alpha)
