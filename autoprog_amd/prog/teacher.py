"""Token-label targets from a teacher network, on the device, every step.

The reference takes its (class, score) pairs from label maps that were computed once with NFNet-F6 and exist for ImageNet-1k only
(main_prog.py:994-1004 -> tlt create_token_label_target).  For any other label set -- and for every stage resolution r of an AutoProg
run, each with its own (r // 16)^2 token grid -- the pairs come from a trained network of this library instead: the teacher sees the
batch the student sees, resized as the student's stem resizes it, runs its forward-only path (VOLO.forward_dense: class logits and the
aux head's logits of every token), and ops.softmax_topk turns the logits into a SparseTokenLabelTarget in two launches.

    labeler = TeacherLabeler(teacher, k=5, num_classes=student.num_classes)
    driver = AutoProgDriver(student, TokenLabelCrossEntropy(...), ..., get_batch=lambda r: (images, labels), teacher=labeler)
"""
import torch

from ..loss.cross_entropy import SPARSE_CE_MAX_PAIRS, SparseTokenLabelTarget


class TeacherLabeler:
    def __init__(self, teacher, k=5, temperature=1.0, smoothing=0.1, num_classes=None):
        """teacher: a VOLO of this library with its aux head (return_dense=True); it is put in eval() and only ever run under no_grad.
        k, temperature, smoothing: SparseTokenLabelTarget.from_logits.  num_classes: the student's class count, when given it must be
        the teacher's."""
        if not (getattr(teacher, "return_dense", False) and hasattr(teacher, "aux_head") and hasattr(teacher, "forward_dense")):
            raise ValueError("TeacherLabeler: the teacher needs an aux head (a VOLO built with return_dense=True)")
        if not 1 <= int(k) <= SPARSE_CE_MAX_PAIRS // 2:
            raise ValueError("TeacherLabeler: k must be 1 .. %d, got %d" % (SPARSE_CE_MAX_PAIRS // 2, int(k)))
        if not float(temperature) > 0:
            raise ValueError("TeacherLabeler: temperature must be positive")
        self.num_classes = int(teacher.num_classes)
        if num_classes is not None and int(num_classes) != self.num_classes:
            raise ValueError("TeacherLabeler: the teacher has %d classes, the student %d" % (self.num_classes, int(num_classes)))
        self.teacher, self.k, self.temperature, self.smoothing = teacher.eval(), int(k), float(temperature), float(smoothing)
        self._targets = {}                    # (B, r) -> the target buffer of that configuration, refilled by every call

    @torch.no_grad()
    def __call__(self, images, labels, r):
        """images: fp32 [B, 3, H, W] or a data.PreparedBatch (the teacher then sees the erased, normalised pixels); labels: int [B];
        r: the student's stage resolution.  -> the SparseTokenLabelTarget [B, 2 + (r // 16)^2, k] of this (B, r), overwritten by the
        next call with the same (B, r)."""
        from ..data import PreparedBatch
        if isinstance(images, PreparedBatch) and images.mix:
            raise NotImplementedError("Mixup / CutMix with token labels is not supported (the label maps would have to be cut too)")
        t = self.teacher
        if t.training:
            t.eval()
        pe = t.patch_embed
        pe.resize_to, pe.resize_in_eval = int(r), True      # the same pixels, resized as the student's stem resizes them
        x_cls, x_aux = t.forward_dense(images)
        if not labels.is_cuda:
            labels = labels.to(x_cls.device)
        key = (x_cls.shape[0], int(r))
        out = SparseTokenLabelTarget.from_logits(labels, x_cls, x_aux, self.k, self.temperature, self.smoothing, out=self._targets.get(key))
        self._targets[key] = out
        return out


class TeacherLogits:
    """The teacher of DeiT's distillation objective (loss.DistillationLoss), on the device, every step: the teacher sees the batch the
    student sees and its class logits travel to the loss beside the labels.

        teacher = TeacherLogits(create_model("deit_small_patch16_224").cuda(), num_classes=student.num_classes)
        driver = AutoProgDriver(student, DistillationLoss(SoftTargetCrossEntropy(), "hard"), ..., teacher=teacher)
    """

    def __init__(self, teacher, num_classes=None):
        """teacher: any nn.Module whose eval() forward returns [B, C] logits on the device; it is put in eval() and only ever run under
        no_grad.  num_classes: the student's class count, when given it must be the teacher's."""
        tc = getattr(teacher, "num_classes", None)
        if num_classes is not None and tc is not None and int(num_classes) != int(tc):
            raise ValueError("TeacherLogits: the teacher has %d classes, the student %d" % (int(tc), int(num_classes)))
        self.num_classes = int(tc) if tc is not None else (int(num_classes) if num_classes is not None else None)
        self.teacher = teacher.eval()

    @torch.no_grad()
    def __call__(self, images, labels, r):
        """images: fp32 [B, 3, H, W] or a data.PreparedBatch, mixed or not (the teacher then sees the mixed, erased, normalised pixels the
        student sees, and the base target is the batch's own: images.target(labels)); labels: int [B]; r: the student's stage resolution --
        a VOLO teacher resizes the batch to it as the student's stem does, any other teacher sees the images as given (a DeiT interpolates
        its position embedding).  -> loss.DistillTarget(base, the teacher's logits [B, C])"""
        from ..data import PreparedBatch
        from ..loss.distillation import DistillTarget
        t = self.teacher
        if t.training:
            t.eval()
        pe = getattr(t, "patch_embed", None)
        if pe is not None and hasattr(pe, "resize_to") and hasattr(pe, "resize_in_eval"):
            pe.resize_to, pe.resize_in_eval = int(r), True
        logits = t(images)
        if not (torch.is_tensor(logits) and logits.dim() == 2):
            raise ValueError("TeacherLogits: the teacher's eval() forward must return [B, C] logits")
        if self.num_classes is not None and logits.shape[1] != self.num_classes:
            raise ValueError("TeacherLogits: the teacher returned %d classes, %d were announced" % (logits.shape[1], self.num_classes))
        if torch.is_tensor(labels) and not labels.is_cuda and logits.is_cuda:
            labels = labels.to(logits.device)
        base = images.target(labels) if isinstance(images, PreparedBatch) else labels
        return DistillTarget(base, logits)
