"""Token-labeling losses (reference loss/cross_entropy.py) on the HIP dense soft-target CE
kernel: loss and d(loss)/d(logits) come out of ONE pass over (logits, target); the class-major
token-label tensor [B,C,2+N] is consumed in place through strides (no transpose copy).
Same constructor arguments and forward contracts as the reference classes."""
import torch
import torch.nn as nn

from .. import functional as AF


def _ce_rows(x2d, target, sb, sc, sn, rows_per_batch):
    return AF.SoftTargetCEFn.apply(x2d, target, sb, sc, sn, rows_per_batch)


def _dense_ce(x, target2d):
    """mean_i(-sum_c t_ic log_softmax(x_i)_c) for a [M,C] target (rows repeated when x has more rows,
    loss/cross_entropy.py:30-36)"""
    M, C = x.shape
    t = target2d.float()
    if not t.is_contiguous():
        t = t.contiguous()
    reps = M // t.shape[0]
    # row r of x uses target row r % t.shape[0]  (target.repeat(reps, 1))
    if reps == 1:
        return _ce_rows(x, t, C, 1, 0, 1)
    losses = [_ce_rows(x[i * t.shape[0]:(i + 1) * t.shape[0]], t, C, 1, 0, 1) for i in range(reps)]
    return torch.stack(losses).mean()


class SoftTargetCrossEntropy(nn.Module):
    """reference SoftTargetCrossEntropy (loss/cross_entropy.py:21-36)"""

    def forward(self, x, target):
        from ..data import MixedLabelTarget
        if isinstance(target, MixedLabelTarget):
            # a Mixup / CutMix batch of data.DeviceBatchPrep: (labels, lam) go to the sparse kernel as they are, at every class count; only a
            # target that does not pair up with the logits row for row is densified (timm's mixup_target) and takes the dense kernel
            C = x.shape[-1]
            if x.dim() == 2 and target.labels.is_cuda and x.shape[0] == target.labels.shape[0]:
                lam = target if target.from_device else target.lam
                return AF.MixedLabelCEFn.apply(x.to(torch.bfloat16), target.labels, target.ones, target.smoothing, lam)
            if target.from_device:
                raise NotImplementedError("a graph-mode step (lam in device memory) needs the sparse soft-target kernel")
            target = target.dense(C)
        return _dense_ce(x.to(torch.bfloat16), target)


class TokenLabelSoftTargetCrossEntropy(nn.Module):
    """reference TokenLabelSoftTargetCrossEntropy (loss/cross_entropy.py:92-109)"""

    def forward(self, x, target):
        if target.dim() == 3 and target.shape[-1] == 2:
            target = target[:, :, 1]
        return _dense_ce(x.to(torch.bfloat16), target)


SPARSE_CE_MAX_PAIRS = 16        # CE_MAXK of csrc/softce.hip; the class count is not limited here (rows of up to 65 536 padded columns)
SPARSE_GT_MAX_K = 8             # CE_GT_MAXK: pairs per slot on the class rows of TokenLabelGTCrossEntropy


class _TokenLabelBase(nn.Module):
    def __init__(self, dense_weight=1.0, cls_weight=1.0, mixup_active=True, classes=1000):
        super().__init__()
        self.CE = SoftTargetCrossEntropy()
        self.dense_weight = dense_weight
        self.mixup_active = mixup_active
        self.classes = classes
        self.cls_weight = cls_weight
        assert dense_weight + cls_weight > 0

    def _adjust_cls(self, target_cls, target):
        return target_cls

    def forward(self, x, target):
        output, aux_output, bb = x
        dev_box = getattr(bb, "scalars", None)                  # graph.DeviceBox: the step's box / lam live in device memory (graph replay)
        B, N, C = aux_output.shape
        if dev_box is None:
            bbx1, bby1, bbx2, bby2 = bb
            host_lam = 1 - ((bbx2 - bbx1) * (bby2 - bby1) / N)
            lam = float(host_lam)                               # what the fused paths are given: a host float, or the device box
        else:
            lam = dev_box
        if isinstance(target, SparseTokenLabelTarget):
            # the sparse kernel takes up to 16 (class, score) pairs per row -- the mix-token class row carries 2K -- at every class count (a
            # dense [B, C, 2 + N] tensor at 21 843 classes could not exist); more pairs are densified and take the dense kernels
            K = target.idx.shape[-1]
            if (type(self)._adjust_cls is _TokenLabelBase._adjust_cls and target.idx.is_cuda and target.idx.shape[1] == 2 + N
                    and 2 * K <= SPARSE_CE_MAX_PAIRS):
                return AF.SparseTokenLabelCEFn.apply(output.to(torch.bfloat16), aux_output.to(torch.bfloat16), target.idx, target.val,
                                                     target.smoothing, lam, float(self.cls_weight), float(self.dense_weight))
            # the ground-truth variant's class row carries 4 K pairs (slot 1 and slot 0 of the image and of its mix-token partner) and the
            # kernel takes 32: functional.SparseTokenLabelGTCEFn.  A subclass with an _adjust_cls of its own is densified as before.
            if (type(self)._adjust_cls is TokenLabelGTCrossEntropy._adjust_cls and target.idx.is_cuda and target.idx.shape[1] == 2 + N
                    and K <= SPARSE_GT_MAX_K):
                return AF.SparseTokenLabelGTCEFn.apply(output.to(torch.bfloat16), aux_output.to(torch.bfloat16), target.idx, target.val,
                                                       target.smoothing, lam, float(self.cls_weight), float(self.dense_weight))
            target = target.dense(C)
        target = target.float()
        if target.dim() == 3 and type(self)._adjust_cls is _TokenLabelBase._adjust_cls and target.is_cuda:
            # the production case (TokenLabelCrossEntropy with token labels): three launches, see functional.TokenLabelCEFn
            return AF.TokenLabelCEFn.apply(output.to(torch.bfloat16), aux_output.to(torch.bfloat16), target, lam,
                                           float(self.cls_weight), float(self.dense_weight))
        # the ground-truth variant on a dense [B, C, 2 + N] target in a graph-mode step takes the route below op for op -- the adjusted class
        # target from torch ops, the dense kernels -- with lam read from device memory, so a replay gives the eager step's bits wherever lam
        # and 1 - lam are exact in fp32 (a token grid of 2^k tokens); 2-D targets and other subclasses have no graph-mode route
        dev_gt = (dev_box is not None and target.dim() == 3 and target.is_cuda
                  and type(self)._adjust_cls is TokenLabelGTCrossEntropy._adjust_cls)
        if dev_box is not None and not dev_gt:
            raise NotImplementedError("a graph-mode forward (device-resident mix box) needs the fused token-label loss paths")
        aux2d = aux_output.reshape(B * N, C).to(torch.bfloat16)
        if target.dim() == 2:
            target_cls = target
            t = target.contiguous()
            loss_aux = _ce_rows(aux2d, t, C, 1, 0, N)                 # target.repeat(1,N): every token sees row b
        else:
            target_cls = self._adjust_cls(target[:, :, 1], target)
            taux = target[:, :, 2:]                                   # [B,C,N] class-major view, consumed in place
            loss_aux = _ce_rows(aux2d, taux, target.stride(0), target.stride(1), target.stride(2), N)
        if dev_gt:
            # no host decision: lam = 1 blends nothing (1 * t + 0 * t' = t exactly)
            lam = dev_box.dev.view(torch.float32)[4]            # graph.StepScalars: word 4 is lam
            target_cls = lam * target_cls + (1 - lam) * target_cls.flip(0)
        elif host_lam < 1:
            target_cls = host_lam * target_cls + (1 - host_lam) * target_cls.flip(0)
        loss_cls = _dense_ce(output.to(torch.bfloat16), target_cls)
        return self.cls_weight * loss_cls + self.dense_weight * loss_aux


class TokenLabelCrossEntropy(_TokenLabelBase):
    """reference TokenLabelCrossEntropy (loss/cross_entropy.py:112-156)"""


class SparseTokenLabelTarget:
    """The token-label target before it is densified: `idx` int32 and `val` fp32, both [B, 2 + N, K] (slot 0 ground truth, slot 1
    image level, slots 2.. tokens: SURVEY.md appendix A.2), and the label-smoothing strength.  dense() is what the reference's
    create_token_label_target hands to its loss: [B, C, 2 + N] with t = (1 - s) * scatter(val) + s / C."""

    def __init__(self, idx, val, smoothing=0.1):
        if idx.shape != val.shape or idx.dim() != 3:
            raise ValueError("SparseTokenLabelTarget: idx and val must both be [B, 2 + N, K]")
        self.idx, self.val, self.smoothing = idx.to(torch.int32), val.float(), float(smoothing)

    @classmethod
    def from_logits(cls, labels, cls_logits, aux_logits, k=5, temperature=1.0, smoothing=0.1, out=None):
        """The target a teacher network gives: labels int [B], cls_logits [B, C], aux_logits [B, N, C] (bf16; the last dimension may be a
        padded view, as functional.linear returns it at a class count that is no multiple of 8) -> [B, 2 + N, k] with slot 0 the ground
        truth ((label, 1.0), then (-1, 0.0): an index outside [0, C) adds nothing), slot 1 the top-k of softmax(cls_logits / temperature)
        and slots 2.. those of every token -- two launches of ops.softmax_topk that write in place, equal logits by ascending class.
        out: a target [B, 2 + N, k] of an earlier call to fill (nothing is allocated then; graph-capturable).
        k <= 8: the mix-token class row of TokenLabelCrossEntropy carries 2 k pairs and the sparse kernel takes SPARSE_CE_MAX_PAIRS = 16 --
        beyond that the loss would densify the target, which the wide label sets this exists for cannot do."""
        from .. import ops
        k = int(k)
        if not 1 <= k <= SPARSE_CE_MAX_PAIRS // 2:
            raise ValueError("from_logits: k must be 1 .. %d (2 k pairs of the mix-token class row), got %d" % (SPARSE_CE_MAX_PAIRS // 2, k))
        if not float(temperature) > 0:
            raise ValueError("from_logits: temperature must be positive")
        if aux_logits.dim() != 3 or cls_logits.dim() != 2 or labels.dim() != 1:
            raise ValueError("from_logits: labels [B], cls_logits [B, C], aux_logits [B, N, C]")
        B, N, C = aux_logits.shape
        if tuple(cls_logits.shape) != (B, C) or labels.shape[0] != B or k > C:
            raise ValueError("from_logits: labels [B], cls_logits [B, C], aux_logits [B, N, C] with k <= C")
        if not (cls_logits.is_cuda and aux_logits.is_cuda and labels.is_cuda):
            raise ops.AutoProgHipError("from_logits: CUDA tensors (the HIP path has no CPU fallback)")
        if out is None:
            out = cls(torch.empty((B, 2 + N, k), dtype=torch.int32, device=aux_logits.device),
                      torch.empty((B, 2 + N, k), dtype=torch.float32, device=aux_logits.device), smoothing)
        elif not (isinstance(out, cls) and tuple(out.idx.shape) == (B, 2 + N, k) and out.idx.is_contiguous() and out.val.is_contiguous()
                  and out.idx.device == aux_logits.device):
            raise ValueError("from_logits: out must be a contiguous SparseTokenLabelTarget [%d, %d, %d] on the logits' device" % (B, 2 + N, k))
        out.smoothing = float(smoothing)
        out.idx[:, 0].fill_(-1)
        out.idx[:, 0, 0].copy_(labels)
        out.val[:, 0].zero_()
        out.val[:, 0, 0].fill_(1.0)
        fi, fv, S = out.idx.view(-1), out.val.view(-1), (2 + N) * k
        inv_temp = 1.0 / float(temperature)
        ops.softmax_topk(ops.padded_view_rows(aux_logits.reshape(B * N, C)), C, k, inv_temp, fi[2 * k:], fv[2 * k:], S, k, N)
        ops.softmax_topk(ops.padded_view_rows(cls_logits), C, k, inv_temp, fi[k:], fv[k:], S, 0, 1)
        return out

    def dense(self, classes):
        B, S, K = self.idx.shape
        t = torch.zeros(B, classes, S, dtype=torch.float32, device=self.val.device)
        t.scatter_add_(1, self.idx.long().permute(0, 2, 1), self.val.permute(0, 2, 1))
        return t * (1.0 - self.smoothing) + self.smoothing / classes


class TokenLabelGTCrossEntropy(_TokenLabelBase):
    """reference TokenLabelGTCrossEntropy (loss/cross_entropy.py:39-89): mixes the ground truth
    slot [:,:,0] into the image-level soft label"""

    def __init__(self, dense_weight=1.0, cls_weight=1.0, mixup_active=True, smoothing=0.1, classes=1000):
        super().__init__(dense_weight, cls_weight, mixup_active, classes)
        self.smoothing = smoothing

    def _adjust_cls(self, target_cls, target):
        gt = target[:, :, 0]
        same = (gt.max(-1)[1] == target_cls.max(-1)[1])
        ratio = (0.9 - 0.4 * same.to(target_cls.dtype)).unsqueeze(-1)
        return target_cls * ratio + gt * (1 - ratio)
