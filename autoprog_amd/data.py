"""From a loader's batch to the model's input, on the device ("data pipeline").

The reference hands its model a tensor that timm's PrefetchLoader, RandomErasing and Mixup produce on the GPU every step: the uint8
`[B,3,H,W]` batch of `fast_collate` is cast, normalised (`.float().sub_(mean).div_(std)`), random-erased (main_prog.py builds the
loader with `re_prob`, and AutoProg re-scales it per stage: prog/progressive.py:31), mixed (DeiT: `--mixup` / `--cutmix`,
main_prog.py:195-207, 978-979) and resized to the stage's resolution (main_prog.py:973-974).  Here the per-step DECISIONS are drawn on
the host -- timm 0.4.5's rules, restated below -- and written into one small pinned block; the pixels are touched once, by
`ops.input_prep` (csrc/input_prep.hip), inside the model's patch embedding:

    prep = DeviceBatchPrep(mean, std, mixup_alpha=0.8, cutmix_alpha=1.0, re_prob=0.25)
    batch = prep.prep(u8)                       # uint8 [B,3,H,W] on the device; draws the step, no launch yet
    loss = SoftTargetCrossEntropy()(model(batch), batch.target(labels))

Differences from timm, on purpose: batch mode only (`--mixup-mode batch`, the default of every shipped script; "pair" / "elem" raise);
no `cutmix_minmax`; the collate-time blend is done in fp32 on the normalised values where timm's FastCollateMixup blends the uint8
images and rounds the result to uint8 again (at most half a grey level, 0.009 after normalisation); the per-pixel erase noise comes
from a counter-based generator keyed by (seed, step) so that a launch is a pure function of its inputs (replayable in a HIP graph);
and token labels are not mixed here: tlt's TokenLabelMixup also cuts the label maps, which is out of scope -- with a
SparseTokenLabelTarget only normalise / erase / resize apply, and asking for Mixup there raises."""
import math
import random

import numpy as np
import torch

from . import ops

MIX_NONE, MIX_MIXUP, MIX_CUTMIX = 0, 1, 2


def normalisation_table(mean, std):
    """fp32 [3, 256] on the CPU: table[c][v] = (v - 255 mean[c]) / (255 std[c]), the expression of timm's PrefetchLoader
    (`mean = tensor([x * 255 for x in mean])`, `.float().sub_(mean).div_(std)`) for every byte value -- the kernel looks the quotient
    up and so reproduces torch's subtraction and division bit for bit without dividing"""
    m = torch.tensor([x * 255 for x in mean]).view(3, 1)
    s = torch.tensor([x * 255 for x in std]).view(3, 1)
    return torch.arange(256, dtype=torch.float32).view(1, 256).sub(m).div(s).contiguous()


class MixedLabelTarget:
    """the target of a mixed batch in its source form: integer labels [B] and lam.  Row b of the dense target is timm's mixup_target,
    lam * one_hot(y[b]) + (1 - lam) * one_hot(y[B-1-b]) with one_hot = 1 - s + s / C on the label and s / C elsewhere; the loss never
    builds it (loss/cross_entropy.py: the sparse soft-target kernel with one pair per image).  `lam_ptr`: device address of lam (the
    parameter block of the step) for a graph replay; `lam` is the host's copy."""

    def __init__(self, labels, lam=1.0, smoothing=0.1, num_classes=1000, block=None):
        if labels.dim() != 1:
            raise ValueError("MixedLabelTarget: labels must be [B]")
        self.labels = labels.to(torch.int32).contiguous()
        self.ones = torch.ones(labels.shape[0], dtype=torch.float32, device=labels.device)
        self.lam, self.smoothing, self.num_classes = float(lam), float(smoothing), int(num_classes)
        self.block = block
        self.from_device = False               # graph.GraphedStep sets it: the loss reads lam from `block`

    @property
    def lam_ptr(self):
        return self.block.data_ptr() + 4       # word 1 of the parameter block

    def dense(self, classes=None):
        C = self.num_classes if classes is None else int(classes)
        off, on = self.smoothing / C, 1.0 - self.smoothing + self.smoothing / C
        y = self.labels.long().view(-1, 1)
        t = torch.full((y.shape[0], C), off, dtype=torch.float32, device=y.device).scatter_(1, y, on)
        return t * self.lam + t.flip(0) * (1.0 - self.lam)


class PreparedBatch:
    """a uint8 batch plus the step's decisions; `PatchEmbed.forward` / `PatchEmbed16.forward` turn it into their bf16 input with one
    launch of ops.input_prep at the size they would have resized to"""

    def __init__(self, u8, layout, table, block, host, mix, n_boxes, erase_mode, lam, owner):
        self.u8, self.layout, self.table, self.block, self.host = u8, layout, table, block, host
        self.mix, self.n_boxes, self.erase_mode, self.lam, self.owner = mix, n_boxes, erase_mode, lam, owner

    @property
    def shape(self):
        s = self.u8.shape
        return s if self.layout == "nchw" else torch.Size((s[0], s[3], s[1], s[2]))

    @property
    def is_cuda(self):
        return self.u8.is_cuda

    @property
    def device(self):
        return self.u8.device

    def run(self, size, out):
        return ops.input_prep(self.u8, size, out=out, table=self.table, params=self.block, layout=self.layout, mix=self.mix,
                              n_boxes=self.n_boxes, erase_mode=self.erase_mode, host_block=self.host)

    def target(self, labels):
        """integer labels [B] -> the MixedLabelTarget of this batch's draw.  A SparseTokenLabelTarget passes through unchanged, and only
        when this batch cannot have been mixed: token-label Mixup also cuts the label maps (tlt's TokenLabelMixup), which is not done here"""
        from .loss.cross_entropy import SparseTokenLabelTarget
        if isinstance(labels, SparseTokenLabelTarget):
            if self.mix:
                raise NotImplementedError("Mixup / CutMix with token labels is not supported (the label maps would have to be cut too)")
            return labels
        o = self.owner
        return MixedLabelTarget(labels, self.lam, o.label_smoothing, o.num_classes, block=self.block)


class DeviceBatchPrep:
    """timm's Mixup + RandomErasing + PrefetchLoader normalisation as host-side draws and one device launch (argument names as timm's).

    draw(B, H, W) makes the step's decisions from this object's own numpy.random.RandomState / random.Random (never the global
    streams) and writes them into the next slot of a ring of pinned blocks; prep(u8) draws and sends the block to the device in one
    copy.  The rules (timm 0.4.5 mixup.py / random_erasing.py):
      mix    if rand() < prob: with both alphas > 0, use_cutmix = rand() < switch_prob; lam = beta(a, a) of the chosen alpha (with one
             alpha > 0, that one).  lam == 1: no mix.  CutMix box: ratio = sqrt(1 - lam), cut_h, cut_w = int(H ratio), int(W ratio),
             cy = randint(0, H), cx = randint(0, W), yl, yh = clip(cy -/+ cut_h // 2, 0, H), xl, xh likewise, then
             lam = 1 - (yh - yl)(xh - xl) / (H W)  (correct_lam)
      erase  per image: skip if random() > re_prob; per box (re_count of them) up to 10 attempts: target = uniform(0.02, 1/3) H W / count,
             aspect = exp(uniform(log 0.3, log 1/0.3)), h = int(round(sqrt(target aspect))), w = int(round(sqrt(target / aspect))),
             accepted if w < W and h < H, at top = randint(0, H - h), left = randint(0, W - w) (inclusive)
    re_prob is a plain attribute (AutoProgDriver sets it per stage from the schedule's `re` list)."""
    SLOTS = 8

    def __init__(self, mean, std, mixup_alpha=0.0, cutmix_alpha=0.0, prob=1.0, switch_prob=0.5, mode="batch", label_smoothing=0.1,
                 num_classes=1000, re_prob=0.0, re_mode="pixel", re_count=1, seed=0, layout="nchw", device="cuda"):
        if mode != "batch":
            raise NotImplementedError("DeviceBatchPrep: mix mode %r -- batch mode only (image b is mixed with image B-1-b)" % (mode,))
        if re_mode not in ("const", "rand", "pixel"):
            raise ValueError("re_mode must be const, rand or pixel")
        if not 1 <= int(re_count) <= ops.PREP_MAX_BOXES:
            raise ValueError("re_count must be 1..%d" % ops.PREP_MAX_BOXES)
        if layout not in ("nchw", "nhwc"):
            raise ValueError("layout must be nchw or nhwc")
        self.mixup_alpha, self.cutmix_alpha, self.prob, self.switch_prob = float(mixup_alpha), float(cutmix_alpha), float(prob), float(switch_prob)
        self.label_smoothing, self.num_classes = float(label_smoothing), int(num_classes)
        self.re_prob, self.re_mode, self.re_count = float(re_prob), re_mode, int(re_count)
        self.seed, self.layout, self.device = int(seed), layout, torch.device(device)
        self.mix_enabled = self.mixup_alpha > 0 or self.cutmix_alpha > 0
        self.table_cpu = normalisation_table(mean, std)
        self._table = None
        self._np = np.random.RandomState(self.seed & 0xffffffff)
        self._py = random.Random(self.seed)
        self.steps = 0
        self._B = None
        self.last = None                       # the decisions of the last draw, for logs and tests

    # ---- the block: ops.PREP_PARAM_WORDS words of parameters, then B * re_count records of ops.PREP_BOX_WORDS words
    def _alloc(self, B):
        words = ops.PREP_PARAM_WORDS + B * self.re_count * ops.PREP_BOX_WORDS
        ring = torch.zeros(self.SLOTS, words, dtype=torch.int32)
        self._ring = ring.pin_memory() if self.device.type == "cuda" and torch.cuda.is_available() else ring
        self._dev = [None] * self.SLOTS
        self._events = [None] * self.SLOTS
        self._slot, self._B = 0, B

    def draw(self, B, H, W):
        """-> the host block (int32 CPU tensor) of the next step"""
        if self._B != B:
            self._alloc(B)
        self._slot = (self._slot + 1) % self.SLOTS
        ev = self._events[self._slot]
        if ev is not None:
            ev.synchronize()                   # the copy that last read this slot has executed (graph.StepScalars)
        host = self._ring[self._slot]
        a = host.numpy()
        a[:] = 0
        f, u = a.view(np.float32), a.view(np.uint32)
        rs = self._np
        mode, lam, box = MIX_NONE, 1.0, (0, 0, 0, 0)
        if self.mix_enabled and rs.rand() < self.prob:
            if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
                use_cutmix = rs.rand() < self.switch_prob
                alpha = self.cutmix_alpha if use_cutmix else self.mixup_alpha
            else:
                use_cutmix = self.cutmix_alpha > 0
                alpha = self.cutmix_alpha if use_cutmix else self.mixup_alpha
            lam = float(rs.beta(alpha, alpha))
            if lam != 1.0:
                if use_cutmix:
                    ratio = np.sqrt(1.0 - lam)
                    cut_h, cut_w = int(H * ratio), int(W * ratio)
                    cy, cx = rs.randint(0, H), rs.randint(0, W)
                    yl, yh = int(np.clip(cy - cut_h // 2, 0, H)), int(np.clip(cy + cut_h // 2, 0, H))
                    xl, xh = int(np.clip(cx - cut_w // 2, 0, W)), int(np.clip(cx + cut_w // 2, 0, W))
                    box = (yl, yh, xl, xh)
                    lam = 1.0 - (yh - yl) * (xh - xl) / float(H * W)
                    mode = MIX_CUTMIX
                else:
                    mode = MIX_MIXUP
        a[0] = mode
        f[1] = lam
        a[2:6] = box
        u[6], u[7] = self.seed & 0xffffffff, self.steps & 0xffffffff          # the noise of step t is keyed by (seed, t)
        f[8] = 1.0 - lam
        boxes = []
        py = self._py
        area, count = H * W, self.re_count
        lo, hi = math.log(0.3), math.log(1 / 0.3)
        for b in range(B):
            if py.random() > self.re_prob:
                continue
            for r in range(count):
                for _ in range(10):
                    target = py.uniform(0.02, 1 / 3) * area / count
                    aspect = math.exp(py.uniform(lo, hi))
                    h, w = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
                    if w < W and h < H:
                        top, left = py.randint(0, H - h), py.randint(0, W - w)
                        o = ops.PREP_PARAM_WORDS + (b * count + r) * ops.PREP_BOX_WORDS
                        a[o:o + 4] = (top, left, h, w)
                        if self.re_mode == "rand":
                            f[o + 4:o + 7] = rs.standard_normal(3)
                        boxes.append((b, top, left, h, w))
                        break
        self.steps += 1
        self.last = dict(mode=mode, lam=lam, box=box, boxes=boxes)
        return host

    def table(self):
        if self._table is None:
            self._table = self.table_cpu.to(self.device)
        return self._table

    def prep(self, u8):
        """uint8 device batch -> PreparedBatch: draws the step and enqueues the one copy of its block"""
        if u8.dtype != torch.uint8 or u8.dim() != 4 or not u8.is_cuda:
            raise ValueError("DeviceBatchPrep.prep: a uint8 [B,3,H,W] / [B,H,W,3] batch on the device")
        B = u8.shape[0]
        H, W = (u8.shape[2], u8.shape[3]) if self.layout == "nchw" else (u8.shape[1], u8.shape[2])
        host = self.draw(B, H, W)
        dev = self._dev[self._slot]
        if dev is None:
            dev = self._dev[self._slot] = torch.empty(host.numel(), dtype=torch.int32, device=u8.device)
        dev.copy_(host, non_blocking=True)
        ev = self._events[self._slot]
        if ev is None:
            ev = self._events[self._slot] = torch.cuda.Event()
        ev.record()
        return PreparedBatch(u8.contiguous(), self.layout, self.table(), dev, host, self.mix_enabled, self.re_count, self.re_mode,
                             self.last["lam"], self)
