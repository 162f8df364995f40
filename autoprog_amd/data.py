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
SparseTokenLabelTarget only normalise / erase / resize apply, and asking for Mixup there raises.

In front of it, DeviceRandomResizedCrop does the loader's random-resized crop and horizontal flip on the device as well: one box and one
flip per image drawn on the host, one launch of `ops.crop_resize_u8` (csrc/crop.hip) from the loader's fixed-size uint8 canvases to the
uint8 batch at the stage's resolution that `prep` takes -- the per-stage crop scale of AutoProg's schedule is then an attribute, where
the reference rebuilds its loader (main_prog.py:651-653, 840-846).

Between the two, where timm's transform chain has it, DeviceRandAugment applies the auto-augment step (`--aa rand-m9-mstd0.5-inc1`) to
that uint8 batch: the ops and their arguments drawn on the host in timm's order, one launch of `ops.randaug_u8` (csrc/randaug.hip) per
layer, every op Pillow's bytes -- the per-stage magnitude of AutoProg's schedule is an attribute as well.

Beside the crop, DeviceLabelMapCrop cuts the stored token-label maps of the batch (StoredLabelMaps: tlt's top-k (score, class) maps) to
the boxes the crop just drew and flips them with the images: one launch of `ops.label_map_crop` (csrc/labelmap.hip) fills the
SparseTokenLabelTarget of the stage's token grid, where the reference's loader ROI-aligns the maps on the CPU (main_prog.py:994-1004)."""
import math
import random
import re

import numpy as np
import torch

from . import ops
from .ring import PinnedRing

MIX_NONE, MIX_MIXUP, MIX_CUTMIX = 0, 1, 2


def _layout(layout):
    if layout not in ("nchw", "nhwc"):
        raise ValueError("layout must be nchw or nhwc")
    return layout


def _device_batch(u8, layout, who):
    """-> (B, H, W) of a uint8 [B,3,H,W] / [B,H,W,3] batch on the device"""
    if not torch.is_tensor(u8) or u8.dtype != torch.uint8 or u8.dim() != 4 or not u8.is_cuda:
        raise ValueError("%s: a uint8 [B,3,H,W] / [B,H,W,3] batch on the device" % who)
    return (u8.shape[0],) + ((u8.shape[2], u8.shape[3]) if layout == "nchw" else (u8.shape[1], u8.shape[2]))


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
    SLOTS = PinnedRing.SLOTS

    def __init__(self, mean, std, mixup_alpha=0.0, cutmix_alpha=0.0, prob=1.0, switch_prob=0.5, mode="batch", label_smoothing=0.1,
                 num_classes=1000, re_prob=0.0, re_mode="pixel", re_count=1, seed=0, layout="nchw", device="cuda"):
        if mode != "batch":
            raise NotImplementedError("DeviceBatchPrep: mix mode %r -- batch mode only (image b is mixed with image B-1-b)" % (mode,))
        if re_mode not in ("const", "rand", "pixel"):
            raise ValueError("re_mode must be const, rand or pixel")
        if not 1 <= int(re_count) <= ops.PREP_MAX_BOXES:
            raise ValueError("re_count must be 1..%d" % ops.PREP_MAX_BOXES)
        self.mixup_alpha, self.cutmix_alpha, self.prob, self.switch_prob = float(mixup_alpha), float(cutmix_alpha), float(prob), float(switch_prob)
        self.label_smoothing, self.num_classes = float(label_smoothing), int(num_classes)
        self.re_prob, self.re_mode, self.re_count = float(re_prob), re_mode, int(re_count)
        self.seed, self.layout, self.device = int(seed), _layout(layout), torch.device(device)
        self.mix_enabled = self.mixup_alpha > 0 or self.cutmix_alpha > 0
        self.table_cpu = normalisation_table(mean, std)
        self._table = None
        self._np = np.random.RandomState(self.seed & 0xffffffff)
        self._py = random.Random(self.seed)
        self.steps = 0
        self._ring = PinnedRing(self.device)
        self.last = None                       # the decisions of the last draw, for logs and tests

    def draw(self, B, H, W):
        """-> the host block (int32 CPU tensor) of the next step: ops.PREP_PARAM_WORDS words of parameters, then B * re_count records of
        ops.PREP_BOX_WORDS words"""
        host = self._ring.next(ops.PREP_PARAM_WORDS + B * self.re_count * ops.PREP_BOX_WORDS)
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
        host = self.draw(*_device_batch(u8, self.layout, "DeviceBatchPrep.prep"))
        dev = self._ring.send(u8.device)
        return PreparedBatch(u8.contiguous(), self.layout, self.table(), dev, host, self.mix_enabled, self.re_count, self.re_mode,
                             self.last["lam"], self)


class DeviceRandomResizedCrop:
    """timm's RandomResizedCropAndInterpolation + RandomHorizontalFlip as host-side draws and one device launch (ops.crop_resize_u8,
    csrc/crop.hip).  The loader hands over one fixed-size decoded uint8 canvas per image; `crop(u8, size)` draws a box and a flip per
    image and lands each box at size x size directly -- the stage's resolution r, one bilinear resample without antialiasing where the
    reference does two (RandomResizedCrop to 224 in the loader, F.interpolate to r on the GPU, main_prog.py:973-974).  The result is the
    uint8 batch DeviceBatchPrep.prep takes.

    The decisions come from this object's own random.Random(seed) (never the global streams) and are written into the next slot of a
    ring of pinned blocks that reaches the device in one small copy, as DeviceBatchPrep's do.  The rule (timm 0.4.5 transforms.py,
    `get_params`), per image over its extent (eh, ew), in this draw order:
      box    up to 10 attempts: target = uniform(scale[0], scale[1]) * (eh ew), aspect = exp(uniform(log ratio[0], log ratio[1])),
             w = int(round(sqrt(target aspect))), h = int(round(sqrt(target / aspect))), accepted iff 0 < w <= ew and 0 < h <= eh (the
             `0 <` is added here: timm can return an empty box on a tiny image), then top = randint(0, eh - h), left = randint(0, ew - w)
             (inclusive).  After 10 refusals the central crop with the ratio clamped: ew / eh < ratio[0]: w = ew, h = int(round(w / ratio[0]));
             ew / eh > ratio[1]: h = eh, w = int(round(h * ratio[1])); otherwise the whole extent; top = (eh - h) // 2, left = (ew - w) // 2
      flip   one random(), ALWAYS drawn; the image is flipped iff it is below hflip (so the stream does not depend on hflip)
    scale, ratio and hflip are plain attributes (AutoProgDriver sets `scale` per stage from the schedule's `resize` list); `last` holds the
    records of the last draw or centre crop, one (top, left, h, w, flip) per image.

    interpolation (a plain attribute too): None is the two-tap bilinear sample above.  "bilinear", "bicubic" or "random" resample each
    box as the reference's loader does, with Pillow's antialiased filter (ops.crop_resample_u8, csrc/resample.hip: byte for byte
    Image.crop(box).resize((size, size), filter), flipped afterwards).  `last` then holds (top, left, h, w, flip, filter) with filter
    ops.RESAMPLE_BILINEAR / RESAMPLE_BICUBIC.  A fixed filter draws nothing more; "random" is timm 0.4.5's
    `random.choice(self.interpolation)` inside `__call__`, after `get_params` and before the flip transform: per image the draw order
    is box, then choice((bilinear, bicubic)), then flip."""
    SLOTS = PinnedRing.SLOTS
    FILTERS = {"bilinear": ops.RESAMPLE_BILINEAR, "bicubic": ops.RESAMPLE_BICUBIC}

    def __init__(self, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), hflip=0.5, size=None, seed=0, layout="nchw", device="cuda",
                 interpolation=None):
        self._filter(interpolation, True)
        self.interpolation = interpolation
        self.scale, self.ratio, self.hflip = tuple(scale), tuple(ratio), float(hflip)
        self.size, self.seed, self.layout, self.device = size, int(seed), _layout(layout), torch.device(device)
        self._py = random.Random(self.seed)
        self._ring = PinnedRing(self.device)
        self.last = None
        self.last_extents = None               # the (eh, ew) of every image of the last draw or centre crop (DeviceLabelMapCrop reads both)

    def _next(self, B):
        """-> the next slot's host block, zeroed, and its view as a [B, 8] int32 array"""
        host = self._ring.next(max(B, 1) * ops.CROP_RECORD_WORDS)
        a = host.numpy().reshape(max(B, 1), ops.CROP_RECORD_WORDS)
        a[:] = 0
        return host, a

    @staticmethod
    def _extents(B, H, W, extents):
        if extents is None:
            return [(H, W)] * B
        e = np.asarray(extents.cpu() if torch.is_tensor(extents) else extents)
        if e.shape != (B, 2) or not np.issubdtype(e.dtype, np.integer):
            raise ValueError("extents: an integer [B, 2] array of (eh, ew)")
        if B and (e.min() < 1 or e[:, 0].max() > H or e[:, 1].max() > W):
            raise ValueError("extents: 1 <= eh <= %d and 1 <= ew <= %d" % (H, W))
        return [(int(eh), int(ew)) for eh, ew in e]

    def _box(self, eh, ew):
        py, area = self._py, eh * ew
        lo, hi = math.log(self.ratio[0]), math.log(self.ratio[1])
        for _ in range(10):
            target = py.uniform(self.scale[0], self.scale[1]) * area
            aspect = math.exp(py.uniform(lo, hi))
            w, h = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
            if 0 < w <= ew and 0 < h <= eh:
                return py.randint(0, eh - h), py.randint(0, ew - w), h, w
        in_ratio = ew / eh
        if in_ratio < self.ratio[0]:
            w = ew
            h = min(max(int(round(w / self.ratio[0])), 1), eh)
        elif in_ratio > self.ratio[1]:
            h = eh
            w = min(max(int(round(h * self.ratio[1])), 1), ew)
        else:
            h, w = eh, ew
        return (eh - h) // 2, (ew - w) // 2, h, w

    @classmethod
    def _filter(cls, interpolation, random_too):
        """None -> 0 (the two-tap sample), a named filter -> its code, "random" -> None"""
        if interpolation is None:
            return 0
        if interpolation == "random" and random_too:
            return None
        if interpolation not in cls.FILTERS:
            raise ValueError("interpolation must be None, 'bilinear', 'bicubic'%s, got %r" % (" or 'random'" if random_too else "", interpolation))
        return cls.FILTERS[interpolation]

    def draw(self, B, H, W, extents=None):
        """-> the host block (int32 CPU tensor, B records of 8 words) of the next crop: one box and one flip per image, and with
        interpolation "random" one filter"""
        ext = self.last_extents = self._extents(B, H, W, extents)
        host, a = self._next(B)
        rnd, hflip = self._py.random, self.hflip
        filt = self._filter(self.interpolation, True)
        if filt == 0:
            self.last = [self._box(eh, ew) + (int(rnd() < hflip),) for eh, ew in ext]
        elif filt is None:
            choice, both = self._py.choice, (ops.RESAMPLE_BILINEAR, ops.RESAMPLE_BICUBIC)
            self.last = []
            for eh, ew in ext:
                box, f = self._box(eh, ew), choice(both)            # box, filter, flip: timm's order
                self.last.append(box + (int(rnd() < hflip), f))
        else:
            self.last = [self._box(eh, ew) + (int(rnd() < hflip), filt) for eh, ew in ext]
        if B:
            a[:B, :5 + (filt != 0)] = self.last    # (one assignment: a per-image write costs more host time than the draw)
        return host

    def center_records(self, B, H, W, crop_pct=0.875, extents=None, interpolation=None):
        """-> the host block of the central square boxes of side int(round(crop_pct * min(eh, ew))), no flip; nothing is drawn.
        interpolation: None (the object's setting), "bilinear" or "bicubic"; "random" is refused, here and as the object's setting"""
        filt = self._filter(self.interpolation if interpolation is None else interpolation, False)
        ext = self.last_extents = self._extents(B, H, W, extents)
        host, a = self._next(B)
        self.last = []
        for eh, ew in ext:
            side = min(max(int(round(crop_pct * min(eh, ew))), 1), min(eh, ew))
            self.last.append(((eh - side) // 2, (ew - side) // 2, side, side, 0) + ((filt,) if filt else ()))
        if B:
            a[:B, :5 + (filt != 0)] = self.last
        return host

    def _launch(self, u8, size, host, antialias):
        dev = self._ring.send(u8.device)
        return (ops.crop_resample_u8 if antialias else ops.crop_resize_u8)(u8.contiguous(), size, dev, layout=self.layout, host_records=host)

    def _size(self, size):
        size = self.size if size is None else size
        if size is None or int(size) < 1:
            raise ValueError("DeviceRandomResizedCrop: an output size >= 1 (crop(u8, size) or the constructor's size)")
        return int(size)

    def crop(self, u8, size=None, extents=None):
        """uint8 device batch -> uint8 [B,3,S,S] / [B,S,S,3]: draws a box and a flip per image, one copy and one launch.  extents: optional
        integer [B,2] (eh, ew) for images that fill only the top-left part of a padded canvas (default: the whole canvas)"""
        size = self._size(size)
        B, H, W = _device_batch(u8, self.layout, "DeviceRandomResizedCrop")
        return self._launch(u8, size, self.draw(B, H, W, extents), self.interpolation is not None)

    def center(self, u8, size, crop_pct=0.875, extents=None, interpolation=None):
        """the same launch on the central square box of side int(round(crop_pct * min(eh, ew))), no flip, no draw: on a fixed canvas the
        validation-time resize and centre crop.  interpolation as center_records'.  With "bicubic" and crop_pct = 0.96 this stands where
        the reference's validation transform does (Pillow bicubic), in the other order: the reference resizes the shorter side to
        floor(size / crop_pct) and then cuts the central size x size; this cuts the central square of side round(crop_pct * min(eh, ew))
        and resizes it to size x size"""
        size = self._size(size)
        B, H, W = _device_batch(u8, self.layout, "DeviceRandomResizedCrop")
        host = self.center_records(B, H, W, crop_pct, extents, interpolation)
        return self._launch(u8, size, host, (self.interpolation if interpolation is None else interpolation) is not None)


class StoredLabelMaps:
    """the stored token labels of a batch, as the loader hands them over beside the canvases: integer labels [B] and the top-k label maps
    of the same images.  maps: tlt's tensor [B, 2, Kin, Hm, Wm] (half or float: [:, 0] the scores, [:, 1] the classes, read as two views
    without a copy), or (scores [B, Kin, Hm, Wm], classes) with int32 classes -- label sets beyond 2048 classes need the second form,
    fp16 does not hold their class numbers exactly.  A map covers its image's extent, not the padded canvas."""

    def __init__(self, labels, maps):
        if torch.is_tensor(maps):
            if maps.dim() != 5 or maps.shape[1] != 2 or maps.dtype not in (torch.float16, torch.float32):
                raise ValueError("StoredLabelMaps: a half or float [B, 2, Kin, Hm, Wm] tensor, or (scores, classes)")
            scores, classes = maps[:, 0], maps[:, 1]
        else:
            scores, classes = maps
            if not (torch.is_tensor(scores) and torch.is_tensor(classes)) or scores.dim() != 4 or scores.shape != classes.shape:
                raise ValueError("StoredLabelMaps: scores and classes must both be [B, Kin, Hm, Wm]")
            if scores.dtype not in (torch.float16, torch.float32) or classes.dtype not in (torch.int32, scores.dtype):
                raise ValueError("StoredLabelMaps: half or float scores, classes int32 or in the scores' dtype")
        if not torch.is_tensor(labels) or labels.dim() != 1 or labels.dtype.is_floating_point or labels.shape[0] != scores.shape[0]:
            raise ValueError("StoredLabelMaps: integer labels [B] for the B images of the maps")
        self.labels, self.scores, self.classes = labels.to(device=scores.device, dtype=torch.int64).contiguous(), scores, classes


class DeviceLabelMapCrop:
    """tlt's token labels from stored maps, cut where the box is known: `target(stored, crop, r)` ROI-aligns the StoredLabelMaps of a
    batch to the boxes DeviceRandomResizedCrop just drew for it (crop.last, crop.last_extents), flips them with the images, and returns
    the SparseTokenLabelTarget [B, 2 + P P, k] at the stage's token grid P = r // 16 -- one small copy of the B box records and one
    launch of ops.label_map_crop (csrc/labelmap.hip).  The reference's loader does this on the CPU before create_token_label_target
    (main_prog.py:994-1004), where the box still belongs to the loader.

    The records are formed on the host in float64 and rounded to fp32: with the box (top, left, h, w) on an image of extent (eh, ew) and
    maps of Hm x Wm,  x1 = left Wm / ew,  y1 = top Hm / eh,  x2 = (left + w) Wm / ew,  y2 = (top + h) Hm / eh,  then the flip.  They go
    into this object's own ring of pinned blocks, as the crop's do.  The target of a (B, r) is kept and refilled in place by the next call
    (as prog.teacher.TeacherLabeler's).  k <= 8: the mix-token class row of the loss carries 2 k pairs.  Scores are written raw; smoothing
    is the target's attribute, applied where the loss reads the pairs.  Mixup / CutMix of token labels is not done."""
    SLOTS = PinnedRing.SLOTS

    def __init__(self, k=8, smoothing=0.1, num_classes=1000):
        if not 1 <= int(k) <= ops.LABEL_MAP_MAX_K:
            raise ValueError("DeviceLabelMapCrop: k must be 1 .. %d, got %d" % (ops.LABEL_MAP_MAX_K, int(k)))
        if not 1 <= int(num_classes) <= 65536:
            raise ValueError("DeviceLabelMapCrop: num_classes must be 1 .. 65536")
        self.k, self.smoothing, self.num_classes = int(k), float(smoothing), int(num_classes)
        self._ring = PinnedRing("cuda")
        self._targets = {}                     # (B, r) -> the target of that configuration, refilled by every call
        self.last = None                       # the records of the last call: (x1, y1, x2, y2, flip) per image, as fp32 values

    def records(self, crop, B, Hm, Wm):
        """-> the host block (fp32 CPU tensor, B records of 8 words) of the boxes `crop` drew last, in the pixel units of Hm x Wm maps"""
        last, ext = getattr(crop, "last", None), getattr(crop, "last_extents", None)
        if last is None or ext is None or len(last) != B or len(ext) != B:
            raise ValueError("DeviceLabelMapCrop: crop.last does not belong to a batch of %d images (crop the batch first)" % B)
        host = self._ring.next(max(B, 1) * ops.LABEL_MAP_BOX_WORDS, torch.float32)
        a = host.numpy().reshape(max(B, 1), ops.LABEL_MAP_BOX_WORDS)
        a[:] = 0
        if B:
            box = np.asarray([rec[:5] for rec in last], dtype=np.float64)           # top, left, h, w, flip
            e = np.asarray(ext, dtype=np.float64)
            a[:B, 0], a[:B, 1] = box[:, 1] * Wm / e[:, 1], box[:, 0] * Hm / e[:, 0]
            a[:B, 2], a[:B, 3] = (box[:, 1] + box[:, 3]) * Wm / e[:, 1], (box[:, 0] + box[:, 2]) * Hm / e[:, 0]
            a[:B, 4] = box[:, 4]
        self.last = [tuple(float(v) for v in row[:5]) for row in a[:B]]
        return host

    def target(self, stored, crop, r, out=None):
        """stored: the StoredLabelMaps of the batch `crop` cropped last; r: the resolution it was cropped to.  -> the
        SparseTokenLabelTarget [B, 2 + (r // 16)^2, k] of this (B, r), overwritten by the next call with the same (B, r).  out: a target of
        that shape to fill instead."""
        from .loss.cross_entropy import SparseTokenLabelTarget
        if not isinstance(stored, StoredLabelMaps):
            raise ValueError("DeviceLabelMapCrop.target: a StoredLabelMaps")
        if not stored.scores.is_cuda:
            raise ops.AutoProgHipError("DeviceLabelMapCrop.target: maps on the device (the HIP path has no CPU fallback)")
        B, _, Hm, Wm = stored.scores.shape
        P = int(r) // 16
        if P < 1:
            raise ValueError("DeviceLabelMapCrop.target: r = %d has no token grid (r // 16 < 1)" % int(r))
        host = self.records(crop, B, Hm, Wm)
        dev = self._ring.send(stored.scores.device)
        key, shape = (B, int(r)), (B, 2 + P * P, self.k)
        if out is None:
            out = self._targets.get(key)
            if out is None or out.idx.device != stored.scores.device:
                out = self._targets[key] = SparseTokenLabelTarget(torch.empty(shape, dtype=torch.int32, device=stored.scores.device),
                                                                  torch.empty(shape, dtype=torch.float32, device=stored.scores.device))
        elif not (isinstance(out, SparseTokenLabelTarget) and tuple(out.idx.shape) == shape and out.idx.is_contiguous()
                  and out.val.is_contiguous() and out.idx.device == stored.scores.device):
            raise ValueError("DeviceLabelMapCrop.target: out must be a contiguous SparseTokenLabelTarget %s on the maps' device" % (shape,))
        out.smoothing = self.smoothing
        ops.label_map_crop(stored.scores, stored.classes, stored.labels, dev, P, self.k, self.num_classes, out=(out.idx, out.val),
                           host_records=host)
        return out


IMAGENET_MEAN = (0.485, 0.456, 0.406)
RANDAUG_OPS =("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast", "Brightness",
               "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")      # timm's _RAND_TRANSFORMS, in its order
_RA_MAX_LEVEL = 10.0
_RA_ENHANCE = {"Color": ops.RA_COLOR, "Contrast": ops.RA_CONTRAST, "Brightness": ops.RA_BRIGHTNESS, "Sharpness": ops.RA_SHARPNESS}
_RA_NO_MATRIX = (0.0,) * 6
RANDAUG_NONE = (ops.RA_NONE, 0, 0, 0.0, _RA_NO_MATRIX)                                 # the record of a skipped op


def parse_randaug_spec(spec):
    """'rand-m9-mstd0.5-inc1' -> dict(magnitude, n, mstd, inc); '' or None -> None (no auto-augment).  timm 0.4.5's
    rand_augment_transform: sections split at '-', the first is 'rand', each other one a key and a number: m (magnitude, int; 10 where it
    is missing), n (layers, default 2), mstd (float), inc (0 / 1: here inc0 selects the non-increasing level rules, where timm's
    `bool('0')` selects the increasing ones).  w (op weights) and any other key are refused with ValueError"""
    if spec is None or spec == "":
        return None
    parts = str(spec).split("-")
    if parts[0] != "rand":
        raise ValueError("DeviceRandAugment: a 'rand-...' spec, got %r (AutoAugment and AugMix policies are not implemented)" % (spec,))
    cfg = dict(magnitude=int(_RA_MAX_LEVEL), n=2, mstd=0.0, inc=False)
    for sec in parts[1:]:
        cs = re.split(r"(\d.*)", sec)
        if len(cs) < 2:
            raise ValueError("DeviceRandAugment: section %r of %r has no number" % (sec, spec))
        key, val = cs[:2]
        if key == "m":
            cfg["magnitude"] = int(val)
        elif key == "n":
            cfg["n"] = int(val)
        elif key == "mstd":
            cfg["mstd"] = float(val)
        elif key == "inc":
            cfg["inc"] = bool(int(val))
        elif key == "w":
            raise ValueError("DeviceRandAugment: op weights (%r) are not implemented: the ops are drawn uniformly" % (sec,))
        else:
            raise ValueError("DeviceRandAugment: unknown section %r of %r" % (sec, spec))
    if not 1 <= cfg["n"] <= ops.RANDAUG_MAX_LAYERS:
        raise ValueError("DeviceRandAugment: n must be 1..%d" % ops.RANDAUG_MAX_LAYERS)
    return cfg


class DeviceRandAugment:
    """timm 0.4.5's rand_augment_transform + RandAugment + AugmentOp as host-side draws and one device launch per layer
    (ops.randaug_u8, csrc/randaug.hip: every op byte for byte what Pillow makes of it).  In timm's transform chain the step sits between
    RandomResizedCropAndInterpolation + RandomHorizontalFlip and the normalisation: `aug(u8)` takes the uint8 [B,3,S,S] / [B,S,S,3] batch
    DeviceRandomResizedCrop.crop returns and gives a uint8 batch of the same shape, which DeviceBatchPrep.prep takes.  The input is not
    modified; the result lives in a buffer kept per shape and is overwritten by the next call at that shape.

    The decisions come from this object's own numpy.random.RandomState(seed) -- timm draws the ops with numpy -- and random.Random(seed)
    -- and everything else with `random` -- never from the global streams, and are written into the next slot of a ring of pinned record
    blocks that reaches the device in one small copy.  Per image, first the ops: RandomState.choice(15, n), uniform with replacement,
    over RANDAUG_OPS.  Then per op, in this order:
      1. prob < 1 and random() > prob: the op is skipped (a "none" record) and draws nothing more
      2. mag = gauss(magnitude, magnitude_std) if magnitude_std > 0 else magnitude, clipped to [0, 10]
      3. the level, with L = mag / 10 and neg(v) = -v if random() > 0.5 else v:
           Rotate neg(30 L) degrees; ShearX / ShearY neg(0.3 L); TranslateXRel / TranslateYRel neg(0.45 L) * S pixels;
           Color / Contrast / Brightness / Sharpness the factor 1.0 + neg(0.9 L) (inc0: 1.8 L + 0.1, no draw);
           Posterize 4 - int(4 L) bits (inc0: int(4 L)); Solarize the threshold 256 - int(256 L) (inc0: int(256 L));
           SolarizeAdd int(110 L); AutoContrast, Equalize and Invert draw nothing
      4. the five geometric ops: choice((bilinear, bicubic)), timm's _RANDOM_INTERPOLATION
    The affine matrices are built here in Python floats, as Pillow's Python layer does: ShearX (1, s, 0, 0, 1, 0), ShearY (1, 0, 0, s, 1, 0),
    TranslateX (1, 0, p, 0, 1, 0), TranslateY (1, 0, 0, 0, 1, p), Rotate Image.rotate's (a = -radians(deg % 360), entries rounded to 15
    digits, centred on (S / 2, S / 2); deg % 360 == 0 is a copy).  Enhance factors are stored as float32, as Pillow's C layer takes them.
    The fill colour of the geometric ops is timm's img_mean: tuple(min(255, round(255 x)) for x in mean).

    magnitude, magnitude_std and prob are plain attributes read at draw time (AutoProgDriver sets the magnitude per stage from the
    schedule's `aa` list through set_spec, where the reference rebuilds its loader and its worker processes); `last` holds the records of
    the last draw: per image a list of n_layers tuples (op, filter, int argument, factor, matrix) with op one of ops.RA_*.
    A spec of "" or None disables the object: `aug(u8)` then returns its input and draws nothing.
    Not implemented: op weights (w), mstd = inf (uniform magnitudes), the constant-pixel translate ops, AutoAugment and AugMix policies."""
    SLOTS = PinnedRing.SLOTS

    def __init__(self, spec="rand-m9-mstd0.5-inc1", mean=IMAGENET_MEAN, seed=0, layout="nchw", device="cuda"):
        self.prob = 0.5
        self.magnitude, self.magnitude_std, self.n_layers, self.increasing = int(_RA_MAX_LEVEL), 0.0, 2, False
        self.set_spec(spec)
        self.fill = tuple(min(255, round(255 * x)) for x in mean)
        self.seed, self.layout, self.device = int(seed), _layout(layout), torch.device(device)
        self._np = np.random.RandomState(self.seed & 0xffffffff)
        self._py = random.Random(self.seed)
        self._ring = PinnedRing(self.device)
        self._buffers = {}
        self.last = None

    def set_spec(self, spec):
        """takes magnitude, magnitude_std, n_layers and the level rules from a spec; "" / None disables the object and keeps them"""
        cfg = parse_randaug_spec(spec)
        self.spec, self.enabled = spec, cfg is not None
        if cfg is not None:
            self.magnitude, self.magnitude_std, self.n_layers, self.increasing = cfg["magnitude"], cfg["mstd"], cfg["n"], cfg["inc"]

    # ---- the draw
    def _neg(self, v):
        return -v if self._py.random() > 0.5 else v

    @staticmethod
    def rotate_matrix(deg, S):
        """Image.rotate's matrix for an S x S image about its centre; None where Pillow returns a copy"""
        deg = deg % 360.0
        if deg == 0:
            return None
        a = -math.radians(deg)
        m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
        c = S / 2.0
        m[2] = m[0] * -c + m[1] * -c + m[2] + c
        m[5] = m[3] * -c + m[4] * -c + m[5] + c
        return tuple(m)

    def _draw_op(self, name, S):
        py = self._py
        if self.prob < 1.0 and py.random() > self.prob:
            return RANDAUG_NONE
        mag = self.magnitude
        if self.magnitude_std > 0:
            mag = py.gauss(mag, self.magnitude_std)
        L = min(_RA_MAX_LEVEL, max(0, mag)) / _RA_MAX_LEVEL
        if name == "AutoContrast":
            return (ops.RA_AUTOCONTRAST, 0, 0, 0.0, _RA_NO_MATRIX)
        if name == "Equalize":
            return (ops.RA_EQUALIZE, 0, 0, 0.0, _RA_NO_MATRIX)
        if name == "Invert":
            return (ops.RA_INVERT, 0, 0, 0.0, _RA_NO_MATRIX)
        if name in _RA_ENHANCE:
            f = 1.0 + self._neg(L * 0.9) if self.increasing else L * 1.8 + 0.1
            return (_RA_ENHANCE[name], 0, 0, float(np.float32(f)), _RA_NO_MATRIX)
        if name == "Posterize":
            bits = 4 - int(L * 4) if self.increasing else int(L * 4)
            return (ops.RA_POSTERIZE, 0, bits, 0.0, _RA_NO_MATRIX) if bits < 8 else RANDAUG_NONE
        if name == "Solarize":
            return (ops.RA_SOLARIZE, 0, 256 - int(L * 256) if self.increasing else int(L * 256), 0.0, _RA_NO_MATRIX)
        if name == "SolarizeAdd":
            return (ops.RA_SOLARIZE_ADD, 0, int(L * 110), 0.0, _RA_NO_MATRIX)
        if name == "Rotate":
            m = self.rotate_matrix(self._neg(L * 30.0), S)
        elif name in ("ShearX", "ShearY"):
            s = self._neg(L * 0.3)
            m = (1.0, s, 0.0, 0.0, 1.0, 0.0) if name == "ShearX" else (1.0, 0.0, 0.0, s, 1.0, 0.0)
        elif name in ("TranslateXRel", "TranslateYRel"):
            p = self._neg(L * 0.45) * S
            m = (1.0, 0.0, p, 0.0, 1.0, 0.0) if name == "TranslateXRel" else (1.0, 0.0, 0.0, 0.0, 1.0, p)
        else:
            raise ValueError("unknown op %r" % (name,))
        filt = py.choice((ops.RESAMPLE_BILINEAR, ops.RESAMPLE_BICUBIC))      # drawn before Pillow decides that a rotation is a copy
        return (ops.RA_AFFINE, filt, 0, 0.0, tuple(float(v) for v in m)) if m is not None else RANDAUG_NONE

    @staticmethod
    def pack(records, block):
        """per-image lists of record tuples -> the int32 words of `block` (a numpy int32 array of B * n * 16 words at least)"""
        flat = [r for image in records for r in image]
        a = block[:len(flat) * ops.RANDAUG_RECORD_WORDS].reshape(len(flat), ops.RANDAUG_RECORD_WORDS)
        a[:] = 0
        if flat:
            a[:, 0:3] = [r[:3] for r in flat]
            a[:, 3:4].view(np.float32)[:, 0] = [r[3] for r in flat]
            a[:, 4:16].view(np.float64)[:] = [r[4] for r in flat]

    @staticmethod
    def unpack(block, B, n_layers):
        """the inverse of pack: -> per-image lists of n_layers record tuples"""
        a = np.ascontiguousarray(np.asarray(block).reshape(-1)[:B * n_layers * ops.RANDAUG_RECORD_WORDS]).reshape(B * n_layers, ops.RANDAUG_RECORD_WORDS)
        f, m = a[:, 3:4].view(np.float32)[:, 0], a[:, 4:16].view(np.float64)
        flat = [(int(a[i, 0]), int(a[i, 1]), int(a[i, 2]), float(f[i]), tuple(float(v) for v in m[i])) for i in range(B * n_layers)]
        return [flat[b * n_layers:(b + 1) * n_layers] for b in range(B)]

    def draw(self, B, S):
        """-> the host block (int32 CPU tensor, B x n_layers records of 16 words) of the next call on B images of S x S pixels"""
        n = int(self.n_layers)
        if not 1 <= n <= ops.RANDAUG_MAX_LAYERS:
            raise ValueError("DeviceRandAugment: n_layers must be 1..%d" % ops.RANDAUG_MAX_LAYERS)
        host = self._ring.next(max(B * n, 1) * ops.RANDAUG_RECORD_WORDS)
        # one call for the batch: RandomState.choice(15, B n) is the stream of B calls of choice(15, n) (32 bits and one rejection test
        # per element either way), without a numpy call per image on the host's critical path
        picks = self._np.choice(len(RANDAUG_OPS), B * n).reshape(B, n).tolist() if B else []
        draw_op = self._draw_op
        self.last = [[draw_op(RANDAUG_OPS[k], S) for k in image] for image in picks]
        self.pack(self.last, host.numpy())
        return host

    def __call__(self, u8):
        """uint8 device batch -> the augmented uint8 batch: draws n_layers ops per image, one copy and n_layers launches"""
        if not self.enabled:
            return u8
        B, S, W = _device_batch(u8, self.layout, "DeviceRandAugment")
        if S != W:
            raise ValueError("DeviceRandAugment: square images (the crop's output), got %s" % (tuple(u8.shape),))
        key = (tuple(u8.shape), u8.device)
        if key not in self._buffers:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("DeviceRandAugment: the buffers for %s do not exist yet: call the object once outside the capture" % (key[0],))
            self._buffers[key] = (torch.empty_like(u8, memory_format=torch.contiguous_format),
                                  torch.empty_like(u8, memory_format=torch.contiguous_format))
        out, scratch = self._buffers[key]
        host = self.draw(B, S)
        dev = self._ring.send(u8.device)
        return ops.randaug_u8(u8.contiguous(), dev, self.n_layers, self.fill, layout=self.layout, out=out, scratch=scratch, host_records=host)
