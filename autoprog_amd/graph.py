"""A training step as ONE HIP graph (missing 4; SURVEY.md section 8(f) row N2 / BASELINE configs[2]).

The early AutoProg stages -- (l, r) = (9, 128), (12, 160): main_prog.py:973-974 resizes every batch to the stage's resolution,
:1824-1836 picks a sub-network per step in a search -- are launch-gap bound on an MI355X: ~450 kernels of ~10 us each, and the GPU-side
gap between two dependent launches (~1.5 us) is a tenth of the kernel it precedes.  A graph replay removes those gaps (stage 1: 5.36 ->
4.25 ms per step, profiles/r04_exp_graph.txt).  What stood in the way was that a step reads HOST scalars that change every step:

    the mix-token box and its lam            models/volo.py:319-339, 649-658, 684-691 ; loss/cross_entropy.py:149-152
    the learning rate and Adam's bias corrections   main_prog.py:1019-1027 (scheduler writes param_groups[i]["lr"]; torch.optim.AdamW's step count)

DropPath's draws are device-side already (torch's generator is graph-safe: a replay advances its philox offset).  Here those scalars
live in a small DEVICE buffer (`StepScalars`: ABI 6 entry points ap_mix_token_swap_dev, ap_soft_ce_*_dev, the `step_scalars` argument of
ap_adamw_ema_step) that is refreshed by one 64-byte host-to-device copy in front of every replay; the host draws the box with the
same numpy calls in the same order as the eager forward, so a graphed run and an eager run with the same seeds see the same boxes.

    gs = GraphedStep(model, loss_fn, reducer, opt, images, target)      # static input buffers (copied from the given tensors)
    gs.capture()                                                        # warm-up steps on a side stream, then one captured step
    loss = gs.step(new_images, new_target)                              # copies the batch in, refreshes the scalars, replays

`images` may be a data.PreparedBatch (a loader's uint8 batch with the step's Mixup / CutMix / RandomErasing decisions) and `target` its
MixedLabelTarget: the static buffers are then the uint8 batch, the labels and the batch's parameter block.

One graph per elastic configuration: `set_sample_config` changes which kernels run, so the driver keeps a GraphedStep per (l, r).
Single-rank only (RCCL collectives are not captured here): with world > 1 the eager step runs."""
import numpy as np
import torch

from . import ops
from .ring import PinnedRing


CLIP_MODES = ("norm", "value", "agc")        # the reference's --clip-mode (main_prog.py:129-132)


class StepScalars:
    """the per-step host scalars of a training step in device memory.  Layout (16 x 4 bytes; include/autoprog_hip.h ap_step_scalars):
         int32 [0..3]  mix-token box on the token-label grid: bbx1, bbx2, bby1, bby2 (rows [bbx1, bbx2), columns [bby1, bby2))
         fp32  [4]     lam of the loss = 1 - box area / N
         fp32  [5..7]  learning rate, 1 - beta1^t, sqrt(1 - beta2^t)
       The host side is a ring.PinnedRing of 64-byte slots: push() is one asynchronous copy of the slot being prepared into the one
       device buffer, and begin() takes the next slot, so the host, which runs many replays ahead of the GPU (a replay costs it tens
       of microseconds, the step milliseconds), never overwrites step t's scalars before the copy of step t has run."""
    SLOTS = PinnedRing.SLOTS

    def __init__(self, device):
        self._ring = PinnedRing(device)
        self.dev = torch.zeros(16, dtype=torch.int32, device=device)
        self._take()
        self._hf[4] = 1.0
        self.push()

    def _take(self):
        self.host = self._ring.next(16)
        self._hf = self.host.view(torch.float32)

    @property
    def slot(self):
        return self._ring.slot

    def begin(self):
        """start preparing a step: the next slot of the ring, once the copy that last read it has executed; the values of the
        previous step carry over (a caller may set only the box or only the optimizer scalars)"""
        prev = self.host
        self._take()
        self.host.copy_(prev)

    @property
    def box_ptr(self):
        return self.dev.data_ptr()

    @property
    def lam_ptr(self):
        return self.dev.data_ptr() + 4 * 4

    @property
    def adam_ptr(self):
        return self.dev.data_ptr() + 5 * 4

    def set_box(self, box, n_tokens):
        bbx1, bby1, bbx2, bby2 = (int(v) for v in box)
        self.host[0], self.host[1], self.host[2], self.host[3] = bbx1, bbx2, bby1, bby2
        self._hf[4] = 1.0 - ((bbx2 - bbx1) * (bby2 - bby1) / float(n_tokens))
        self.box = (bbx1, bby1, bbx2, bby2)

    def set_adam(self, lr, beta1, beta2, step):
        # exactly what ap_adamw_ema_step derives from its float arguments (csrc/optim.hip): double arithmetic on the fp32-rounded betas
        b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
        self._hf[5] = float(lr)
        self._hf[6] = 1.0 - b1 ** int(step)
        self._hf[7] = float(np.sqrt(1.0 - b2 ** int(step)))

    def push(self):
        self.dev.copy_(self.host, non_blocking=True)
        self._ring.record()


class DeviceBox:
    """what a VOLO forward in graph mode returns in place of the (bbx1, bby1, bbx2, bby2) tuple: the loss reads lam from the device"""

    def __init__(self, scalars):
        self.scalars = scalars

    def __iter__(self):                      # callers that unpack the box get the host copy of the step being prepared
        return iter(self.scalars.box)


class GraphedStep:
    def __init__(self, model, loss_fn, reducer, opt, images, target, clip_grad=None, clip_mode="norm", skip_nonfinite=False):
        """skip_nonfinite: FlatAdamWEma.step's flag.  The guarded launch sequence reads its decision, its counters and Adam's step number
        from device memory (ap_guard_state), so a replay skips or applies like an eager step and needs no further per-step copy.
        clip_mode: 'norm' / 'value' go to FlatAdamWEma.step; 'agc' is opt.adaptive_clip_grad(clip_grad) between reducer.finish() and a
        step() without clip arguments (clip_grad is then timm's clip_factor).  Any other mode is refused here."""
        if clip_mode not in CLIP_MODES:
            raise ValueError("GraphedStep: clip_mode %r, expected one of %s" % (clip_mode, ", ".join(repr(m) for m in CLIP_MODES)))
        if getattr(reducer, "world", 1) > 1:
            raise ValueError("GraphedStep: single-rank only (the gradient exchange is not captured)")
        self.model, self.loss_fn, self.reducer, self.opt = model, loss_fn, reducer, opt
        self.clip_grad, self.clip_mode = clip_grad, clip_mode
        self._agc = clip_mode == "agc" and clip_grad is not None and float(clip_grad) > 0
        self.skip_nonfinite = bool(skip_nonfinite)
        # a data.PreparedBatch in place of the images: a static uint8 buffer and a static copy of the step's parameter block (mix mode, lam,
        # CutMix box, noise key, erase records), refreshed by ONE device copy in front of every replay; the loss reads lam from that block
        self.images = _clone_images(images)
        self.target = _clone_target(target, self.images)
        self.scalars = StepScalars(self.images.device)
        self.graph = None
        self.loss = None
        # the resolution of the elastic configuration this graph is built on (the model's at construction): a replay's mix-token draw is for THIS
        # configuration's token grid whatever configuration the model object was switched to since (a search replays a different graph every step)
        pe = getattr(model, "patch_embed", None)
        self._res = (getattr(pe, "resize_to", None) or self.images.shape[-1]) if pe is not None else self.images.shape[-1]

    # ---- host side of a step: the draws VOLO.forward makes (models/volo.py:649-653: beta, then rand_bbox's two randint calls)
    def _draw(self):
        m = self.model
        if getattr(m, "mix_token", False) and m.training:
            from .models.volo import rand_bbox
            r = self._res
            pe = m.patch_embed
            patch = pe.proj.kernel_size[0] * (pe.conv[0].stride[0] if pe.stem_conv else 1)
            g1 = r // patch                                       # token grid in front of the first stage (patch size 8 in every VOLO)
            lam = np.random.beta(m.beta, m.beta)
            box = rand_bbox((self.images.shape[0], g1, g1, 0), lam, scale=m.pooling_scale)
            n = (g1 // m.pooling_scale) ** 2
        else:
            box, n = (0, 0, 0, 0), 1
        self.scalars.set_box(box, n)

    def _prepare(self):
        self.scalars.begin()
        self._draw()
        o = self.opt
        g0 = o.param_groups[0]
        self.scalars.set_adam(float(g0["lr"]) * float(g0.get("lr_scale", 1.0)), o.betas[0], o.betas[1], o.step_count + 1)
        self.scalars.push()
        if getattr(o, "grouped", False):       # per-group rates and decays: the replay reads the table as it stands at THIS step
            o.push_groups()

    def _step_body(self):
        self.reducer.zero_grad()
        loss = self.loss_fn(self.model(self.images), self.target)
        loss.backward()
        self.reducer.finish()
        kw = {"skip_nonfinite": True} if self.skip_nonfinite else {}
        if self._agc:                                             # the slab is rewritten in front of the update, which then clips nothing
            self.opt.adaptive_clip_grad(self.clip_grad)
            self.opt.step(scalars=self.scalars, **kw)
        else:
            self.opt.step(clip_grad=self.clip_grad, clip_mode=self.clip_mode, scalars=self.scalars, **kw)
        return loss

    def capture(self, warmup=3):
        self.model.step_scalars = self.scalars
        # whatever this step's optimizer calls allocate on first use is never first allocated inside the capture (optim._outside_capture)
        self.opt.prepare_capture(self.images.device, clip_grad=self.clip_grad, clip_mode=self.clip_mode, skip_nonfinite=self.skip_nonfinite,
                                 agc=self._agc)
        # which optimizer launch the graph holds: the one with a parameter-group table or the one without; step() refuses to replay once
        # the optimizer's groups ask for the other launch
        self._grouped = bool(getattr(self.opt, "grouped", False))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self._prepare()
                self._step_body()
        torch.cuda.current_stream().wait_stream(s)
        rng = np.random.get_state()            # the capture prepares a step it does not run: its mix-token draw is handed back
        self._prepare()
        count = self.opt.step_count
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = self._step_body()
        self.opt.step_count = count            # the capture recorded a step, it did not run one
        np.random.set_state(rng)
        return self

    def step(self, images=None, target=None):
        if self.graph is None:
            raise RuntimeError("GraphedStep.step() before capture()")
        if bool(getattr(self.opt, "grouped", False)) != self._grouped:
            raise RuntimeError("GraphedStep.step(): the optimizer's parameter groups now need the %s launch, the graph holds the other one: "
                               "recapture" % ("grouped" if not self._grouped else "ungrouped"))
        if images is not None:
            _copy_images(self.images, images)
        if target is not None:
            _copy_target(self.target, target)
        self.model.step_scalars = self.scalars
        self._prepare()
        self.graph.replay()
        self.opt.step_count += 1
        return self.loss

    def release(self):
        if getattr(self.model, "step_scalars", None) is self.scalars:
            self.model.step_scalars = None


def _clone_images(images):
    from .data import PreparedBatch
    if isinstance(images, PreparedBatch):
        # (no host copy of the block: the records were checked when the batch was prepared, and a replay goes through no entry point)
        return PreparedBatch(images.u8.clone(), images.layout, images.table, images.block.clone(), None, images.mix, images.n_boxes,
                             images.erase_mode, images.lam, images.owner)
    return images.clone()


def _copy_images(dst, src):
    from .data import PreparedBatch
    if isinstance(dst, PreparedBatch):
        if not isinstance(src, PreparedBatch):
            raise TypeError("this graph was captured on a PreparedBatch")
        dst.u8.copy_(src.u8, non_blocking=True)
        dst.block.copy_(src.block, non_blocking=True)
        dst.lam = src.lam
    else:
        dst.copy_(src, non_blocking=True)


def _clone_target(t, images=None):
    from .data import MixedLabelTarget, PreparedBatch
    from .loss.cross_entropy import SparseTokenLabelTarget
    from .loss.distillation import DistillTarget
    if isinstance(t, DistillTarget):
        raise NotImplementedError("a DistillTarget cannot be captured yet: run the distillation step eagerly (use_graphs=False)")
    if isinstance(t, SparseTokenLabelTarget):
        return SparseTokenLabelTarget(t.idx.clone(), t.val.clone(), t.smoothing)
    if isinstance(t, MixedLabelTarget):
        if not isinstance(images, PreparedBatch):
            raise TypeError("a MixedLabelTarget goes with the PreparedBatch whose parameter block holds its lam")
        m = MixedLabelTarget(t.labels.clone(), t.lam, t.smoothing, t.num_classes, block=images.block)
        m.from_device = True                 # lam of the loss: word 1 of the static block (mix_lam_dev), whatever the replay's draw was
        return m
    return t.clone()


def _copy_target(dst, src):
    from .data import MixedLabelTarget
    from .loss.cross_entropy import SparseTokenLabelTarget
    if isinstance(dst, SparseTokenLabelTarget):
        dst.idx.copy_(src.idx, non_blocking=True)
        dst.val.copy_(src.val, non_blocking=True)
    elif isinstance(dst, MixedLabelTarget):
        dst.labels.copy_(src.labels, non_blocking=True)
        dst.lam = src.lam
    else:
        dst.copy_(src, non_blocking=True)
