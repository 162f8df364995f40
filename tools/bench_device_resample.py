"""The antialiased device crop (csrc/resample.hip, ops.crop_resample_u8: per-image box + Pillow's bilinear / bicubic resize + flip of a uint8
batch, one launch) beside the two-tap kernel it stands next to and the composition a user can write in torch today, in ONE process with the
cases alternated; then a volo_d1 training step at batch 128 with the antialiased random crop in front and with the two-tap crop in front.

    python tools/bench_device_resample.py [--out profiles/device_resample.txt] [--no-step] [--no-rows]

Rows: B = 128, canvases 256 x 256 and 512 x 512 -> S in {128, 160, 192, 224} and B = 64, canvas 512 x 512 -> 448; both layouts; both
filters; boxes from data.DeviceRandomResizedCrop's own seeded draws at scale (0.08, 1) and at (0.35, 1).  Per row
  kernel   one launch of ap_crop_resample_u8 (the records are on the device already, as they are for the other cases)
  two-tap  one launch of ap_crop_resize_u8 on the same boxes: what antialiasing costs, informational
  torch    per image: slice the box, .float(), F.interpolate(bilinear | bicubic, antialias=True, align_corners=False), flip, round, clamp,
           cast, write into the batch
microseconds per call over device events around a window of >= 0.15 s after warm-up calls of the same shape; every call takes the next of
several canvas batches, so that more than 600 MB are touched before one comes round again.  Three rounds, the cases interleaved inside
each; spread = (max - min) / min over the rounds.  Algorithmic bytes = the boxes' bytes in + the output's bytes out; their rate over the
kernel's time is printed beside the rate ap_calib_copy reaches in the same process (read + write of a 256 MiB buffer).  Taps = the
multiply-adds of the two passes without any redundancy, 3 S (h kw + S kh) per image with k = 2 sup0 max(extent / S, 1).

Condition for the kernel to exist: faster than the torch composition in every round of every row.  Everything else is recorded, not
gated, including how far torch's float antialias path is from Pillow's bytes."""
import argparse
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from bench_device_crop import ROTATE_BYTES, ROUNDS, WINDOW_S, copy_rate, window_us  # noqa: E402

FILTER_NAME = {1: "bilinear", 2: "bicubic"}


class Row:
    def __init__(self, torch, B, H, S, layout, scale, filt):
        from autoprog_amd.data import DeviceRandomResizedCrop
        self.B, self.H, self.S, self.layout, self.scale, self.filt = B, H, S, layout, scale, filt
        shape = (B, 3, H, H) if layout == "nchw" else (B, H, H, 3)
        self.sets = int(math.ceil(ROTATE_BYTES / (B * 3 * H * H))) + 1
        g = torch.Generator(device="cuda").manual_seed(H + S)
        self.u8 = [torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g) for _ in range(self.sets)]
        crop = DeviceRandomResizedCrop(scale=scale, seed=S, layout=layout, interpolation=FILTER_NAME[filt])
        self.rec = crop.draw(B, H, H).clone().cuda()
        self.boxes = list(crop.last)
        plain = self.rec.clone().view(-1, 8)
        plain[:, 5] = 0
        self.rec_plain = plain.view(-1)
        self.bytes = sum(h * w * 3 for _, _, h, w, _, _ in self.boxes) + B * S * S * 3
        sup = 2.0 * filt
        self.taps = sum(3 * S * (h * sup * max(w / S, 1.0) + S * sup * max(h / S, 1.0)) for _, _, h, w, _, _ in self.boxes)
        self.i = 0

    def _next(self):
        self.i = (self.i + 1) % self.sets
        return self.u8[self.i]

    def kernel(self, torch, ops):
        return ops.crop_resample_u8(self._next(), self.S, self.rec, layout=self.layout)

    def twotap(self, torch, ops):
        return ops.crop_resize_u8(self._next(), self.S, self.rec_plain, layout=self.layout)

    def torch(self, torch, ops):
        import torch.nn.functional as F
        u8, S, mode = self._next(), self.S, FILTER_NAME[self.filt]
        out = torch.empty((self.B, 3, S, S) if self.layout == "nchw" else (self.B, S, S, 3), dtype=torch.uint8, device="cuda")
        for b, (top, left, h, w, flip, _) in enumerate(self.boxes):
            box = u8[b, :, top:top + h, left:left + w] if self.layout == "nchw" else u8[b, top:top + h, left:left + w].permute(2, 0, 1)
            y = F.interpolate(box.float().unsqueeze(0), size=(S, S), mode=mode, align_corners=False, antialias=True)[0]
            if flip:
                y = y.flip(2)
            y = y.round_().clamp_(0, 255).to(torch.uint8)
            out[b] = y if self.layout == "nchw" else y.permute(1, 2, 0)
        return out


def bench_rows(torch, ops, out):
    rate = copy_rate(torch, ops)
    out("ap_calib_copy: %.0f GB/s (read + write of 256 MiB)" % (rate / 1e9))
    ok_all = True
    for B, H, sizes in ((128, 256, (128, 160, 192, 224)), (128, 512, (128, 160, 192, 224)), (64, 512, (448,))):
        for layout in ("nchw", "nhwc"):
            for S in sizes:
                for scale in ((0.08, 1.0), (0.35, 1.0)):
                    for filt in (1, 2):
                        r = Row(torch, B, H, S, layout, scale, filt)
                        variants = [("kernel", r.kernel), ("two-tap", r.twotap), ("torch", r.torch)]
                        iters = {}
                        for name, fn in variants:
                            for _ in range(2):
                                fn(torch, ops)
                            torch.cuda.synchronize()
                            iters[name] = max(3, int(math.ceil(WINDOW_S * 1e6 / window_us(torch, lambda: fn(torch, ops), 3))))
                        r.i = 0
                        k = r.kernel(torch, ops).int()
                        r.i = 0
                        d = (k - r.torch(torch, ops).int()).abs()
                        agree = "torch's float antialias path differs from the kernel's (Pillow's) bytes in %.2f %%, by at most %d" % (
                            100.0 * float((d > 0).float().mean()), int(d.max()))
                        del k, d
                        times = {name: [] for name, _ in variants}
                        for _ in range(ROUNDS):
                            for name, fn in variants:
                                times[name].append(window_us(torch, lambda: fn(torch, ops), iters[name]))
                        out("B %d  %s  %d -> %d  scale %s  %s: %.1f MB algorithmic, %.2f G taps (%d canvas batches); %s" % (
                            B, layout, H, S, scale, FILTER_NAME[filt], r.bytes / 1e6, r.taps / 1e9, r.sets, agree))
                        for name, _ in variants:
                            t = times[name]
                            out("    %-7s us per call, rounds 1-3: %s   spread %5.1f %%" % (name, "  ".join("%9.1f" % v for v in t), 100.0 * (max(t) - min(t)) / min(t)))
                        faster = all(kk < a for kk, a in zip(times["kernel"], times["torch"]))
                        ok_all = ok_all and faster
                        best = min(times["kernel"]) * 1e-6
                        out("    kernel faster than torch in every round: %s (torch / kernel = %s; kernel / two-tap = %s); %.0f GB/s algorithmic = %.1f %% of the copy "
                            "rate; %.2f T taps/s" % ("yes" if faster else "NO", "  ".join("%.1fx" % (a / kk) for kk, a in zip(times["kernel"], times["torch"])),
                                                   "  ".join("%.1fx" % (kk / a) for kk, a in zip(times["kernel"], times["two-tap"])),
                                                   r.bytes / best / 1e9, 100.0 * r.bytes / best / rate, r.taps / best / 1e12))
                        del r
                        torch.cuda.empty_cache()
    out("condition for merging (kernel faster than the torch composition in all three rounds of all rows): %s" % ("holds" if ok_all else "FAILS"))


def bench_step(torch, out, steps=10):
    """volo_d1, batch 128, a fixed sparse token-label target, eager: the step at (l, r) = (9, 128) and (18, 224) fed 512 x 512 uint8 canvases
    through DeviceRandomResizedCrop(interpolation="random").crop(u8, r) + DeviceBatchPrep.prep, against the same step with the two-tap crop
    (interpolation=None) in front"""
    from autoprog_amd.data import DeviceBatchPrep, DeviceRandomResizedCrop
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import SparseTokenLabelTarget, TokenLabelCrossEntropy
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import FlatAdamWEma
    torch.manual_seed(0)
    B = 128
    model = create_model("volo_d1", drop_path_rate=0.1).cuda().train()
    red = GradientBucketReducer(list(model.parameters()), world_size=1, defer_mean=True)
    red.install_sink(model)
    opt = FlatAdamWEma(model, red, lr=1e-3, weight_decay=0.05, ema_decays=[0.99996])
    loss_fn = TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=1000)
    prep = DeviceBatchPrep((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), re_prob=0.25, re_mode="pixel", seed=1)
    crops = {True: DeviceRandomResizedCrop(seed=2, interpolation="random"), False: DeviceRandomResizedCrop(seed=2)}
    g = torch.Generator(device="cuda").manual_seed(3)
    canvases = [torch.randint(0, 256, (B, 3, 512, 512), dtype=torch.uint8, device="cuda", generator=g) for _ in range(4)]
    for l, r in ((9, 128), (18, 224)):
        model.set_sample_config(dict(layer_num=l, min_layer_num=9, max_layer_num=18, input_size=r, token_label_size=r // 16))
        n = (r // 16) ** 2
        idx = torch.randint(0, 1000, (B, 2 + n, 5), generator=g, device="cuda", dtype=torch.int32)
        val = torch.rand(B, 2 + n, 5, generator=g, device="cuda").sort(-1, descending=True)[0]
        target = SparseTokenLabelTarget(idx, val / val.sum(-1, keepdim=True), smoothing=0.1)
        count = [0]

        def step(antialiased):
            count[0] += 1
            u8 = crops[antialiased].crop(canvases[count[0] % 4], r)
            red.zero_grad()
            loss_fn(model(prep.prep(u8)), target).backward()
            red.finish()
            opt.step()

        def window_ms(antialiased):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                step(antialiased)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / steps
        for antialiased in (True, False):
            for _ in range(4):
                step(antialiased)
        torch.cuda.synchronize()
        t = {True: [], False: []}
        for _ in range(ROUNDS):
            for antialiased in (True, False):
                t[antialiased].append(window_ms(antialiased))
        span = max(max(v) - min(v) for v in t.values())
        out("volo_d1 step at (l, r) = (%d, %d), batch 128, eager, 512 x 512 canvases, %d steps per window, rounds 1-3 (ms per step):" % (l, r, steps))
        out("    antialiased random crop in front: %s" % "  ".join("%.3f" % v for v in t[True]))
        out("    two-tap crop in front:            %s" % "  ".join("%.3f" % v for v in t[False]))
        out("    difference of the means %+.3f ms; run-to-run span %.3f ms" % (sum(t[True]) / ROUNDS - sum(t[False]) / ROUNDS, span))
    red.remove()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_resample.txt"))
    ap.add_argument("--no-step", action="store_true", help="the kernel rows only")
    ap.add_argument("--no-rows", action="store_true", help="the training steps only")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    assert torch.cuda.is_available(), "this benchmark measures an MI355X; there is nothing to report without one"
    from autoprog_amd import ops
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out("device: %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    out("tools/bench_device_resample.py: microseconds per call, windows of >= %.2f s, %d rounds with kernel / two-tap / torch interleaved" % (WINDOW_S, ROUNDS))
    if not args.no_rows:
        bench_rows(torch, ops, out)
    if not args.no_step:
        bench_step(torch, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
