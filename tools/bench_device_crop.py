"""The device crop (csrc/crop.hip, ops.crop_resize_u8: per-image box + flip + bilinear resize of a uint8 batch, one launch) beside the two
compositions a user can write in torch today, in ONE process with the cases alternated; then a volo_d1 training step at batch 128 with
the crop in front of it and with pre-cropped uint8 batches.

    python tools/bench_device_crop.py [--out profiles/device_crop.txt] [--no-step]

Rows: B = 128, canvas 256 x 256 -> S in {224, 192, 160, 128} and B = 64, canvas 512 x 512 -> 448; both layouts; boxes from
data.DeviceRandomResizedCrop's own seeded draws at scale (0.08, 1) and at (0.35, 1).  Per row
  kernel   one launch of ap_crop_resize_u8 (the records are on the device already, as they are for the torch cases)
  loop     per image: slice the box, .float(), F.interpolate(bilinear, align_corners=False), flip, round, clamp, cast, write into the batch
  grid     u8.float() + F.affine_grid + F.grid_sample(bilinear, border, align_corners=False) + round + clamp + cast (the affine matrices are
           built beforehand and not charged; this form reads across a box's border where the kernel clamps, so its bytes differ slightly)
microseconds per call over device events around a window of >= 0.15 s after warm-up calls of the same shape; every call takes the next of
several canvas batches, so that more than 600 MB are touched before one comes round again.  Three rounds, the cases interleaved inside
each; spread = (max - min) / min over the rounds.  Algorithmic bytes = the boxes' bytes in + the output's bytes out; their rate over the
kernel's time is printed as a fraction of the rate ap_calib_copy reaches in the same process (read + write of a 256 MiB buffer).

Condition for the kernel to exist: faster than both compositions in every round of every row.  The byte rate and the step pairs are
recorded, not gated."""
import argparse
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ROUNDS, WINDOW_S, ROTATE_BYTES = 3, 0.15, 600e6


def window_us(torch, fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def copy_rate(torch, ops):
    n = 256 << 20
    src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    for _ in range(3):
        ops.calib_copy(src, dst)
    return 2 * n / (min(window_us(torch, lambda: ops.calib_copy(src, dst), 20) for _ in range(3)) * 1e-6)


class Row:
    def __init__(self, torch, B, H, S, layout, scale):
        from autoprog_amd.data import DeviceRandomResizedCrop
        self.B, self.H, self.S, self.layout, self.scale = B, H, S, layout, scale
        shape = (B, 3, H, H) if layout == "nchw" else (B, H, H, 3)
        self.sets = int(math.ceil(ROTATE_BYTES / (B * 3 * H * H))) + 1
        g = torch.Generator(device="cuda").manual_seed(H + S)
        self.u8 = [torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g) for _ in range(self.sets)]
        crop = DeviceRandomResizedCrop(scale=scale, seed=S, layout=layout)
        self.host = crop.draw(B, H, H).clone()
        self.boxes = list(crop.last)
        self.rec = self.host.cuda()
        self.bytes = sum(h * w * 3 for _, _, h, w, _ in self.boxes) + B * S * S * 3
        # the affine matrices of `grid`: normalised source x = (2 cx / W - 1) + (w / W) x_out (negated slope when flipped), rows likewise
        th = torch.zeros(B, 2, 3)
        for b, (top, left, h, w, flip) in enumerate(self.boxes):
            th[b, 0, 0] = (-1.0 if flip else 1.0) * w / H
            th[b, 0, 2] = 2.0 * (left + w / 2.0) / H - 1.0
            th[b, 1, 1] = h / H
            th[b, 1, 2] = 2.0 * (top + h / 2.0) / H - 1.0
        self.theta = th.cuda()
        self.i = 0

    def _next(self):
        self.i = (self.i + 1) % self.sets
        return self.u8[self.i]

    def kernel(self, torch, ops):
        return ops.crop_resize_u8(self._next(), self.S, self.rec, layout=self.layout)

    def loop(self, torch, ops):
        import torch.nn.functional as F
        u8, S = self._next(), self.S
        out = torch.empty((self.B, 3, S, S) if self.layout == "nchw" else (self.B, S, S, 3), dtype=torch.uint8, device="cuda")
        for b, (top, left, h, w, flip) in enumerate(self.boxes):
            box = u8[b, :, top:top + h, left:left + w] if self.layout == "nchw" else u8[b, top:top + h, left:left + w].permute(2, 0, 1)
            y = F.interpolate(box.float().unsqueeze(0), size=(S, S), mode="bilinear", align_corners=False)[0]
            if flip:
                y = y.flip(2)
            y = y.round_().clamp_(0, 255).to(torch.uint8)
            out[b] = y if self.layout == "nchw" else y.permute(1, 2, 0)
        return out

    def grid(self, torch, ops):
        import torch.nn.functional as F
        u8, S = self._next(), self.S
        x = u8.float() if self.layout == "nchw" else u8.permute(0, 3, 1, 2).float()
        y = F.grid_sample(x, F.affine_grid(self.theta, (self.B, 3, S, S), align_corners=False), mode="bilinear", padding_mode="border", align_corners=False)
        y = y.round_().clamp_(0, 255).to(torch.uint8)
        return y if self.layout == "nchw" else y.permute(0, 2, 3, 1).contiguous()


def bench_rows(torch, ops, out):
    rate = copy_rate(torch, ops)
    out("ap_calib_copy: %.0f GB/s (read + write of 256 MiB)" % (rate / 1e9))
    ok_all = True
    for B, H, sizes in ((128, 256, (224, 192, 160, 128)), (64, 512, (448,))):
        for layout in ("nchw", "nhwc"):
            for S in sizes:
                for scale in ((0.08, 1.0), (0.35, 1.0)):
                    r = Row(torch, B, H, S, layout, scale)
                    variants = [("kernel", r.kernel), ("loop", r.loop), ("grid", r.grid)]
                    iters = {}
                    for name, fn in variants:
                        for _ in range(2):
                            fn(torch, ops)
                        torch.cuda.synchronize()
                        iters[name] = max(3, int(math.ceil(WINDOW_S * 1e6 / window_us(torch, lambda: fn(torch, ops), 3))))
                    r.i = 0
                    k = r.kernel(torch, ops).int()
                    r.i = 0
                    dl = (k - r.loop(torch, ops).int()).abs()
                    r.i = 0
                    dg = (k - r.grid(torch, ops).int()).abs()
                    agree = "kernel against loop: %.3f %% of bytes differ, max %d; against grid: %.3f %%, max %d" % (
                        100.0 * float((dl > 0).float().mean()), int(dl.max()), 100.0 * float((dg > 0).float().mean()), int(dg.max()))
                    del k, dl, dg
                    times = {name: [] for name, _ in variants}
                    for _ in range(ROUNDS):
                        for name, fn in variants:
                            times[name].append(window_us(torch, lambda: fn(torch, ops), iters[name]))
                    out("B %d  %s  %d -> %d  scale %s: %.1f MB algorithmic (%d canvas batches); %s" % (B, layout, H, S, scale, r.bytes / 1e6, r.sets, agree))
                    for name, _ in variants:
                        t = times[name]
                        out("    %-7s us per call, rounds 1-3: %s   spread %5.1f %%" % (name, "  ".join("%9.1f" % v for v in t), 100.0 * (max(t) - min(t)) / min(t)))
                    faster = all(kk < a and kk < b for kk, a, b in zip(times["kernel"], times["loop"], times["grid"]))
                    ok_all = ok_all and faster
                    out("    kernel faster than both in every round: %s (loop / kernel = %s; grid / kernel = %s); %.0f GB/s algorithmic = %.1f %% of the copy rate" % (
                        "yes" if faster else "NO", "  ".join("%.1fx" % (a / kk) for kk, a in zip(times["kernel"], times["loop"])),
                        "  ".join("%.1fx" % (a / kk) for kk, a in zip(times["kernel"], times["grid"])),
                        r.bytes / min(times["kernel"]) / 1e3, 100.0 * r.bytes / (min(times["kernel"]) * 1e-6) / rate))
                    del r
                    torch.cuda.empty_cache()
    out("condition for merging (kernel faster than both torch compositions in all three rounds of all rows): %s" % ("holds" if ok_all else "FAILS"))


def bench_step(torch, out, steps=10):
    """volo_d1, batch 128, a fixed sparse token-label target, eager: the step at (l, r) = (9, 128) and (18, 224) fed 256 x 256 uint8 canvases
    through DeviceRandomResizedCrop.crop(u8, r) + DeviceBatchPrep.prep, against the same step fed uint8 batches that are r x r already"""
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
    crop = DeviceRandomResizedCrop(seed=2)
    g = torch.Generator(device="cuda").manual_seed(3)
    canvases = [torch.randint(0, 256, (B, 3, 256, 256), dtype=torch.uint8, device="cuda", generator=g) for _ in range(4)]
    for l, r in ((9, 128), (18, 224)):
        model.set_sample_config(dict(layer_num=l, min_layer_num=9, max_layer_num=18, input_size=r, token_label_size=r // 16))
        n = (r // 16) ** 2
        idx = torch.randint(0, 1000, (B, 2 + n, 5), generator=g, device="cuda", dtype=torch.int32)
        val = torch.rand(B, 2 + n, 5, generator=g, device="cuda").sort(-1, descending=True)[0]
        target = SparseTokenLabelTarget(idx, val / val.sum(-1, keepdim=True), smoothing=0.1)
        small = [torch.randint(0, 256, (B, 3, r, r), dtype=torch.uint8, device="cuda", generator=g) for _ in range(4)]
        count = [0]

        def step(cropped):
            count[0] += 1
            u8 = crop.crop(canvases[count[0] % 4], r) if cropped else small[count[0] % 4]
            red.zero_grad()
            loss_fn(model(prep.prep(u8)), target).backward()
            red.finish()
            opt.step()

        def window_ms(cropped):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                step(cropped)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / steps
        for cropped in (True, False):
            for _ in range(4):
                step(cropped)
        torch.cuda.synchronize()
        t = {True: [], False: []}
        for _ in range(ROUNDS):
            for cropped in (True, False):
                t[cropped].append(window_ms(cropped))
        span = max(max(v) - min(v) for v in t.values())
        out("volo_d1 step at (l, r) = (%d, %d), batch 128, eager, %d steps per window, rounds 1-3 (ms per step):" % (l, r, steps))
        out("    crop of 256 x 256 canvases in front: %s" % "  ".join("%.3f" % v for v in t[True]))
        out("    uint8 batches at r already:          %s" % "  ".join("%.3f" % v for v in t[False]))
        out("    difference of the means %+.3f ms; run-to-run span %.3f ms" % (sum(t[True]) / ROUNDS - sum(t[False]) / ROUNDS, span))
    red.remove()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_crop.txt"))
    ap.add_argument("--no-step", action="store_true", help="the kernel rows only")
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
    out("tools/bench_device_crop.py: microseconds per call, windows of >= %.2f s, %d rounds with kernel / loop / grid interleaved" % (WINDOW_S, ROUNDS))
    bench_rows(torch, ops, out)
    if not args.no_step:
        bench_step(torch, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
