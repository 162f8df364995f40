"""Device RandAugment (csrc/randaug.hip, ops.randaug_u8: n_layers launches over a uint8 batch, every op byte for byte Pillow's) beside a
device copy of the same bytes and beside Pillow applying the same records on 16 CPU threads, in ONE process with the cases alternated;
then a volo_d1 training step at batch 128 with crop + prep in front, with and without the augment step between them.

    python tools/bench_device_randaug.py [--out profiles/device_randaug.txt] [--no-step] [--no-rows] [--no-pillow]

Rows: B = 128, S in {224, 128}, both layouts.  Per row
  natural   the launch pair on records drawn by data.DeviceRandAugment("rand-m9-mstd0.5-inc1") from its seed: the spec's own op mix, about
            half the records "none" (prob = 0.5)
  worst     the launch pair with every image a bicubic Rotate by 30 degrees, twice
  copy      two device copies of the batch (ap_calib_copy), the bytes the pair moves at the least: read + write, twice
  pillow    the natural records applied image by image through Pillow (the calls timm's auto_augment.py makes) on 16 threads, host clock
and for S = 224, NCHW, one launch with every image the same op (table, statistics, Color, Sharpness, bilinear and bicubic Rotate): which
ops run at the copy's pace and which are bound by instruction issue.
Microseconds per call over device events around a window of >= 0.15 s after warm-up calls of the same shape; every call takes the next
of several input batches, so that more than 600 MB are touched before one comes round again.  Three rounds, the cases interleaved inside
each; spread = (max - min) / min over the rounds.  Nothing is gated: nobody had timed this before, the file records what was measured."""
import argparse
import math
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from bench_device_crop import ROTATE_BYTES, ROUNDS, WINDOW_S, copy_rate, window_us  # noqa: E402

SPEC = "rand-m9-mstd0.5-inc1"
FILL = (124, 116, 104)
THREADS = 16


def pillow_apply(img, recs):
    """one uint8 [S,S,3] image through its records with the calls timm makes"""
    from PIL import Image, ImageEnhance, ImageOps
    from autoprog_amd import ops
    enh = {ops.RA_BRIGHTNESS: ImageEnhance.Brightness, ops.RA_CONTRAST: ImageEnhance.Contrast, ops.RA_COLOR: ImageEnhance.Color,
           ops.RA_SHARPNESS: ImageEnhance.Sharpness}
    im = Image.fromarray(img, "RGB")
    for op, filt, iarg, farg, m in recs:
        if op == ops.RA_AUTOCONTRAST:
            im = ImageOps.autocontrast(im)
        elif op == ops.RA_EQUALIZE:
            im = ImageOps.equalize(im)
        elif op == ops.RA_INVERT:
            im = ImageOps.invert(im)
        elif op == ops.RA_SOLARIZE:
            im = im.point([i if i < iarg else 255 - i for i in range(256)] * 3)
        elif op == ops.RA_SOLARIZE_ADD:
            im = im.point([min(255, i + iarg) if i < 128 else i for i in range(256)] * 3)
        elif op == ops.RA_POSTERIZE:
            im = ImageOps.posterize(im, iarg)
        elif op in enh:
            im = enh[op](im).enhance(farg)
        elif op == ops.RA_AFFINE:
            im = im.transform(im.size, Image.AFFINE, m, resample=Image.BICUBIC if filt == ops.RESAMPLE_BICUBIC else Image.BILINEAR, fillcolor=FILL)
    return im


class Row:
    def __init__(self, torch, B, S, layout):
        from autoprog_amd import ops
        from autoprog_amd.data import DeviceRandAugment
        self.B, self.S, self.layout = B, S, layout
        shape = (B, 3, S, S) if layout == "nchw" else (B, S, S, 3)
        self.sets = int(math.ceil(ROTATE_BYTES / (B * 3 * S * S))) + 1
        g = torch.Generator(device="cuda").manual_seed(S)
        self.u8 = [torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g) for _ in range(self.sets)]
        self.out, self.scratch = torch.empty_like(self.u8[0]), torch.empty_like(self.u8[0])
        aug = DeviceRandAugment(SPEC, seed=S, layout=layout)
        self.natural = aug.draw(B, S).clone().cuda()
        self.records = aug.last
        rot = (ops.RA_AFFINE, ops.RESAMPLE_BICUBIC, 0, 0.0, DeviceRandAugment.rotate_matrix(30.0, S))
        self.worst = self.block(torch, [[rot, rot]] * B)
        self.bytes = 2 * 2 * B * 3 * S * S
        self.i = 0

    @staticmethod
    def block(torch, records):
        from autoprog_amd import ops
        from autoprog_amd.data import DeviceRandAugment
        t = torch.zeros(len(records) * len(records[0]) * ops.RANDAUG_RECORD_WORDS, dtype=torch.int32)
        DeviceRandAugment.pack(records, t.numpy())
        return t.cuda()

    def _next(self):
        self.i = (self.i + 1) % self.sets
        return self.u8[self.i]

    def run(self, ops, block, n=2):
        return ops.randaug_u8(self._next(), block, n, FILL, layout=self.layout, out=self.out, scratch=self.scratch)

    def copy(self, ops):
        ops.calib_copy(self._next(), self.scratch)
        ops.calib_copy(self.scratch, self.out)

    def pillow_ms(self, pool):
        import numpy as np
        host = self.u8[0].cpu().numpy()
        host = host.transpose(0, 2, 3, 1) if self.layout == "nchw" else host
        imgs = [np.ascontiguousarray(h) for h in host]
        t0 = time.perf_counter()
        list(pool.map(lambda a: np.asarray(pillow_apply(*a)), zip(imgs, self.records)))
        return (time.perf_counter() - t0) * 1e3


def timed(torch, variants, out, label):
    iters = {}
    for name, fn in variants:
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        iters[name] = max(3, int(math.ceil(WINDOW_S * 1e6 / window_us(torch, fn, 3))))
    times = {name: [] for name, _ in variants}
    for _ in range(ROUNDS):
        for name, fn in variants:
            times[name].append(window_us(torch, fn, iters[name]))
    out(label)
    for name, _ in variants:
        t = times[name]
        out("    %-16s us per call, rounds 1-3: %s   spread %5.1f %%" % (name, "  ".join("%9.1f" % v for v in t), 100.0 * (max(t) - min(t)) / min(t)))
    return times


def bench_rows(torch, ops, out, with_pillow):
    from collections import Counter
    rate = copy_rate(torch, ops)
    out("ap_calib_copy: %.0f GB/s (read + write of 256 MiB)" % (rate / 1e9))
    pool = None
    if with_pillow:
        try:
            import PIL
            from concurrent.futures import ThreadPoolExecutor
            pool = ThreadPoolExecutor(THREADS)
            out("Pillow %s on %d threads" % (PIL.__version__, THREADS))
        except ImportError:
            out("Pillow does not import here: the pillow rows are not measured")
    names = ["none", "AutoContrast", "Equalize", "Invert", "Solarize", "SolarizeAdd", "Posterize", "Brightness", "Contrast", "Color", "Sharpness", "Affine"]
    for S in (224, 128):
        for layout in ("nchw", "nhwc"):
            r = Row(torch, 128, S, layout)
            mix = Counter(names[rec[0]] + ("" if rec[0] != ops.RA_AFFINE else (" bicubic" if rec[1] == 2 else " bilinear")) for image in r.records for rec in image)
            t = timed(torch, [("natural", lambda: r.run(ops, r.natural)), ("worst", lambda: r.run(ops, r.worst)), ("copy", lambda: r.copy(ops))], out,
                      "B 128  %s  S %d  n_layers 2: %.1f MB moved by the pair at the least (%d input batches); natural mix: %s" % (
                          layout, S, r.bytes / 1e6, r.sets, ", ".join("%s %d" % kv for kv in sorted(mix.items()))))
            for name in ("natural", "worst"):
                best = min(t[name]) * 1e-6
                out("    %s: %.0f GB/s over the pair's least bytes = %.1f %% of the copy rate; %.1fx the two copies" % (
                    name, r.bytes / best / 1e9, 100.0 * r.bytes / best / rate, min(t[name]) / min(t["copy"])))
            if pool is not None:
                ms = [r.pillow_ms(pool) for _ in range(ROUNDS)]
                out("    pillow (%d threads, host clock) ms per batch, rounds 1-3: %s; over the natural pair: %.0fx" % (
                    THREADS, "  ".join("%8.1f" % v for v in ms), min(ms) * 1e3 / min(t["natural"])))
            if S == 224 and layout == "nchw":
                from autoprog_amd.data import DeviceRandAugment
                m = DeviceRandAugment.rotate_matrix(30.0, S)
                single = [("Invert (table)", (ops.RA_INVERT, 0, 0, 0.0, (0.0,) * 6)), ("Equalize (stats)", (ops.RA_EQUALIZE, 0, 0, 0.0, (0.0,) * 6)),
                          ("Contrast (stats)", (ops.RA_CONTRAST, 0, 0, 1.9, (0.0,) * 6)), ("Color", (ops.RA_COLOR, 0, 0, 1.9, (0.0,) * 6)),
                          ("Sharpness", (ops.RA_SHARPNESS, 0, 0, 1.9, (0.0,) * 6)), ("Rotate bilinear", (ops.RA_AFFINE, 1, 0, 0.0, m)),
                          ("Rotate bicubic", (ops.RA_AFFINE, 2, 0, 0.0, m))]
                blocks = [(name, Row.block(torch, [[rec]] * 128)) for name, rec in single]
                variants = [(name, (lambda b: lambda: r.run(ops, b, 1))(b)) for name, b in blocks] + [("one copy", lambda: ops.calib_copy(r._next(), r.out))]
                timed(torch, variants, out, "B 128  nchw  S 224  ONE launch, every image the same op (19.3 MB read + 19.3 MB written):")
            del r
            torch.cuda.empty_cache()


def bench_step(torch, out, steps=10):
    """volo_d1, batch 128, a fixed sparse token-label target, eager: the step at (l, r) = (9, 128) and (18, 224) fed 256 x 256 uint8 canvases
    through DeviceRandomResizedCrop(interpolation="random").crop(u8, r) + DeviceBatchPrep.prep, with DeviceRandAugment between them and
    without it"""
    from autoprog_amd.data import DeviceBatchPrep, DeviceRandAugment, DeviceRandomResizedCrop
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
    crop = DeviceRandomResizedCrop(seed=2, interpolation="random")
    aug = DeviceRandAugment(SPEC, seed=3)
    g = torch.Generator(device="cuda").manual_seed(3)
    canvases = [torch.randint(0, 256, (B, 3, 256, 256), dtype=torch.uint8, device="cuda", generator=g) for _ in range(8)]
    for l, r in ((9, 128), (18, 224)):
        model.set_sample_config(dict(layer_num=l, min_layer_num=9, max_layer_num=18, input_size=r, token_label_size=r // 16))
        n = (r // 16) ** 2
        idx = torch.randint(0, 1000, (B, 2 + n, 5), generator=g, device="cuda", dtype=torch.int32)
        val = torch.rand(B, 2 + n, 5, generator=g, device="cuda").sort(-1, descending=True)[0]
        target = SparseTokenLabelTarget(idx, val / val.sum(-1, keepdim=True), smoothing=0.1)
        count = [0]

        def step(augmented):
            count[0] += 1
            u8 = crop.crop(canvases[count[0] % 8], r)
            if augmented:
                u8 = aug(u8)
            red.zero_grad()
            loss_fn(model(prep.prep(u8)), target).backward()
            red.finish()
            opt.step()

        def window_ms(augmented):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                step(augmented)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / steps
        for augmented in (True, False):
            for _ in range(4):
                step(augmented)
        torch.cuda.synchronize()
        t = {True: [], False: []}
        for _ in range(ROUNDS):
            for augmented in (True, False):
                t[augmented].append(window_ms(augmented))
        span = max(max(v) - min(v) for v in t.values())
        out("volo_d1 step at (l, r) = (%d, %d), batch 128, eager, 256 x 256 canvases, %d steps per window, rounds 1-3 (ms per step):" % (l, r, steps))
        out("    crop + augment + prep in front: %s" % "  ".join("%.3f" % v for v in t[True]))
        out("    crop + prep in front:           %s" % "  ".join("%.3f" % v for v in t[False]))
        out("    difference of the means %+.3f ms; run-to-run span %.3f ms" % (sum(t[True]) / ROUNDS - sum(t[False]) / ROUNDS, span))
    red.remove()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_randaug.txt"))
    ap.add_argument("--no-step", action="store_true", help="the kernel rows only")
    ap.add_argument("--no-rows", action="store_true", help="the training steps only")
    ap.add_argument("--no-pillow", action="store_true", help="skip the CPU rows")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    assert torch.cuda.is_available(), "this benchmark measures an MI355X; there is nothing to report without one"
    from autoprog_amd import _lib, ops
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out("device: %s   torch %s   library %s" % (torch.cuda.get_device_name(0), torch.__version__, os.path.relpath(_lib.LIB_PATH, ROOT)))
    out("tools/bench_device_randaug.py: microseconds per call, windows of >= %.2f s, %d rounds with the cases interleaved" % (WINDOW_S, ROUNDS))
    if not args.no_rows:
        bench_rows(torch, ops, out, not args.no_pillow)
    if not args.no_step:
        bench_step(torch, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
