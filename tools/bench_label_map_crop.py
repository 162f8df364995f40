"""Token labels from stored maps (csrc/labelmap.hip, ops.label_map_crop) beside a device copy of the bytes it moves and beside the torch
composition of the same result, in ONE process with the cases alternated; then a VOLO-D1 training step at batch 128 with the device crop
and the batch preparation in front, on a fixed sparse target and with one label-map launch per step.

    python tools/bench_label_map_crop.py [--out profiles/label_map_crop.txt] [--no-step]

Shapes: B = 128 images, Kin = 5, 18 x 18 maps in fp16 (tlt's [B, 2, 5, 18, 18] tensor), C = 1000, K = 5 and 8, P = 8 and 14.  Per shape
  kernel   one launch of ap_label_map_crop into a [128, 2 + P P, K] target, with `dropped`
  copy     ops.calib_copy of as many bytes as the launch reads plus writes (maps, records, labels; idx, val, dropped)
  torch    scatter_add of the maps into a dense [B, C, 18, 18], two batched matmuls with the separable ROI-align weight matrices of the
           boxes (built on the host beforehand, outside the timing), topk, and the writes into the same target
microseconds per launch over device events around a window of >= 0.3 s; every launch takes the next of several operand sets (maps, records
and outputs of their own), so that more than 600 MB are touched before a set comes round again (the 256-MiB Infinity Cache holds none of
it).  Three rounds, the cases interleaved inside each.

The maps are synthetic: every image draws 8 classes, every pixel ranks them by smooth random fields and keeps the best five with scores
that fall off geometrically, so neighbouring pixels mostly share their classes, as stored label maps do.  The boxes are the draws of a
seeded DeviceRandomResizedCrop on 256 x 256 canvases.  `dropped` is reported per slot kind as a share of the bin's whole score mass.

Expectation (nobody has measured this before): the launch beats the torch composition in every round, and the step moves by no more
than its run-to-run span."""
import argparse
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ROUNDS, WINDOW_S, ROTATE_BYTES = 3, 0.3, 600e6
B_IMG, KIN, HM, WM, C_CLS = 128, 5, 18, 18, 1000
BOX_SETS = 8


def synthetic_maps(torch, sets, gen):
    """-> fp16 [sets, B, 2, Kin, Hm, Wm] on the device"""
    out = torch.empty(sets, B_IMG, 2, KIN, HM, WM, dtype=torch.float16, device="cuda")
    fall = torch.tensor([0.5, 0.2, 0.1, 0.05, 0.03], device="cuda").view(1, KIN, 1, 1)
    for s in range(sets):
        pool = torch.rand(B_IMG, C_CLS, device="cuda", generator=gen).argsort(dim=1)[:, :8]                              # [B, 8] distinct classes
        field = torch.nn.functional.interpolate(torch.randn(B_IMG, 8, 5, 5, device="cuda", generator=gen), size=(HM, WM), mode="bilinear")
        order = (field + 0.3 * torch.randn(B_IMG, 8, HM, WM, device="cuda", generator=gen)).argsort(dim=1, descending=True)[:, :KIN]
        out[s, :, 1] = torch.gather(pool.view(B_IMG, 8, 1, 1).expand(-1, -1, HM, WM), 1, order).to(torch.float16)
        out[s, :, 0] = (fall * (0.75 + 0.5 * torch.rand(B_IMG, KIN, HM, WM, device="cuda", generator=gen))).to(torch.float16)
    return out


def axis_weights(np, a1, a2, flip, pn, n):
    """the separable ROI-align weights of one axis, fp64 [B, pn, n]: W[b, p, x] = (1 / g) sum over the samples of bin p of pixel x's share;
    the bins of a flipped image are stored in reverse order (columns only: the caller passes flip = 0 for rows)"""
    Bn = len(a1)
    W = np.zeros((Bn, pn, n))
    for b in range(Bn):
        roi = max(float(a2[b]) - float(a1[b]), 1.0)
        bin_, g = roi / pn, int(math.ceil(roi / pn))
        for p in range(pn):
            for i in range(g):
                v = float(a1[b]) + p * bin_ + (i + 0.5) * bin_ / g
                if v < -1.0 or v > n:
                    continue
                v = max(v, 0.0)
                lo = int(v)
                if lo >= n - 1:
                    lo = hi = n - 1
                    v = float(lo)
                else:
                    hi = lo + 1
                q = pn - 1 - p if flip[b] else p
                W[b, q, lo] += (1.0 - (v - lo)) / g
                W[b, q, hi] += (v - lo) / g
    return W


class Shape:
    def __init__(self, torch, np, P, K, maps, records_host):
        self.P, self.K, self.maps = P, K, maps
        self.sets = maps.shape[0]
        slots = 2 + P * P
        self.idx = torch.zeros(self.sets, B_IMG, slots, K, dtype=torch.int32, device="cuda")
        self.val = torch.zeros(self.sets, B_IMG, slots, K, dtype=torch.float32, device="cuda")
        self.drp = torch.zeros(self.sets, B_IMG, slots - 1, dtype=torch.float32, device="cuda")
        self.labels = torch.randint(0, C_CLS, (B_IMG,), device="cuda")
        self.records_host = records_host                                       # BOX_SETS host blocks [B * 8]
        self.records = [r.cuda() for r in records_host]
        self.bytes_in = maps[0].numel() * 2 + B_IMG * 8 * 4 + B_IMG * 8
        self.bytes_out = self.idx[0].numel() * 4 + self.val[0].numel() * 4 + self.drp[0].numel() * 4
        nb = (self.bytes_in + self.bytes_out + 15) // 16 * 16
        self.copy_sets = int(math.ceil(ROTATE_BYTES / (2 * nb))) + 1
        self.src = torch.zeros(self.copy_sets, nb, dtype=torch.uint8, device="cuda")
        self.dst = torch.zeros(self.copy_sets, nb, dtype=torch.uint8, device="cuda")
        # the weight matrices of the torch composition, bins 0 .. P-1 the token grid and bin P the class slot; columns flipped with the image
        self.Wy, self.WxT = [], []
        for r in records_host:
            a = r.numpy().reshape(B_IMG, 8)
            none = np.zeros(B_IMG)
            wy = np.concatenate([axis_weights(np, a[:, 1], a[:, 3], none, P, HM), axis_weights(np, a[:, 1], a[:, 3], none, 1, HM)], axis=1)
            wx = np.concatenate([axis_weights(np, a[:, 0], a[:, 2], a[:, 4], P, WM), axis_weights(np, a[:, 0], a[:, 2], none, 1, WM)], axis=1)
            self.Wy.append(torch.from_numpy(wy).float().cuda().view(B_IMG, 1, P + 1, HM))
            self.WxT.append(torch.from_numpy(wx).float().cuda().transpose(1, 2).contiguous().view(B_IMG, 1, WM, P + 1))
        self.i = 0

    def _next(self):
        self.i = (self.i + 1) % self.sets
        return self.i

    def kernel(self, torch, ops):
        i = self._next()
        m, j = self.maps[i], i % BOX_SETS
        ops.label_map_crop(m[:, 0], m[:, 1], self.labels, self.records[j], self.P, self.K, C_CLS, out=(self.idx[i], self.val[i]),
                           dropped=self.drp[i], host_records=self.records_host[j])

    def torch_composition(self, torch, ops):
        i = self._next()
        m, j, P, K = self.maps[i], i % BOX_SETS, self.P, self.K
        dense = torch.zeros(B_IMG, C_CLS, HM * WM, dtype=torch.float32, device="cuda")
        dense.scatter_add_(1, m[:, 1].reshape(B_IMG, KIN, HM * WM).long(), m[:, 0].reshape(B_IMG, KIN, HM * WM).float())
        t = torch.matmul(torch.matmul(self.Wy[j], dense.view(B_IMG, C_CLS, HM, WM)), self.WxT[j])           # [B, C, P + 1, P + 1]
        rows = torch.cat([t[:, :, P, P].unsqueeze(2), t[:, :, :P, :P].reshape(B_IMG, C_CLS, P * P)], dim=2).transpose(1, 2)
        v, k = rows.topk(K, dim=2)
        idx, val = self.idx[i], self.val[i]
        idx[:, 1:] = torch.where(v > 0, k, -1)
        val[:, 1:] = v
        idx[:, 0] = -1
        idx[:, 0, 0] = self.labels
        val[:, 0] = 0
        val[:, 0, 0] = 1
        self.drp[i] = rows.sum(2) - v.sum(2)

    def copy(self, torch, ops):
        self.i = (self.i + 1) % self.copy_sets
        ops.calib_copy(self.src[self.i], self.dst[self.i])


def window_us(torch, fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def draw_records(torch, n):
    """n host blocks of B box records: the draws of a seeded DeviceRandomResizedCrop on 256 x 256 canvases, in map pixel units"""
    from autoprog_amd.data import DeviceLabelMapCrop, DeviceRandomResizedCrop
    crop, lm = DeviceRandomResizedCrop(seed=0, device="cpu"), DeviceLabelMapCrop(k=8)
    out = []
    for _ in range(n):
        crop.draw(B_IMG, 256, 256)
        out.append(lm.records(crop, B_IMG, HM, WM).clone())
    return out


def bench_shapes(torch, np, ops, out):
    gen = torch.Generator(device="cuda").manual_seed(0)
    records_host = draw_records(torch, BOX_SETS)
    ok_all = True
    size = lambda P, K: B_IMG * 2 * KIN * HM * WM * 2 + B_IMG * (2 + P * P) * K * 8 + B_IMG * (1 + P * P) * 4
    all_maps = synthetic_maps(torch, int(math.ceil(ROTATE_BYTES / size(8, 5))) + 1, gen)       # (the shape with the smallest outputs takes the most sets)
    for P in (8, 14):
        for K in (5, 8):
            per_set = size(P, K)
            sets = int(math.ceil(ROTATE_BYTES / per_set)) + 1
            s = Shape(torch, np, P, K, all_maps[:sets], records_host)
            variants = [("kernel", s.kernel), ("copy", s.copy), ("torch", s.torch_composition)]
            iters = {}
            for name, fn in variants:
                for _ in range(2):
                    fn(torch, ops)
                torch.cuda.synchronize()
                iters[name] = max(3, int(math.ceil(WINDOW_S * 1e6 / window_us(torch, lambda: fn(torch, ops), 3))))
            # the two forms on one operand set
            s.i = 0
            s.kernel(torch, ops)
            ik, vk, dk = s.idx[1].clone(), s.val[1].clone(), s.drp[1].clone()
            s.i = 0
            s.torch_composition(torch, ops)
            rel = ((vk - s.val[1]).abs() / s.val[1].clamp_min(1e-30)).max()
            out("P = %d, K = %d: %d operand sets of %.2f MB (%.0f KB read, %.0f KB written per launch)" % (
                P, K, sets, per_set / 1e6, s.bytes_in / 1e3, s.bytes_out / 1e3))
            out("    kernel against torch on one operand set: %.4f%% of the indices differ (near-ties: fp32 sums in another order), scores max rel diff %.2e, "
                "dropped max |diff| %.2e" % (100.0 * float((ik != s.idx[1]).float().mean()), float(rel), float((dk - s.drp[1]).abs().max())))
            total = s.val[1][:, 1:].sum(2) + dk
            share = dk / total.clamp_min(1e-30)
            out("    dropped / whole score mass of the bin on these maps: class slot mean %.4f max %.4f; token slots mean %.4f max %.4f; bins that dropped "
                "anything: class %.1f%%, token %.1f%%" % (float(share[:, 0].mean()), float(share[:, 0].max()), float(share[:, 1:].mean()),
                                                        float(share[:, 1:].max()), 100.0 * float((dk[:, 0] > 0).float().mean()),
                                                        100.0 * float((dk[:, 1:] > 0).float().mean())))
            times = {name: [] for name, _ in variants}
            for _ in range(ROUNDS):
                for name, fn in variants:
                    times[name].append(window_us(torch, lambda: fn(torch, ops), iters[name]))
            for name, _ in variants:
                out("    %-7s us per launch, rounds 1-3: %s" % (name, "  ".join("%9.1f" % v for v in times[name])))
            faster = all(k < t for k, t in zip(times["kernel"], times["torch"]))
            ok_all = ok_all and faster
            out("    kernel faster than the torch composition in every round: %s (torch / kernel = %s); kernel / copy of the same bytes: %s" % (
                "yes" if faster else "NO", "  ".join("%.1fx" % (t / k) for k, t in zip(times["kernel"], times["torch"])),
                "  ".join("%.2f" % (k / c) for k, c in zip(times["kernel"], times["copy"]))))
            del s, variants
            torch.cuda.empty_cache()
    out("expectation (the launch beats the torch composition in all three rounds at all four shapes): %s" % ("holds" if ok_all else "FAILS"))


def bench_step(torch, out, steps=20):
    """VOLO-D1, batch 128, 256 x 256 uint8 canvases -> device crop to 224 -> batch preparation -> the step with the token-label loss on a
    sparse target: a fixed precomputed one, and DeviceLabelMapCrop.target on the box just drawn, alternated"""
    import numpy as np
    from autoprog_amd.data import DeviceBatchPrep, DeviceLabelMapCrop, DeviceRandomResizedCrop, StoredLabelMaps
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import SparseTokenLabelTarget, TokenLabelCrossEntropy
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import FlatAdamWEma
    torch.manual_seed(0)
    np.random.seed(0)
    student = create_model("volo_d1", drop_path_rate=0.1).cuda().train()
    red = GradientBucketReducer(list(student.parameters()), world_size=1, defer_mean=True)
    red.install_sink(student)
    opt = FlatAdamWEma(student, red, lr=1.6e-3, weight_decay=0.05, ema_decays=[0.998, 0.9986, 0.999, 0.9996])
    loss_fn = TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=1000)
    crop = DeviceRandomResizedCrop(seed=1)
    prep = DeviceBatchPrep((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), re_prob=0.25, num_classes=1000, seed=2)
    lm = DeviceLabelMapCrop(k=5, num_classes=1000)
    canvases = torch.randint(0, 256, (B_IMG, 3, 256, 256), dtype=torch.uint8, device="cuda")
    stored = StoredLabelMaps(torch.randint(0, 1000, (B_IMG,), device="cuda"),
                             synthetic_maps(torch, 1, torch.Generator(device="cuda").manual_seed(3))[0])
    crop.crop(canvases, 224)
    first = lm.target(stored, crop, 224)
    fixed = SparseTokenLabelTarget(first.idx.clone(), first.val.clone(), first.smoothing)

    def step(from_maps):
        batch = prep.prep(crop.crop(canvases, 224))
        target = lm.target(stored, crop, 224) if from_maps else fixed
        red.zero_grad()
        loss_fn(student(batch), target).backward()
        red.finish()
        opt.step()

    def window_ms(from_maps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            step(from_maps)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps
    try:
        for from_maps in (False, True):
            for _ in range(5):
                step(from_maps)
        torch.cuda.synchronize()
        t = {False: [], True: []}
        for _ in range(ROUNDS):
            for from_maps in (False, True):
                t[from_maps].append(window_ms(from_maps))
        span = max(max(v) - min(v) for v in t.values())
        moved = sum(t[True]) / ROUNDS - sum(t[False]) / ROUNDS
        out("VOLO-D1 step, batch 128, crop 256 -> 224 + preparation in front, eager, %d steps per window, rounds 1-3 (ms per step):" % steps)
        out("    fixed precomputed sparse target:        %s" % "  ".join("%.3f" % v for v in t[False]))
        out("    one label-map launch per step (k = 5):  %s" % "  ".join("%.3f" % v for v in t[True]))
        out("    the step moves by %+.3f ms (means); run-to-run span of a variant %.3f ms: %s" % (
            moved, span, "within the span" if abs(moved) <= span else "MORE than the span"))
    finally:
        red.remove()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_map_crop.txt"))
    ap.add_argument("--no-step", action="store_true", help="the kernel shapes only")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "this benchmark measures an MI355X; there is nothing to report without one"
    from autoprog_amd import ops
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out("device: %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    out("tools/bench_label_map_crop.py: microseconds per launch, windows of >= %.1f s, %d rounds with kernel / copy / torch interleaved; "
        "B = %d, Kin = %d, %d x %d fp16 maps, C = %d" % (WINDOW_S, ROUNDS, B_IMG, KIN, HM, WM, C_CLS))
    bench_shapes(torch, np, ops, out)
    if not args.no_step:
        bench_step(torch, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
