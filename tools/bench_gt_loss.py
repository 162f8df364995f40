"""TokenLabelGTCrossEntropy on the sparse target (functional.SparseTokenLabelGTCEFn, csrc/softce.hip) beside the route the loss took before
-- SparseTokenLabelTarget.dense followed by the eager dense path -- in ONE process with the cases alternated; the class-row kernel beside the
plain sparse kernel on the same rows; and a volo_d1 training step at batch 128 with this loss and with TokenLabelCrossEntropy.

    python tools/bench_gt_loss.py [--out profiles/gt_loss.txt] [--no-step]

Shapes: B = 128, N = 196, K = 5 at C = 1000 and C = 21 843.  Slot 0 of every target is (label, 1.0) followed by pairs of score 0 on class 0
(they add nothing, like the -1 fillers of SparseTokenLabelTarget.from_logits, and unlike those they can be densified, so that both routes see
the same input).
  sparse   the loss forward plus backward on the sparse target: aux rows on k_soft_ce_sparse / k_soft_ce_wide, class rows on the GT form
  dense    (C = 1000 only: at 21 843 classes the [B, C, 2 + N] tensor is 2.2 TB) target.dense(C), then the loss forward plus backward on it
  copy     ops.calib_copy of the logits' bytes, B * (1 + N) * ld * 2: the calibration line of this device on this day
  gt rows  ops.soft_ce_sparse_gt_fwd_bwd on the 128 class rows, lam = 0.5 (4 K pairs per row)
  rows     ops.soft_ce_sparse_fwd_bwd on the same rows and slot 1 alone, lam = 0.5 (2 K pairs per row)
microseconds per call over device events around a window of >= 0.3 s; every call takes the next of several operand sets, so that more than
600 MB are touched before a set comes round again.  Three rounds, the cases interleaved inside each.

Condition: sparse faster than dense in every round at C = 1000.  The ratio gt rows / rows is recorded (128 rows are latency, not traffic)."""
import argparse
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ROUNDS, WINDOW_S, ROTATE_BYTES = 3, 0.3, 600e6
B, N, K, SMOOTHING = 128, 196, 5, 0.1


def round_up(v, m):
    return (v + m - 1) // m * m


def make_target(torch, C, gen):
    from autoprog_amd.loss import SparseTokenLabelTarget
    idx = torch.randint(0, C, (B, 2 + N, K), generator=gen, device="cuda", dtype=torch.int32)
    val = torch.rand(B, 2 + N, K, generator=gen, device="cuda").sort(-1, descending=True)[0]
    val = val / val.sum(-1, keepdim=True)
    idx[:, 0], val[:, 0] = 0, 0.0
    idx[:, 0, 0] = torch.where(torch.arange(B, device="cuda") % 2 == 0, idx[:, 1, 0], idx[:, 1, 1])     # half the labels are the teacher's top class
    val[:, 0, 0] = 1.0
    return SparseTokenLabelTarget(idx, val, smoothing=SMOOTHING)


class Shape:
    def __init__(self, torch, C):
        self.C, self.ld = C, round_up(C, 8)
        g = torch.Generator(device="cuda").manual_seed(C)
        self.target = make_target(torch, C, g)
        self.bytes = B * (1 + N) * self.ld * 2
        self.sets = int(math.ceil(ROTATE_BYTES / self.bytes)) + 1

        def operand(rows):
            x = torch.empty(rows, self.ld, dtype=torch.bfloat16, device="cuda")
            for r0 in range(0, rows, 3136):                    # (filled in slices: no fp32 temporary of the whole operand)
                x[r0:r0 + 3136] = (torch.randn(min(3136, rows - r0), self.ld, device="cuda", generator=g) * 2).to(torch.bfloat16)
            return x
        self.aux = [operand(B * N) for _ in range(self.sets)]
        self.cls = [operand(B) for _ in range(self.sets)]
        # the class rows alone: 128 rows are 256 KB at 1000 classes, so the rotation needs many sets -- one allocation, sliced
        self.row_sets = int(math.ceil(ROTATE_BYTES / (B * self.ld * 2))) + 1
        self.rows = operand(self.row_sets * B).view(self.row_sets, B, self.ld)
        self.src = [torch.zeros(self.bytes // 2, dtype=torch.bfloat16, device="cuda") for _ in range(self.sets)]
        self.dst = torch.empty(self.bytes // 2, dtype=torch.bfloat16, device="cuda")
        self.i = self.j = 0

    def _logits(self, torch):
        self.i = (self.i + 1) % self.sets
        xc = self.cls[self.i][:, :self.C].detach().requires_grad_(True)
        xa = self.aux[self.i].view(B, N, self.ld)[:, :, :self.C].detach().requires_grad_(True)
        return xc, xa

    def sparse(self, torch, ops, loss_fn, bb):
        xc, xa = self._logits(torch)
        loss = loss_fn((xc, xa, bb), self.target)
        loss.backward()
        return loss, xc.grad, xa.grad

    def dense(self, torch, ops, loss_fn, bb):
        xc, xa = self._logits(torch)
        loss = loss_fn((xc, xa, bb), self.target.dense(self.C))
        loss.backward()
        return loss, xc.grad, xa.grad

    def copy(self, torch, ops, loss_fn, bb):
        self.i = (self.i + 1) % len(self.src)
        ops.calib_copy(self.src[self.i], self.dst)

    def _rows(self):
        self.j = (self.j + 1) % self.row_sets
        return self.rows[self.j]

    def gt_rows(self, torch, ops, loss_fn, bb):
        t = self.target
        return ops.soft_ce_sparse_gt_fwd_bwd(self._rows(), self.C, t.idx, t.val, (2 + N) * K, 0, K, SMOOTHING, 1.0 / B, mix_lam=0.5, mix_batches=B)

    def plain_rows(self, torch, ops, loss_fn, bb):
        t = self.target
        return ops.soft_ce_sparse_fwd_bwd(self._rows(), self.C, t.idx[:, 1], t.val[:, 1], (2 + N) * K, 0, 1, SMOOTHING, 1.0 / B, mix_lam=0.5, mix_batches=B)


def window_us(torch, fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def interleaved(torch, variants, call):
    """-> {name: [us per call, one per round]}"""
    iters = {}
    for name, fn in variants:
        for _ in range(2):
            call(fn)
        torch.cuda.synchronize()
        iters[name] = max(3, int(math.ceil(WINDOW_S * 1e6 / window_us(torch, lambda: call(fn), 3))))
    times = {name: [] for name, _ in variants}
    for _ in range(ROUNDS):
        for name, fn in variants:
            times[name].append(window_us(torch, lambda: call(fn), iters[name]))
    return times


def bench_loss(torch, ops, out):
    from autoprog_amd.loss import TokenLabelGTCrossEntropy
    ok_all = True
    bb = (0, 0, 7, 7)                                            # 49 of 196 tokens: lam = 0.75, the class rows are mixed
    for C in (1000, 21843):                                      # one shape's operands at a time: a 21 843-class set is 1.1 GB
        s = Shape(torch, C)
        loss_fn = TokenLabelGTCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=C)
        out("C = %d (ld %d), B = %d, N = %d, K = %d: %.1f MB of logits per call, %d operand sets (class rows alone: %d sets)" % (
            C, s.ld, B, N, K, s.bytes / 1e6, s.sets, s.row_sets))
        variants = [("sparse", s.sparse), ("copy", s.copy)] + ([("dense", s.dense)] if C == 1000 else [])
        if C == 1000:
            s.i = 0
            a = s.sparse(torch, ops, loss_fn, bb)
            s.i = 0
            d = s.dense(torch, ops, loss_fn, bb)
            out("  sparse against dense on one operand set: loss %.7f / %.7f, d cls rel %.2e, d aux rel %.2e" % (
                float(a[0].detach()), float(d[0].detach()), float((a[1].float() - d[1].float()).norm() / d[1].float().norm()),
                float((a[2].float() - d[2].float()).norm() / d[2].float().norm())))
            del a, d
        t = interleaved(torch, variants, lambda fn: fn(torch, ops, loss_fn, bb))
        for name, _ in variants:
            out("    %-7s us per call, rounds 1-3: %s" % (name, "  ".join("%9.1f" % v for v in t[name])))
        out("    copy: %s GB/s read + written" % "  ".join("%6.0f" % (2 * s.bytes / v / 1e3) for v in t["copy"]))
        out("    sparse / copy of the logits' bytes: %s" % "  ".join("%.2f" % (a / c) for a, c in zip(t["sparse"], t["copy"])))
        if C == 1000:
            faster = all(a < d for a, d in zip(t["sparse"], t["dense"]))
            ok_all = ok_all and faster
            out("    sparse faster than densify + dense in every round: %s (dense / sparse = %s)" % (
                "yes" if faster else "NO", "  ".join("%.1fx" % (d / a) for a, d in zip(t["sparse"], t["dense"]))))
        r = interleaved(torch, [("gt rows", s.gt_rows), ("rows", s.plain_rows)], lambda fn: fn(torch, ops, None, None))
        for name in ("gt rows", "rows"):
            out("    %-7s us per launch on the %d class rows, rounds 1-3: %s" % (name, B, "  ".join("%9.2f" % v for v in r[name])))
        out("    gt rows / rows (recorded, not gated): %s" % "  ".join("%.2f" % (a / b) for a, b in zip(r["gt rows"], r["rows"])))
        del s
        torch.cuda.empty_cache()
    out("condition (the sparse route faster than densify + dense in all three rounds at C = 1000): %s" % ("holds" if ok_all else "FAILS"))


def bench_step(torch, out, steps=10):
    """volo_d1, batch 128, 224 px, a fixed sparse target: the eager step with TokenLabelGTCrossEntropy and with TokenLabelCrossEntropy, alternated"""
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import TokenLabelCrossEntropy, TokenLabelGTCrossEntropy
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import FlatAdamWEma
    torch.manual_seed(0)
    model = create_model("volo_d1", drop_path_rate=0.1).cuda().train()
    red = GradientBucketReducer(list(model.parameters()), world_size=1, defer_mean=True)
    red.install_sink(model)
    opt = FlatAdamWEma(model, red, lr=1e-3, weight_decay=0.05, ema_decays=[0.99996])
    images = torch.randn(B, 3, 224, 224, device="cuda")
    target = make_target(torch, 1000, torch.Generator(device="cuda").manual_seed(1))
    variants = [("TokenLabelGTCrossEntropy", TokenLabelGTCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=1000)),
                ("TokenLabelCrossEntropy", TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=1000))]

    def step(loss_fn):
        red.zero_grad()
        loss_fn(model(images), target).backward()
        red.finish()
        opt.step()

    def window_ms(loss_fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            step(loss_fn)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps
    for _, fn in variants:
        for _ in range(4):
            step(fn)
    torch.cuda.synchronize()
    t = {name: [] for name, _ in variants}
    for r in range(ROUNDS):
        for name, fn in (variants if r % 2 == 0 else variants[::-1]):      # the order alternates: neither loss always runs behind the other
            t[name].append(window_ms(fn))
    out("volo_d1 step, batch 128, 224 px, eager, sparse target, %d steps per window, rounds 1-3 (ms per step; the order alternates by round):" % steps)
    for name, _ in variants:
        out("    %-26s %s" % (name + ":", "  ".join("%.2f" % v for v in t[name])))
    a, b = t["TokenLabelGTCrossEntropy"], t["TokenLabelCrossEntropy"]
    span = max(max(b) - min(b), max(a) - min(a))
    diff = sum(a) / len(a) - sum(b) / len(b)
    out("    mean difference %+.3f ms; the larger of the two run-to-run spans %.3f ms -> %s" % (
        diff, span, "within the span" if abs(diff) <= span else "OUTSIDE the span"))
    red.remove()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gt_loss.txt"))
    ap.add_argument("--no-step", action="store_true", help="the loss and the kernels only")
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
    out("tools/bench_gt_loss.py: microseconds per call, windows of >= %.1f s, %d rounds with the cases interleaved" % (WINDOW_S, ROUNDS))
    bench_loss(torch, ops, out)
    if not args.no_step:
        bench_step(torch, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
