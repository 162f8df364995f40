"""The distillation loss kernel (csrc/distill.hip, ops.distill_fwd_bwd) beside the torch composition it replaces and beside a plain copy of
the bytes it must move, in ONE process with the cases alternated; then a deit_small_distilled training step at batch 128 with a
deit_small teacher in front of it, without one, and with the torch-composed loss.

    python tools/bench_distill.py [--out profiles/distill_loss.txt] [--no-step]

Shapes: 128 x 1000 (the DeiT step's own: latency-bound, microseconds only), 25 088 x 1000 and 25 088 x 21 848 (21 843 classes), each in soft
mode at T = 1 and in hard mode.  Per shape
  kernel   one launch of ap_distill_fwd_bwd: row losses and the student's gradient
  torch    soft: two log_softmax, kl_div(reduction="sum", log_target=True) * T^2 / numel, backward; hard: argmax, cross_entropy, backward
  copy     ops.calib_copy of 3 * M * ld bytes: 6 B moved per (row, column) -- the kernel's two 2-byte reads and one 2-byte write
microseconds per launch over device events around a window of >= 0.3 s; every launch takes the next of several operand sets, so that more
than 600 MB are touched before a set comes round again.  Three rounds, the cases interleaved inside each.  GB/s = 6 * M * ld bytes over the
time.

Condition for the kernel to exist: faster than the torch composition in every round at every shape.  The ratio to the copy is reported."""
import argparse
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ROUNDS, WINDOW_S, ROTATE_BYTES = 3, 0.3, 600e6


def round_up(v, m):
    return (v + m - 1) // m * m


class Shape:
    def __init__(self, torch, M, C):
        self.M, self.C, self.ld = M, C, round_up(C, 8)
        self.bytes = 6 * self.M * self.ld
        self.sets = int(math.ceil(ROTATE_BYTES / (4 * self.M * self.ld))) + 1
        g = torch.Generator(device="cuda").manual_seed(C + M)

        def operand():
            x = torch.empty(self.M, self.ld, dtype=torch.bfloat16, device="cuda")
            for r0 in range(0, self.M, 3136):                  # (filled in slices: no fp32 temporary of the whole operand)
                x[r0:r0 + 3136] = (torch.randn(min(3136, self.M - r0), self.ld, device="cuda", generator=g) * 2).to(torch.bfloat16)
            return x
        self.xs = [operand() for _ in range(self.sets)]
        self.xt = [operand() for _ in range(self.sets)]
        half = self.M * self.ld * 3 // 2                        # bf16 elements of 3 * M * ld bytes
        self.src = [torch.zeros(half, dtype=torch.bfloat16, device="cuda") for _ in range(self.sets)]
        self.dst = torch.empty(half, dtype=torch.bfloat16, device="cuda")
        self.i = 0

    def _next(self):
        self.i = (self.i + 1) % self.sets
        return self.i

    def kernel(self, torch, ops, mode):
        i = self._next()
        return ops.distill_fwd_bwd(self.xs[i][:, :self.C], self.C, self.xt[i][:, :self.C], mode, 1.0, 1.0 / self.M)

    def torch_composition(self, torch, ops, mode):
        import torch.nn.functional as F
        i = self._next()
        s = self.xs[i][:, :self.C].detach().requires_grad_(True)
        t = self.xt[i][:, :self.C]
        if mode == 0:
            loss = F.kl_div(F.log_softmax(s.float(), dim=1), F.log_softmax(t.float(), dim=1), reduction="sum", log_target=True) / s.numel()
        else:
            loss = F.cross_entropy(s.float(), t.argmax(dim=1))
        loss.backward()
        return loss, s.grad

    def copy(self, torch, ops, mode):
        ops.calib_copy(self.src[self._next()], self.dst)


def window_us(torch, fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def bench_shapes(torch, ops, out):
    ok_all = True
    for M, C in [(128, 1000), (25088, 1000), (25088, 21843)]:   # one shape's operands at a time: the 21 843-class sets are 1.1 GB each
        s = Shape(torch, M, C)
        out("%d x %d (ld %d): %.1f MB moved per launch, %d operand sets" % (M, C, s.ld, s.bytes / 1e6, s.sets))
        for mode, mname in ((0, "soft T=1"), (1, "hard")):
            variants = [("kernel", s.kernel), ("torch", s.torch_composition), ("copy", s.copy)]
            iters = {}
            for name, fn in variants:
                for _ in range(2):
                    fn(torch, ops, mode)
                torch.cuda.synchronize()
                iters[name] = max(3, int(math.ceil(WINDOW_S * 1e6 / window_us(torch, lambda: fn(torch, ops, mode), 3))))
            s.i = 0
            rows, dk = s.kernel(torch, ops, mode)
            s.i = 0
            lt, dt = s.torch_composition(torch, ops, mode)
            scale = (1.0 / C) if mode == 0 else 1.0             # the kernel ran with grad_scale 1 / M; torch's soft form divides by M * C
            out("  %s: kernel against torch on one operand set: loss %.7f / %.7f, gradient rel %.2e" % (
                mname, float(rows.sum()) / M * scale, float(lt), float((dk[:, :C].float() * scale - dt.float()).norm() / dt.float().norm())))
            del rows, dk, lt, dt
            times = {name: [] for name, _ in variants}
            for _ in range(ROUNDS):
                for name, fn in variants:
                    times[name].append(window_us(torch, lambda: fn(torch, ops, mode), iters[name]))
            for name, _ in variants:
                t = times[name]
                line = "    %-7s us per launch, rounds 1-3: %s" % (name, "  ".join("%9.1f" % v for v in t))
                if M > 128:
                    line += "   GB/s on 6 * M * ld bytes: %s" % "  ".join("%6.0f" % (s.bytes / v / 1e3) for v in t)
                out(line)
            faster = all(k < t for k, t in zip(times["kernel"], times["torch"]))
            ok_all = ok_all and faster
            out("    kernel faster than the torch composition in every round: %s (torch / kernel = %s)" % (
                "yes" if faster else "NO", "  ".join("%.1fx" % (t / k) for k, t in zip(times["kernel"], times["torch"]))))
            if M > 128:
                out("    kernel / copy of the same bytes: %s" % "  ".join("%.2f" % (k / c) for k, c in zip(times["kernel"], times["copy"])))
        del s
        torch.cuda.empty_cache()
    out("condition for merging (kernel faster than the torch composition in all three rounds at all shapes and modes): %s" % ("holds" if ok_all else "FAILS"))


def bench_step(torch, out, steps=10):
    """deit_small_distilled, batch 128, 224 px, integer labels with smoothing 0.1, alpha 0.5: the step with a deit_small teacher running in
    front of it, with a fixed DistillTarget, and with the distillation term composed in torch on the fixed target; alternated"""
    import torch.nn.functional as F
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import DistillationLoss, DistillTarget, SoftTargetCrossEntropy
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import FlatAdamWEma
    from autoprog_amd.prog.teacher import TeacherLogits
    torch.manual_seed(0)
    B = 128
    student = create_model("deit_small_distilled_patch16_224", drop_path_rate=0.1).cuda().train()
    teach = TeacherLogits(create_model("deit_small_patch16_224").cuda(), num_classes=1000)
    red = GradientBucketReducer(list(student.parameters()), world_size=1, defer_mean=True)
    red.install_sink(student)
    opt = FlatAdamWEma(student, red, lr=1e-3, weight_decay=0.05, ema_decays=[0.99996])
    images = torch.randn(B, 3, 224, 224, device="cuda")
    labels = torch.randint(0, 1000, (B,), device="cuda")
    fixed = teach(images, labels, 224)
    fixed = DistillTarget(labels, fixed.teacher_logits.clone())
    ce = SoftTargetCrossEntropy()

    for kind, tau in (("hard", 1.0), ("soft", 3.0)):
        hip = DistillationLoss(ce, kind, alpha=0.5, tau=tau)
        base_only = DistillationLoss(ce, "none")

        def torch_loss(outputs, target):
            base = base_only(outputs, target)
            x_dist, t = outputs[1].float(), target.teacher_logits.float()
            if kind == "soft":
                d = F.kl_div(F.log_softmax(x_dist / tau, dim=1), F.log_softmax(t / tau, dim=1), reduction="sum", log_target=True) * (tau * tau) / x_dist.numel()
            else:
                d = F.cross_entropy(x_dist, t.argmax(dim=1))
            return base * 0.5 + d * 0.5

        def step(taught, loss_fn):
            target = teach(images, labels, 224) if taught else fixed
            red.zero_grad()
            loss_fn(student(images), target).backward()
            red.finish()
            opt.step()

        def window_ms(taught, loss_fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                step(taught, loss_fn)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / steps
        variants = [("with the teacher, kernel loss", True, hip), ("fixed target, kernel loss", False, hip), ("fixed target, torch-composed loss", False, torch_loss)]
        for _, taught, fn in variants:
            for _ in range(4):
                step(taught, fn)
        torch.cuda.synchronize()
        t = {name: [] for name, _, _ in variants}
        for _ in range(ROUNDS):
            for name, taught, fn in variants:
                t[name].append(window_ms(taught, fn))
        out("deit_small_distilled step, %s distillation, batch 128, 224 px, eager, %d steps per window, rounds 1-3 (ms per step):" % (kind, steps))
        for name, _, _ in variants:
            out("    %-34s %s" % (name + ":", "  ".join("%.2f" % v for v in t[name])))
    red.remove()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill_loss.txt"))
    ap.add_argument("--no-step", action="store_true", help="the kernel shapes only")
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
    out("tools/bench_distill.py: microseconds per launch, windows of >= %.1f s, %d rounds with kernel / torch / copy interleaved" % (WINDOW_S, ROUNDS))
    bench_shapes(torch, ops, out)
    if not args.no_step:
        bench_step(torch, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
