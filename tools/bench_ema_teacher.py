#!/usr/bin/env python
"""What an EMA teacher costs (FlatAdamWEma.ema_model, ap_adamw_ema_step_ema16).  Prints one line per figure and ONE JSON line at the end.

  --part launch   the optimizer launch alone, through the C ABI, on synthetic slabs of --n parameters (VOLO-D1: 26.6 M) with 4 EMA copies:
                    plain        ap_adamw_ema_step of this tree
                    emit0/1/4    ap_adamw_ema_step_ema16 with 0, 1 and 4 bf16 EMA copies emitted (0: four null pointers, which the library
                                 sends to the instantiation without them)
                    plain+cast   `plain` followed by a stand-alone cast of one EMA slab to bf16 (what a user had to do per use)
                    parent       ap_adamw_ema_step of the library of another tree (--parent-tree PATH: a built checkout of the parent commit)
  --part step     a volo_d1 eager training step, batch --batch, TokenLabelGTCrossEntropy with a TeacherLabeler in front of it, three ways:
                    shadow       the teacher is opt.ema_model(3)
                    separate     the teacher is another D1 module (the same forward; the optimizer launches the plain entry point)
                    swap         the student itself inside `with opt.ema_weights(3)` in front of every step

Times are HIP events around --iters calls after --warmup calls, three rounds with the variants interleaved.  The operand set of the
launch is about 850 MB, far over the Infinity Cache: nothing is rotated.  Conditions (exit status 1 when one fails):
  launch: emit1 < plain+cast in every round; with --parent-tree, |mean emit0 - mean parent| within the span of the parent's own rounds
  step:   shadow < swap in every round
Needs a GPU: without one it fails."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def events_ms(torch, fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def part_launch(args, torch, out):
    from autoprog_amd import ops
    from autoprog_amd._lib import _SIGNATURES, lib
    n = args.n // 4 * 4
    gen = torch.Generator(device="cuda").manual_seed(0)
    p, g, m = (torch.randn(n, device="cuda", generator=gen) for _ in range(3))
    m *= 0.1
    v = torch.rand(n, device="cuda", generator=gen) * 0.01
    ema = [p.clone() for _ in range(4)]
    mask = (torch.rand(n, device="cuda", generator=gen) < 0.7).to(torch.uint8)
    p16 = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    e16 = [torch.empty(n, dtype=torch.bfloat16, device="cuda") for _ in range(4)]
    ema_arr = (ctypes.c_void_p * 4)(*[e.data_ptr() for e in ema])
    dec = (ctypes.c_float * 4)(0.998, 0.9986, 0.999, 0.9996)
    base = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), mask.data_ptr(), n, 1e-6, 0.9, 0.999, 1e-8, 0.05, 10, 1.0, None, 0.0, 0.0, None,
            ema_arr, dec, 4, p16.data_ptr())

    def ptrs(k):                                   # the last k copies
        return (ctypes.c_void_p * 4)(*[e16[e].data_ptr() if e >= 4 - k else None for e in range(4)])
    arrs = {k: ptrs(k) for k in (0, 1, 4)}

    def ok(rc):
        if rc != 0:
            raise SystemExit("bench_ema_teacher: a launch returned %d" % rc)
    variants = {"plain": lambda: ok(lib.ap_adamw_ema_step(*base, ops._stream()))}
    for k in (0, 1, 4):
        variants["emit%d" % k] = (lambda a: lambda: ok(lib.ap_adamw_ema_step_ema16(*base, a, None, ops._stream())))(arrs[k])

    def plain_cast():
        ok(lib.ap_adamw_ema_step(*base, ops._stream()))
        e16[3].copy_(ema[3])
    variants["plain+cast"] = plain_cast
    if args.parent_tree:
        path = os.path.join(os.path.abspath(args.parent_tree), "autoprog_amd", "libautoprog_hip.so")
        old = ctypes.CDLL(path)
        if hasattr(old, "ap_adamw_ema_step_ema16"):
            raise SystemExit("bench_ema_teacher: %s already has the new entry point: not a parent tree" % path)
        old.ap_adamw_ema_step.restype, old.ap_adamw_ema_step.argtypes = _SIGNATURES["ap_adamw_ema_step"]
        variants["parent"] = lambda: ok(old.ap_adamw_ema_step(*base, ops._stream()))
    rounds = {k: [] for k in variants}
    for r in range(3):
        for name, fn in variants.items():
            rounds[name].append(events_ms(torch, fn, args.iters, args.warmup))
    bytes_per = {"plain": 62, "parent": 62, "emit0": 62, "emit1": 64, "emit4": 70, "plain+cast": 68}
    for name, ms in rounds.items():
        mean = sum(ms) / 3
        print("launch %-10s rounds %s ms  mean %.5f ms  %d B/parameter -> %.2f TB/s" % (name, " ".join("%.5f" % t for t in ms), mean, bytes_per[name],
                                                                                       bytes_per[name] * n / mean / 1e9))
    out["launch"] = {"n": n, "rounds_ms": rounds}
    good = all(a < b for a, b in zip(rounds["emit1"], rounds["plain+cast"]))
    print("condition: emit1 < plain+cast in every round: %s" % ("holds" if good else "FAILS"))
    if "parent" in rounds:
        span = max(rounds["parent"]) - min(rounds["parent"])
        delta = abs(sum(rounds["emit0"]) / 3 - sum(rounds["parent"]) / 3)
        level = delta <= span
        print("condition: |emit0 - parent| = %.6f ms within the parent's span of %.6f ms: %s" % (delta, span, "holds" if level else "FAILS"))
        delta_plain = abs(sum(rounds["plain"]) / 3 - sum(rounds["parent"]) / 3)
        print("recorded:  |plain - parent| = %.6f ms (the same instruction stream)" % delta_plain)
        good = good and level
    return good


def part_step(args, torch, out):
    import numpy as np
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import SparseTokenLabelTarget, TokenLabelGTCrossEntropy
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import FlatAdamWEma
    from autoprog_amd.prog.teacher import TeacherLabeler
    torch.manual_seed(0)
    np.random.seed(0)
    student = create_model("volo_d1", num_classes=1000, img_size=224).cuda().train()
    other = create_model("volo_d1", num_classes=1000, img_size=224).cuda().eval()
    red = GradientBucketReducer(list(student.parameters()), world_size=1, defer_mean=True)
    red.install_sink(student)
    opt = FlatAdamWEma(student, red, lr=1e-6, weight_decay=0.05, ema_decays=[0.998, 0.9986, 0.999, 0.9996])
    loss_fn = TokenLabelGTCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=1000)
    x = torch.randn(args.batch, 3, 224, 224, device="cuda")
    labels = torch.randint(0, 1000, (args.batch,), device="cuda")

    def train(target):
        red.zero_grad()
        loss_fn(student(x), target).backward()
        red.finish()
        opt.step()

    kept = {}

    def swap_step():
        student.eval()
        with opt.ema_weights(3), torch.no_grad():
            x_cls, x_aux = student.forward_dense(x)
            kept["t"] = SparseTokenLabelTarget.from_logits(labels, x_cls, x_aux, 5, 1.0, 0.1, out=kept.get("t"))     # (one buffer, as the labeler keeps)
        student.train()
        train(kept["t"])
    rounds = {"shadow": [], "separate": [], "swap": []}
    try:
        for r in range(3):
            labeler = TeacherLabeler(opt.ema_model(3), k=5, num_classes=1000)
            rounds["shadow"].append(events_ms(torch, lambda: train(labeler(x, labels, 224)), args.iters, args.warmup))
            opt.release_ema_model(3)
            del labeler
            labeler = TeacherLabeler(other, k=5, num_classes=1000)
            rounds["separate"].append(events_ms(torch, lambda: train(labeler(x, labels, 224)), args.iters, args.warmup))
            rounds["swap"].append(events_ms(torch, swap_step, args.iters, args.warmup))
    finally:
        red.remove()
    for name, ms in rounds.items():
        print("step   %-10s rounds %s ms  mean %.3f ms" % (name, " ".join("%.3f" % t for t in ms), sum(ms) / 3))
    out["step"] = {"batch": args.batch, "rounds_ms": rounds}
    good = all(a < c for a, c in zip(rounds["shadow"], rounds["swap"]))
    print("condition: shadow < swap in every round: %s" % ("holds" if good else "FAILS"))
    return good


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--part", choices=["launch", "step", "both"], default="both")
    ap.add_argument("--n", type=int, default=26_600_000)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema_teacher: needs a GPU")
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    good = True
    iters, warmup = args.iters, args.warmup
    if args.part in ("launch", "both"):
        args.iters, args.warmup = iters or 2000, warmup if warmup is not None else 100
        good = part_launch(args, torch, out) and good
    if args.part in ("step", "both"):
        args.iters, args.warmup = iters or 40, warmup if warmup is not None else 5
        good = part_step(args, torch, out) and good
    print(json.dumps(out))
    sys.exit(0 if good else 1)


if __name__ == "__main__":
    main()
