"""Cost of the non-finite gradient guard (FlatAdamWEma.step(skip_nonfinite=True)): three comparisons, each in ONE process with the variants
alternated, warm-up first, HIP events around the timed calls.

  (a) the health pass (ap_grad_health: per-tensor sums and non-finite counts, the step's decision) against ap_sumsq_f32 on the same slab,
      at the VOLO-D1 and VOLO-D5 slab sizes with their real segment tables.  Both read 4 B per element and are bound by that read.
  (b) the full training step of bench.py's default shape (volo_h12_l18, 224 px, batch 128) with the guard off and on, eager and from a
      HIP graph, one model, the four step functions alternated.
  (c) the guard-OFF step of this tree against another tree (the parent commit, built in a directory of its own: --parent-tree), each
      measurement a fresh process, alternated parent / this / parent / this ...; the parent's own run-to-run spread is printed beside
      the difference.

    python tools/bench_grad_guard.py --parent-tree _ab_prev > profiles/grad_guard_ab.txt

A child process (--child) times the guard-off step of --tree and prints one JSON line; it uses only what both trees have."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
WARM, ITERS, REPEATS = 10, 50, 3


def events_us(torch, fn, warm, iters):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def spread(v):
    return 100.0 * (max(v) - min(v)) / min(v)


# ---------------------------------------------------------------------------------------------------------------- (a)
def part_a(torch):
    from autoprog_amd import ops
    from autoprog_amd.models import create_model
    print("(a) health pass against ap_sumsq_f32, same slab; microseconds per call, %d calls after %d warm-up calls, %d alternated repeats (min; spread = (max-min)/min)"
          % (ITERS, WARM, REPEATS))
    print("%-8s %12s %8s %11s %8s %12s %8s %8s %11s %11s" % ("model", "elements", "tensors", "sumsq", "spread", "grad_health", "spread", "ratio", "sumsq GB/s", "health GB/s"))
    worst = 0.0
    for name, kw in (("volo_d1", dict(img_size=224)), ("volo_d5", dict(img_size=448))):
        model = create_model(name, **kw)                                     # on the host: only the parameter sizes are used
        lens = [p.numel() for p in reversed([p for p in model.parameters() if p.requires_grad])]      # the reducer's slab order
        del model
        offsets = [0]
        for n_ in lens:
            offsets.append(offsets[-1] + n_)
        n, n_seg = offsets[-1], len(lens)
        g = torch.randn(n, device="cuda") * 0.01
        table = torch.tensor(offsets, dtype=torch.int64).cuda()
        sumsq, count = torch.zeros(n_seg, dtype=torch.float64, device="cuda"), torch.zeros(n_seg, dtype=torch.int32, device="cuda")
        state = torch.zeros(8, dtype=torch.int32, device="cuda")
        ws = torch.empty(ops.grad_health_workspace(n, n_seg) // 8, dtype=torch.float64, device="cuda")
        out1 = torch.zeros(1, device="cuda")
        ws1 = torch.empty(1024, dtype=torch.float64, device="cuda")

        def a():
            ops.sumsq(g, out1, ws1)

        def b():
            ops.grad_health(g, table, sumsq, count, state, ws)
        ta, tb = [], []
        for _ in range(REPEATS):
            ta.append(events_us(torch, a, WARM, ITERS))
            tb.append(events_us(torch, b, WARM, ITERS))
        assert int(count.sum()) == 0 and abs(float(sumsq.sum()) - float(out1[0])) < 1e-4 * float(out1[0])
        ratio = min(tb) / min(ta)
        worst = max(worst, ratio)
        print("%-8s %12d %8d %11.1f %7.1f%% %12.1f %7.1f%% %8.2f %11.0f %11.0f" % (name, n, n_seg, min(ta), spread(ta), min(tb), spread(tb), ratio,
                                                                           4 * n / min(ta) / 1e3, 4 * n / min(tb) / 1e3))
        del g
    print("bound: the health pass may take 1.5x ap_sumsq_f32; worst ratio measured %.2f -> %s" % (worst, "within" if worst <= 1.5 else "OVER"))
    return worst


# ---------------------------------------------------------------------------------------------------------------- (b) and the child of (c)
def build_step(torch, batch, res, variant):
    """bench.py's default workload with only what every tree since the flat optimizer has -> (model, loss_fn, reducer, opt, images, target)"""
    import numpy as np
    from bench import make_target
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import TokenLabelCrossEntropy
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import FlatAdamWEma
    torch.manual_seed(42)
    np.random.seed(42)
    model = create_model("model_variant", variant=variant, drop_path_rate=0.1).cuda().train()
    loss_fn = TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=1000)
    red = GradientBucketReducer(list(model.parameters()), world_size=1, defer_mean=True)
    red.install_sink(model)
    opt = FlatAdamWEma(model, red, lr=1.6e-3, weight_decay=0.05, ema_decays=[0.998, 0.9986, 0.999, 0.9996])
    gen = torch.Generator().manual_seed(42)
    images = torch.randn(batch, 3, res, res, generator=gen).cuda()
    target = make_target(batch, 1000, (res // 16) ** 2, "cuda", gen, sparse=True)
    return model, loss_fn, red, opt, images, target


def eager_step(model, loss_fn, red, opt, images, target, **kw):
    def step():
        red.zero_grad()
        loss = loss_fn(model(images), target)
        loss.backward()
        red.finish()
        opt.step(**kw)
        return loss
    return step


def part_b(torch, args, health_us):
    from autoprog_amd.graph import GraphedStep
    model, loss_fn, red, opt, images, target = build_step(torch, args.batch, args.res, args.variant)
    fns = {"eager, guard off": eager_step(model, loss_fn, red, opt, images, target),
           "eager, guard on": eager_step(model, loss_fn, red, opt, images, target, skip_nonfinite=True)}
    for _ in range(3):
        for f in fns.values():
            f()
    g_off = GraphedStep(model, loss_fn, red, opt, images, target).capture()
    g_on = GraphedStep(model, loss_fn, red, opt, images, target, skip_nonfinite=True).capture()
    fns["graph, guard off"] = g_off.step
    fns["graph, guard on"] = g_on.step
    times = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, f in fns.items():
            times[k].append(events_us(torch, f, 5, args.steps) / 1e3)
    counts = opt.guard_counts()
    print("\n(b) training step, %s %d px batch %d, one model, the four step functions alternated; milliseconds per step, %d steps after 5 warm-up steps,"
          " %d repeats (min; spread)" % (args.variant, args.res, args.batch, args.steps, REPEATS))
    for k, v in times.items():
        print("    %-18s %8.3f ms %6.1f%%" % (k, min(v), spread(v)))
    for mode in ("eager", "graph"):
        off, on = min(times["%s, guard off" % mode]), min(times["%s, guard on" % mode])
        print("    %s: guard on - off = %+.1f us per step (%+.2f%%); the health pass alone in this process: %.1f us" % (mode, (on - off) * 1e3, 100 * (on - off) / off, health_us))
    print("    guard counters after the run: %s (every gradient was finite)" % counts)
    red.remove()


def child(args):
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    import torch
    import autoprog_amd
    assert os.path.abspath(autoprog_amd.__file__).startswith(tree + os.sep), (autoprog_amd.__file__, tree)
    from autoprog_amd.graph import GraphedStep
    model, loss_fn, red, opt, images, target = build_step(torch, args.batch, args.res, args.variant)
    step = eager_step(model, loss_fn, red, opt, images, target)
    eager = min(events_us(torch, step, 8, args.steps) for _ in range(2)) / 1e3
    gs = GraphedStep(model, loss_fn, red, opt, images, target).capture()
    graph = min(events_us(torch, gs.step, 5, args.steps) for _ in range(2)) / 1e3
    red.remove()
    print(json.dumps({"tree": tree, "eager_ms": eager, "graph_ms": graph}))


def part_c(args):
    this = os.path.dirname(HERE)
    parent = os.path.abspath(args.parent_tree)
    order = [("parent", parent), ("this", this)] * args.rounds + [("parent", parent)]
    res = {"parent": [], "this": []}
    for label, tree in order:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--steps", str(args.steps), "--batch", str(args.batch),
               "--res", str(args.res), "--variant", args.variant]
        r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:                                   # one failed child ends the comparison: nothing more is started
            print("    child for %s failed (exit %d): %s" % (label, r.returncode, r.stderr[-800:]))
            return
        res[label].append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    print("\n(c) guard-OFF step of this tree against the parent commit's tree, one fresh process per measurement, alternated %s; milliseconds per step (min of 2 x %d steps)"
          % (" / ".join(l for l, _ in order), args.steps))
    for key in ("eager_ms", "graph_ms"):
        p, t = [d[key] for d in res["parent"]], [d[key] for d in res["this"]]
        print("    %-9s parent %s   this %s" % (key, " ".join("%.3f" % v for v in p), " ".join("%.3f" % v for v in t)))
        diff = sum(t) / len(t) - sum(p) / len(p)
        print("    %-9s mean difference this - parent %+.3f ms; the parent against itself spans %.3f ms -> %s" % (
            key, diff, max(p) - min(p), "within the parent's own spread" if abs(diff) <= max(p) - min(p) else "OUTSIDE the parent's own spread"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=2, help="(c): parent / this pairs before the closing parent run")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--res", type=int, default=224)
    ap.add_argument("--variant", default="volo_h12_l18")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    args = ap.parse_args()
    if args.child:
        return child(args)
    sys.path.insert(0, os.path.dirname(HERE))
    import torch
    assert torch.cuda.is_available(), "this benchmark measures an MI355X; there is nothing to report without one"
    print("device: %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    health_us = float("nan")
    if "a" in args.parts:
        part_a(torch)
    if "b" in args.parts:
        # the health pass alone on this model's own slab, for the line that sets it beside the step's difference
        from autoprog_amd import ops
        from autoprog_amd.models import create_model
        m = create_model("model_variant", variant=args.variant)
        lens = [p.numel() for p in reversed([p for p in m.parameters() if p.requires_grad])]
        del m
        offsets = [0]
        for n_ in lens:
            offsets.append(offsets[-1] + n_)
        g = torch.randn(offsets[-1], device="cuda") * 0.01
        table = torch.tensor(offsets, dtype=torch.int64).cuda()
        bufs = (torch.zeros(len(lens), dtype=torch.float64, device="cuda"), torch.zeros(len(lens), dtype=torch.int32, device="cuda"),
                torch.zeros(8, dtype=torch.int32, device="cuda"), torch.empty(ops.grad_health_workspace(offsets[-1], len(lens)) // 8, dtype=torch.float64, device="cuda"))
        health_us = min(events_us(torch, lambda: ops.grad_health(g, table, *bufs), WARM, ITERS) for _ in range(REPEATS))
        del g
        part_b(torch, args, health_us)
    if "c" in args.parts:
        if not args.parent_tree:
            print("\n(c) skipped: no --parent-tree")
        else:
            torch.cuda.synchronize()
            part_c(args)


if __name__ == "__main__":
    main()
