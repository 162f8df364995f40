"""Cost of adaptive gradient clipping on the flat slab (ap_agc_clip; FlatAdamWEma.adaptive_clip_grad).  One process, the variants
alternated in three rounds, warm-up first, HIP events around the timed calls.

  (a) ap_agc_clip on volo_d1's slab with its real unit table, with nothing clipping and with about 5 % and 100 % of the units clipping,
      beside two baselines: a device copy of the bytes the launch reads (8 B per parameter; a copy writes as many again) and the torch
      composition -- the per-parameter loop of tests/_agc_ref.py, in fp32, written back in place.  The operands rotate over four
      (g, p) pairs, 852 MB: the 256 MiB Infinity Cache does not serve them.  A clipped unit sits exactly on its bound afterwards, so the
      clipping variants lower clip_factor by 10 % from call to call: every unit that clipped clips again, and the quiet units (1e-4 of
      the bound) never do.
      The same launch at the volo_d5 / 448 px unit table, where pos_embed is one unit of 28 x 28 x 768 elements on ONE workgroup: the
      whole table, the long units alone (every short unit skipped) and every unit skipped (the sweep over the table).
  (b) the training step of bench.py's default shape (volo_h12_l18 = VOLO-D1, 224 px, batch 128) without clipping and with
      clip_mode="agc", eager and from a HIP graph, one model, the four step functions alternated.

    python tools/bench_agc.py > profiles/agc.txt"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
WARM, ITERS, ROUNDS, SETS = 8, 40, 3, 4

from tools.bench_grad_guard import build_step, eager_step, events_us, spread      # noqa: E402


def unit_table(name, **kw):
    """-> (offsets, skip, names, shapes in slab order) of a model built on the host: only the parameter sizes are used"""
    import torch
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import agc_units, grad_segments
    model = create_model(name, **kw)
    red = GradientBucketReducer(list(model.parameters()), world_size=1)
    offsets, skip, names = agc_units(red, model)
    by_name = dict(model.named_parameters())
    shapes = [tuple(by_name[n].shape) for n in grad_segments(red, model)[1]]
    return offsets, skip, names, shapes


def make_sets(torch, offsets, loud_share, seed):
    """SETS (g, p) pairs: p ~ N(0, 1); g ~ N(0, 1) times 1e-4 of the bound per unit, times 1e5 for a `loud_share` of the units"""
    lens = torch.tensor(offsets[1:], dtype=torch.int64) - torch.tensor(offsets[:-1], dtype=torch.int64)
    gen = torch.Generator().manual_seed(seed)
    loud = torch.rand(lens.numel(), generator=gen) < loud_share
    scale = torch.where(loud, torch.tensor(0.01 * 10.0), torch.tensor(0.01 * 1e-4)).cuda()
    per_el = torch.repeat_interleave(scale, lens.cuda())
    sets = []
    for _ in range(SETS):
        sets.append((torch.randn(offsets[-1], device="cuda") * per_el, torch.randn(offsets[-1], device="cuda")))
    return sets, int(loud.sum())


def part_a(torch):
    from autoprog_amd import ops
    from tests._agc_ref import unitwise_norm
    offsets, skip, names, shapes = unit_table("volo_d1", img_size=224)
    n, n_units = offsets[-1], len(names)
    lens = [b - a for a, b in zip(offsets[:-1], offsets[1:])]
    T = ops.agc_short_max()
    print("(a) ap_agc_clip on volo_d1's slab: %d parameters, %d units (%d skipped, %d longer than the short path's %d, longest %d); microseconds per call,"
          % (n, n_units, sum(skip), sum(1 for v in lens if v > T), T, max(lens)))
    print("    %d calls after %d warm-up calls, operands rotating over %d (g, p) pairs = %.0f MB, %d alternated rounds (min; spread = (max-min)/min)"
          % (ITERS, WARM, SETS, SETS * 8 * n / 1e6, ROUNDS))
    table = torch.tensor(offsets, dtype=torch.int64).cuda()
    skip_d = torch.tensor(skip, dtype=torch.uint8).cuda()
    factor = torch.zeros(n_units, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    variants = {}
    for label, share in (("no unit clips", 0.0), ("~5 % clip", 0.05), ("all clip", 1.0)):
        sets, loud = make_sets(torch, offsets, share, seed=1)
        state = {"i": 0, "cf": 0.01}

        def call(sets=sets, state=state, moving=share > 0):
            g, p = sets[state["i"] % SETS]
            state["i"] += 1
            if moving and state["i"] % SETS == 0:
                state["cf"] *= 0.9
            ops.agc_clip(g, p, table, skip_d, state["cf"], unit_factor=factor, counts=counts)
        variants[label] = (call, state, loud, sets)
    src = [torch.randn(2 * n, device="cuda") for _ in range(SETS)]
    dst = torch.empty(2 * n, device="cuda")
    cstate = {"i": 0}

    def copy():
        dst.copy_(src[cstate["i"] % SETS])
        cstate["i"] += 1
    times = {k: [] for k in list(variants) + ["device copy of 8 B/param"]}
    clipped_seen = {}
    for _ in range(ROUNDS):
        for k, (call, state, loud, _) in variants.items():                  # (clip_factor keeps falling across the rounds: 36 reductions
            times[k].append(events_us(torch, call, WARM, ITERS))            # of 10 % in all, the quiet units stay under 1 % of the bound)
            clipped_seen[k] = (int(counts[0]), loud)
        times["device copy of 8 B/param"].append(events_us(torch, copy, WARM, ITERS))
    for k, v in times.items():
        note = ""
        if k in clipped_seen:
            note = "   last call clipped %d units (loud units: %d of %d, the skipped ones among them)" % (clipped_seen[k][0], clipped_seen[k][1], n_units)
        print("    %-26s %9.1f us %6.1f%%   %7.0f GB/s of the 8 B/param read%s" % (k, min(v), spread(v), 8 * n / min(v) / 1e3, note))
    # the torch composition: timm's loop, fp32, in place
    params, grads, off = [], [], 0
    g0, p0 = variants["~5 % clip"][3][0]
    for shape in shapes:
        cnt = 1
        for d in shape:
            cnt *= d
        params.append(p0[off:off + cnt].view(shape))
        grads.append(g0[off:off + cnt].view(shape))
        off += cnt

    def torch_loop(cf=0.01, eps=1e-3):
        for p, g in zip(params, grads):
            max_norm = unitwise_norm(p).clamp_(min=eps).mul_(cf)
            grad_norm = unitwise_norm(g)
            clipped = g * (max_norm / grad_norm.clamp(min=1e-6))
            g.copy_(torch.where(grad_norm < max_norm, g, clipped))
    tl = [events_us(torch, torch_loop, 2, 5) for _ in range(ROUNDS)]
    best = min(times["no unit clips"])
    print("    %-26s %9.1f us %6.1f%%   (%d parameter tensors, all of them clipped: the loop has no exclusion) = %.0fx the no-clip launch"
          % ("torch per-parameter loop", min(tl), spread(tl), len(params), min(tl) / best))
    print("    expectation: 8 B/param at the optimizer launch's 4.97 TB/s = %.1f us; measured %.1f us -> %s"
          % (8 * n / 4.97e6, best, "held" if best <= 1.25 * 8 * n / 4.97e6 else "NOT held"))
    print("    expectation: the torch loop two orders of magnitude slower; measured %.0fx -> %s" % (min(tl) / best, "held" if min(tl) / best >= 100 else "NOT held"))
    del variants, src, dst, params, grads
    torch.cuda.empty_cache()
    return best


def part_a_d5(torch):
    from autoprog_amd import ops
    offsets, skip, names, shapes = unit_table("volo_d5", img_size=448)
    n, n_units = offsets[-1], len(names)
    lens = [b - a for a, b in zip(offsets[:-1], offsets[1:])]
    T = ops.agc_short_max()
    long_lens = sorted(lens[i] for i in range(n_units) if lens[i] > T and not skip[i])
    by_len = ", ".join("%d x %d" % (long_lens.count(v), v) for v in sorted(set(long_lens)))
    print("\n    the volo_d5 / 448 px table: %d parameters, %d units; longer than %d (count x elements): %s; pos_embed is the %d"
          % (n, n_units, T, by_len, lens[names.index("pos_embed")]))
    table = torch.tensor(offsets, dtype=torch.int64).cuda()
    sets, _ = make_sets(torch, offsets, 0.0, seed=2)
    sets = sets[:2]                                                          # (2 x 2.4 GB: far past the Infinity Cache already)
    st = {"i": 0}
    masks = {"whole table": torch.tensor(skip, dtype=torch.uint8).cuda(),
             "long units alone": torch.tensor([0 if (lens[i] > T and not skip[i]) else 1 for i in range(n_units)], dtype=torch.uint8).cuda(),
             "every unit skipped": torch.ones(n_units, dtype=torch.uint8).cuda()}
    times = {k: [] for k in masks}
    for _ in range(ROUNDS):
        for k, m in masks.items():
            def call(m=m):
                g, p = sets[st["i"] % len(sets)]
                st["i"] += 1
                ops.agc_clip(g, p, table, m, 0.01)
            times[k].append(events_us(torch, call, 4, 20))
    for k, v in times.items():
        print("    %-26s %9.1f us %6.1f%%" % (k, min(v), spread(v)))
    whole, tail, floor = (min(times[k]) for k in masks)
    print("    the long-unit path alone takes %.1f us (%.1f us over the table sweep), %.0f %% of the whole launch's %.1f us -> %s"
          % (tail, tail - floor, 100 * tail / whole, whole, "the one-workgroup tail DOMINATES the launch" if tail > 0.5 * whole else
             "the tail does not dominate the launch"))
    del sets
    torch.cuda.empty_cache()


def part_b(torch, args, launch_us):
    from autoprog_amd.graph import GraphedStep
    model, loss_fn, red, opt, images, target = build_step(torch, args.batch, args.res, args.variant)
    plain = eager_step(model, loss_fn, red, opt, images, target)

    def agc():
        red.zero_grad()
        loss = loss_fn(model(images), target)
        loss.backward()
        red.finish()
        opt.adaptive_clip_grad(0.01)
        opt.step()
        return loss
    fns = {"eager, no clipping": plain, "eager, agc": agc}
    for _ in range(3):
        for f in fns.values():
            f()
    fns["graph, no clipping"] = GraphedStep(model, loss_fn, red, opt, images, target).capture().step
    fns["graph, agc"] = GraphedStep(model, loss_fn, red, opt, images, target, clip_grad=0.01, clip_mode="agc").capture().step
    times = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, f in fns.items():
            times[k].append(events_us(torch, f, 5, args.steps) / 1e3)
    rep = opt.agc_report()
    print("\n(b) training step, %s %d px batch %d, one model, the four step functions alternated; milliseconds per step, %d steps after 5 warm-up steps,"
          " %d rounds (min; spread)" % (args.variant, args.res, args.batch, args.steps, ROUNDS))
    for k, v in times.items():
        print("    %-20s %8.3f ms %6.1f%%" % (k, min(v), spread(v)))
    for mode in ("eager", "graph"):
        off, on = min(times["%s, no clipping" % mode]), min(times["%s, agc" % mode])
        print("    %s: agc - none = %+.1f us per step (%+.2f%%); the launch alone in (a): %.1f us -> the step moves by %s 1 %%"
              % (mode, (on - off) * 1e3, 100 * (on - off) / off, launch_us, "under" if abs(on - off) / off < 0.01 else "OVER"))
    print("    the last pass: %d of %d units clipped, %d non-finite; worst %s" % (rep["clipped"], rep["units"], rep["nonfinite"], rep["worst"]))
    red.remove()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--res", type=int, default=224)
    ap.add_argument("--variant", default="volo_h12_l18")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this benchmark measures an MI355X; there is nothing to report without one"
    print("device: %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    launch_us = float("nan")
    if "a" in args.parts:
        launch_us = part_a(torch)
        part_a_d5(torch)
    if "b" in args.parts:
        part_b(torch, args, launch_us)


if __name__ == "__main__":
    main()
