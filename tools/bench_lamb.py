"""Cost of the fused LAMB step (ap_lamb_ema_step; optim.FlatLambEma).  One process, the variants alternated in three rounds, warm-up first,
HIP events around the timed calls.

  (a) on slabs of volo_d1's parameters in slab order, four EMA copies and the bf16 weight slab, layer-decay groups: the LAMB call, its
      three launches on their own (`passes`), ap_adamw_ema_step_groups on the same slabs, a device copy that moves the bytes the LAMB call
      moves, and the per-parameter torch loop (tests/_lamb_ref.lamb_per_parameter's arithmetic in fp32, with four foreach EMA lerps).
      The operands rotate over two full sets of slabs, 1.9 GB: the 256 MiB Infinity Cache serves none of them.
  (b) the training step of bench.py's default shape (volo_h12_l18 = VOLO-D1, 224 px, batch 128), eager, with FlatAdamWEma and with
      FlatLambEma, two models in one process, the two step functions alternated; `--order lamb,adamw` builds the two models the other
      way round (the second model of a process sits elsewhere in memory: the order is part of what is measured).

    python tools/bench_lamb.py > profiles/lamb.txt; python tools/bench_lamb.py --parts b --order lamb,adamw >> profiles/lamb.txt"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
WARM, ITERS, ROUNDS, SETS = 8, 40, 3, 2
DECAYS = [0.998, 0.9986, 0.999, 0.9996]
MARGIN = 0.10                                     # how far over the byte ratio the call may be for the expectation to count as held
B_LAMB, B_ADAM = 80.0, 63.0                       # bytes per parameter: csrc/lamb.hip's header, and the grouped AdamW launch on the same slabs

from tools.bench_grad_guard import eager_step, events_us, spread      # noqa: E402


def slab_tables():
    """volo_d1 on the host: -> (tensor offsets, names, shapes in slab order, group byte per element, the [G, 2] table of layer-decay groups)"""
    import torch
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import grad_segments, layer_decay_param_groups
    model = create_model("volo_d1", img_size=224)
    red = GradientBucketReducer(list(model.parameters()), world_size=1)
    offsets, names = grad_segments(red, model)
    by_name = dict(model.named_parameters())
    groups = layer_decay_param_groups(model, 0.05, 0.75)
    group_of = {id(p): gi for gi, g in enumerate(groups) for p in g["params"]}
    gid = torch.zeros((offsets[-1] + 3) // 4 * 4, dtype=torch.uint8)
    for a, b, n in zip(offsets[:-1], offsets[1:], names):
        gid[a:b] = group_of[id(by_name[n])]
    tab = torch.tensor([[1.6e-3 * g["lr_scale"], g["weight_decay"]] for g in groups], dtype=torch.float32)
    return offsets, names, [tuple(by_name[n].shape) for n in names], gid, tab


def part_a(torch):
    import ctypes
    from autoprog_amd import ops
    from autoprog_amd._lib import check, lib
    offsets, names, shapes, gid_h, tab_h = slab_tables()
    n, n_pad, n_t = offsets[-1], gid_h.numel(), len(names)
    table = ops.lamb_chunk_table(offsets)
    chunks, first = (t.cuda() for t in ops.lamb_pack_chunks(table))
    n_chunks = int(table["start"].size)
    gid, tab = gid_h.cuda(), tab_h.cuda()
    trust = torch.zeros(3, n_t, device="cuda")
    ws = torch.zeros(2 * n_chunks, dtype=torch.float64, device="cuda")
    print("(a) volo_d1's slab: %d parameters in %d tensors (longest %d), %d chunks of at most %d, %d groups; 4 EMA copies + bf16 weights; microseconds per call,"
          % (n, n_t, max(b - a for a, b in zip(offsets[:-1], offsets[1:])), n_chunks, ops.lamb_chunk(), tab.shape[0]))
    print("    %d calls after %d warm-up calls, operands rotating over %d sets of slabs = %.0f MB, %d alternated rounds (min; spread = (max-min)/min)"
          % (ITERS, WARM, SETS, SETS * (8 * 4 + 2 + 1) * n_pad / 1e6, ROUNDS))
    sets = []
    for s in range(SETS):
        gen = torch.Generator(device="cuda").manual_seed(s)
        p = torch.randn(n_pad, device="cuda", generator=gen) * 0.05
        sets.append({"p": p, "g": torch.randn(n_pad, device="cuda", generator=gen) * 0.01, "m": torch.zeros(n_pad, device="cuda"),
                     "v": torch.zeros(n_pad, device="cuda"), "ema": [p.clone() for _ in DECAYS], "p16": p.to(torch.bfloat16)})
    st = {"i": 0, "t": 0}

    def nxt():
        st["i"] += 1
        return sets[st["i"] % SETS]

    def lamb(passes=0):
        s = nxt()
        st["t"] += 1
        ops.lamb_ema_step(s["p"], s["g"], s["m"], s["v"], gid, tab, chunks, first, trust, ws, min(st["t"], 1000), ema=s["ema"], ema_decay=DECAYS, p16=s["p16"], passes=passes)
    ema_ptrs = [(ctypes.c_void_p * 4)(*[e.data_ptr() for e in s["ema"]]) for s in sets]
    decays = (ctypes.c_float * 4)(*DECAYS)

    def adamw():
        st["i"] += 1
        k = st["i"] % SETS
        s = sets[k]
        st["t"] += 1
        check(lib.ap_adamw_ema_step_groups(s["p"].data_ptr(), s["g"].data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), gid.data_ptr(), n_pad, 1.6e-3, 0.9, 0.999,
                                           1e-8, 0.05, min(st["t"], 1000), 1.0, None, 0.0, 0.0, None, ema_ptrs[k], decays, 4, s["p16"].data_ptr(), None, None,
                                           tab.data_ptr(), tab.shape[0], ops._stream()), "ap_adamw_ema_step_groups")
    half = int(B_LAMB * n_pad / 2 / 4)                                        # a copy reads and writes: half the bytes each way
    src = [torch.randn(half, device="cuda") for _ in range(SETS)]
    dst = torch.zeros(half, device="cuda")

    def copy():
        st["i"] += 1
        dst.copy_(src[st["i"] % SETS])
    variants = {"ap_lamb_ema_step": lamb, "  pass 1, norms": lambda: lamb(1), "  pass 2, trust": lambda: lamb(2), "  pass 3, update": lambda: lamb(4),
                "ap_adamw_ema_step_groups": adamw, "device copy of %d B/param" % B_LAMB: copy}
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, f in variants.items():
            times[k].append(events_us(torch, f, WARM, ITERS))
    for k, v in times.items():
        print("    %-28s rounds %s us   min %9.1f us %6.1f%%" % (k, " ".join("%9.1f" % x for x in v), min(v), spread(v)))
    # the torch spelling: a loop over parameter tensors in fp32, then four foreach lerps
    s = sets[0]
    lr_t, wd_t = tab_h[gid_h[torch.tensor(offsets[:-1])].long(), 0].tolist(), tab_h[gid_h[torch.tensor(offsets[:-1])].long(), 1].tolist()
    views = {k: [s[k][a:b].view(sh) for a, b, sh in zip(offsets[:-1], offsets[1:], shapes)] for k in ("p", "g", "m", "v")}
    ema_views = [[e[a:b].view(sh) for a, b, sh in zip(offsets[:-1], offsets[1:], shapes)] for e in s["ema"]]

    def torch_loop(b1=0.9, b2=0.999, eps=1e-6, bc1=0.271, bc2s=0.0547):
        for p, g, m, v, lr, wd in zip(views["p"], views["g"], views["m"], views["v"], lr_t, wd_t):
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            update = (m / bc1).div_(v.sqrt().div_(bc2s).add_(eps))
            if wd != 0:
                update.add_(p, alpha=wd)
                wn, un = p.norm(2), update.norm(2)
                update.mul_(torch.where(wn > 0, torch.where(un > 0, wn / un, 1.0), 1.0))
            p.add_(update, alpha=-lr)
        for e, d in zip(ema_views, DECAYS):
            torch._foreach_lerp_(e, views["p"], 1.0 - d)
    tl = [events_us(torch, torch_loop, 1, 3) for _ in range(ROUNDS)]
    print("    %-28s rounds %s us   min %9.1f us %6.1f%%   (%d tensors, fp32, no read-back)" % ("torch per-parameter loop", " ".join("%9.1f" % x for x in tl), min(tl), spread(tl), n_t))
    t_lamb, t_adam, t_copy = times["ap_lamb_ema_step"], times["ap_adamw_ema_step_groups"], times["device copy of %d B/param" % B_LAMB]
    best_l, best_a = min(t_lamb), min(t_adam)
    print("    LAMB moves %.0f B/param -> %.2f TB/s; AdamW %.0f B/param -> %.2f TB/s; the copy -> %.2f TB/s" % (B_LAMB, B_LAMB * n_pad / best_l / 1e6, B_ADAM,
                                                                                                           B_ADAM * n_pad / best_a / 1e6, B_LAMB * n_pad / min(t_copy) / 1e6))
    sum_passes = sum(min(times[k]) for k in ("  pass 1, norms", "  pass 2, trust", "  pass 3, update"))
    print("    the three launches on their own add up to %.1f us (the call: %.1f us)" % (sum_passes, best_l))
    ratio, want = best_l / best_a, B_LAMB / B_ADAM
    print("    expectation: the call takes the AdamW launch's time times the byte ratio %.2f; measured %.1f / %.1f = %.2f -> %s (held: within %d %% of the ratio)"
          % (want, best_l, best_a, ratio, "held" if ratio <= (1 + MARGIN) * want else "NOT held", round(100 * MARGIN)))
    every = all(l < t for l, t in zip(t_lamb, tl))
    print("    LAMB against the torch loop, round by round: %s -> LAMB %s the torch loop in every round (%.0fx at the minima)"
          % (" ".join("%.1f<%.1f" % (l, t) if l < t else "%.1f>=%.1f" % (l, t) for l, t in zip(t_lamb, tl)), "beat" if every else "did NOT beat", min(tl) / best_l))
    print("    the AdamW launch of this tree: %.1f us, spread %.1f%% over its rounds; csrc/optim.hip is the parent's file, byte for byte (profiles/param_groups.txt"
          " has the parent's own 298.2 us for this launch on these slabs WITHOUT rotation)" % (best_a, spread(t_adam)))
    del sets, src, dst, views, ema_views
    torch.cuda.empty_cache()


def build(torch, name, batch, res, variant):
    """bench.py's default workload (tools/bench_grad_guard.build_step) with the optimizer chosen by name"""
    import numpy as np
    from bench import make_target
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import TokenLabelCrossEntropy
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import make_flat_optimizer
    torch.manual_seed(42)
    np.random.seed(42)
    model = create_model("model_variant", variant=variant, drop_path_rate=0.1).cuda().train()
    loss_fn = TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=1000)
    red = GradientBucketReducer(list(model.parameters()), world_size=1, defer_mean=True)
    red.install_sink(model)
    opt = make_flat_optimizer(name, model, red, lr=1.6e-3, weight_decay=0.05, ema_decays=DECAYS)
    gen = torch.Generator().manual_seed(42)
    images = torch.randn(batch, 3, res, res, generator=gen).cuda()
    target = make_target(batch, 1000, (res // 16) ** 2, "cuda", gen, sparse=True)
    return model, loss_fn, red, opt, images, target


def part_b(torch, args):
    built = {name: build(torch, name, args.batch, args.res, args.variant) for name in args.order.split(",")}     # (built and timed in this order)
    label = {"adamw": "eager, FlatAdamWEma", "lamb": "eager, FlatLambEma"}
    fns = {label[name]: eager_step(*b) for name, b in built.items()}
    for _ in range(3):
        for f in fns.values():
            f()
    times = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, f in fns.items():
            times[k].append(events_us(torch, f, 5, args.steps) / 1e3)
    print("\n(b) training step, %s %d px batch %d, eager, one model per optimizer (built in the order %s), the two step functions alternated; milliseconds per step,"
          " %d steps after 5 warm-up steps, %d rounds" % (args.variant, args.res, args.batch, args.order, args.steps, ROUNDS))
    for k, v in times.items():
        print("    %-22s rounds %s ms   min %8.3f ms %6.1f%%" % (k, " ".join("%8.3f" % x for x in v), min(v), spread(v)))
    a, l = min(times["eager, FlatAdamWEma"]), min(times["eager, FlatLambEma"])
    print("    LAMB - AdamW = %+.1f us per step (%+.2f%%)" % ((l - a) * 1e3, 100 * (l - a) / a))
    rep = built["lamb"][3].trust_report()
    phis = sorted(r[3] for r in rep)
    print("    the last LAMB step: %d tensors, trust ratios min %.3g median %.3g max %.3g, %d at exactly 1 (groups without decay)"
          % (len(rep), phis[0], phis[len(phis) // 2], phis[-1], sum(1 for x in phis if x == 1.0)))
    for b in built.values():
        b[2].remove()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--order", default="adamw,lamb", help="(b): the order in which the two models are built and their steps alternated")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--res", type=int, default=224)
    ap.add_argument("--variant", default="volo_h12_l18")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this benchmark measures an MI355X; there is nothing to report without one"
    print("device: %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    if "a" in args.parts:
        part_a(torch)
    if "b" in args.parts:
        part_b(torch, args)


if __name__ == "__main__":
    main()
