#!/usr/bin/env python
"""What per-group learning rates and decays cost in the fused optimizer launch (ap_adamw_ema_step_groups).  Prints one line per figure, ONE
JSON line at the end, and writes the lines to --out (default profiles/param_groups.txt).

The launch alone, through the C ABI, on slabs of volo_d1's length (its parameters in slab order: the reversed parameter order) with 4 EMA
copies, as tools/bench_ema_teacher.py times it:
    legacy      ap_adamw_ema_step: one rate, one decay, the one-byte decay mask of volo_d1's no-decay rule
    grouped2    ap_adamw_ema_step_groups with the two-group table that restates `legacy` (the mask's bytes as group numbers)
    layerdecay  ap_adamw_ema_step_groups with optim.layer_decay_param_groups(volo_d1, 0.05, 0.75): one group per (layer, decayed or not)

Times are HIP events around --iters launches after --warmup, three rounds with the variants interleaved.  The operand set is about 850 MB,
far over the Infinity Cache: nothing is rotated.  The expectation: the grouped launch moves the same bytes (the byte per parameter it
reads is the byte the mask was; the table is 2 KB at most, staged in LDS once per workgroup), so it should sit inside the span of the
legacy launch's own rounds.  The tool states what it measured, a loss included; it fails only when a launch fails.  Needs a GPU."""
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


def slab_maps(torch, weight_decay, layer_decay):
    """-> (n padded to 4, decay mask [n] uint8, group bytes [n] uint8, table [G, 2] fp32) of volo_d1 in slab order, built on the host"""
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import layer_decay_param_groups
    model = create_model("volo_d1", num_classes=1000, img_size=224)
    groups = layer_decay_param_groups(model, weight_decay, layer_decay, lr=1e-6)
    group_of = {id(p): gi for gi, g in enumerate(groups) for p in g["params"]}
    skip = set(model.no_weight_decay())
    order = list(reversed([(n, p) for n, p in model.named_parameters() if p.requires_grad]))
    n = sum(p.numel() for _, p in order)
    n_pad = (n + 3) // 4 * 4
    mask, gid = torch.zeros(n_pad, dtype=torch.uint8), torch.zeros(n_pad, dtype=torch.uint8)
    off = 0
    for name, p in order:
        k = p.numel()
        mask[off:off + k] = 0 if (p.dim() == 1 or name.endswith(".bias") or name in skip) else 1
        gid[off:off + k] = group_of[id(p)]
        off += k
    table = torch.tensor([[g["lr"] * g["lr_scale"], g["weight_decay"]] for g in groups], dtype=torch.float64).to(torch.float32)
    return n_pad, mask, gid, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "param_groups.txt"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_param_groups: needs a GPU")
    from autoprog_amd import ops
    from autoprog_amd._lib import lib
    lines = []

    def say(text):
        print(text)
        lines.append(text)
    lr, wd = 1e-6, 0.05
    n, mask, gid, table = slab_maps(torch, wd, 0.75)
    mask, gid, table = mask.cuda(), gid.cuda(), table.cuda()
    two = torch.tensor([[lr, wd], [lr, 0.0]], dtype=torch.float32, device="cuda")
    gid2 = 1 - mask                                    # decayed elements: group 0 {lr, wd}; the others: group 1 {lr, 0}
    gen = torch.Generator(device="cuda").manual_seed(0)
    p, g, m = (torch.randn(n, device="cuda", generator=gen) for _ in range(3))
    m *= 0.1
    v = torch.rand(n, device="cuda", generator=gen) * 0.01
    ema = [p.clone() for _ in range(4)]
    p16 = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    ema_arr = (ctypes.c_void_p * 4)(*[e.data_ptr() for e in ema])
    dec = (ctypes.c_float * 4)(0.998, 0.9986, 0.999, 0.9996)

    def base(byte_slab):
        return (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), byte_slab.data_ptr(), n, lr, 0.9, 0.999, 1e-8, wd, 10, 1.0, None, 0.0, 0.0, None,
                ema_arr, dec, 4, p16.data_ptr())

    def ok(rc):
        if rc != 0:
            raise SystemExit("bench_param_groups: a launch returned %d" % rc)
    a_legacy, a_two, a_layer = base(mask), base(gid2), base(gid)
    variants = {
        "legacy": lambda: ok(lib.ap_adamw_ema_step(*a_legacy, ops._stream())),
        "grouped2": lambda: ok(lib.ap_adamw_ema_step_groups(*a_two, None, None, two.data_ptr(), 2, ops._stream())),
        "layerdecay": lambda: ok(lib.ap_adamw_ema_step_groups(*a_layer, None, None, table.data_ptr(), table.shape[0], ops._stream())),
    }
    rounds = {k: [] for k in variants}
    for _ in range(3):
        for name, fn in variants.items():
            rounds[name].append(events_ms(torch, fn, args.iters, args.warmup))
    say("device: %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    say("tools/bench_param_groups.py: HIP events around %d launches after %d warm-up calls, three rounds with the variants interleaved;" % (args.iters, args.warmup))
    say("slabs of volo_d1's %d parameters in slab order, 4 EMA copies, 62 B/parameter, about 850 MB of operands, nothing is rotated" % n)
    say("  legacy = ap_adamw_ema_step, grouped2 = ap_adamw_ema_step_groups with the two-group table that restates it,")
    say("  layerdecay = ap_adamw_ema_step_groups with layer_decay_param_groups(volo_d1, 0.05, 0.75): %d groups" % table.shape[0])
    mean = {}
    for name, ms in rounds.items():
        mean[name] = sum(ms) / 3
        say("launch %-10s rounds %s ms  mean %.5f ms  -> %.2f TB/s" % (name, " ".join("%.5f" % t for t in ms), mean[name], 62 * n / mean[name] / 1e9))
    span = max(rounds["legacy"]) - min(rounds["legacy"])
    say("span of the legacy launch's own rounds: %.6f ms" % span)
    for name in ("grouped2", "layerdecay"):
        delta = mean[name] - mean["legacy"]
        say("%-10s - legacy = %+.6f ms (%+.3f %%): %s" % (name, delta, 100.0 * delta / mean["legacy"],
                                                       "inside the span" if abs(delta) <= span else ("OUTSIDE the span: a loss" if delta > 0 else "outside the span: a gain")))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({"device": torch.cuda.get_device_name(0), "n": n, "groups": int(table.shape[0]), "rounds_ms": rounds, "legacy_span_ms": span}))


if __name__ == "__main__":
    main()
