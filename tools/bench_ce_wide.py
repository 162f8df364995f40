"""Soft-target CE kernels on rows wider than 1024 classes (csrc/softce.hip: k_soft_ce_wide, k_soft_ce_wide_cm) beside the register kernels and
beside a plain copy, in ONE process with the cases alternated.

    python tools/bench_ce_wide.py [--parent-tree _ab_prev] [--out profiles/wide_ce.txt]

Per case: microseconds per launch (device events around a window of >= 0.5 s, after a warm-up of the same shape; minimum over the alternated
repeats, with their spread) and algorithmic bytes per second -- logits 2 B + gradient 2 B per (row, column), + 4 B per (row, class) for a
dense target.  Every launch of a case takes the next of several operand sets, so that more than 600 MB are touched before a set comes round
again (the 256-MiB Infinity Cache holds none of it).  ops.calib_copy over 1 GiB runs in the same rotation: its rate counts the bytes read
plus the bytes written, as the CE figures do.

  (a) sparse  25 088 rows  1000 classes  ldx 1000   the register kernel: the yardstick
  (b) sparse  25 088 rows  1000 classes  ldx 1040   same rows and classes through the wide kernel: (b)/(a) is what the general structure costs
  (c) sparse  25 088 rows  8142 classes             iNaturalist-2018
  (d) sparse  25 088 rows  21 843 classes           ImageNet-21k
  (e) dense, row-major [M, C]  128 rows  21 843 classes     the DeiT / Mixup target
  (f) dense, class-major [B, C, 2 + N]  128 x 196 rows  1100 classes

--parent-tree: tools/bench_ce.py (the 1000-class loss, narrow kernels: their code is the parent's) in that tree and in this one, a fresh
process each, alternated parent / this / parent / this / parent; the parent's own spread is printed beside the difference."""
import argparse
import math
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REPEATS, WINDOW_S, ROTATE_BYTES = 3, 0.5, 600e6


def round_up(v, m):
    return (v + m - 1) // m * m


class Case:
    def __init__(self, torch, lib, tag, form, B, N, C, ldx=None, note=""):
        self.tag, self.form, self.B, self.N, self.C, self.note = tag, form, B, N, C, note
        self.M = M = B * N
        self.ldx = ldx = round_up(C, 8) if ldx is None else ldx
        self.alg_bytes = M * ldx * 4 + (M * C * 4 if form != "sparse" else 0)
        self.sets = sets = int(math.ceil(ROTATE_BYTES / self.alg_bytes)) + 1
        g = torch.Generator(device="cuda").manual_seed(B + N + C)
        self.x = [(torch.randn(M, ldx, device="cuda", generator=g) * 2).to(torch.bfloat16) for _ in range(sets)]
        self.dl = [torch.empty(M, ldx, dtype=torch.bfloat16, device="cuda") for _ in range(sets)]
        self.loss = [torch.empty(M, device="cuda") for _ in range(sets)]
        K = 5
        if form == "sparse":
            self.idx = [torch.randint(0, C, (B, N, K), device="cuda", generator=g, dtype=torch.int32) for _ in range(sets)]
            self.val = [torch.rand(B, N, K, device="cuda", generator=g) / K for _ in range(sets)]
        elif form == "class-major":
            self.t = [torch.softmax(torch.randn(B, C, 2 + N, device="cuda", generator=g) * 3, dim=1) for _ in range(sets)]
        else:
            self.t = [torch.softmax(torch.randn(M, C, device="cuda", generator=g) * 3, dim=1) for _ in range(sets)]
        self.i, self.lib, self.K = 0, lib, K
        self.stream = torch.cuda.current_stream().cuda_stream

    def __call__(self):
        i = self.i = (self.i + 1) % self.sets
        lib, M, N, C, K = self.lib, self.M, self.N, self.C, self.K
        if self.form == "sparse":
            rc = lib.ap_soft_ce_sparse_fwd_bwd(self.x[i].data_ptr(), self.ldx, self.idx[i].data_ptr(), self.val[i].data_ptr(), K, N * K, K, N, 0.1,
                                               self.loss[i].data_ptr(), self.dl[i].data_ptr(), 1.0 / M, M, C, 1.0, 0, self.stream)
        elif self.form == "class-major":
            t = self.t[i]
            rc = lib.ap_soft_ce_fwd_bwd(self.x[i].data_ptr(), self.ldx, t[:, :, 2:].data_ptr(), t.stride(0), t.stride(1), t.stride(2), N,
                                        self.loss[i].data_ptr(), self.dl[i].data_ptr(), 1.0 / M, M, C, 1.0, 0, self.stream)
        else:
            rc = lib.ap_soft_ce_fwd_bwd(self.x[i].data_ptr(), self.ldx, self.t[i].data_ptr(), C, 1, 0, 1,
                                        self.loss[i].data_ptr(), self.dl[i].data_ptr(), 1.0 / M, M, C, 1.0, 0, self.stream)
        if rc != 0:
            raise RuntimeError("case %s: code %d" % (self.tag, rc))


class Copy:
    tag, form, note = "copy", "ops.calib_copy", "1 GiB in, 1 GiB out"

    def __init__(self, torch, ops):
        n = 1 << 30
        self.src, self.dst, self.ops = torch.empty(n, dtype=torch.uint8, device="cuda").random_(), torch.empty(n, dtype=torch.uint8, device="cuda"), ops
        self.alg_bytes = 2 * n

    def __call__(self):
        self.ops.calib_copy(self.src, self.dst)


def window_us(torch, fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def bench_ce_pairs(parent, out):
    """tools/bench_ce.py of the parent tree and of this tree, alternated, one fresh process each"""
    order = [("parent", os.path.abspath(parent)), ("this", ROOT)] * 2 + [("parent", os.path.abspath(parent))]
    res = {"parent": {}, "this": {}}
    for label, tree in order:
        r = subprocess.run([sys.executable, os.path.join(tree, "tools", "bench_ce.py")], cwd=tree, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:                                   # one failed child ends the comparison: nothing more is started
            out("    bench_ce.py in the %s tree failed (exit %d): %s" % (label, r.returncode, r.stderr[-600:]))
            return
        for line in r.stdout.splitlines():
            if " us per loss forward" in line:
                name = line[:12].strip()
                res[label].setdefault(name, []).append(float(line[12:].split()[0]))
    out("\ntools/bench_ce.py (1000 classes, B = 128, N = 196: the register kernels, whose code this tree does not touch), one fresh process per run,")
    out("alternated %s; microseconds per loss forward" % " / ".join(l for l, _ in order))
    for name in res["parent"]:
        p, t = res["parent"][name], res["this"].get(name, [])
        diff = sum(t) / len(t) - sum(p) / len(p)
        verdict = "within the parent's own spread" if abs(diff) <= max(p) - min(p) else "OUTSIDE the parent's own spread"
        out("    %-12s parent %s   this %s   mean difference %+.1f us; the parent against itself spans %.1f us -> %s"
            % (name, " ".join("%.1f" % v for v in p), " ".join("%.1f" % v for v in t), diff, max(p) - min(p), verdict))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_ce.txt"))
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--cases", default="abcdef")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    assert torch.cuda.is_available(), "this benchmark measures an MI355X; there is nothing to report without one"
    from autoprog_amd import ops
    from autoprog_amd._lib import lib
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out("device: %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    spec = {"a": ("sparse", 128, 196, 1000, 1000, "register kernel (yardstick)"), "b": ("sparse", 128, 196, 1000, 1040, "wide kernel, same rows and classes"),
            "c": ("sparse", 128, 196, 8142, None, "iNaturalist-2018"), "d": ("sparse", 128, 196, 21843, None, "ImageNet-21k"),
            "e": ("row-major", 128, 1, 21843, None, "DeiT / Mixup target"), "f": ("class-major", 128, 196, 1100, None, "token-label tensor")}
    work = [Case(torch, lib, "(%s)" % k, *spec[k][:5], note=spec[k][5]) for k in args.cases] + [Copy(torch, ops)]
    iters = {}
    for w in work:                                             # warm-up of every shape; the window length from a first timing
        for _ in range(3):
            w()
        torch.cuda.synchronize()
        iters[w.tag] = max(10, int(math.ceil(WINDOW_S * 1e6 / window_us(torch, w, 5))))
    times = {w.tag: [] for w in work}
    for _ in range(REPEATS):
        for w in work:
            times[w.tag].append(window_us(torch, w, iters[w.tag]))
    out("microseconds per launch: minimum of %d alternated windows of >= %.1f s each (spread = (max - min) / min); GB/s on algorithmic bytes" % (REPEATS, WINDOW_S))
    out("%-6s %-14s %7s %7s %6s %5s %8s %10s %7s %9s  %s" % ("case", "target", "rows", "classes", "ldx", "sets", "launches", "us", "spread", "GB/s", "note"))
    rate = {}
    for w in work:
        t = min(times[w.tag])
        rate[w.tag] = w.alg_bytes / t / 1e3
        sp = 100.0 * (max(times[w.tag]) - t) / t
        if isinstance(w, Copy):
            out("%-6s %-14s %7s %7s %6s %5d %8d %10.1f %6.1f%% %9.0f  %s" % (w.tag, w.form, "-", "-", "-", 1, iters[w.tag], t, sp, rate[w.tag], w.note))
        else:
            out("%-6s %-14s %7d %7d %6d %5d %8d %10.1f %6.1f%% %9.0f  %s" % (w.tag, w.form, w.M, w.C, w.ldx, w.sets, iters[w.tag], t, sp, rate[w.tag], w.note))
    if "(a)" in rate and "(b)" in rate:
        r = min(times["(b)"]) / min(times["(a)"])
        out("(b)/(a) = %.2f (the wide structure at the register kernel's work; to be explained above 1.5)%s" % (r, "" if r <= 1.5 else "  <-- ABOVE 1.5"))
    if "(d)" in rate:
        r = rate["(d)"] / rate["copy"]
        out("(d) runs at %.2f of the copy rate (to be explained below 0.5)%s" % (r, "" if r >= 0.5 else "  <-- BELOW 0.5"))
    del work
    torch.cuda.empty_cache()
    if args.parent_tree:
        torch.cuda.synchronize()
        bench_ce_pairs(args.parent_tree, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
