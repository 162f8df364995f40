#!/usr/bin/env python
"""The wide-row kernels (rows wider than 1024 columns: csrc/softce.hip, topk.hip, distill.hip) of this tree against the library of another
tree, in one process.  --parent-tree PATH: a built checkout of the parent commit.

  bits   every wide entry point at widths either side of the launchers' thresholds and of the staging walk's batches (1025, 2040, 2041,
         2049, 4096, 4104, 8185, 8193, 21843, 65536), 5 rows: ap_soft_ce_fwd_bwd on a row-major target, ap_soft_ce_sparse_fwd_bwd plain and
         mixed, ap_soft_ce_sparse_gt_fwd_bwd, ap_softmax_topk_rows at K = 5 and 16, ap_distill_fwd_bwd soft and hard (soft above 40 704
         columns: the student row alone in LDS).  Every output tensor must be torch.equal to the other library's.
  time   --rows rows (25 088) at 21 848 columns (a team of four waves) and at 4096 (a team of one): sparse CE, top-K at K = 5, distillation
         hard and soft.  HIP events around --iters calls, operand sets rotating over more than 600 MB, three rounds with the two libraries
         interleaved.  Condition per kernel and shape: |mean(this tree) - mean(parent)| within the span of the parent's own three rounds, or
         this tree faster.

Prints one line per figure; exit status 1 when a condition fails.  Needs a GPU: without one it fails."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
WIDTHS = [1025, 2040, 2041, 2049, 4096, 4104, 8185, 8193, 21843, 65536]
ENTRY_POINTS = ["ap_soft_ce_fwd_bwd", "ap_soft_ce_sparse_fwd_bwd", "ap_soft_ce_sparse_gt_fwd_bwd", "ap_softmax_topk_rows", "ap_distill_fwd_bwd"]
SMOOTHING = 0.1


def round_up(a, b):
    return (a + b - 1) // b * b


class Operands:
    """seeded inputs of every entry point for M rows of C columns, and fresh outputs per call"""

    def __init__(self, torch, M, C, seed):
        self.torch, self.M, self.C, self.ld = torch, M, C, round_up(C, 8)
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.x = (torch.randn(M, self.ld, device="cuda", generator=g) * 2).to(torch.bfloat16)
        self.xt = (torch.randn(M, self.ld, device="cuda", generator=g) * 2).to(torch.bfloat16)
        self.idx = torch.randint(0, C, (M, 2, 8), device="cuda", generator=g, dtype=torch.int32)       # [row, slot, pair]
        self.val = torch.rand(M, 2, 8, device="cuda", generator=g) + 0.05
        self.bytes = self.x.numel() * 2                                    # what every kernel here reads at the least: the logits

    def dense_target(self):
        g = self.torch.Generator(device="cuda").manual_seed(self.C)
        return self.torch.rand(self.M, self.C, device="cuda", generator=g) / self.C

    def outputs(self, K=0):
        t = self.torch
        o = {"loss": t.full((self.M,), float("nan"), device="cuda"), "grad": t.full((self.M, self.ld), float("nan"), dtype=t.bfloat16, device="cuda")}
        if K:
            o = {"idx": t.full((self.M, K), -7, dtype=t.int32, device="cuda"), "val": t.full((self.M, K), float("nan"), device="cuda")}
        return o


def calls(lib, op, st, target=None):
    """name -> (function of an output dict that launches and returns the status, K of the top-K outputs or 0)"""
    M, C, ld, gs = op.M, op.C, op.ld, 0.5 / op.M
    x, xt, idx, val = op.x.data_ptr(), op.xt.data_ptr(), op.idx.data_ptr(), op.val.data_ptr()
    c = {}
    if target is not None:
        c["ce dense row-major"] = (lambda o: lib.ap_soft_ce_fwd_bwd(x, ld, target.data_ptr(), C, 1, C, 1, o["loss"].data_ptr(), o["grad"].data_ptr(), gs, M, C, 1.0, 0, st), 0)
    # one row per image: the pairs of slot 0 (8 per row, the image stride is both slots)
    c["ce sparse"] = (lambda o: lib.ap_soft_ce_sparse_fwd_bwd(x, ld, idx, val, 8, 16, 8, 1, SMOOTHING, o["loss"].data_ptr(), o["grad"].data_ptr(), gs, M, C, 1.0, 0, st), 0)
    c["ce sparse mixed"] = (lambda o: lib.ap_soft_ce_sparse_fwd_bwd(x, ld, idx, val, 8, 16, 8, 1, SMOOTHING, o["loss"].data_ptr(), o["grad"].data_ptr(), gs, M, C, 0.3, M, st), 0)
    c["ce sparse gt mixed"] = (lambda o: lib.ap_soft_ce_sparse_gt_fwd_bwd(x, ld, idx, val, 8, 16, 0, 8, SMOOTHING, o["loss"].data_ptr(), o["grad"].data_ptr(), gs, M, C, 0.3, M,
                                                                         None, st), 0)
    for K in (5, 16):
        c["top-K %d" % K] = ((lambda K: lambda o: lib.ap_softmax_topk_rows(x, ld, C, K, 0.5, o["idx"].data_ptr(), o["val"].data_ptr(), K, K, 1, M, st))(K), K)
    c["distill soft"] = (lambda o: lib.ap_distill_fwd_bwd(x, ld, xt, ld, C, 0, 1.0 / 3.0, o["loss"].data_ptr(), o["grad"].data_ptr(), gs, M, st), 0)
    c["distill hard"] = (lambda o: lib.ap_distill_fwd_bwd(x, ld, xt, ld, C, 1, 1.0, o["loss"].data_ptr(), o["grad"].data_ptr(), gs, M, st), 0)
    return c


def part_bits(torch, new, old, st):
    good = True
    for C in WIDTHS:
        op = Operands(torch, 5, C, seed=C)
        target = op.dense_target()
        cn, co = calls(new, op, st, target), calls(old, op, st, target)
        for name, (fn, K) in cn.items():
            on, oo = op.outputs(K), op.outputs(K)
            rcs = (fn(on), co[name][0](oo))
            torch.cuda.synchronize()
            same = rcs == (0, 0) and all(torch.equal(on[k].view(torch.int32 if on[k].element_size() == 4 else torch.int16),
                                                     oo[k].view(torch.int32 if oo[k].element_size() == 4 else torch.int16)) for k in on)
            finite = all(bool(torch.isfinite(on[k].float()).all()) for k in on)
            print("bits  C %5d  %-20s status %s  %s%s" % (C, name, rcs, "equal" if same else "DIFFERENT", "" if finite else "  (non-finite outputs)"))
            good = good and same and finite
    print("condition: every output of every wide entry point equal to the parent's: %s" % ("holds" if good else "FAILS"))
    return good


def events_ms(torch, fns, iters, warmup):
    for i in range(warmup):
        fns[i % len(fns)]()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fns[i % len(fns)]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def part_time(torch, new, old, st, rows, iters, warmup):
    good = True
    for C in (21848, 4096):
        sets = [Operands(torch, rows, C, seed=s) for s in range(2)]
        while sum(s.bytes for s in sets) <= 600e6:
            sets.append(Operands(torch, rows, C, seed=len(sets)))
        outs = {0: sets[0].outputs(), 5: sets[0].outputs(5)}                  # (written, never read: one set)
        for name in ("ce sparse", "top-K 5", "distill hard", "distill soft"):
            def bound(lib):
                fs = []
                for op in sets:
                    fn, K = calls(lib, op, st)[name]
                    fs.append((lambda fn, o: lambda: fn(o))(fn, outs[K]))
                assert all(f() == 0 for f in fs), "%s at %d columns failed" % (name, C)
                return fs
            variants = {"parent": bound(old), "this tree": bound(new)}
            rounds = {k: [] for k in variants}
            for r in range(3):
                for k, fs in variants.items():
                    rounds[k].append(events_ms(torch, fs, iters, warmup))
            mean = {k: sum(v) / 3 for k, v in rounds.items()}
            span = max(rounds["parent"]) - min(rounds["parent"])
            ok = mean["this tree"] <= mean["parent"] or mean["this tree"] - mean["parent"] <= span
            for k, v in rounds.items():
                print("time  %5d x %5d  %-13s %-10s rounds %s ms  mean %.4f ms" % (rows, C, name, k, " ".join("%.4f" % t for t in v), mean[k]))
            print("condition: %s at %d columns: this tree - parent = %+.4f ms, the parent's span %.4f ms (%d operand sets, %.0f MB): %s"
                  % (name, C, mean["this tree"] - mean["parent"], span, len(sets), sum(s.bytes for s in sets) / 1e6, "holds" if ok else "FAILS"))
            good = good and ok
        del sets, outs
        torch.cuda.empty_cache()
    return good


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--parent-tree", required=True)
    ap.add_argument("--part", choices=["bits", "time", "both"], default="both")
    ap.add_argument("--rows", type=int, default=25088)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=6)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ab_wide_rows: needs a GPU")
    from autoprog_amd import ops
    from autoprog_amd._lib import _SIGNATURES, lib
    old = ctypes.CDLL(os.path.join(os.path.abspath(args.parent_tree), "autoprog_amd", "libautoprog_hip.so"))
    for name in ENTRY_POINTS:
        getattr(old, name).restype, getattr(old, name).argtypes = _SIGNATURES[name]
    print("device %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    st = ops._stream()
    good = True
    if args.part in ("bits", "both"):
        good = part_bits(torch, lib, old, st) and good
    if args.part in ("time", "both"):
        good = part_time(torch, lib, old, st, args.rows, args.iters, args.warmup) and good
    sys.exit(0 if good else 1)


if __name__ == "__main__":
    main()
