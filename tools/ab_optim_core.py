"""Same bits: the flat-slab optimizer entry points of this tree's libautoprog_hip.so against another tree's (the parent commit, built in a
directory of its own), in one process, from the same inputs, every output buffer compared byte for byte.

    python tools/ab_optim_core.py --parent-tree _ab_prev

Cases: the eight AdamW launches (guard x bf16 EMA emission x group table) through their four entry points; ap_sumsq_f32; ap_grad_health on
segments that cross its 8192-element chunks; ap_agc_clip with unit lengths 1, 3, 510, 517, 2048 (its short limit), 2049 and 20001 -- both
short code paths, the long walk, every head / tail residue; ap_lamb_ema_step with tensor lengths 1, 5, 4095, 4096, 4099 and 20001 around
its 4096 chunk, with and without always_adapt / trust_clip and a guard record.  Prints one line per case and exits 1 on any difference.
Not a test: the parent's library does not exist in a clean checkout."""
import argparse
import ctypes
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LR, B1, B2, EPS, WD, GSCALE, STEP = 1.6e-3, 0.9, 0.999, 1e-8, 0.05, 0.5, 3
DECAYS = (0.998, 0.9996)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", required=True)
    args = ap.parse_args()
    import torch
    from autoprog_amd import ops
    from autoprog_amd._lib import _SIGNATURES, lib
    old = ctypes.CDLL(os.path.join(os.path.abspath(args.parent_tree), "autoprog_amd", "libautoprog_hip.so"))
    for name in ("ap_adamw_ema_step", "ap_adamw_ema_step_guarded", "ap_adamw_ema_step_ema16", "ap_adamw_ema_step_groups", "ap_sumsq_f32",
                 "ap_sumsq_workspace", "ap_grad_health", "ap_grad_health_workspace", "ap_agc_clip", "ap_lamb_ema_step", "ap_lamb_workspace"):
        getattr(old, name).restype, getattr(old, name).argtypes = _SIGNATURES[name]
    dev, failures = "cuda", []

    def rand(n, scale=1.0, seed=0):
        return (scale * torch.randn(n, generator=torch.Generator().manual_seed(seed))).to(dev)

    def compare(case, run):
        """run(library) -> {name: tensor}; both libraries from fresh clones (run clones its inputs itself)"""
        a, b = run(lib), run(old)
        torch.cuda.synchronize()
        bad = [k for k in a if not torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8))]
        print("%-64s %s" % (case, "identical (%d buffers, %d bytes)" % (len(a), sum(t.numel() * t.element_size() for t in a.values()))
                            if not bad else "DIFFERS in " + ", ".join(bad)))
        if bad:
            failures.append(case)

    def ok(rc, what):
        if rc != 0:
            raise SystemExit("ab_optim_core: %s returned %d" % (what, rc))

    def guard_record(which, g, n_seg_table, applied):
        st = torch.zeros(8, dtype=torch.int32, device=dev)
        st[1] = applied
        n_seg = n_seg_table.numel() - 1
        out_s, out_c = torch.zeros(n_seg, dtype=torch.float64, device=dev), torch.zeros(n_seg, dtype=torch.int32, device=dev)
        ws_bytes = int(which.ap_grad_health_workspace(g.numel(), n_seg))
        ws = torch.zeros(ws_bytes // 8, dtype=torch.float64, device=dev)
        ok(which.ap_grad_health(g.data_ptr(), g.numel(), n_seg_table.data_ptr(), n_seg, out_s.data_ptr(), out_c.data_ptr(), st.data_ptr(), B1, B2,
                                ws.data_ptr(), ws_bytes, ops._stream()), "ap_grad_health")
        return st, out_s, out_c

    # ---- the eight AdamW launches on the slab of tests/test_gpu_adamw_dispatch.py (under one sweep) and on one of two sweeps of the capped
    # grid and an odd tail; the group byte changes every 1021 elements, inside float4s
    for n in (4 * (3 * 256 + 5), 2 * 4194304 + 4 * 37):
        p0, g0, m0, v0 = rand(n, seed=1), rand(n, seed=2), rand(n, 0.1, seed=3), rand(n, 0.1, seed=4).abs()
        e0 = [p0 + rand(n, 0.01, seed=5 + i) for i in range(2)]
        byte = ((torch.arange(n, device=dev) // 1021) % 2).to(torch.uint8)
        table = torch.tensor([[0.25 * LR, 0.0], [LR, WD]], dtype=torch.float32, device=dev)
        seg = torch.tensor([0, n // 3, n], dtype=torch.int64, device=dev)
        for nan, (guard, e16, grouped) in itertools.product((False, True), itertools.product((False, True), repeat=3)):
            if nan and not guard:
                continue

            def run(which, guard=guard, e16=e16, grouped=grouped, nan=nan):
                g = g0.clone()
                if nan:
                    g[n // 2 + 1] = float("nan")
                s = {"p": p0.clone(), "m": m0.clone(), "v": v0.clone(), "ema0": e0[0].clone(), "ema1": e0[1].clone(),
                     "p16": p0.to(torch.bfloat16), "e16_0": torch.full((n,), 7, dtype=torch.int16, device=dev),
                     "e16_1": torch.full((n,), 7, dtype=torch.int16, device=dev)}
                st = guard_record(which, g, seg, STEP - 1)[0] if guard else None
                ema_arr = (ctypes.c_void_p * 4)(s["ema0"].data_ptr(), s["ema1"].data_ptr(), None, None)
                dec_arr = (ctypes.c_float * 4)(DECAYS[0], DECAYS[1], 0.0, 0.0)
                ptrs = (ctypes.c_void_p * 4)(None, s["e16_1"].data_ptr(), None, None) if e16 else None
                base = (s["p"].data_ptr(), g.data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), byte.data_ptr(), n, LR, B1, B2, EPS, WD, STEP, GSCALE,
                        None, 0.0, 0.3, None, ema_arr, dec_arr, 2, s["p16"].data_ptr())
                gp = st.data_ptr() if guard else None
                if grouped:
                    ok(which.ap_adamw_ema_step_groups(*base, ptrs, gp, table.data_ptr(), 2, ops._stream()), "ap_adamw_ema_step_groups")
                elif e16:
                    ok(which.ap_adamw_ema_step_ema16(*base, ptrs, gp, ops._stream()), "ap_adamw_ema_step_ema16")
                elif guard:
                    ok(which.ap_adamw_ema_step_guarded(*base, gp, ops._stream()), "ap_adamw_ema_step_guarded")
                else:
                    ok(which.ap_adamw_ema_step(*base, ops._stream()), "ap_adamw_ema_step")
                if st is not None:
                    s["guard"] = st
                return s
            compare("adamw n=%d guard=%d e16=%d grouped=%d%s" % (n, guard, e16, grouped, " one NaN" if nan else ""), run)

    # ---- ap_sumsq_f32 (a slab with an n % 4 tail, one past the 1024-workgroup cap) and ap_grad_health across its 8192-element chunks
    for n in (4 * 1000 + 3, 1024 * 1024 + 4 * 300 + 1):
        x = rand(n, seed=11)

        def run(which, x=x, n=n):
            out = torch.zeros(1, dtype=torch.float32, device=dev)
            ws = torch.zeros(int(which.ap_sumsq_workspace()) // 8, dtype=torch.float64, device=dev)
            ok(which.ap_sumsq_f32(x.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel() * 8, ops._stream()), "ap_sumsq_f32")
            return {"out": out}
        compare("sumsq n=%d" % n, run)
    lens = [5, 8191, 3, 8192, 20001, 1, 16385, 40000, 7]
    offs = [0] + list(itertools.accumulate(lens))
    n = offs[-1]
    for nan in (False, True):
        g = rand(n, seed=12)
        if nan:
            g[offs[4] + 9000] = float("inf")
            g[offs[7] + 1] = float("nan")
        seg = torch.tensor(offs, dtype=torch.int64, device=dev)

        def run(which, g=g, seg=seg):
            st, out_s, out_c = guard_record(which, g, seg, 4)
            return {"state": st, "sumsq": out_s, "count": out_c}
        compare("grad_health n=%d segments=%d%s" % (n, len(lens), " inf+NaN" if nan else ""), run)

    # ---- ap_agc_clip: every head / tail residue (the odd units shift what follows), both short paths, the long walk; scaled so that
    # some units clip and some do not
    lens = [1, 3, 510, 517, 2048, 2049, 20001, 3, 517, 2048, 1, 510, 2049, 20001, 2]
    offs = [0] + list(itertools.accumulate(lens))
    n = offs[-1]
    p0 = rand(n, seed=21)
    g0 = rand(n, 0.02, seed=22) * torch.repeat_interleave(torch.tensor([0.1 if i % 2 else 3.0 for i in range(len(lens))]), torch.tensor(lens)).to(dev)
    skip = torch.tensor([1 if i == 8 else 0 for i in range(len(lens))], dtype=torch.uint8, device=dev)
    unit = torch.tensor(offs, dtype=torch.int64, device=dev)
    for nan in (False, True):
        def run(which, nan=nan):
            g = g0.clone()
            if nan:
                g[offs[6] + 77] = float("nan")
                g[offs[2] + 5] = float("inf")
            factor = torch.zeros(len(lens), dtype=torch.float32, device=dev)
            counts = torch.zeros(2, dtype=torch.int32, device=dev)
            ok(which.ap_agc_clip(g.data_ptr(), p0.data_ptr(), n, unit.data_ptr(), skip.data_ptr(), len(lens), 0.01, 1e-3, 0.5, factor.data_ptr(),
                                 counts.data_ptr(), ops._stream()), "ap_agc_clip")
            return {"g": g, "factor": factor, "counts": counts}
        compare("agc_clip units=%s%s" % (sorted(set(lens)), " inf+NaN" if nan else ""), run)

    # ---- ap_lamb_ema_step around its 4096-element chunk
    lens = [1, 5, 4095, 4096, 4099, 20001, 5, 4099, 1]
    offs = [0] + list(itertools.accumulate(lens))
    n = offs[-1]
    n_pad = (n + 3) // 4 * 4
    tab = ops.lamb_chunk_table(offs)
    chunks, first = (t.to(dev) for t in ops.lamb_pack_chunks(tab))
    n_chunks, n_tensors = int(tab["start"].size), len(lens)
    p0, g0, m0, v0 = rand(n_pad, seed=31), rand(n, seed=32), rand(n_pad, 0.1, seed=33), rand(n_pad, 0.1, seed=34).abs()
    e0 = [p0 + rand(n_pad, 0.01, seed=35 + i) for i in range(2)]
    gid = torch.zeros(n_pad, dtype=torch.uint8, device=dev)
    gid[:n] = torch.repeat_interleave(torch.tensor([i % 3 for i in range(len(lens))], dtype=torch.uint8), torch.tensor(lens)).to(dev)
    table = torch.tensor([[1e-2, 0.05], [3e-3, 0.0], [1e-3, 0.2]], dtype=torch.float32, device=dev)
    seg = torch.tensor(offs, dtype=torch.int64, device=dev)
    gnorm = ops.sumsq(g0)
    for always, tclip, guard, nan, clip in itertools.product((0, 1), (0, 1), (False, True), (False, True), (False, True)):
        if (nan and not guard) or (clip and (always != tclip)):
            continue

        def run(which, always=always, tclip=tclip, guard=guard, nan=nan, clip=clip):
            g = g0.clone()
            if nan:
                g[offs[5] + 4097] = float("nan")
            s = {"p": p0.clone(), "m": m0.clone(), "v": v0.clone(), "ema0": e0[0].clone(), "ema1": e0[1].clone(), "p16": p0.to(torch.bfloat16),
                 "e16_1": torch.full((n_pad,), 7, dtype=torch.int16, device=dev), "trust": torch.full((3, n_tensors), -7.0, device=dev),
                 "ws": torch.zeros(int(which.ap_lamb_workspace(n_chunks)) // 8, dtype=torch.float64, device=dev)}
            st = guard_record(which, g, seg, STEP - 1)[0] if guard else None
            ema_arr = (ctypes.c_void_p * 4)(s["ema0"].data_ptr(), s["ema1"].data_ptr(), None, None)
            dec_arr = (ctypes.c_float * 4)(DECAYS[0], DECAYS[1], 0.0, 0.0)
            ptrs = (ctypes.c_void_p * 4)(None, s["e16_1"].data_ptr(), None, None)
            ok(which.ap_lamb_ema_step(s["p"].data_ptr(), g.data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), gid.data_ptr(), n, B1, B2, 1e-6, STEP, GSCALE,
                                      gnorm.data_ptr() if clip else None, 0.7 if clip else 0.0, 0.3 if clip else 0.0, None, ema_arr, dec_arr, 2,
                                      s["p16"].data_ptr(), ptrs, st.data_ptr() if guard else None, table.data_ptr(), 3, chunks.data_ptr(), n_chunks,
                                      first.data_ptr(), n_tensors, always, tclip, s["trust"].data_ptr(), s["ws"].data_ptr(), s["ws"].numel() * 8, 0, 0,
                                      ops._stream()), "ap_lamb_ema_step")
            if st is not None:
                s["guard"] = st
            return s
        compare("lamb always_adapt=%d trust_clip=%d guard=%d%s%s" % (always, tclip, guard, " one NaN" if nan else "", " clip" if clip else ""), run)

    print("%d case(s) differ" % len(failures) if failures else "every case identical")
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
