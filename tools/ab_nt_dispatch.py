"""Same bits, same launches: ap_gemm_nt / ap_gemm_nt_fp8 of this tree's libautoprog_hip.so against another tree's (the parent commit, built
in a directory of its own).  The kernel choice depends on switches the library reads once per process, so everything here runs once per
switch setting (SETTINGS below; `settings` prints them one per line for a driving shell).

    python tools/ab_nt_dispatch.py bytes --parent-tree _ab_prev
        both libraries in one process, every case from the same inputs: the return codes and every output buffer (C with its padding, the
        pre-activation / derivative codes, the e4m3 bytes, amax) compared byte for byte.  Exits 1 on any difference.
    rocprofv3 --kernel-trace -f csv -d DIR -o head   -- python tools/ab_nt_dispatch.py run
    rocprofv3 --kernel-trace -f csv -d DIR -o parent -- python tools/ab_nt_dispatch.py run --parent-tree _ab_prev
        the same cases through ONE library (no counters, no other tracing), then
    python tools/ab_nt_dispatch.py traces DIR/head_kernel_trace.csv DIR/parent_kernel_trace.csv
        kernel name (it carries the template arguments), grid, workgroup and LDS size of every library launch, in order, must be equal.
    python tools/ab_nt_dispatch.py hostloop --parent-tree _ab_prev
        host microseconds per ap_gemm_nt call on a skinny shape (128 x 384 x 1000), the two libraries alternated.  Informative.

One process per run and setting, one after the other, each under its own timeout, the next behind `&&`.  The entry points are bound by
hand: the parent's library lacks symbols this tree added.  Not a test: the parent's library does not exist in a clean checkout."""
import argparse
import csv
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETTINGS = ["", "AP_GEMM_8P=0", "AP_GEMM_8P=2", "AP_GEMM_BM224=0", "AP_GEMM_WS=0", "AP_GEMM_NT_NO_SKINNY=1", "AP_GEMM_NT_TILE=1", "AP_GEMM_NT_TILE=5",
            "AP_GEMM_NT_TILE=20", "AP_GEMM_NT_192=1", "AP_GEMM_LDS_EPI=0", "AP_GEMM_LDS_EPI=1", "AP_GEMM_NT_RULE=1152,384,2,0;384,384,4,1", "AP_GEMM_DBG=2",
            "AP_GELU_TABLE=0"]
# (M, N, K, epilogue, fp8): the case list of tests/host/nt_plan_check.cpp, the shapes that fit a few seconds (K in bytes for fp8)
CASES = [(25088, 384, 384, "", 0), (25088, 384, 384, "bias", 0), (25088, 384, 384, "bias rs res", 0), (25088, 384, 384, "rs", 0),
         (25088, 1152, 384, "", 0), (8192, 1152, 384, "bias", 0), (12800, 1152, 384, "", 0), (18432, 1152, 384, "", 0), (48608, 768, 768, "", 0),
         (25088, 1536, 384, "bias gelu=3", 0), (25088, 1536, 384, "bias gelu=3 rs", 0), (25088, 1536, 384, "bias gelu=2", 0), (25088, 1536, 384, "bias gelu=1", 0),
         (25088, 1536, 384, "bias gelu=4", 0), (25088, 384, 1536, "dgelu", 0), (25088, 384, 1536, "mul", 0), (25088, 384, 1536, "mul8", 0),
         (25088, 384, 1536, "mul8 rs q8", 0), (25088, 1152, 384, "mul8 q8", 0), (25088, 384, 1536, "mul8 res", 0),
         (4095, 384, 384, "", 0), (4096, 384, 384, "", 0), (8192, 384, 64, "", 0), (8192, 384, 128, "", 0), (8192, 384, 200, "", 0), (8192, 184, 256, "", 0),
         (8192, 192, 256, "", 0), (8192, 1016, 384, "", 0), (8192, 1024, 384, "", 0), (8192, 1030, 384, "bias", 0),
         (128, 384, 1000, "", 0), (128, 384, 1000, "bias gelu=4", 0), (256, 384, 384, "bias res", 0), (257, 384, 384, "", 0),
         (100352, 576, 192, "bias gelu=3", 0), (100352, 576, 192, "bias gelu=4", 0), (100352, 192, 192, "mul8", 0), (16320, 576, 192, "mul8", 0), (16384, 576, 192, "mul8", 0),
         (300, 384, 384, "", 0), (3136, 576, 384, "", 0), (3136, 576, 384, "bias gelu=3", 0), (25088, 486, 192, "", 0), (3000, 512, 256, "", 0), (3000, 576, 256, "", 0),
         (3000, 384, 384, "bias res", 0), (3000, 384, 384, "dgelu res", 0), (3000, 384, 1536, "mul", 0), (25088, 1152, 200, "", 0),
         (4096, 192, 128, "mul8 q8", 0), (4095, 192, 128, "mul8 q8", 0), (4096, 200, 128, "mul8 q8", 0), (4096, 192, 64, "mul8 q8", 0), (3000, 1536, 384, "bias gelu=4", 0),
         (25088, 1152, 384, "", 1), (25088, 1152, 320, "", 1), (25088, 1152, 320, "bias gelu=1 q8", 1), (25088, 1536, 384, "bias gelu=3 q8", 1),
         (25088, 1536, 384, "bias gelu=3 rs", 1), (25088, 384, 384, "bias rs res", 1), (25088, 1536, 320, "bias gelu=3", 1), (4096, 192, 256, "bias gelu=1 q8", 1),
         (4096, 192, 128, "bias gelu=1 q8", 1), (128, 384, 1024, "bias", 1)]
GUARD = 0x5A


def bind(path, names=("ap_gemm_nt", "ap_gemm_nt_fp8")):
    from autoprog_amd._lib import _SIGNATURES
    lib = ctypes.CDLL(path)
    for name in names:
        getattr(lib, name).restype, getattr(lib, name).argtypes = _SIGNATURES[name]
    return lib


def libraries(args, names=("ap_gemm_nt", "ap_gemm_nt_fp8")):
    from autoprog_amd._lib import LIB_PATH
    parent = os.path.join(os.path.abspath(args.parent_tree), "autoprog_amd", "libautoprog_hip.so") if args.parent_tree else None
    return bind(LIB_PATH, names), (bind(parent, names) if parent else None)


def make_case(M, N, K, spec, fp8):
    """-> run(library) -> (return code, {name: output buffer}); the inputs are made once, every run starts from guard-filled outputs"""
    import torch
    from autoprog_amd import ops
    from autoprog_amd._lib import GemmEpilogue
    gen = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    ldc, dev, tok = ops.round_up(N, 8), "cuda", spec.split()
    gelu = next((int(t[5:]) for t in tok if t.startswith("gelu=")), 0)
    if fp8:
        a, b = (torch.randint(0, 256, s, generator=gen, dtype=torch.uint8) for s in ((M, K), (N, K)))
        a, b = (t.masked_fill((t & 0x7F) >= 0x78, 0x30).to(dev) for t in (a, b))
        dq = torch.tensor([2.0 ** -9], device=dev)
    else:
        a = torch.randn(M, K, generator=gen).to(torch.bfloat16).to(dev)
        b = (0.1 * torch.randn(N, K, generator=gen)).to(torch.bfloat16).to(dev)
    bias = torch.randn(N, generator=gen).to(dev)
    second = torch.randn(M, ldc, generator=gen).to(torch.bfloat16).to(dev)            # residual / dgelu_of / mul_by
    codes = torch.randint(0, 256, (M, ldc), generator=gen, dtype=torch.uint8).to(dev)
    rps = max(1, M // 2)
    rs = torch.tensor([0.0, 1.0 / 0.9, 1.0 / 0.9], device=dev)
    scale = torch.tensor([37.0], device=dev)

    def run(lib):
        out = {"C": torch.full((M, ldc), GUARD * 257, dtype=torch.int16, device=dev)}
        epi = GemmEpilogue()
        epi.gelu, epi.rows_per_scale, epi.ldr = gelu, rps, ldc
        if "bias" in tok:
            epi.bias = bias.data_ptr()
        if gelu in (2, 3):
            out["preact"] = torch.full((M, ldc), GUARD, dtype=torch.uint8, device=dev) if gelu == 3 else torch.full((M, ldc), GUARD * 257, dtype=torch.int16, device=dev)
            epi.preact_out = out["preact"].data_ptr()
        if "dgelu" in tok:
            epi.dgelu_of = second.data_ptr()
        if "mul" in tok:
            epi.mul_by = second.data_ptr()
        if "mul8" in tok:
            epi.mul_by8 = codes.data_ptr()
        if "rs" in tok:
            epi.row_scale = rs.data_ptr()
        if "res" in tok:
            epi.residual = second.data_ptr()
        if "q8" in tok:
            out["q8"], out["amax"] = torch.full((M, ldc), GUARD, dtype=torch.uint8, device=dev), torch.zeros(1, device=dev)
            epi.q8_out, epi.q8_scale, epi.q8_amax = out["q8"].data_ptr(), scale.data_ptr(), out["amax"].data_ptr()
        if fp8:
            rc = lib.ap_gemm_nt_fp8(a.data_ptr(), K, b.data_ptr(), K, out["C"].data_ptr(), ldc, M, N, K, dq.data_ptr(), dq.data_ptr(), ctypes.byref(epi), ops._stream())
        else:
            rc = lib.ap_gemm_nt(a.data_ptr(), K, b.data_ptr(), K, out["C"].data_ptr(), ldc, M, N, K, ctypes.byref(epi) if tok else None, ops._stream())
        return rc, out
    return run


def name_of(case):
    return "%s%dx%dx%d %s" % ("fp8 " if case[4] else "", case[0], case[1], case[2], case[3] or "plain")


def cmd_bytes(args):
    import torch
    head, parent = libraries(args)
    failures = launched = 0
    for case in CASES:
        run = make_case(*case)
        (rc_a, a), (rc_b, b) = run(head), run(parent)
        torch.cuda.synchronize()
        bad = [k for k in a if not torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8))] + (["return code %d / %d" % (rc_a, rc_b)] if rc_a != rc_b else [])
        launched += rc_a == 0
        print("%-44s rc %2d  %s" % (name_of(case), rc_a, "identical (%d buffers, %d bytes)" % (len(a), sum(t.numel() * t.element_size() for t in a.values()))
                                    if not bad else "DIFFERS in " + ", ".join(bad)))
        failures += bool(bad)
    print("%s: %d cases, %d launched, %s" % (args.label, len(CASES), launched, "%d DIFFER" % failures if failures else "every case identical"))
    return 1 if failures else 0


def cmd_run(args):
    import torch
    head, parent = libraries(args)
    codes = [make_case(*case)(parent or head)[0] for case in CASES]
    torch.cuda.synchronize()
    print("%s: return codes %s" % ("parent" if parent else "head", " ".join(str(c) for c in codes)))
    return 0


def launches(path, ours=("k_gemm_nt", "k_build_gelu_table")):
    """(kernel name, grid, workgroup, LDS bytes) of the library's own kernels (`ours`: parts of their names) in a rocprofv3 kernel trace, in
    dispatch order"""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    key = "Dispatch_Id" if rows and "Dispatch_Id" in rows[0] else "Start_Timestamp"
    rows.sort(key=lambda r: int(r[key]))
    cols = [c for c in rows[0] if c.startswith(("Grid_Size", "Workgroup_Size", "LDS_Block_Size"))] if rows else []
    assert not rows or len(cols) >= 7, "unexpected columns: %s" % list(rows[0])
    return [(r["Kernel_Name"],) + tuple(int(r[c]) for c in cols) for r in rows if any(k in r["Kernel_Name"] for k in ours)]


def cmd_traces(args, ours=("k_gemm_nt", "k_build_gelu_table")):
    a, b = launches(args.head_csv, ours), launches(args.parent_csv, ours)
    bad = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y]
    for i, x, y in bad[:10]:
        print("launch %d differs:\n  head   %s\n  parent %s" % (i, x, y))
    same = not bad and len(a) == len(b) and len(a) > 0
    print("%s: %d / %d launches, %d distinct kernels, %s" % (args.label, len(a), len(b), len({x[0] for x in a}), "every launch equal" if same else "DIFFERENT"))
    return 0 if same else 1


def cmd_hostloop(args):
    import torch
    from autoprog_amd import ops
    head, parent = libraries(args)
    M, N, K, calls = 128, 384, 1000, 20000
    a = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    b = torch.randn(N, K, device="cuda").to(torch.bfloat16)
    c = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    st = ops._stream()
    for which in ("parent", "head") * 4:            # (the first pair warms up)
        lib = parent if which == "parent" else head
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            lib.ap_gemm_nt(a.data_ptr(), K, b.data_ptr(), K, c.data_ptr(), N, M, N, K, None, st)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        print("%-6s %6.2f us per call on the launching thread (%d calls; %.2f us with the queue drained)" % (which, (t1 - t0) / calls * 1e6, calls, (time.perf_counter() - t0) / calls * 1e6))
    return 0


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("settings")
    for name in ("bytes", "run", "hostloop"):
        p = sub.add_parser(name)
        p.add_argument("--parent-tree", required=name != "run")
        p.add_argument("--label", default=os.environ.get("AB_SETTING", "default"))
    p = sub.add_parser("traces")
    p.add_argument("head_csv"); p.add_argument("parent_csv"); p.add_argument("--label", default="default")
    args = ap.parse_args()
    if args.cmd == "settings":
        print("\n".join(s or "-" for s in SETTINGS))
        return 0
    return {"bytes": cmd_bytes, "run": cmd_run, "traces": cmd_traces, "hostloop": cmd_hostloop}[args.cmd](args)


if __name__ == "__main__":
    sys.exit(main())
