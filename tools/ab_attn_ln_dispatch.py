"""Same bits, same launches: the attention, class-attention, outlook, LayerNorm and convolution entry points (and one ap_mlp_fused / one
ap_gemm_nt gelu = 3 launch for their two switches) of this tree's libautoprog_hip.so against another tree's (the parent commit, built in a
directory of its own).  The kernel choice depends on switches the library reads once per process, so everything here runs once per switch
setting (SETTINGS below; `settings` prints them one per line for a driving shell).

    python tools/ab_attn_ln_dispatch.py bytes --parent-tree _ab_prev
        both libraries in one process, every case from the same seeded inputs and guard-filled outputs: the return codes and every output
        buffer compared byte for byte -- refused and invalid-argument calls included.  Exits 1 on any difference.
    rocprofv3 --kernel-trace -f csv -d DIR -o head   -- python tools/ab_attn_ln_dispatch.py run
    rocprofv3 --kernel-trace -f csv -d DIR -o parent -- python tools/ab_attn_ln_dispatch.py run --parent-tree _ab_prev
        the same cases through ONE library (no counters, no other tracing), then
    python tools/ab_attn_ln_dispatch.py traces DIR/head_kernel_trace.csv DIR/parent_kernel_trace.csv
        kernel name (it carries the template arguments), grid, workgroup and LDS size of every library launch, in order, must be equal.
    python tools/ab_attn_ln_dispatch.py hostloop --parent-tree _ab_prev
        host microseconds per ap_layernorm_bwd and ap_conv7_s2d_ld call in a tight loop, the two libraries alternated.  Informative.

One process per run and setting, one after the other, each under its own timeout, the next behind `&&`.  Not a test: the parent's library
does not exist in a clean checkout."""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ab_nt_dispatch as nt            # noqa: E402  (the library pair, the trace reader and the GEMM case)

SETTINGS = ["", "AP_MHSA_FLASH=1", "AP_MHSA_FWD_P=0", "AP_MHSA_BWD_DS=0",
            "AP_OUTLOOK_P=0", "AP_OUTLOOK_P=2", "AP_OUTLOOK_P=0 AP_OUTLOOK_MFMA=0", "AP_OUTLOOK_SR=1", "AP_OUTLOOK_SR=2", "AP_OUTLOOK_P=0 AP_OUTLOOK_SRW=2",
            "AP_LN_FWD_LP=0", "AP_LN_FWD_RPG=4", "AP_LN_FWD_WIDE=1", "AP_LN_BWD_PF=0", "AP_LN_BWD_PF=2", "AP_LN_BWD_PF=3", "AP_LN_BWD_GRID=8", "AP_LN_BWD_GRID=2000",
            "AP_CONV_WAVES=4", "AP_CONV_GRID=3", "AP_CONV_WGRAD_GRID=3 AP_CONV_WGRAD_P=0", "AP_CONV128_GRID=3", "AP_CONV7_GRID=3 AP_CONV7_WGRAD_GRID=3",
            "AP_MLP_FUSED_V=1", "AP_GELU_TABLE=0"]
OURS = ("k_mhsa", "k_class_attn", "k_attn_delta", "k_outlook", "k_ln_", "k_conv", "k_mlp_fused", "k_gemm", "k_build_gelu_table")
GUARD = nt.GUARD
N_LIST = [1, 96, 97, 112, 113, 196, 197, 208, 209, 224, 225, 256, 257, 784]
HW_LIST = [(2, 2), (7, 5), (14, 14), (28, 28), (56, 56), (28, 66)]
C_LIST = [8, 96, 192, 256, 384, 512, 520, 768, 1000, 1024, 1536, 2048, 2056, 12]


def bind_all(path):
    """every entry point this library has (the parent lacks the symbols this tree added)"""
    from autoprog_amd._lib import _SIGNATURES
    lib = ctypes.CDLL(path)
    for name, (res, args) in _SIGNATURES.items():
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def libraries(args):
    from autoprog_amd._lib import LIB_PATH
    parent = os.path.join(os.path.abspath(args.parent_tree), "autoprog_amd", "libautoprog_hip.so") if args.parent_tree else None
    return bind_all(LIB_PATH), (bind_all(parent) if parent else None)


def _guard(shape, dtype):
    import torch
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(GUARD)
    return t


def _bf16(gen, *shape, scale=1.0):
    import torch
    return (scale * torch.randn(*shape, generator=gen)).to(torch.bfloat16).cuda()


def mhsa_cases():
    """(name, run(lib) -> (rc, outputs)): forward, forward with the e4m3 output, workspace query + backward; class attention; refused calls"""
    import torch
    from autoprog_amd import ops
    bf, f32, u8 = torch.bfloat16, torch.float32, torch.uint8
    shapes = [(2, 3, N, hd) for hd in (32, 48, 64) for N in N_LIST] + [(64, 12, 196, 32), (64, 12, 97, 32), (25, 12, 196, 32), (64, 12, 196, 64), (2, 3, 196, 40), (0, 3, 196, 32)]

    def one(B, heads, N, hd):
        C, gen = heads * hd, torch.Generator().manual_seed(N * 131 + hd)
        qkv, dout = _bf16(gen, max(B, 1), N, 3 * C), _bf16(gen, max(B, 1) * N, C)
        rs = (torch.rand(max(B, 1), generator=gen) > 0.3).float().cuda()
        scale8 = torch.tensor([16.0], device="cuda")

        def fwd(lib):
            o = {"out": _guard((max(B, 1) * N, C), bf), "lse": _guard((max(B, 1), heads, N), f32)}
            return lib.ap_mhsa_fwd(qkv.data_ptr(), o["out"].data_ptr(), o["lse"].data_ptr(), B, N, heads, hd, hd ** -0.5, rs.data_ptr(), ops._stream()), o

        def fwd8(lib):
            o = {"out": _guard((max(B, 1) * N, C), bf), "lse": _guard((max(B, 1), heads, N), f32), "out8": _guard((max(B, 1) * N, C), u8), "amax": torch.zeros(1, device="cuda")}
            return lib.ap_mhsa_fwd_fp8(qkv.data_ptr(), o["out"].data_ptr(), o["out8"].data_ptr(), scale8.data_ptr(), o["amax"].data_ptr(), o["lse"].data_ptr(), B, N, heads, hd,
                                       hd ** -0.5, None, ops._stream()), o

        def bwd(lib, short=0):
            rc0, f = fwd(lib)
            ws_bytes = lib.ap_mhsa_bwd_workspace(B, N, heads, hd)
            ws = _guard((ws_bytes // 4 + 1,), f32)
            o = {"dqkv": _guard((max(B, 1), N, 3 * C), bf), "ws_bytes": torch.tensor([ws_bytes]), "ws": ws}
            return lib.ap_mhsa_bwd(qkv.data_ptr(), f["out"].data_ptr(), dout.data_ptr(), f["lse"].data_ptr(), o["dqkv"].data_ptr(), B, N, heads, hd, hd ** -0.5,
                                   ws.data_ptr(), max(ws_bytes - short, 0), ops._stream()), o
        tag = "%dx%d N=%d hd=%d" % (B, heads, N, hd)
        return [("mhsa fwd " + tag, fwd), ("mhsa fwd fp8 " + tag, fwd8), ("mhsa bwd " + tag, bwd)] + ([("mhsa bwd short workspace " + tag, lambda lib: bwd(lib, 4))] if N == 257 else [])

    def null_ptr(lib):
        o = {"lse": _guard((1, 3, 196), f32)}
        return lib.ap_mhsa_fwd(None, None, o["lse"].data_ptr(), 1, 196, 3, 32, 0.1, None, ops._stream()), o

    def class_attn(N, hd):
        B, heads = 2, 3
        C, gen = heads * hd, torch.Generator().manual_seed(N * 17 + hd)
        q, kv, dout = _bf16(gen, B, C), _bf16(gen, B, N, 2 * C), _bf16(gen, B, C)

        def run(lib):
            o = {"out": _guard((B, C), bf), "probs": _guard((B, heads, N), f32), "dq": _guard((B, C), bf), "dkv": _guard((B, N, 2 * C), bf)}
            rc = lib.ap_class_attn_fwd(q.data_ptr(), kv.data_ptr(), None, o["out"].data_ptr(), o["probs"].data_ptr(), B, N, heads, hd, hd ** -0.5, ops._stream())
            rc2 = lib.ap_class_attn_bwd(q.data_ptr(), kv.data_ptr(), None, o["probs"].data_ptr(), dout.data_ptr(), o["dq"].data_ptr(), o["dkv"].data_ptr(), None,
                                        B, N, heads, hd, hd ** -0.5, ops._stream())
            return rc * 100 + rc2, o
        return ("class attention N=%d hd=%d" % (N, hd), run)
    cases = [c for s in shapes for c in one(*s)] + [("mhsa fwd null pointers", null_ptr)]
    return cases + [class_attn(N, hd) for hd in (32, 48, 64, 40) for N in (1, 196, 14336, 14337)]


def outlook_cases():
    import torch
    from autoprog_amd import ops
    bf = torch.bfloat16

    def one(B, H, W, heads, hd=32, ldl_short=0):
        C, h, w = heads * 32, (H + 1) // 2, (W + 1) // 2
        ldl = ops.round_up(heads * 81, 8) - ldl_short * 1000
        gen = torch.Generator().manual_seed(H * 100 + W + heads)
        v, dy, logits = _bf16(gen, B, H, W, C), _bf16(gen, B, H, W, C), _bf16(gen, B, h, w, max(ldl, 8), scale=2.0)

        def run(lib):
            o = {"y": _guard((B, H, W, C), bf), "dv": _guard((B, H, W, C), bf), "dlogits": _guard((B, h, w, max(ldl, 8)), bf)}
            rc = lib.ap_outlook_fwd(v.data_ptr(), logits.data_ptr(), ldl, o["y"].data_ptr(), B, H, W, heads, hd, 32 ** -0.5, ops._stream())
            rc2 = lib.ap_outlook_bwd(v.data_ptr(), logits.data_ptr(), ldl, dy.data_ptr(), o["dv"].data_ptr(), o["dlogits"].data_ptr(), B, H, W, heads, hd, 32 ** -0.5, ops._stream())
            return rc * 100 + rc2, o
        return ("outlook %dx%d B=%d heads=%d hd=%d%s" % (H, W, B, heads, hd, " short ldl" if ldl_short else ""), run)
    return [one(B, H, W, heads) for (H, W) in HW_LIST for heads in (1, 6) for B in (1, 16)] + [one(128, 28, 28, 6), one(2, 14, 14, 6, hd=48), one(2, 14, 14, 6, ldl_short=1)]


def ln_cases():
    """all five LayerNorm entry points at every width of the plan check; rows 0 / 1 / 300 / 25088 (pool: 3 x 10 x 10, 32 x 28 x 28 tokens)"""
    import torch
    from autoprog_amd import ops
    bf, f32, u8 = torch.bfloat16, torch.float32, torch.uint8

    def one(rows, C, pool_shape=None):
        Ca, R = max(C, 8), max(rows, 1)
        gen = torch.Generator().manual_seed(rows * 7 + C)
        x, dy, dres = _bf16(gen, R, Ca), _bf16(gen, R, Ca), _bf16(gen, R, Ca)
        gamma, beta = torch.randn(Ca, generator=gen).cuda(), torch.randn(Ca, generator=gen).cuda()
        scale8 = torch.tensor([8.0], device="cuda")
        dp = _bf16(gen, pool_shape[0], (pool_shape[1] + 1) // 2, (pool_shape[2] + 1) // 2, Ca) if pool_shape else None

        def run(lib):
            st = ops._stream()
            o = {"y": _guard((R, Ca), bf), "mean": _guard((R,), f32), "rstd": _guard((R,), f32), "y_": _guard((R, Ca), bf), "y8": _guard((R, Ca), u8), "amax": torch.zeros(1, device="cuda"),
                 "mean_": _guard((R,), f32), "rstd_": _guard((R,), f32)}
            rcs = [lib.ap_layernorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), o["y"].data_ptr(), o["mean"].data_ptr(), o["rstd"].data_ptr(), rows, C, 1e-5, st),
                   lib.ap_layernorm_fwd_fp8(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), o["y_"].data_ptr(), o["y8"].data_ptr(), scale8.data_ptr(), o["amax"].data_ptr(),
                                            o["mean_"].data_ptr(), o["rstd_"].data_ptr(), rows, C, 1e-5, st)]
            ws_bytes = lib.ap_layernorm_bwd_workspace(rows, C) if 0 < C <= 4096 else 64
            n = [ctypes.c_int(-7), ctypes.c_int(-7)]
            for k in ("", "p", "q"):
                o["dx" + k], o["ws" + k] = _guard((R, Ca), bf), _guard((ws_bytes // 4,), f32)
            o["dgamma"], o["dbeta"] = torch.ones(Ca, device="cuda"), torch.ones(Ca, device="cuda")
            operands = (x.data_ptr(), gamma.data_ptr(), o["mean"].data_ptr(), o["rstd"].data_ptr(), dres.data_ptr())
            rcs.append(lib.ap_layernorm_bwd(dy.data_ptr(), *operands, o["dx"].data_ptr(), o["dgamma"].data_ptr(), o["dbeta"].data_ptr(), rows, C, o["ws"].data_ptr(), ws_bytes, st))
            rcs.append(lib.ap_layernorm_bwd_partial(dy.data_ptr(), *operands, o["dxp"].data_ptr(), rows, C, o["wsp"].data_ptr(), ws_bytes, ctypes.byref(n[0]), st))
            if pool_shape:
                rcs.append(lib.ap_layernorm_bwd_partial_pool(dy.data_ptr(), dp.data_ptr(), *pool_shape, *operands, o["dxq"].data_ptr(), C, o["wsq"].data_ptr(), ws_bytes, ctypes.byref(n[1]), st))
            # refused calls: a short workspace, no n_partial, no dgamma
            rcs.append(lib.ap_layernorm_bwd(dy.data_ptr(), *operands, o["dx"].data_ptr(), o["dgamma"].data_ptr(), o["dbeta"].data_ptr(), rows, C, o["ws"].data_ptr(), ws_bytes - 4, st))
            rcs.append(lib.ap_layernorm_bwd_partial(dy.data_ptr(), *operands, o["dxp"].data_ptr(), rows, C, o["wsp"].data_ptr(), ws_bytes, None, st))
            rcs.append(lib.ap_layernorm_bwd(dy.data_ptr(), *operands, o["dx"].data_ptr(), None, o["dbeta"].data_ptr(), rows, C, o["ws"].data_ptr(), ws_bytes, st))
            o["codes"] = torch.tensor(rcs + [n[0].value, n[1].value])
            return sum(abs(r) for r in rcs), o
        return ("layernorm rows=%d C=%d%s" % (rows, C, " pool %dx%dx%d" % pool_shape if pool_shape else ""), run)
    cases = [one(rows, C, {300: (3, 10, 10), 25088: (32, 28, 28)}.get(rows)) for C in C_LIST for rows in (0, 1, 300, 25088)]
    return cases + [one(1, 384, (1, 1, 1)), one(2, 384, (1, 2, 1))]


def _through_ops(lib, fn):
    """run fn() with autoprog_amd.ops launching through `lib`"""
    from autoprog_amd import ops
    saved, ops.lib = ops.lib, lib
    try:
        return fn()
    finally:
        ops.lib = saved


def conv_cases():
    """every convolution entry point at one small ragged shape each, through the ops wrappers (which size the statistics and workspaces by the
    library's own queries)"""
    import torch
    from autoprog_amd import ops

    def one(B, H, W):
        gen = torch.Generator().manual_seed(B * 1000 + H * 10 + W)
        x64, dy64, x128, dy128 = _bf16(gen, B, H, W, 64), _bf16(gen, B, H, W, 64), _bf16(gen, B, H, W, 128), _bf16(gen, B, H, W, 128)
        xs, dz128 = _bf16(gen, B, H, W, 16), _bf16(gen, B, H, W, 128)
        w64, w128, w7, w7b = (0.05 * torch.randn(s, generator=gen).cuda() for s in ((64, 64, 3, 3), (128, 128, 3, 3), (64, 3, 7, 7), (128, 3, 7, 7)))
        bn = tuple(t.cuda() for t in (torch.randn(64, generator=gen), torch.rand(64, generator=gen) + 0.5, torch.randn(64, generator=gen), torch.randn(64, generator=gen)))

        def run(lib):
            def body():
                o = {}
                wf, wb = ops.conv3x3_pack(w64)
                o["y"], o["stats"] = ops.conv3x3_c64(x64, wf, want_stats=True)
                o["y_plain"] = ops.conv3x3_c64(x64, wf)
                o["y_bn"], o["stats_bn"] = ops.conv3x3_c64(x64, wf, want_stats=True, bn_in=bn)
                o["y_bn_plain"] = ops.conv3x3_c64(x64, wf, bn_in=bn)
                o["da"], o["bwd_stats"] = ops.conv3x3_c64_bwd_stats(dy64, wb, x64, bn)
                o["dw"] = ops.conv3x3_c64_wgrad(x64, dy64, torch.zeros(64, 64, 3, 3, device="cuda"))
                o["dw_bn"] = ops.conv3x3_c64_wgrad(x64, dy64, torch.zeros(64, 64, 3, 3, device="cuda"), bn_in=bn)
                wf8, wb8 = ops.conv3x3_pack(w128)
                o["y128"], o["stats128"] = ops.conv3x3_c64(x128, wf8, want_stats=True)
                o["da128"] = ops.conv3x3_c64(dy128, wb8)
                o["dw128"] = ops.conv3x3_c64_wgrad(x128, dy128, torch.zeros(128, 128, 3, 3, device="cuda"))
                p7, p7b = ops.conv7_pack(w7), ops.conv7_pack(w7b)
                o["y7"], o["stats7"] = ops.conv7_s2d(xs, p7, want_stats=True)
                o["y7_plain"] = ops.conv7_s2d(xs, p7)
                o["y7_128"], o["stats7_128"] = ops.conv7_s2d(xs, p7b, want_stats=True)
                o["dw7"] = ops.conv7_s2d_wgrad(xs, dy64, torch.zeros(64, 3, 7, 7, device="cuda"))
                o["dw7_128"] = ops.conv7_s2d_wgrad(xs, dz128, torch.zeros(128, 3, 7, 7, device="cuda"))
                o["queries"] = torch.tensor([lib.ap_conv3x3_c64_stat_rows(B, H, W), lib.ap_conv3x3_c128_stat_rows(B, H, W), lib.ap_conv7_s2d_stat_rows(B, H, W),
                                             lib.ap_conv3x3_c64_wgrad_workspace(B, H, W), lib.ap_conv3x3_c128_wgrad_workspace(B, H, W), lib.ap_conv7_s2d_wgrad_workspace(B, H, W)])
                return 0, o
            return _through_ops(lib, body)
        return ("convolutions %dx%dx%d" % (B, H, W), run)
    return [one(2, 20, 37), one(1, 7, 5)]


def mlp_cases():
    """AP_MLP_FUSED_V and AP_GELU_TABLE: one ap_mlp_fused forward + backward at its smallest shape (one 128-row block), one ap_gemm_nt gelu = 3"""
    import torch
    from autoprog_amd import ops

    def fused(lib):
        gen = torch.Generator().manual_seed(5)
        x, wa, wb = _bf16(gen, 128, 384), _bf16(gen, 1152, 384, scale=0.05), _bf16(gen, 384, 1152, scale=0.05)
        b1, b2 = torch.randn(1152, generator=gen).cuda(), torch.randn(384, generator=gen).cuda()

        def body():
            f = ops.mlp_fused(x, wa, wb, bias1=b1, bias2=b2, residual=x)
            if f is None:
                return -2, {}
            b = ops.mlp_fused(x, wb.t().contiguous(), wa.t().contiguous(), backward=True, codes=f[2])
            return (0, dict(zip(("out", "hid", "codes", "dx", "dh"), f + b[:2]))) if b is not None else (-2, dict(zip(("out", "hid", "codes"), f)))
        return _through_ops(lib, body)
    return [("mlp_fused 128x384", fused), ("gemm_nt 25088x1536x384 bias gelu=3", nt.make_case(25088, 1536, 384, "bias gelu=3", 0)),
            ("gemm_nt 300x384x384 bias gelu=3", nt.make_case(300, 384, 384, "bias gelu=3", 0))]


FAMILIES = {"mhsa": mhsa_cases, "outlook": outlook_cases, "ln": ln_cases, "conv": conv_cases, "mlp": mlp_cases}


def all_cases(args):
    """--families: a setting's own kernel families (a switch reaches no other); the default setting runs them all"""
    return [c for f in args.families.split(",") for c in FAMILIES[f]()]


def cmd_bytes(args):
    import torch
    head, parent = libraries(args)
    failures = launched = total = 0
    for name, run in all_cases(args):
        (rc_a, a), (rc_b, b) = run(head), run(parent)
        torch.cuda.synchronize()
        bad = [k for k in a if k not in b or a[k].shape != b[k].shape or not torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8))]
        bad += ["return code %d / %d" % (rc_a, rc_b)] if rc_a != rc_b else []
        launched += rc_a == 0
        total += 1
        print("%-52s rc %5d  %s" % (name, rc_a, "identical (%d buffers, %d bytes)" % (len(a), sum(t.numel() * t.element_size() for t in a.values()))
                                    if not bad else "DIFFERS in " + ", ".join(bad)))
        failures += bool(bad)
    print("%s: %d cases, %d with every call accepted, %s" % (args.label, total, launched, "%d DIFFER" % failures if failures else "every case identical"))
    return 1 if failures else 0


def cmd_run(args):
    import torch
    head, parent = libraries(args)
    codes = [run(parent or head)[0] for _, run in all_cases(args)]
    torch.cuda.synchronize()
    print("%s: return codes %s" % ("parent" if parent else "head", " ".join(str(c) for c in codes)))
    return 0


def cmd_hostloop(args):
    import torch
    from autoprog_amd import ops
    head, parent = libraries(args)
    calls, st = 20000, ops._stream()
    rows, C = 64, 384
    x, dy = torch.randn(rows, C, device="cuda").to(torch.bfloat16), torch.randn(rows, C, device="cuda").to(torch.bfloat16)
    gamma, mean, rstd, dg, db = (torch.ones(n, device="cuda") for n in (C, rows, rows, C, C))
    dx = torch.empty_like(x)
    ws_bytes = head.ap_layernorm_bwd_workspace(rows, C)
    ws = torch.empty(ws_bytes // 4, device="cuda")
    xs, w7, y7 = torch.randn(1, 8, 8, 16, device="cuda").to(torch.bfloat16), torch.randn(16 * 64 * 16, device="cuda").to(torch.bfloat16), torch.empty(1, 8, 8, 64, dtype=torch.bfloat16, device="cuda")
    loops = {"ap_layernorm_bwd": lambda lib: lib.ap_layernorm_bwd(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None, dx.data_ptr(), dg.data_ptr(),
                                                                  db.data_ptr(), rows, C, ws.data_ptr(), ws_bytes, st),
             "ap_conv7_s2d_ld": lambda lib: lib.ap_conv7_s2d_ld(xs.data_ptr(), w7.data_ptr(), y7.data_ptr(), 64, 1, 8, 8, None, st)}
    for name, call in loops.items():
        for which in ("parent", "head") * 4:            # (the first pair warms up)
            lib = parent if which == "parent" else head
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                call(lib)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            print("%-18s %-6s %6.2f us per call on the launching thread (%d calls; %.2f us with the queue drained)" % (name, which, (t1 - t0) / calls * 1e6, calls, (time.perf_counter() - t0) / calls * 1e6))
    return 0


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("settings")
    for name in ("bytes", "run", "hostloop"):
        p = sub.add_parser(name)
        p.add_argument("--parent-tree", required=name != "run")
        p.add_argument("--label", default=os.environ.get("AB_SETTING", "default"))
        p.add_argument("--families", default=",".join(FAMILIES))
    p = sub.add_parser("traces")
    p.add_argument("head_csv"); p.add_argument("parent_csv"); p.add_argument("--label", default="default")
    args = ap.parse_args()
    if args.cmd == "settings":
        print("\n".join(s or "-" for s in SETTINGS))
        return 0
    if args.cmd == "traces":
        return nt.cmd_traces(args, OURS)
    return {"bytes": cmd_bytes, "run": cmd_run, "hostloop": cmd_hostloop}[args.cmd](args)


if __name__ == "__main__":
    sys.exit(main())
