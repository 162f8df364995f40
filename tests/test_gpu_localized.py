"""Localised kernel errors: per-tile parity, guard bands around every output, operands with padded leading dimensions.

tests/test_gpu_kernels.py holds each kernel to a whole-tensor rel-L2; here every 16 x 8 tile of an output is held to twice that tolerance
(tests/_tilecheck.py; tests/test_tilecheck_host.py derives the factor from the reference alone), and every case runs its kernel twice:

  compact  the operands exactly as the other tests pass them
  guarded  every output inside one allocation with 3 sentinel rows before and after and 8 .. 24 sentinel columns to its right (the alignment
           the entry point's dispatch looks at is kept, so the SAME kernel runs); every input with a widened leading dimension
           (lda = K + 8, ldb = K + 16, ldr = N + 8) whose padding columns and guard rows hold bf16 NaNs

The two outputs must be bit-identical (the weight gradients' fp32 atomics: within TOL_F32), every tile within its bound, every element
finite and every guard element unchanged.  The GEMM and attention cases run the guarded launch once more behind ops.poison_lds: a kernel
that pads its tile from LDS it never wrote is the same class of bug.  Shapes are the smallest at which ap_gemm_nt's dispatch
(csrc/nt_plan.h: nt_use_8p, the 224-row rule, the weight-stationary rule and the variant choice of nt_plan) still selects the path named in the case id with a ragged edge.

Every pointer handed to a kernel lies inside an allocation of the test: an out-of-bounds store lands in memory the test owns and inspects.
Each comparison prints one `TILED` line (whole rel, worst tile and its origin, bit identity): profiles/tiled_parity.txt is that output.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as R
from tests._tilecheck import assert_tiled, guarded, nan_padded, rel, round_up

pytestmark = pytest.mark.gpu
TOL_BF16 = 1e-2
TOL_F32 = 3e-3


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from autoprog_amd import ops as _ops
    return _ops


@pytest.fixture
def case(request):
    return request.node.name


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


def frand(*shape, seed=0, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift


def dev(t):
    return t.cuda().contiguous()


def P(t):
    return t.data_ptr() if t is not None else None


def stream():
    return torch.cuda.current_stream().cuda_stream


def gbuf(rows, cols, ld=None, dtype=torch.bfloat16, what=""):
    """a guarded 2-D output on the device: 3 sentinel rows before and after"""
    return guarded(rows, cols, ld, dtype, device="cuda", what=what)


def gflat(n, dtype=torch.float32, what=""):
    """a guarded contiguous vector of n elements on the device (mean, rstd, lse, probs, colsum, row_loss): one sentinel row before and after,
    sentinel elements behind it; 256-byte aligned like an allocation of its own -> (view [n], Guard)"""
    view, g = guarded(1, n, round_up(n, 64) + 64, dtype, pre=1, post=1, device="cuda", what=what)
    return view[0, :n], g


def padded(t, extra):
    """an input with its leading dimension widened by `extra` NaN columns, NaN guard rows around it, on the device"""
    t2 = t.reshape(-1, t.shape[-1])
    return nan_padded(t2, round_up(t2.shape[1], 8) + extra, device="cuda")


def report(case, what, rep, bit):
    print("TILED %s | %s | whole %.3e | worst tile %.3e at (%d, %d) | guarded run bit-identical: %s" % (case, what, rep.whole, rep.worst, rep[2], rep[3], bit))


def same_bits(case, what, compact, guarded_view, ref, tol, exact=True):
    """the compact output against the reference tile by tile; the guarded run bit-identical to it (hence inside the same bounds: the tile
    check of identical bits is not computed twice) -- or, exact = False (fp32 atomics), inside the bounds itself and within tol of the compact run"""
    rep = assert_tiled(compact, ref, tol, "%s %s (compact)" % (case, what))
    if exact:
        bit = torch.equal(compact, guarded_view)
        if not bit:
            assert_tiled(guarded_view, ref, tol, "%s %s (guarded; NOT bit-identical to the compact run)" % (case, what))
    else:
        bit = torch.equal(compact, guarded_view)
        assert_tiled(guarded_view, ref, tol, "%s %s (guarded)" % (case, what))
        assert rel(guarded_view, compact) < tol
    report(case, what, rep, "yes" if bit else "NO")
    assert bit or not exact, "%s %s: the guarded run differs from the compact run in %d elements" % (case, what, int((compact != guarded_view).sum()))
    return rep


# ======================================================================================================================== ap_gemm_nt
class GemmCase:
    """seeded operands of one (M, N, K) and the fp64 product, shared by the flavours of the shape"""
    _last = None

    def __init__(self, M, N, K):
        self.M, self.N, self.K = M, N, K
        self.a, self.w = rnd(M, K, seed=1), rnd(N, K, scale=K ** -0.5, seed=2)
        self.bias = frand(N, seed=3)
        self.res = rnd(M, N, seed=4)
        self.rps = rps = 16 if M <= 256 else 64
        self.rs = (torch.rand((M + rps - 1) // rps, generator=torch.Generator().manual_seed(5)) > 0.2).float() / 0.8
        self.rs[0], self.rs[-1] = 0.0, 1.25                # a dropped DropPath sample (the residual passes through); the ragged last group is kept
        self.lin = self.a.double() @ self.w.double().t()
        self.rsr = self.rs.double().repeat_interleave(rps)[:M, None]

    @property
    def mulb(self):
        return rnd(self.M, self.N, seed=6)

    @property
    def mul8(self):
        return torch.randint(0, 256, (self.M, self.N), dtype=torch.uint8, generator=torch.Generator().manual_seed(7))

    @classmethod
    def get(cls, M, N, K):
        if cls._last is None or (cls._last.M, cls._last.N, cls._last.K) != (M, N, K):
            cls._last = cls(M, N, K)
        return cls._last


def gemm_launch(ops, c, flavour, extra_ldc):
    """extra_ldc = None: the compact run; else the guarded run with ldc = round_up(N, 8) + extra_ldc -> (out [M, N], codes [M, N] or None, guards)"""
    M, N, K = c.M, c.N, c.K
    n8 = round_up(N, 8)
    guards = []
    if extra_ldc is None:
        side = lambda t: dev(F.pad(t, (0, n8 - N)))                              # residual / mul_by with the output's leading dimension
        a, w, ldc = dev(c.a), dev(c.w), n8
        out = torch.empty(M, ldc, dtype=torch.bfloat16, device="cuda")
        codes = torch.empty(M, ldc, dtype=torch.uint8, device="cuda")
    else:
        ldc = n8 + extra_ldc
        a, w = padded(c.a, 8), padded(c.w, 16)
        out, g = gbuf(M, N, ldc, what="C")
        guards.append(g)
        codes, g = gbuf(M, N, ldc, torch.uint8, what="gelu' codes")
        side = lambda t: nan_padded(t, ldc, device="cuda")                        # (mul_by / mul_by8: ld = ldc, include/autoprog_hip.h)
        if flavour == "gelu8":
            guards.append(g)
    kw = dict(n=N, k=K, out=out)
    if flavour == "plain":
        pass
    elif flavour == "bias_res_rs":
        res = side(c.res) if extra_ldc is None else nan_padded(c.res, n8 + 8, device="cuda")          # ldr = N + 8
        kw.update(bias=dev(c.bias), residual=res, row_scale=dev(c.rs), rows_per_scale=c.rps)
    elif flavour == "gelu8":
        kw.update(bias=dev(c.bias), gelu=True, preact_out=codes, preact_grad=2)
    elif flavour == "mulby":
        kw.update(mul_by=side(c.mulb))
    elif flavour == "mul8":
        kw.update(mul_by=side(c.mul8))
    else:
        raise ValueError(flavour)
    ops.gemm_nt(a, w, **kw)
    torch.cuda.synchronize()
    return out, (codes if flavour == "gelu8" else None), guards


def gemm_reference(ops, c, flavour):
    """-> (fp64 output, fp64 gelu' of the bf16-rounded pre-activation or None)"""
    if flavour == "plain":
        return c.lin, None
    if flavour == "bias_res_rs":
        return (c.lin + c.bias.double()) * c.rsr + c.res.double(), None
    if flavour == "mulby":
        return c.lin * c.mulb.double(), None
    if flavour == "mul8":
        return c.lin * ((c.mul8.double() - ops.GELU_CODE_ZERO) / ops.GELU_CODE_SCALE), None
    h = (c.lin + c.bias.double()).to(torch.bfloat16).double().requires_grad_(True)
    F.gelu(h).sum().backward()
    return F.gelu(h.detach()), h.grad


# (id prefix = the path the shape is meant to hit, M, N, K, flavours, extra ldc columns of the guarded run)
_ALL = ("plain", "bias_res_rs", "gelu8")
GEMM_CASES = [
    ("few-rows", 65, 40, 40, _ALL, 8),
    ("few-rows-ragged-N", 65, 37, 40, _ALL, 8),                       # N % 8 != 0: the last chunk's padding columns must stay untouched
    ("few-rows", 256, 1000, 384, _ALL, 24),
    ("64x64", 257, 200, 72, _ALL, 8),                                 # N <= 512, K <= 256
    ("64x64-ragged-N", 257, 197, 72, _ALL, 8),
    ("128x64-direct-epilogue", 257, 576, 264, _ALL, 8),               # N % 128 != 0, N % 64 == 0
    ("128x128", 257, 392, 264, _ALL + ("mulby",), 8),                 # bias_res_rs / mulby: the prefetching instantiation (residual xor mul_by)
    ("128x128-ragged-N", 257, 390, 264, _ALL + ("mulby",), 8),        # the prefetched 16-byte chunk of residual / mul_by straddles column N
    ("8p-192-224rows", 4097, 192, 128, ("plain", "bias_res_rs"), 8),  # 19 tiles of 224 rows > 17 of 256: nt_plan takes the 224-row instantiation
    ("8p-192-256rows", 4097, 192, 128, ("gelu8",), 8),                # (no 224-row instantiation of this flavour: nt_has224)
    ("8p-192-224rows", 4100, 384, 1152, ("plain", "bias_res_rs"), 8),
    ("8p-192-256rows", 4100, 384, 1152, ("gelu8",), 8),
    ("8p-256-masked-last-column-tile", 4097, 1032, 128, _ALL, 8),     # N >= 1024: 256-wide tiles, the fifth holds 8 columns
    ("8p-256-second-tile-per-workgroup", 8193, 2056, 128, ("plain", "bias_res_rs"), 8),   # 33 x 9 = 297 tiles on at most 256 workgroups
    # 256-row x 192 tiles by default: fewer than #CU tiles of 256 rows but MORE than #CU of 224 (2 * 129 = 258 > 256 >= 2 * 113): the smallest such M at N = 384
    ("8p-192-256rows-224-does-not-fit", 28673, 384, 128, ("plain",), 8),
    # K = 192, M >= 16384, M % 64 == 0, N % 192 == 0: ldc % 16 == 0 keeps nt_plan's choice of the weight-stationary kernel (ldc = N + 16)
    ("weight-stationary-ldc16", 16384 + 64, 576, 192, ("gelu8", "mul8"), 16),
]
GEMM_PARAMS = [pytest.param(p, M, N, K, f, e, id="%s-%dx%dx%d-%s" % (p, M, N, K, f)) for (p, M, N, K, fl, e) in GEMM_CASES for f in fl]


@pytest.mark.parametrize("path,M,N,K,flavour,extra", GEMM_PARAMS)
def test_gemm_nt_localized(ops, case, path, M, N, K, flavour, extra):
    """Columns N .. ldc-1 of C and of preact_out are never written: include/autoprog_hip.h says so at ap_gemm_nt (every kernel stores through
    epi_chunk, csrc/gemm_epi.h, which stores min(8, N - n) elements of a chunk; the 8-phase and weight-stationary kernels take N % 8 == 0 only) --
    so the guard checks run with pad="untouched"."""
    c = GemmCase.get(M, N, K)
    ref, dgelu = gemm_reference(ops, c, flavour)
    out_c, codes_c, _ = gemm_launch(ops, c, flavour, None)
    for poison in (False, True):
        if poison:
            ops.poison_lds()
        out_g, codes_g, guards = gemm_launch(ops, c, flavour, extra)
        tag = "C behind poisoned LDS" if poison else "C"
        same_bits(case, tag, out_c[:, :N], out_g[:, :N], ref, TOL_BF16)
        for g in guards:
            g.check(pad="untouched")
        if codes_c is not None:
            assert torch.equal(codes_c[:, :N], codes_g[:, :N]), "%s: the gelu' codes of the guarded run differ" % case
    if codes_c is not None:
        # the codes against fp64 as tests/test_gpu_kernels.py::test_gemm_nt_weight_stationary_k192 holds them: the kernel rounds ITS fp32
        # pre-activation to bf16; where that lands on the other side of a rounding tie the fp64 code differs by more than one
        want = torch.clamp(torch.round(dgelu * ops.GELU_CODE_SCALE) + ops.GELU_CODE_ZERO, 0, 255)
        dcode = (codes_c[:, :N].cpu().double() - want).abs()
        assert float((dcode <= 1).double().mean()) > 0.999 and float(dcode.max()) < 6, (float((dcode <= 1).double().mean()), float(dcode.max()))


# ====================================================================================================================== ap_mlp_fused
def _mlp_args(**kw):
    from autoprog_amd._lib import MlpFusedArgs
    a = MlpFusedArgs()
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("m", [128, 384])
@pytest.mark.parametrize("ln", [False, True], ids=["rows-given", "layernorm-in-launch"])
def test_mlp_fused_localized(ops, case, m, ln):
    """ap_mlp_fused through the library itself (the ops wrapper allocates its own outputs), forward and backward: out, hidden_out, codes,
    ln_out, ln_mean, ln_rstd guarded; ldx, ldo, ldh, ldr, ld_ln, ld_lno wider than the widths.  ap_mlp_fused accepts any stride that is a
    multiple of 8 and at least the width (csrc/mlp_fused.hip: the checks in front of mf_launch) and answers AP_ERR_SHAPE to anything else."""
    from autoprog_amd._lib import lib
    C, H, rps = 384, 1152, 64
    x, w1, w2 = rnd(m, C, seed=1), rnd(H, C, scale=C ** -0.5, seed=2), rnd(C, H, scale=H ** -0.5, seed=3)
    b1, b2 = frand(H, seed=4, scale=0.3), frand(C, seed=5, scale=0.3)
    res, dy = rnd(m, C, seed=6), rnd(m, C, seed=7)
    keep = torch.ones(m // rps)
    keep[0] = 0.0
    lg, lb = frand(C, seed=8, scale=0.3, shift=1.0), frand(C, seed=9, scale=0.2)
    xin = (x.float() * 2.5 + 1.5).to(torch.bfloat16)                           # rows with a mean and a spread for the LayerNorm
    st = stream()
    dw1, dw2, db1, db2, dkeep, drs = dev(w1), dev(w2), dev(b1), dev(b2), dev(keep), dev(keep / 0.8)
    dlg, dlb = dev(lg), dev(lb)

    def forward(wide):
        ex = (lambda k: k) if wide else (lambda k: 0)
        guards = []
        mk = (lambda rows, cols, extra, dt, what: gbuf(rows, cols, cols + ex(extra), dt, what)) if wide else \
             (lambda rows, cols, extra, dt, what: (torch.empty(rows, cols, dtype=dt, device="cuda"), None))
        mkv = (lambda n, what: gflat(n, what=what)) if wide else (lambda n, what: (torch.empty(n, device="cuda"), None))
        out, g0 = mk(m, C, 8, torch.bfloat16, "out")
        hid, g1 = mk(m, H, 8, torch.bfloat16, "hidden_out")
        codes, g2 = mk(m, H, 8, torch.uint8, "codes")
        rows_in = xin if ln else x
        xd = padded(rows_in, 8) if wide else dev(rows_in)
        rd = padded(rows_in if ln else res, 16) if wide else dev(rows_in if ln else res)      # (with the LayerNorm the residual is its input, as in the block)
        a = _mlp_args(wa=P(dw1), ldwa=C, wb=P(dw2), ldwb=H, out=P(out), ldo=out.shape[1], hidden_out=P(hid), ldh=hid.shape[1], codes=P(codes),
                      bias1=P(db1), bias2=P(db2), row_scale_hidden=P(dkeep), row_scale_out=P(drs), rows_per_scale=rps,
                      residual=P(rd), ldr=rd.shape[1], m=m, c=C, hidden=H, backward=0)
        assert codes.shape[1] == hid.shape[1]                                    # the codes' row stride is ldh bytes
        extra_out = ()
        if ln:
            lno, g3 = mk(m, C, 24, torch.bfloat16, "ln_out")
            mean, g4 = mkv(m, "ln_mean")
            rstd, g5 = mkv(m, "ln_rstd")
            a.x, a.ln_in, a.ld_ln, a.ln_out, a.ld_lno = None, P(xd), xd.shape[1], P(lno), lno.shape[1]
            a.ln_gamma, a.ln_beta, a.ln_eps, a.ln_mean, a.ln_rstd = P(dlg), P(dlb), 1e-5, P(mean), P(rstd)
            extra_out = (lno[:, :C], mean, rstd)
            guards += [g3, g4, g5]
        else:
            a.x, a.ldx = P(xd), xd.shape[1]
        rc = lib.ap_mlp_fused(ctypes.byref(a), st)
        assert rc == 0, "ap_mlp_fused refused a launch it is built for (code %d)" % rc
        torch.cuda.synchronize()
        keepalive = (xd, rd)
        return (out[:, :C], hid[:, :H], codes[:, :H]) + extra_out, [g for g in [g0, g1, g2] + guards if g is not None], a, keepalive

    outs_c, _, _, _ = forward(False)
    outs_g, guards, a_g, alive = forward(True)
    for g in guards:
        g.check(pad="untouched")
    rows_in = xin if ln else x
    if ln:
        xr = rows_in.double()
        mu, var = xr.mean(1, keepdim=True), xr.var(1, unbiased=False, keepdim=True)
        same_bits(case, "ln_out", outs_c[3], outs_g[3], (xr - mu) / (var + 1e-5).sqrt() * lg.double() + lb.double(), TOL_BF16)
        # fp32 statistics of 384 values: 6e-8 * sqrt(384) ~ 1e-6 from the fp64 ones
        assert torch.equal(outs_c[4], outs_g[4]) and torch.equal(outs_c[5], outs_g[5])
        assert rel(outs_c[4], mu[:, 0]) < 1e-5 and rel(outs_c[5], (var[:, 0] + 1e-5).rsqrt()) < 1e-5
        fc1_in = outs_c[3].double().cpu()                                        # fc1 reads the ROUNDED normalised rows
    else:
        fc1_in = x.double()
    kk = keep.double().repeat_interleave(rps)[:, None]
    h = (fc1_in @ w1.double().t() + b1.double()).to(torch.bfloat16).double().requires_grad_(True)
    F.gelu(h).sum().backward()
    same_bits(case, "hidden_out", outs_c[1], outs_g[1], F.gelu(h.detach()) * kk, TOL_BF16)
    assert torch.equal(outs_c[2], outs_g[2]), "codes differ"
    want = torch.clamp(torch.round(h.grad * ops.GELU_CODE_SCALE) + ops.GELU_CODE_ZERO, 0, 255)
    dcode = (outs_c[2].cpu().double() - want).abs()
    assert float((dcode <= 1).double().mean()) > 0.999 and float(dcode.max()) < 6
    resid = rows_in if ln else res
    yref = (outs_c[1].double().cpu() @ w2.double().t() + b2.double()) * (kk / 0.8) + resid.double()      # fc2 reads the ROUNDED hidden activation
    same_bits(case, "out", outs_c[0], outs_g[0], yref, TOL_BF16)
    # what the entry point refuses: strides that are no multiple of 8 or narrower than the width -> AP_ERR_SHAPE, nothing launched
    for field, bad in (("ldo", C + 4), ("ldh", H - 8), ("ldr", C + 2)) + ((("ld_ln", C + 4), ("ld_lno", C - 8)) if ln else (("ldx", C + 4),)):
        good = getattr(a_g, field)
        setattr(a_g, field, bad)
        assert lib.ap_mlp_fused(ctypes.byref(a_g), st) == -1, field
        setattr(a_g, field, good)
    if ln:
        return
    # backward: dL/dh = (dy W2) gelu'(code) rs, dL/dx = dL/dh W1 -- on the forward's own codes
    codes = outs_c[2].contiguous()
    w2t, w1t = dev(w2.t().contiguous()), dev(w1.t().contiguous())

    def backward(wide):
        if wide:
            out, g0 = gbuf(m, C, C + 8, what="dx")
            hid, g1 = gbuf(m, H, H + 8, what="dL/dh")
            cd = nan_padded(codes.cpu(), H + 8, device="cuda")
            dyd = padded(dy, 8)
        else:
            out, hid, cd, dyd, g0, g1 = torch.empty(m, C, dtype=torch.bfloat16, device="cuda"), torch.empty(m, H, dtype=torch.bfloat16, device="cuda"), codes, dev(dy), None, None
        a = _mlp_args(x=P(dyd), ldx=dyd.shape[1], wa=P(w2t), ldwa=C, wb=P(w1t), ldwb=H, out=P(out), ldo=out.shape[1], hidden_out=P(hid), ldh=hid.shape[1],
                      codes=P(cd), row_scale_hidden=P(drs), rows_per_scale=rps, m=m, c=C, hidden=H, backward=1)
        assert lib.ap_mlp_fused(ctypes.byref(a), st) == 0
        torch.cuda.synchronize()
        return out[:, :C], hid[:, :H], [g for g in (g0, g1) if g is not None]
    dx_c, dh_c, _ = backward(False)
    dx_g, dh_g, guards = backward(True)
    for g in guards:
        g.check(pad="untouched")
    gp = (codes.cpu().double() - ops.GELU_CODE_ZERO) / ops.GELU_CODE_SCALE
    same_bits(case, "dL/dh", dh_c, dh_g, (dy.double() @ w2.double()) * gp * (kk / 0.8), TOL_BF16)
    same_bits(case, "dL/dx", dx_c, dx_g, dh_c.double().cpu() @ w1.double(), TOL_BF16)


# ============================================================================================= ap_gemm_tn_acc, ap_gemm_tn_acc_grouped
def _wgrad_problem(i, M, N1, N2, wide):
    """-> (problem tuple for ops.gemm_tn_acc_grouped, reference C, reference colsum, guards, C view [N1, N2], colsum view).  C and the column sum
    start from a seeded NON-ZERO base: the contract is += (include/autoprog_hip.h, ap_gemm_tn_acc)."""
    a, b = rnd(M, N1, seed=10 + i), rnd(M, N2, seed=40 + i)
    c0, cs0 = frand(N1, N2, seed=70 + i), frand(N1, seed=90 + i)
    ref_c = c0.double() + a.double().t() @ b.double()
    ref_cs = cs0.double() + a.double().sum(0)
    if wide:
        ad, bd = padded(a, 8), padded(b, 16)
        c, g0 = gbuf(N1, N2, round_up(N2, 8) + 8, torch.float32, "C")
        cs, g1 = gflat(N1, what="colsum_A")
        guards = [g0, g1]
    else:
        ad, bd = dev(F.pad(a, (0, round_up(N1, 8) - N1))), dev(F.pad(b, (0, round_up(N2, 8) - N2)))
        c = torch.empty(N1, round_up(N2, 8), device="cuda")
        cs, guards = torch.empty(N1, device="cuda"), []
    c[:, :N2] = c0.cuda()
    cs.copy_(cs0)
    if wide:                                  # the base was written through the view: the guards' picture of the buffer is taken now
        for g in guards:
            g.before = g.whole.detach().cpu().view(g.before.dtype).clone()
    return (ad, bd, c, N1, N2, cs), ref_c, ref_cs, guards, c[:, :N2], cs


WGRAD_SINGLE = [pytest.param(4160, 192, 384, id="8p-tile-kernel-4160x192x384"),                      # N1, N2 % 192 == 0, M % 64 == 0, M >= 4096 (tn8_fits)
                pytest.param(4161, 192, 384, id="128x128-ragged-token-tail-4161x192x384"),          # one token more: not the tile kernel's any more
                pytest.param(130, 200, 75, id="small-ragged-N2-130x200x75"), pytest.param(4161, 1000, 40, id="ragged-widths-4161x1000x40")]


@pytest.mark.parametrize("M,N1,N2", WGRAD_SINGLE)
def test_gemm_tn_acc_localized(ops, case, M, N1, N2):
    """C[N1, N2] += A^T B: nothing outside [N1, N2] is written (fp32: no 16-byte chunk to round up to), so pad="untouched" """
    pc, ref_c, ref_cs, _, c_c, cs_c = _wgrad_problem(0, M, N1, N2, False)
    ops.gemm_tn_acc(pc[0], pc[1], pc[2], n1=N1, n2=N2, colsum=pc[5])
    pg, _, _, guards, c_g, cs_g = _wgrad_problem(0, M, N1, N2, True)
    ops.gemm_tn_acc(pg[0], pg[1], pg[2], n1=N1, n2=N2, colsum=pg[5])
    torch.cuda.synchronize()
    for g in guards:
        g.check(pad="untouched")
    same_bits(case, "C", c_c, c_g, ref_c, TOL_F32, exact=False)
    assert bool(torch.isfinite(cs_g).all())
    assert rel(cs_c, ref_cs) < TOL_F32 and rel(cs_g, ref_cs) < TOL_F32


@pytest.mark.parametrize("mode", ["atomic", "workspace"])
def test_gemm_tn_acc_grouped_localized(ops, case, mode):
    """one launch whose problems differ in shape, so that a problem's last tile borders another problem's first: tile-kernel problems
    (192-multiples, M % 64 == 0) next to ragged ones.  workspace: the deterministic mode -- its guarded run is bit-identical."""
    shapes = [(4160, 192, 384), (130, 200, 72), (4161, 40, 1000), (4224, 384, 192), (77, 37, 96)]
    old = ops.deterministic
    try:
        ops.deterministic = mode == "workspace"
        built_c = [_wgrad_problem(i, *s, False) for i, s in enumerate(shapes)]
        ops.gemm_tn_acc_grouped([b[0] for b in built_c])
        built_g = [_wgrad_problem(i, *s, True) for i, s in enumerate(shapes)]
        ops.gemm_tn_acc_grouped([b[0] for b in built_g])
        torch.cuda.synchronize()
    finally:
        ops.deterministic = old
    for s, bc, bg in zip(shapes, built_c, built_g):
        for g in bg[3]:
            g.check(pad="untouched")
        same_bits(case, "C of %dx%dx%d" % s, bc[4], bg[4], bc[1], TOL_F32, exact=mode == "workspace")
        assert bool(torch.isfinite(bg[5]).all())
        assert rel(bc[5], bc[2]) < TOL_F32 and rel(bg[5], bc[2]) < TOL_F32
        if mode == "workspace":
            assert torch.equal(bc[5], bg[5])


# ============================================================================================================ ap_mhsa_fwd / ap_mhsa_bwd
MHSA_CASES = [pytest.param(1, 193, 1, 32, id="resident-one-key-last-tile-1x193x1x32"),          # 12 full key tiles + one key; a query tile of one row
              pytest.param(2, 208, 2, 32, id="resident-full-last-tile-2x208x2x32"),
              pytest.param(1, 257, 1, 32, id="blocked-1x257x1x32"), pytest.param(1, 130, 2, 48, id="blocked-hd48-1x130x2x48"),
              pytest.param(65, 100, 4, 32, id="persistent-260-items-on-256-workgroups-65x100x4x32")]      # 7 query tiles: the persistent kernels, some workgroups take two items


@pytest.mark.parametrize("B,N,heads,hd", MHSA_CASES)
def test_mhsa_localized(ops, case, B, N, heads, hd):
    """out, lse, dqkv guarded (the entry points take no leading dimensions: guard rows around each, and sentinel elements behind lse);
    qkv / dout between NaN guard rows; once more behind poisoned LDS"""
    from autoprog_amd._lib import lib
    C = heads * hd
    qkv, do = rnd(B * N, 3 * C, seed=1), rnd(B * N, C, seed=2)
    scale = hd ** -0.5
    qr = qkv.double().reshape(B, N, 3 * C).requires_grad_(True)
    orf = R.mhsa_core(qr, heads)
    orf.backward(do.double().reshape(B, N, C))
    q, k, _ = qkv.double().reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    lse_ref = torch.logsumexp(q @ k.transpose(-1, -2) * scale, dim=-1)
    o_c, lse_c = ops.mhsa_fwd(dev(qkv), B, N, heads, scale)
    d_c = ops.mhsa_bwd(dev(qkv), o_c, dev(do), lse_c, B, N, heads, scale)
    assert float((lse_c.cpu().double() - lse_ref).abs().max()) < 2e-3
    ws_bytes = lib.ap_mhsa_bwd_workspace(B, N, heads, hd)
    for poison in (False, True):
        if poison:
            ops.poison_lds()
        qd, dod = padded(qkv, 0), padded(do, 0)
        o_g, g0 = gbuf(B * N, C, C, what="out")
        lse_g, g1 = gflat(B * heads * N, what="lse")
        d_g, g2 = gbuf(B * N, 3 * C, 3 * C, what="dqkv")
        ws = torch.empty(max(ws_bytes // 4, 1), device="cuda")
        st = stream()
        assert lib.ap_mhsa_fwd(P(qd), P(o_g), P(lse_g), B, N, heads, hd, scale, None, st) == 0
        assert lib.ap_mhsa_bwd(P(qd), P(o_g), P(dod), P(lse_g), P(d_g), B, N, heads, hd, scale, P(ws) if ws_bytes else None, ws_bytes, st) == 0
        torch.cuda.synchronize()
        for g in (g0, g1, g2):
            g.check(pad="untouched")
        tag = " behind poisoned LDS" if poison else ""
        same_bits(case, "out" + tag, o_c, o_g, orf.reshape(B * N, C), TOL_BF16)
        assert torch.equal(lse_c.reshape(-1), lse_g), "lse differs"
        gr, dc, dg = qr.grad.reshape(B * N, 3, C), d_c.reshape(B * N, 3, C), d_g.reshape(B * N, 3, C)
        for i, nm in enumerate("qkv"):
            same_bits(case, "d" + nm + tag, dc[:, i], dg[:, i], gr[:, i], 1.5e-2)


# ================================================================================================== ap_class_attn_fwd / ap_class_attn_bwd
@pytest.mark.parametrize("B,N,heads,hd", [(3, 65, 2, 32), (2, 50, 2, 48)])
def test_class_attention_localized(ops, case, B, N, heads, hd):
    from autoprog_amd._lib import lib
    C = heads * hd
    q, kv, do = rnd(B, C, seed=1), rnd(B * N, 2 * C, seed=2), rnd(B, C, seed=3)
    scale = hd ** -0.5
    qr = q.double().requires_grad_(True)
    kvr = kv.double().reshape(B, N, 2, heads, hd).requires_grad_(True)
    kk, vv = kvr[:, :, 0].transpose(1, 2), kvr[:, :, 1].transpose(1, 2)
    att = torch.softmax((qr.reshape(B, heads, 1, hd) * scale) @ kk.transpose(-1, -2), dim=-1)
    orf = (att @ vv).transpose(1, 2).reshape(B, C)
    orf.backward(do.double())
    o_c, p_c = ops.class_attn_fwd(dev(q), dev(kv), B, N, heads, scale)
    dq_c, dkv_c = ops.class_attn_bwd(dev(q), dev(kv), p_c, dev(do), B, N, heads, scale)
    assert rel(p_c, att.reshape(B, heads, N)) < 1e-3
    for poison in (False, True):
        if poison:
            ops.poison_lds()
        qd, kvd, dod = padded(q, 0), padded(kv, 0), padded(do, 0)
        o_g, g0 = gbuf(B, C, C, what="out")
        p_g, g1 = gflat(B * heads * N, what="probs")
        dq_g, g2 = gbuf(B, C, C, what="dq")
        dkv_g, g3 = gbuf(B * N, 2 * C, 2 * C, what="dkv")
        st = stream()
        assert lib.ap_class_attn_fwd(P(qd), P(kvd), None, P(o_g), P(p_g), B, N, heads, hd, scale, st) == 0
        assert lib.ap_class_attn_bwd(P(qd), P(kvd), None, P(p_g), P(dod), P(dq_g), P(dkv_g), None, B, N, heads, hd, scale, st) == 0
        torch.cuda.synchronize()
        for g in (g0, g1, g2, g3):
            g.check(pad="untouched")
        tag = " behind poisoned LDS" if poison else ""
        same_bits(case, "out" + tag, o_c, o_g, orf, TOL_BF16)
        assert torch.equal(p_c.reshape(-1), p_g), "probs differ"
        same_bits(case, "dq" + tag, dq_c, dq_g, qr.grad, TOL_BF16)
        same_bits(case, "dkv" + tag, dkv_c, dkv_g, kvr.grad.reshape(B * N, 2 * C), TOL_BF16)


# ====================================================================================================== ap_outlook_fwd / ap_outlook_bwd
@pytest.mark.parametrize("B,H,W,heads", [(2, 7, 7, 2), (1, 5, 9, 1)])
def test_outlook_localized(ops, case, B, H, W, heads):
    """odd maps; the logits' ldl wider than round_up(heads * 81, 8) with NaN padding.  dlogits shares ldl: its columns heads * 81 .. ldl-1 are
    ZEROED (include/autoprog_hip.h at ap_outlook_bwd; tests/test_gpu_kernels.py::test_outlook_core asserts it for the compact ldl)."""
    from autoprog_amd._lib import lib
    C, hd = heads * 32, 32
    h, w = (H + 1) // 2, (W + 1) // 2
    nl = heads * 81
    ldl_c, ldl_g = round_up(nl, 8), round_up(nl, 8) + 16
    v, dy = rnd(B, H, W, C, seed=1), rnd(B, H, W, C, seed=3)
    lg = rnd(B * h * w, nl, scale=2.0, seed=2)
    scale = hd ** -0.5
    vr = v.double().requires_grad_(True)
    lr = lg.double().reshape(B, h, w, nl).requires_grad_(True)
    yr = R.outlook_core(vr, lr, heads)
    yr.backward(dy.double())
    lg_c = dev(F.pad(lg, (0, ldl_c - nl)))
    y_c = ops.outlook_fwd(dev(v), lg_c, heads, scale)
    dv_c, dl_c = ops.outlook_bwd(dev(v), lg_c, dev(dy), heads, scale)
    vd, dyd, lgd = padded(v, 0), padded(dy, 0), nan_padded(lg, ldl_g, device="cuda")
    y_g, g0 = gbuf(B * H * W, C, C, what="y")
    dv_g, g1 = gbuf(B * H * W, C, C, what="dv")
    dl_g, g2 = gbuf(B * h * w, ldl_g, ldl_g, what="dlogits")
    st = stream()
    assert lib.ap_outlook_fwd(P(vd), P(lgd), ldl_g, P(y_g), B, H, W, heads, hd, scale, st) == 0
    assert lib.ap_outlook_bwd(P(vd), P(lgd), ldl_g, P(dyd), P(dv_g), P(dl_g), B, H, W, heads, hd, scale, st) == 0
    torch.cuda.synchronize()
    for g in (g0, g1, g2):
        g.check(pad="untouched")
    same_bits(case, "y", y_c.reshape(-1, C), y_g, yr.reshape(-1, C), TOL_BF16)
    same_bits(case, "dv", dv_c.reshape(-1, C), dv_g, vr.grad.reshape(-1, C), TOL_BF16)
    same_bits(case, "dlogits", dl_c[:, :nl], dl_g[:, :nl], lr.grad.reshape(-1, nl), TOL_BF16)
    assert float(dl_c[:, nl:].float().abs().sum()) == 0.0 and bool((dl_g[:, nl:].view(torch.int16) == 0).all())


# ============================================================================================================================ LayerNorm
@pytest.mark.parametrize("rows,C", [(33, 64), (777, 384), (20, 1152)])
def test_layernorm_localized(ops, case, rows, C):
    """row counts that do not fill the last workgroup's row groups; y, mean, rstd, dx guarded; x / dy / dres between NaN guard rows.
    dgamma / dbeta are ACCUMULATED (include/autoprog_hip.h, ap_layernorm_bwd): they start from a seeded non-zero base."""
    from autoprog_amd._lib import lib
    x = rnd(rows, C, scale=2.0, seed=1) + 0.5
    g, b = frand(C, seed=2, scale=0.3, shift=1.0), frand(C, seed=3, scale=0.3)
    dy, dres = rnd(rows, C, seed=4), rnd(rows, C, seed=5)
    dg0, db0 = frand(C, seed=6), frand(C, seed=7)
    xr, gr, br = x.double().requires_grad_(True), g.double().requires_grad_(True), b.double().requires_grad_(True)
    yr = R.layernorm(xr, gr, br, 1e-5)
    yr.backward(dy.double())
    y_c, mean_c, rstd_c = ops.layernorm_fwd(dev(x), dev(g), dev(b), 1e-5)
    dg_c, db_c = dev(dg0), dev(db0)
    dx_c = ops.layernorm_bwd(dev(dy), dev(x), dev(g), mean_c, rstd_c, dev(dres), dg_c, db_c)
    xd, dyd, dresd = padded(x, 0), padded(dy, 0), padded(dres, 0)
    y_g, g0 = gbuf(rows, C, C, what="y")
    mean_g, g1 = gflat(rows, what="mean")
    rstd_g, g2 = gflat(rows, what="rstd")
    dx_g, g3 = gbuf(rows, C, C, what="dx")
    dg_g, g4 = gflat(C, what="dgamma")
    db_g, g5 = gflat(C, what="dbeta")
    dg_g.copy_(dg0)
    db_g.copy_(db0)
    ws_bytes = lib.ap_layernorm_bwd_workspace(rows, C)
    ws = torch.empty(max(ws_bytes // 4, 1), device="cuda")
    st, gd = stream(), dev(g)
    assert lib.ap_layernorm_fwd(P(xd), P(gd), P(dev(b)), P(y_g), P(mean_g), P(rstd_g), rows, C, 1e-5, st) == 0
    assert lib.ap_layernorm_bwd(P(dyd), P(xd), P(gd), P(mean_g), P(rstd_g), P(dresd), P(dx_g), P(dg_g), P(db_g), rows, C, P(ws), ws_bytes, st) == 0
    torch.cuda.synchronize()
    for gq in (g0, g1, g2, g3):
        gq.check(pad="untouched")
    for gq in (g4, g5):                       # (accumulated in place: only what lies around the vector is guarded)
        now = gq.whole.detach().cpu().view(torch.int32)
        assert torch.equal(now[0], gq.before[0]) and torch.equal(now[2], gq.before[2]) and torch.equal(now[1, C:], gq.before[1, C:]), gq.what
    same_bits(case, "y", y_c, y_g, yr.detach(), TOL_BF16)
    assert torch.equal(mean_c, mean_g) and torch.equal(rstd_c, rstd_g)
    mu = x.double().mean(1)
    assert rel(mean_c, mu) < 1e-5 and rel(rstd_c, (x.double().var(1, unbiased=False) + 1e-5).rsqrt()) < 1e-5      # fp32 statistics of <= 1152 values
    same_bits(case, "dx", dx_c, dx_g, xr.grad + dres.double(), TOL_BF16)
    assert torch.equal(dg_c, dg_g) and torch.equal(db_c, db_g)                  # the two-pass column reduction is deterministic
    assert rel(dg_c, dg0.double() + gr.grad) < TOL_F32 and rel(db_c, db0.double() + br.grad) < TOL_F32


@pytest.mark.parametrize("B,H,W,C", [(1, 3, 11, 64), (3, 7, 37, 384), (1, 4, 5, 1152)])
def test_layernorm_bwd_partial_pool_localized(ops, case, B, H, W, C):
    """the same row counts as token grids (33 = 3 x 11, 777 = 3 x 7 x 37, 20 = 4 x 5); C = 1152 is refused (AP_ERR_UNSUPPORTED: C > 512)"""
    from autoprog_amd._lib import lib
    rows = B * H * W
    gen = torch.Generator().manual_seed(B * 100 + H)
    x, dy, dres = (torch.randn(B, H, W, C, generator=gen).bfloat16() for _ in range(3))
    hh, ww = (H + 1) // 2, (W + 1) // 2
    dp = torch.randn(B, hh, ww, C, generator=gen).bfloat16()
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)
    xd = dev(x)
    yk, mean, rstd = ops.layernorm_fwd(xd.view(-1, C), dev(gamma), dev(beta), 1e-5)
    ws_bytes = lib.ap_layernorm_bwd_workspace(rows, C)
    st, gd = stream(), dev(gamma)

    def run(wide):
        if wide:
            dyd, dpd, xq, dresd = padded(dy, 0), padded(dp, 0), padded(x, 0), padded(dres, 0)
            dx, g0 = gbuf(rows, C, C, what="dx")
        else:
            dyd, dpd, xq, dresd, g0 = dev(dy), dev(dp), xd, dev(dres), None
            dx = torch.empty(rows, C, dtype=torch.bfloat16, device="cuda")
        ws = torch.empty(max(ws_bytes // 4, 1), device="cuda")
        n = ctypes.c_int(0)
        rc = lib.ap_layernorm_bwd_partial_pool(P(dyd), P(dpd), B, H, W, P(xq), P(gd), P(mean), P(rstd), P(dresd), P(dx), C, P(ws), ws_bytes, ctypes.byref(n), st)
        torch.cuda.synchronize()
        return rc, dx, g0
    rc, dx_c, _ = run(False)
    if C > 512:
        assert rc == -2
        return
    assert rc == 0
    rc, dx_g, g0 = run(True)
    assert rc == 0
    g0.check(pad="untouched")
    x64 = x.double().requires_grad_(True)
    y = F.layer_norm(x64, (C,), gamma.double(), beta.double(), 1e-5)
    pooled = F.avg_pool2d(y.permute(0, 3, 1, 2), 2, 2, ceil_mode=True, count_include_pad=False).permute(0, 2, 3, 1)
    ((y * dy.double()).sum() + (pooled * dp.double()).sum()).backward()
    same_bits(case, "dx", dx_c, dx_g, (x64.grad + dres.double()).reshape(rows, C), TOL_BF16)


# ============================================================================================================================ soft CE
@pytest.mark.parametrize("B,N,C", [(2, 9, 20), (5, 1, 1000)])
@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_soft_ce_localized(ops, case, kind, B, N, C):
    """row_loss and the gradient guarded, ldx > C with NaN padding in the logits.  Columns C .. ldx-1 of dlogits are zeroed (include/autoprog_hip.h,
    ap_soft_ce_fwd_bwd) -- all of them, the gradient shares the logits' leading dimension."""
    from autoprog_amd._lib import lib
    M = B * N
    gen = torch.Generator().manual_seed(B * 31 + N)
    logits = (torch.randn(M, C, generator=gen) * 2).to(torch.bfloat16)
    gs = 0.5 / M
    xr = logits.double().requires_grad_(True)
    if kind == "dense":
        target = torch.rand(B, C, 2 + N, generator=gen) * (torch.rand(B, C, 2 + N, generator=gen) < 0.05) + 0.1 / C
        t = target[:, :, 2:].transpose(1, 2).reshape(-1, C).double()
        tdev = dev(target)
    else:
        K, smoothing = 5, 0.1
        idx = torch.randint(0, C, (B, N, K), generator=gen, dtype=torch.int32)
        val = torch.rand(B, N, K, generator=gen)
        t = torch.full((M, C), smoothing / C, dtype=torch.float64)
        t.scatter_add_(1, idx.reshape(M, K).long(), (1 - smoothing) * val.reshape(M, K).double())
        idev, vdev = dev(idx), dev(val)
    rows_ref = -(t * (xr - torch.logsumexp(xr, -1, keepdim=True))).sum(-1)
    (rows_ref.sum() * gs).backward()
    st = stream()

    def run(wide):
        if wide:
            ldx = round_up(C, 8) + 8
            ld = nan_padded(logits, ldx, device="cuda")
            loss, g0 = gflat(M, what="row_loss")
            dl, g1 = gbuf(M, ldx, ldx, what="dlogits")
        else:
            ldx = round_up(C, 8)
            ld = dev(F.pad(logits, (0, ldx - C)))
            loss, dl, g0, g1 = torch.empty(M, device="cuda"), torch.empty(M, ldx, dtype=torch.bfloat16, device="cuda"), None, None
        if kind == "dense":
            tv = tdev[:, :, 2:]
            rc = lib.ap_soft_ce_fwd_bwd(P(ld), ldx, tv.data_ptr(), tdev.stride(0), tdev.stride(1), tdev.stride(2), N, P(loss), P(dl), gs, M, C, 1.0, 0, st)
        else:
            rc = lib.ap_soft_ce_sparse_fwd_bwd(P(ld), ldx, P(idev), P(vdev), K, N * K, K, N, smoothing, P(loss), P(dl), gs, M, C, 1.0, 0, st)
        assert rc == 0
        torch.cuda.synchronize()
        return loss, dl, [g for g in (g0, g1) if g is not None]
    loss_c, dl_c, _ = run(False)
    loss_g, dl_g, guards = run(True)
    for g in guards:
        g.check(pad="untouched")
    assert torch.equal(loss_c, loss_g) and rel(loss_c, rows_ref) < 1e-4
    same_bits(case, "dlogits", dl_c[:, :C], dl_g[:, :C], xr.grad, TOL_BF16)
    assert bool((dl_g[:, C:].view(torch.int16) == 0).all()) and bool((dl_c[:, C:].view(torch.int16) == 0).all())
