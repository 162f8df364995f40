"""Operands past 2 GiB and 4 GiB: every kernel family once on a tensor whose byte offsets pass 2^31 and 2^32 (one-byte operands: whose
element index passes 2^31), the whole output checked.

The method is tests/_bigaddr.py's: the big operand is periodic (row m holds base[m % P], P an odd prime counted in rows or in images), so the
big output must equal the output of a launch on P rows (or on a few periods, where the dispatch needs more rows to pick the same kernel) bit
for bit, and that small output is held against fp64 with the suite's tolerances.  Reductions over the rows are held against the exact fp64
value (M // P) * S_P + S_(M % P), next to an fp32 emulation in torch, chunked by 65 536 rows, that does not involve the kernel under test.
Every output lives inside one allocation pre-filled with sentinels, 3 sentinel rows before and after; the fill of every big operand is
checked on the host on both sides of each boundary before the kernel runs; no torch operation touches more than 2^28 elements at a time.

Row counts come from BA.rows_past: the smallest count with three whole tiles and a ragged one behind the highest boundary of the case.  The
audit of the address arithmetic behind these cases is DESIGN.md, "Operand size limits"; the documented refusals are asserted in
tests/test_bigaddr_host.py.  Each case prints one `BIGADDR` line per operand / comparison and one with its wall time and peak device
memory: profiles/large_operands.txt is that output."""
import ctypes
import gc
import time

import pytest
import torch
import torch.nn.functional as F

from tests import _bigaddr as BA
from tests._tilecheck import assert_tiled, rel
from tests._topk_ref import check_pairs, topk_ref

pytestmark = pytest.mark.gpu
TOL_BF16 = 1e-2
TOL_F32 = 3e-3
BF, F32, U8, I32 = torch.bfloat16, torch.float32, torch.uint8, torch.int32
P_ROWS = 4099                        # the period of the row-wise cases: an odd prime above the tallest tile (256 rows)
MAX_PEAK = 24 * 2 ** 30


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from autoprog_amd._lib import lib as _lib
    return _lib


class Rec:
    """the lines of one case"""

    def __init__(self, name):
        self.name = name

    def line(self, text):
        print("BIGADDR %s | %s" % (self.name, text))

    def operand(self, what, rows, ld, dtype, bnds):
        self.line("%s [%d, %d] %s, %.3f GB | crosses %s" % (what, rows, ld, str(dtype).replace("torch.", ""), rows * ld * BA.itemsize(dtype) / 1e9,
                                                          ", ".join("%s at row %d" % (s, r) for r, s in bnds) or "nothing"))


@pytest.fixture
def rec(request):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                 # a device error of an earlier case is sticky: nothing more is launched on this device
        pytest.exit("the device reports an error from an earlier case; stopping: %s" % e, returncode=3)
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    r = Rec(request.node.name)
    t0 = time.perf_counter()
    yield r
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated()
    gc.collect()
    torch.cuda.empty_cache()
    r.line("wall %.2f s | peak device memory %.2f GiB" % (dt, peak / 2 ** 30))
    assert peak <= MAX_PEAK, "%s: peak device memory %.2f GiB (bound 24)" % (r.name, peak / 2 ** 30)


def S():
    return torch.cuda.current_stream().cuda_stream


def sync():
    torch.cuda.synchronize()


def rnd(*shape, scale=1.0, seed=0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(BF)


def frand(*shape, seed=0, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift


def dev(t):
    return t.cuda().contiguous()


def check_period(period, what=""):
    """the conditions on P (tests/_bigaddr.py good_period): its prime -- 4099 rows, or 13 or 3 images -- is odd, the period in rows is taller
    than the tallest tile (256 rows; a period of images spans whole images, and no tile spans two), and it divides none of the grid sizes
    the launchers cap their grids at: #CU and #CU rounded down to whole XCD groups (the persistent GEMM, attention and outlook kernels),
    twice #CU (the grouped weight gradients), 2048 (elementwise, LayerNorm forward, BatchNorm), 768 and 512 (LayerNorm backward, conv7)"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    prime = next(q for q in (4099, 13, 3) if period % q == 0)
    assert period > 256 or prime in (3, 13)
    # (768 = 3 * 256 caps the LayerNorm backward alone; the wide-class chain, the only user of 3 images, never launches it)
    for grid in (ncu, ncu & ~7, 2 * ncu, 2048, 512) + ((768,) if prime != 3 else ()):
        assert BA.good_period(prime, grid=grid, tallest_tile=256 if prime == period and prime > 13 else 0), "%s: period %d against grid %d" % (what, prime, grid)
    return prime


def pin(r, what, base, rows, ld=None, pad_pattern=None, powers=(31, 32)):
    """a periodic input of `rows` rows on the device, its fill checked on the host around every boundary.  r = None: the small launch"""
    if r is not None:
        check_period(base.shape[0], what)
    big, b = BA.periodic(base, rows, ld, "cuda", pad_pattern)
    bnds = BA.boundaries(big.shape[1], big.dtype, rows, powers)
    BA.check_bands(big, b, [x for x, _ in bnds], what)
    if r is not None:
        r.operand(what, rows, big.shape[1], big.dtype, bnds)
    return big


def pout(r, what, rows, cols, ld=None, dtype=BF, pre=BA.GUARD_ROWS, post=BA.GUARD_ROWS, powers=(31, 32)):
    o = BA.BigOut(rows, cols, ld, dtype, "cuda", pre, post, what)
    if r is not None:
        r.operand(what + " (output)", rows, o.ld, dtype, BA.boundaries(o.ld, dtype, rows, powers))
    return o


def pvec(r, what, rows, dtype=F32):
    """a guarded output of one element per row (row_loss, mean, rstd): 64 sentinel elements before and after"""
    return pout(r, what, rows, 1, 1, dtype, pre=64, post=64)


def verify(r, what, big, small, period, pad=None, sentinel_ok=False, col0=0):
    """guards of both launches untouched; every row of the big output bit-identical to the small launch's row of the same phase; no sentinel
    left; pad columns as the header says"""
    small.check_guards()
    big.check_guards()
    n = BA.compare_periodic(big.view, small.view[:period], big.cols, "%s %s" % (r.name, what), pad, sentinel_ok=sentinel_ok, col0=col0)
    r.line("%s | %d rows bit-identical to the %d-row period: yes | guards untouched | pad columns: %s" % (what, n, period, pad or "the kernel's"))


def tiled(r, what, got, ref, tol):
    rep = assert_tiled(got, ref, tol, "%s %s (period against fp64)" % (r.name, what))
    r.line("%s | period against fp64: whole %.3e, worst tile %.3e at (%d, %d) (bounds %.1e / %.1e)" % (what, rep.whole, rep.worst, rep[2], rep[3], tol, 2 * tol))
    return rep


def vec_rel(r, what, got, ref, tol):
    e = rel(got, ref)
    r.line("%s | period against fp64: rel %.3e (bound %.1e)" % (what, e, tol))
    assert e < tol, "%s %s: off by %.3e (bound %.1e)" % (r.name, what, e, tol)


def reduction(r, what, got, emu, want, tol=TOL_F32, tile=True):
    """a reduction over the rows against its exact fp64 value; the fp32 emulation in torch beside it must leave three quarters of the bound"""
    e_emu = rel(emu, want)
    r.line("%s | fp32 emulation (torch, 65 536-row chunks) against the exact fp64 value: %.3e (must stay below %.1e)" % (what, e_emu, tol / 4))
    assert e_emu < tol / 4, "%s %s: fp32 accumulation itself is off by %.3e -- widen the operand so that fewer rows cross the boundary" % (r.name, what, e_emu)
    if tile and got.dim() == 2:
        rep = assert_tiled(got, want, tol, "%s %s" % (r.name, what))
        r.line("%s | kernel against the exact fp64 value: whole %.3e, worst tile %.3e (bounds %.1e / %.1e)" % (what, rep.whole, rep.worst, tol, 2 * tol))
    else:
        e = rel(got, want)
        r.line("%s | kernel against the exact fp64 value: %.3e (bound %.1e)" % (what, e, tol))
        assert e < tol, "%s %s: off by %.3e (bound %.1e)" % (r.name, what, e, tol)


def emu_colsum(a, cols, weight=None):
    """sum over the rows of a[:, :cols] in fp32 with torch, 65 536 rows at a time (at most 2^28 elements per operation)"""
    out = torch.zeros(cols, dtype=F32, device=a.device)
    step = min(65536, max(1, BA.CHUNK // a.shape[1]))
    for s in range(0, a.shape[0], step):
        out += a[s:s + step, :cols].float().sum(0)
    return out


def emu_tn(a, n1, b, n2):
    """a[:, :n1]^T . b[:, :n2] in fp32 with torch: 65 536 rows and at most 2048 columns of a at a time"""
    out = torch.zeros(n1, n2, dtype=F32, device=a.device)
    for s in range(0, a.shape[0], 65536):
        bb = b[s:s + 65536, :n2].float()
        for c in range(0, n1, 2048):
            out[c:c + 2048] += a[s:s + 65536, c:min(n1, c + 2048)].float().t() @ bb
    return out


def epilogue(**kw):
    from autoprog_amd._lib import GemmEpilogue
    e = GemmEpilogue()
    e.rows_per_scale = 1
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def gemm_nt(lib, a, lda, w, ldb, c, ldc, M, N, K, epi=None):
    rc = lib.ap_gemm_nt(a, lda, w, ldb, c, ldc, M, N, K, ctypes.byref(epi) if epi is not None else None, S())
    assert rc == 0, "ap_gemm_nt(M = %d, N = %d, K = %d): code %d" % (M, N, K, rc)
    sync()


# ======================================================================================================================== A. the wide-class chain
# 21 843 classes in 21 848 columns, 196 tokens per image, batch 512: M = 100 352 rows, 2 192 490 496 elements, 4 384 980 992 bytes per
# logits-shaped tensor.  Row 98 292 holds byte 2^32.  P = 3 images = 588 rows; 512 % 3 == 2.
WC, WLD, WN, WB, WPI, WK_IN = 21843, 21848, 196, 512, 3, 384
WM, WP = WB * WN, WPI * WN
W_GS = 0.5 / WM


def test_wide_chain_sizes():
    assert BA.good_period(WPI) and WB % WPI != 0
    assert WM * WLD == 2192490496 and BA.boundary_row(WLD, BF, 32) == 98292
    assert WM >= BA.rows_past(WLD, BF, 32, tile=128)                   # three 128-row GEMM tiles and a ragged one behind byte 2^32
    assert WM * WC > 2 ** 31 and WM * WC * 4 > 2 ** 33                   # the dense fp32 target


def wide_logits_base(seed=11):
    return rnd(WP, WC, scale=2.0, seed=seed)


def test_wide_head_forward(lib, rec):
    """1. ap_gemm_nt M x 21 843 x 384 with a bias into ld 21 848: the 128 x 128 kernel at either row count (N % 8 != 0 keeps the 8-phase
    kernel out, 588 rows > 256 the few-rows kernel)"""
    x0 = rnd(WP, WK_IN, seed=1)
    w, bias = rnd(WC, WK_IN, scale=WK_IN ** -0.5, seed=2), frand(WC, seed=3)
    wd, bd = dev(w), dev(bias)

    def go(rows, r):
        x = pin(r, "A", x0, rows)
        out = pout(r, "C", rows, WC, WLD)
        gemm_nt(lib, x.data_ptr(), WK_IN, wd.data_ptr(), WK_IN, out.ptr(), WLD, rows, WC, WK_IN, epilogue(bias=bd.data_ptr()))
        return out
    small = go(WP, None)
    tiled(rec, "C", small.view[:, :WC], x0.double() @ w.double().t() + bias.double(), TOL_BF16)
    big = go(WM, rec)
    verify(rec, "C", big, small, WP, pad="untouched")


def sparse_target_base(K, seed):
    """[P images, (2 + N) K] (class, score) pairs; the first token row of image 0 holds the corners of the class range, the last class of the
    narrow kernel and the first beyond it, a repeated class and two indices outside [0, C)"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, WC, (WPI, 2 + WN, K), generator=g, dtype=I32)
    if K == 8:
        rep = int(idx[0, 2, 4])
        idx[0, 2] = torch.tensor([0, 1023, 1024, WC - 1, rep, rep, -1, WC], dtype=I32)
    val = torch.rand(WPI, 2 + WN, K, generator=g) + 0.05
    return idx.reshape(WPI, -1), val.reshape(WPI, -1)


def sparse_dense_target(idx, val, K, smoothing, images):
    """fp64 [images * N, C] of the pairs of image b % P, token slots 2 .."""
    b = torch.arange(images) % WPI
    i = idx.reshape(WPI, 2 + WN, K)[b][:, 2:].reshape(-1, K).long()
    v = val.reshape(WPI, 2 + WN, K)[b][:, 2:].reshape(-1, K).double()
    t = torch.full((images * WN, WC), smoothing / WC, dtype=torch.float64)
    ok = (i >= 0) & (i < WC)
    t.scatter_add_(1, i.clamp(0, WC - 1), (1 - smoothing) * v * ok)
    return t


def ce_reference(logits, t, gs):
    x = logits.double().requires_grad_(True)
    rows = -(t * (x - torch.logsumexp(x, -1, keepdim=True))).sum(-1)
    (rows.sum() * gs).backward()
    return rows.detach(), x.grad


@pytest.mark.parametrize("mix", [False, True], ids=["plain", "mix-token"])
def test_wide_sparse_ce(lib, rec, mix):
    """2. ap_soft_ce_sparse_fwd_bwd, the wide kernel (four waves per row): K = 8 pairs from a [B, 2 + N, K] target, smoothing 0.1; and with
    mix_batches = B, lam = 0.37.  Image b mixes with image B-1-b, whose phase is (B-1-b) % 3: the small launch has 5 images (5 % 3 == 512 % 3),
    so that its first three images meet partners of the same phases as every image of the big launch."""
    K, smoothing, lam = 8, 0.1, 0.37
    l0 = wide_logits_base()
    i0, v0 = sparse_target_base(K, seed=12)
    small_images = 5 if mix else WPI
    assert small_images % WPI == WB % WPI or not mix

    def go(images, r):
        rows = images * WN
        x = pin(r, "logits", l0, rows, WLD)
        idx, val = pin(r, "idx", i0, images), pin(r, "val", v0, images)
        loss, dl = pvec(r, "row_loss", rows), pout(r, "dlogits", rows, WC, WLD)
        rc = lib.ap_soft_ce_sparse_fwd_bwd(x.data_ptr(), WLD, idx.data_ptr() + 2 * K * 4, val.data_ptr() + 2 * K * 4, K, (2 + WN) * K, K, WN, smoothing,
                                           loss.ptr(), dl.ptr(), W_GS, rows, WC, lam if mix else 1.0, images if mix else 0, S())
        assert rc == 0, "ap_soft_ce_sparse_fwd_bwd: code %d" % rc
        sync()
        return loss, dl
    loss_s, dl_s = go(small_images, None)
    t = sparse_dense_target(i0, v0, K, smoothing, small_images)
    if mix:
        lam32 = float(torch.tensor(lam, dtype=F32))
        t = (lam32 * t.reshape(small_images, WN, WC) + (1 - lam32) * t.reshape(small_images, WN, WC).flip(0)).reshape(-1, WC)
    rows_ref, grad_ref = ce_reference(l0, t[:WP], W_GS)
    vec_rel(rec, "row_loss", loss_s.view[:WP, 0], rows_ref, 1e-4)
    tiled(rec, "dlogits", dl_s.view[:WP, :WC], grad_ref, TOL_BF16)
    loss_b, dl_b = go(WB, rec)
    verify(rec, "row_loss", loss_b, loss_s, WP)
    verify(rec, "dlogits", dl_b, dl_s, WP, pad="zero")


def test_wide_dense_ce_rowmajor_target(lib, rec):
    """3. ap_soft_ce_fwd_bwd on a dense row-major fp32 target [M, C] through its strides: 8.77 GB, past 2^31 elements and 2^33 bytes"""
    l0 = wide_logits_base()
    g = torch.Generator().manual_seed(13)
    t0 = torch.rand(WP, WC, generator=g) * (torch.rand(WP, WC, generator=g) < 0.05) + 0.1 / WC

    def go(images, r):
        rows = images * WN
        x = pin(r, "logits", l0, rows, WLD)
        t = pin(r, "target", t0, rows, powers=(31, 32, 33))
        loss, dl = pvec(r, "row_loss", rows), pout(r, "dlogits", rows, WC, WLD)
        rc = lib.ap_soft_ce_fwd_bwd(x.data_ptr(), WLD, t.data_ptr(), WN * WC, 1, WC, WN, loss.ptr(), dl.ptr(), W_GS, rows, WC, 1.0, 0, S())
        assert rc == 0, "ap_soft_ce_fwd_bwd: code %d" % rc
        sync()
        return loss, dl
    loss_s, dl_s = go(WPI, None)
    rows_ref, grad_ref = ce_reference(l0, t0.double(), W_GS)
    vec_rel(rec, "row_loss", loss_s.view[:, 0], rows_ref, 1e-4)
    tiled(rec, "dlogits", dl_s.view[:, :WC], grad_ref, TOL_BF16)
    loss_b, dl_b = go(WB, rec)
    verify(rec, "row_loss", loss_b, loss_s, WP)
    verify(rec, "dlogits", dl_b, dl_s, WP, pad="zero")


def test_wide_softmax_topk(lib, rec):
    """4. ap_softmax_topk_rows, K = 5, from teacher logits of that size straight into the token slots of a [B, 2 + N, K] target: the slots
    0 and 1 of every image keep their sentinels"""
    K = 5
    l0 = wide_logits_base(seed=14)
    l0[5, 100:108] = l0[5, 100]                                          # a run of equal logits: ties resolve to the smallest class
    row = (2 + WN) * K

    def go(images, r):
        rows = images * WN
        x = pin(r, "logits", l0, rows, WLD)
        idx, val = pout(r, "idx", images, row, row, I32), pout(r, "val", images, row, row, F32)
        rc = lib.ap_softmax_topk_rows(x.data_ptr(), WLD, WC, K, 1.0, idx.ptr() + 2 * K * 4, val.ptr() + 2 * K * 4, row, K, WN, rows, S())
        assert rc == 0, "ap_softmax_topk_rows: code %d" % rc
        sync()
        return idx, val
    idx_s, val_s = go(WPI, None)
    ref_i, ref_v = topk_ref(l0, K)
    check_pairs(idx_s.view[:, 2 * K:].reshape(WP, K), val_s.view[:, 2 * K:].reshape(WP, K), ref_i, ref_v, rec.name)
    idx_b, val_b = go(WB, rec)
    verify(rec, "idx", idx_b, idx_s, WPI, col0=2 * K)
    verify(rec, "val", val_b, val_s, WPI, col0=2 * K)


def test_wide_head_input_gradient(lib, rec):
    """5. ap_gemm_nt with A = dlogits [M, 21 848] (K = the padded width, as functional._linear_bwd passes it: the padding columns of dlogits
    and of the transposed weight are zeros), N = 384: the 128 x 128 kernel (K % 64 != 0)"""
    g0 = rnd(WP, WC, scale=0.05, seed=15)
    wt = torch.zeros(WK_IN, WLD, dtype=BF)
    wt[:, :WC] = rnd(WK_IN, WC, scale=WK_IN ** -0.5, seed=16)
    wd = dev(wt)

    def go(rows, r):
        g = pin(r, "dlogits", g0, rows, WLD, pad_pattern=0)
        out = pout(r, "dx", rows, WK_IN)
        gemm_nt(lib, g.data_ptr(), WLD, wd.data_ptr(), WLD, out.ptr(), WK_IN, rows, WK_IN, WLD)
        return out
    small = go(WP, None)
    tiled(rec, "dx", small.view, g0.double() @ wt[:, :WC].double().t(), TOL_BF16)
    big = go(WM, rec)
    verify(rec, "dx", big, small, WP)


def test_wide_head_weight_gradient(lib, rec):
    """6. ap_gemm_tn_acc with A = dlogits [M, 21 848], B = x [M, 384] and the fused column sum: 100 352 rows reduced, against the exact fp64
    value from the 588 base rows"""
    g0, x0 = rnd(WP, WC, scale=0.05, seed=15), rnd(WP, WK_IN, seed=1)
    g = pin(rec, "dlogits", g0, WM, WLD)                                 # (the columns N1 .. lda-1 may hold anything: NaNs here)
    x = pin(rec, "x", x0, WM)
    dw, db = pout(rec, "dW", WC, WK_IN, dtype=F32), pvec(rec, "db", WC)
    dw.view.zero_()
    db.view.zero_()
    rc = lib.ap_gemm_tn_acc(g.data_ptr(), WLD, x.data_ptr(), WK_IN, dw.ptr(), WK_IN, WM, WC, WK_IN, db.ptr(), S())
    assert rc == 0, "ap_gemm_tn_acc: code %d" % rc
    sync()
    dw.check_guards()
    db.check_guards()
    reduction(rec, "dW", dw.view, emu_tn(g, WC, x, WK_IN), BA.periodic_matmul_tn(g0, x0, WM))
    reduction(rec, "db", db.view[:, 0], emu_colsum(g, WC), BA.periodic_sum(g0.double(), WM))


def test_wide_chain_autograd_pass(lib, rec):
    """7. one autograd pass at batch 512 through functional.LinearFn (both heads), SparseTokenLabelTarget.from_logits and
    TokenLabelCrossEntropy (mix-token box of 7 x 7 tokens: lam = 0.75), against the launches of steps 1 - 6 issued directly on one period:
    the wrappers' own allocations, the padded views of 21 843 columns in rows of 21 848, the strides handed to the ABI and torch's own copies
    of 2.19e9 elements in between.  Bit for bit where the launch is the same (logits, the target's token slots and class slot, the input
    gradient); within TOL_F32 where sums meet (the loss, weight.grad and bias.grad through the grouped weight-gradient launch's atomics)."""
    from autoprog_amd import functional as AF
    from autoprog_amd.loss import SparseTokenLabelTarget, TokenLabelCrossEntropy
    K, smoothing, cw, dw_ = 5, 0.1, 1.0, 0.5
    x0, xc0 = rnd(WP, WK_IN, seed=1), rnd(WPI, WK_IN, seed=17)
    w, bias = rnd(WC, WK_IN, scale=WK_IN ** -0.5, seed=2), frand(WC, seed=3)
    wc_, bc_ = rnd(WC, WK_IN, scale=WK_IN ** -0.5, seed=18), frand(WC, seed=19)
    t0, tc0 = wide_logits_base(seed=14), rnd(WPI, WC, scale=2.0, seed=20)
    # ---- the pass
    x = pin(rec, "x", x0, WM).view(WB, WN, WK_IN).requires_grad_(True)
    xc = pin(rec, "x_cls", xc0, WB)
    head = torch.nn.Linear(WK_IN, WC).cuda()
    head_cls = torch.nn.Linear(WK_IN, WC).cuda()
    with torch.no_grad():
        head.weight.copy_(w.float()); head.bias.copy_(bias); head_cls.weight.copy_(wc_.float()); head_cls.bias.copy_(bc_)
    teacher = pin(rec, "teacher logits", t0, WM, WLD)
    teacher_cls = pin(rec, "teacher class logits", tc0, WB, WLD)
    labels = torch.randint(0, WC, (WB,), generator=torch.Generator().manual_seed(21)).cuda()
    tgt = SparseTokenLabelTarget.from_logits(labels, teacher_cls[:, :WC], teacher[:, :WC].view(WB, WN, WC), k=K, smoothing=smoothing)
    del teacher                                                           # (4.4 GB the rest of the pass does not need)
    aux = AF.LinearFn.apply(x, head.weight, head.bias, False)
    out_cls = AF.LinearFn.apply(xc, head_cls.weight, head_cls.bias, False)
    assert tuple(aux.shape) == (WB, WN, WC) and aux.stride(-2) == WLD, "the head's output is not a view of rows of %d" % WLD
    loss = TokenLabelCrossEntropy(dense_weight=dw_, cls_weight=cw, classes=WC)((out_cls, aux, (0, 0, 7, 7)), tgt)
    lam = float(1 - 49 / WN)
    logits_rows = torch.as_strided(aux.detach(), (WM, WLD), (WLD, 1))       # the rows as they lie in memory, padding included
    loss.backward()
    sync()
    # ---- step 1 on one period, directly: the logits
    wd, bd = dev(w), dev(bias)
    xs = pin(None, "A", x0, WP)
    lg_s = pout(None, "C", WP, WC, WLD)
    gemm_nt(lib, xs.data_ptr(), WK_IN, wd.data_ptr(), WK_IN, lg_s.ptr(), WLD, WP, WC, WK_IN, epilogue(bias=bd.data_ptr()))
    n = BA.compare_periodic(logits_rows, lg_s.view, WC, "%s logits" % rec.name)
    rec.line("logits of LinearFn | %d rows bit-identical to the direct launch on the period: yes" % n)
    del logits_rows, aux
    # ---- step 4: the target's token slots against a direct launch on the teacher's period; the class slot against a direct launch on all images
    row = (2 + WN) * K
    ts = pin(None, "logits", t0, WP, WLD)
    idx_s, val_s = pout(None, "idx", WPI, row, row, I32), pout(None, "val", WPI, row, row, F32)
    assert lib.ap_softmax_topk_rows(ts.data_ptr(), WLD, WC, K, 1.0, idx_s.ptr() + 2 * K * 4, val_s.ptr() + 2 * K * 4, row, K, WN, WP, S()) == 0
    idx_c, val_c = pout(None, "idx", WB, K, K, I32), pout(None, "val", WB, K, K, F32)
    assert lib.ap_softmax_topk_rows(teacher_cls.data_ptr(), WLD, WC, K, 1.0, idx_c.ptr(), val_c.ptr(), K, 0, 1, WB, S()) == 0
    sync()
    ti, tv = tgt.idx.view(WB, row), tgt.val.view(WB, row)
    BA.compare_periodic(ti[:, 2 * K:].contiguous(), idx_s.view[:, 2 * K:].contiguous(), row - 2 * K, "%s target idx" % rec.name)
    BA.compare_periodic(tv[:, 2 * K:].contiguous(), val_s.view[:, 2 * K:].contiguous(), row - 2 * K, "%s target val" % rec.name)
    assert torch.equal(ti[:, K:2 * K], idx_c.view) and torch.equal(tv[:, K:2 * K], val_c.view), "the class slot differs from the direct launch"
    assert torch.equal(ti[:, 0], labels.int()) and bool((ti[:, 1:K] == -1).all()) and bool((tv[:, 0] == 1).all()) and bool((tv[:, 1:K] == 0).all())
    rec.line("target of from_logits | token slots of %d images bit-identical to the direct launch on the period, class slot to the direct launch: yes" % WB)
    # ---- step 2 on one period with that target; the class row on all images (the mix partner B-1-b is not periodic; 512 rows are small)
    loss_s, dl_s = pvec(None, "row_loss", WP), pout(None, "dlogits", WP, WC, WLD)
    ti3, tv3 = ti[:WPI].contiguous(), tv[:WPI].contiguous()
    rc = lib.ap_soft_ce_sparse_fwd_bwd(lg_s.ptr(), WLD, ti3.data_ptr() + 2 * K * 4, tv3.data_ptr() + 2 * K * 4, K, row, K, WN, smoothing, loss_s.ptr(), dl_s.ptr(),
                                       dw_ / WM, WP, WC, 1.0, 0, S())
    assert rc == 0
    cls_rows = torch.as_strided(out_cls.detach(), (WB, WLD), (WLD, 1))
    loss_c, dl_c = pvec(None, "row_loss", WB), pout(None, "dlogits", WB, WC, WLD)
    rc = lib.ap_soft_ce_sparse_fwd_bwd(cls_rows.data_ptr(), WLD, tgt.idx.data_ptr() + K * 4, tgt.val.data_ptr() + K * 4, K, row, 0, 1, smoothing, loss_c.ptr(), dl_c.ptr(),
                                       cw / WB, WB, WC, lam, WB, S())
    assert rc == 0
    sync()
    want_loss = cw / WB * float(loss_c.view.double().sum()) + dw_ / WM * float(BA.periodic_sum(loss_s.view[:, 0].cpu().double(), WM))
    e = abs(float(loss) - want_loss) / abs(want_loss)
    rec.line("loss | the module's %.6f against the row losses of the direct launches summed in fp64 %.6f: %.3e (bound %.1e)" % (float(loss), want_loss, e, TOL_F32))
    assert e < TOL_F32
    # ---- step 5: the input gradient, bit for bit
    wt = torch.zeros(WK_IN, WLD, dtype=BF)
    wt[:, :WC] = w.t()
    wtd = dev(wt)
    dx_s = pout(None, "dx", WP, WK_IN)
    gemm_nt(lib, dl_s.ptr(), WLD, wtd.data_ptr(), WLD, dx_s.ptr(), WK_IN, WP, WK_IN, WLD)
    assert x.grad is not None and x.grad.dtype == BF and x.grad.is_contiguous()
    n = BA.compare_periodic(x.grad.view(WM, WK_IN), dx_s.view, WK_IN, "%s x.grad" % rec.name)
    rec.line("x.grad | %d rows bit-identical to the direct launch on the period: yes" % n)
    # ---- step 6: weight.grad and bias.grad against the exact fp64 value of the period's gradient rows
    g0 = dl_s.view[:, :WC].cpu()
    rep = assert_tiled(head.weight.grad, BA.periodic_matmul_tn(g0, x0, WM), TOL_F32, "%s weight.grad" % rec.name)
    rec.line("weight.grad | against the exact fp64 value: whole %.3e, worst tile %.3e (bounds %.1e / %.1e)" % (rep.whole, rep.worst, TOL_F32, 2 * TOL_F32))
    vec_rel(rec, "bias.grad", head.bias.grad, BA.periodic_sum(g0.double(), WM), TOL_F32)


# ======================================================================================================================== B. ap_gemm_nt
def mirror_use_8p(M, N, K, ncu):
    """csrc/nt_plan.h nt_use_8p for a launch without dgelu_of / a residual beside mul_by -> 0, 192 or 256 (the block tile width)"""
    if (K & 63) or K < 128 or M < 4096 or (N & 7):
        return 0
    bn = 256 if N >= 1024 else (192 if N % 192 == 0 else (256 if N % 256 == 0 else 0))
    if N >= 384 and N % 192 == 0:
        mt = (M + 255) // 256
        r192, r256 = (mt * (N // 192) + ncu - 1) // ncu, (mt * ((N + 255) // 256) + ncu - 1) // ncu
        bn = 192 if r192 * 10 < r256 * 13 else 256
    return 0 if N < 192 else bn


def same_path_rows_8p(M, N, K, period):
    """the smallest whole number of periods at which the dispatch picks the tile width it picks for M rows and fills the persistent grid
    (fewer tiles than CUs may take the 224-row instantiation, csrc/nt_plan.h nt_plan) -> (rows, tile width)"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    bn = mirror_use_8p(M, N, K, ncu)
    assert bn, "not a launch of the 8-phase kernel"
    for n in range(2, 64):
        rows = n * period
        if mirror_use_8p(rows, N, K, ncu) == bn and ((rows + 255) // 256) * ((N + bn - 1) // bn) >= (ncu & ~7):
            return rows, bn
    raise AssertionError("no row count below 64 periods stays on the path of M = %d" % M)


def gelu_refs(h64):
    """fp64 gelu and gelu' of the bf16-rounded pre-activation"""
    h = h64.to(BF).double().requires_grad_(True)
    F.gelu(h).sum().backward()
    return F.gelu(h.detach()), h.grad


def codes_check(r, codes, dref):
    """the 8-bit gelu' codes of a period against fp64, in code units: the bound tests/test_gpu_localized.py holds them to (the kernel rounds the
    pre-activation to bf16 from an fp32 sum: where that lands one bf16 step from the fp64 value the derivative moves by more than one code)"""
    from autoprog_amd import ops
    want = torch.clamp(torch.round(dref * ops.GELU_CODE_SCALE) + ops.GELU_CODE_ZERO, 0, 255)
    d = (codes.cpu().double() - want).abs()
    within, worst = float((d <= 1).double().mean()), float(d.max())
    r.line("gelu' codes | period against fp64: %.5f of the codes within 1, the worst off by %d (bounds > 0.999, < 6)" % (within, worst))
    assert within > 0.999 and worst < 6, (within, worst)


@pytest.mark.parametrize("N,want_bn", [(1152, 192), (1296, 256)], ids=["N1152-192wide", "N1296-256wide-masked-last-tile"])
@pytest.mark.parametrize("flavour", ["plain", "bias_res_rs", "gelu8"])
def test_gemm_nt_8phase_output_past_4gib(lib, rec, flavour, N, want_bn):
    """M x N x 384, C past 2^32 bytes, at N = 1152 (the dispatch picks 256 x 192 tiles at this row count) and N = 1296 (N >= 1024 and no
    multiple of 192: 256 x 256 tiles, the sixth column tile masked down to 16 columns); bias + residual + row_scale with the residual past 2^32 bytes as well; GELU with 8-bit derivative
    codes whose bytes pass 2^31.  The persistent 8-phase kernel; the comparison launch runs at the smallest number of periods at which the
    dispatch picks the same tile width and no 224-row tiles."""
    from autoprog_amd import ops
    K, P = 384, P_ROWS
    M = BA.rows_past(N, BF, 32, tile=256)
    Ms, bn = same_path_rows_8p(M, N, K, P)
    assert bn == want_bn, "the dispatch picks %d-wide tiles for M = %d, N = %d" % (bn, M, N)
    rec.line("path: 8-phase, 256 x %d tiles; comparison launch at %d rows" % (bn, Ms))
    a0, w, bias, res0 = rnd(P, K, seed=1), rnd(N, K, scale=K ** -0.5, seed=2), frand(N, seed=3), rnd(P, N, seed=4)
    rs0 = (torch.rand(P, 1, generator=torch.Generator().manual_seed(5)) > 0.2).float() / 0.8
    rs0[0], rs0[-1] = 0.0, 1.25
    wd, bd = dev(w), dev(bias)

    def go(rows, r):
        a = pin(r, "A", a0, rows)
        out = pout(r, "C", rows, N)
        codes, keep = None, []
        if flavour == "plain":
            epi = None
        elif flavour == "bias_res_rs":
            res, rs = pin(r, "residual", res0, rows), pin(r, "row_scale", rs0, rows)
            keep = [res, rs]
            epi = epilogue(bias=bd.data_ptr(), residual=res.data_ptr(), ldr=N, row_scale=rs.data_ptr(), rows_per_scale=1)
        else:
            codes = pout(r, "gelu' codes", rows, N, dtype=U8)
            epi = epilogue(bias=bd.data_ptr(), gelu=3, preact_out=codes.ptr())
        gemm_nt(lib, a.data_ptr(), K, wd.data_ptr(), K, out.ptr(), N, rows, N, K, epi)
        del keep
        return out, codes
    out_s, codes_s = go(Ms, None)
    lin = a0.double() @ w.double().t()
    if flavour == "plain":
        ref = lin
    elif flavour == "bias_res_rs":
        ref = (lin + bias.double()) * rs0.double() + res0.double()
    else:
        ref, dref = gelu_refs(lin + bias.double())
        codes_check(rec, codes_s.view[:P], dref)
    tiled(rec, "C", out_s.view[:P], ref, TOL_BF16)
    out_b, codes_b = go(M, rec)
    verify(rec, "C", out_b, out_s, P)
    if codes_b is not None:
        verify(rec, "gelu' codes", codes_b, codes_s, P, sentinel_ok=True)


def test_gemm_nt_8phase_a_past_4gib(lib, rec):
    """M x 384 x 1152 with A past 2^32 bytes: 256 x 192 tiles"""
    N, K, P = 384, 1152, P_ROWS
    M = BA.rows_past(K, BF, 32, tile=256)
    Ms, bn = same_path_rows_8p(M, N, K, P)
    rec.line("path: 8-phase, 256 x %d tiles; comparison launch at %d rows" % (bn, Ms))
    a0, w = rnd(P, K, seed=1), rnd(N, K, scale=K ** -0.5, seed=2)
    wd = dev(w)

    def go(rows, r):
        a = pin(r, "A", a0, rows)
        out = pout(r, "C", rows, N)
        gemm_nt(lib, a.data_ptr(), K, wd.data_ptr(), K, out.ptr(), N, rows, N, K)
        return out
    small = go(Ms, None)
    tiled(rec, "C", small.view[:P], a0.double() @ w.double().t(), TOL_BF16)
    big = go(M, rec)
    verify(rec, "C", big, small, P)


@pytest.mark.parametrize("flavour", ["gelu8", "mul8"])
def test_gemm_nt_weight_stationary(lib, rec, flavour):
    """K = 192, N = 576, M % 64 == 0, ldc % 16 == 0: the weight-stationary kernel (M >= 16 384 at either row count).  gelu8 writes C past
    2^32 bytes and code bytes past 2^31; mul8 reads code bytes at the same offsets"""
    from autoprog_amd import ops
    N, K, P = 576, 192, P_ROWS
    M = BA.rows_past(N, BF, 32, tile=64, multiple=64)
    Ms = BA.round_up(max(16384, 4 * P), 64)
    assert M >= 16384 and Ms >= 16384 and N % 16 == 0
    a0, w, bias = rnd(P, K, seed=1), rnd(N, K, scale=K ** -0.5, seed=2), frand(N, seed=3)
    c0 = torch.randint(0, 256, (P, N), dtype=U8, generator=torch.Generator().manual_seed(7))
    wd, bd = dev(w), dev(bias)

    def go(rows, r):
        a = pin(r, "A", a0, rows)
        out = pout(r, "C", rows, N)
        if flavour == "gelu8":
            codes = pout(r, "gelu' codes", rows, N, dtype=U8)
            epi = epilogue(bias=bd.data_ptr(), gelu=3, preact_out=codes.ptr())
            gemm_nt(lib, a.data_ptr(), K, wd.data_ptr(), K, out.ptr(), N, rows, N, K, epi)
            return out, codes
        cin = pin(r, "codes", c0, rows)
        gemm_nt(lib, a.data_ptr(), K, wd.data_ptr(), K, out.ptr(), N, rows, N, K, epilogue(mul_by8=cin.data_ptr()))
        return out, None
    out_s, codes_s = go(Ms, None)
    lin = a0.double() @ w.double().t()
    if flavour == "gelu8":
        ref, dref = gelu_refs(lin + bias.double())
        codes_check(rec, codes_s.view[:P], dref)
    else:
        ref = lin * ((c0.double() - ops.GELU_CODE_ZERO) / ops.GELU_CODE_SCALE)
    tiled(rec, "C", out_s.view[:P], ref, TOL_BF16)
    out_b, codes_b = go(M, rec)
    verify(rec, "C", out_b, out_s, P)
    if codes_b is not None:
        verify(rec, "gelu' codes", codes_b, codes_s, P, sentinel_ok=True)


@pytest.mark.parametrize("flavour", ["plain", "mulby"])
def test_gemm_nt_128x128(lib, rec, flavour):
    """N = 392, K = 264 (K % 64 != 0: no 8-phase kernel; N > 256 and no multiple of 64: 128 x 128 tiles), C past 2^32 bytes; mul_by: the
    prefetching instantiation reads a second operand of that size"""
    N, K, P = 392, 264, P_ROWS
    M = BA.rows_past(N, BF, 32, tile=128)
    a0, w, mb0 = rnd(P, K, seed=1), rnd(N, K, scale=K ** -0.5, seed=2), rnd(P, N, seed=6)
    wd = dev(w)

    def go(rows, r):
        a = pin(r, "A", a0, rows)
        out = pout(r, "C", rows, N)
        if flavour == "plain":
            gemm_nt(lib, a.data_ptr(), K, wd.data_ptr(), K, out.ptr(), N, rows, N, K)
        else:
            mb = pin(r, "mul_by", mb0, rows)
            gemm_nt(lib, a.data_ptr(), K, wd.data_ptr(), K, out.ptr(), N, rows, N, K, epilogue(mul_by=mb.data_ptr()))
        return out
    small = go(P, None)
    lin = a0.double() @ w.double().t()
    tiled(rec, "C", small.view, lin if flavour == "plain" else lin * mb0.double(), TOL_BF16)
    big = go(M, rec)
    verify(rec, "C", big, small, P)


def test_gemm_nt_fp8_a_past_4gib(lib, rec):
    """ap_gemm_nt_fp8 M x 384 x 1152 on e4m3 bytes: A past 2^32 bytes (and 2^31 elements)"""
    N, K, P = 384, 1152, P_ROWS
    M = BA.rows_past(K, U8, 32, tile=256)
    Ms, bn = same_path_rows_8p(M, N, K // 2, P)
    rec.line("path: 8-phase fp8, 256 x %d tiles; comparison launch at %d rows" % (bn, Ms))
    g = torch.Generator().manual_seed(21)
    a8 = torch.randn(P, K, generator=g).clamp(-448, 448).to(torch.float8_e4m3fn)
    w8 = (torch.randn(N, K, generator=g) * K ** -0.5 * 16).to(torch.float8_e4m3fn)
    dq = dev(torch.tensor([1.0, 1.0 / 16], dtype=F32))
    wd = dev(w8.view(U8))

    def go(rows, r):
        a = pin(r, "A", a8.view(U8), rows)
        out = pout(r, "C", rows, N)
        rc = lib.ap_gemm_nt_fp8(a.data_ptr(), K, wd.data_ptr(), K, out.ptr(), N, rows, N, K, dq.data_ptr(), dq.data_ptr() + 4, None, S())
        assert rc == 0, "ap_gemm_nt_fp8: code %d" % rc
        sync()
        return out
    small = go(Ms, None)
    tiled(rec, "C", small.view[:P], a8.float().double() @ (w8.float().double() / 16).t(), TOL_BF16)
    big = go(M, rec)
    verify(rec, "C", big, small, P)


# ======================================================================================================================== B. weight gradients
def test_gemm_tn_acc_two_million_rows(lib, rec):
    """ap_gemm_tn_acc with A [M, 1152] past 2^32 bytes, B [M, 384] and the column sum: ~1.9 M rows reduced in fp32"""
    N1, N2, P = 1152, 384, P_ROWS
    M = BA.rows_past(N1, BF, 32, tile=64)
    a0, b0 = rnd(P, N1, scale=0.05, seed=31), rnd(P, N2, seed=32)
    a, b = pin(rec, "A", a0, M), pin(rec, "B", b0, M)
    dw, db = pout(rec, "dW", N1, N2, dtype=F32), pvec(rec, "colsum", N1)
    dw.view.zero_()
    db.view.zero_()
    rc = lib.ap_gemm_tn_acc(a.data_ptr(), N1, b.data_ptr(), N2, dw.ptr(), N2, M, N1, N2, db.ptr(), S())
    assert rc == 0, "ap_gemm_tn_acc: code %d" % rc
    sync()
    dw.check_guards()
    db.check_guards()
    reduction(rec, "dW", dw.view, emu_tn(a, N1, b, N2), BA.periodic_matmul_tn(a0, b0, M))
    reduction(rec, "colsum", db.view[:, 0], emu_colsum(a, N1), BA.periodic_sum(a0.double(), M))


@pytest.mark.parametrize("mode", ["atomics", "workspace"])
def test_gemm_tn_acc_grouped_two_million_rows(lib, rec, mode):
    """ap_gemm_tn_acc_grouped, one problem of the same widths: with fp32 atomics, and with the deterministic workspace -- two runs of which
    must be bit-identical"""
    from autoprog_amd._lib import TnProblem
    N1, N2, P = 1152, 384, P_ROWS
    M = BA.rows_past(N1, BF, 32, tile=64)
    a0, b0 = rnd(P, N1, scale=0.05, seed=31), rnd(P, N2, seed=32)
    a, b = pin(rec, "A", a0, M), pin(rec, "B", b0, M)
    want_w, want_b = BA.periodic_matmul_tn(a0, b0, M), BA.periodic_sum(a0.double(), M)
    runs = []
    for _ in range(2 if mode == "workspace" else 1):
        dw, db = pout(rec, "dW", N1, N2, dtype=F32), pvec(rec, "colsum", N1)
        dw.view.zero_()
        db.view.zero_()
        prob = TnProblem(A=a.data_ptr(), lda=N1, B=b.data_ptr(), ldb=N2, C=dw.ptr(), ldc=N2, M=M, N1=N1, N2=N2, colsum_A=db.ptr())
        ws, ws_bytes = None, 0
        if mode == "workspace":
            ws_bytes = lib.ap_gemm_tn_grouped_workspace(ctypes.addressof(prob), 1)
            assert ws_bytes > 0
            ws = BA.BigOut(1, ws_bytes // 4, dtype=F32, device="cuda", pre=1, post=1, what="workspace")
        rc = lib.ap_gemm_tn_acc_grouped(ctypes.addressof(prob), 1, ws.ptr() if ws is not None else None, ws_bytes, S())
        assert rc == 0, "ap_gemm_tn_acc_grouped: code %d" % rc
        sync()
        dw.check_guards()
        db.check_guards()
        if ws is not None:
            ws.check_guards()
        runs.append((dw, db))
    reduction(rec, "dW", runs[0][0].view, emu_tn(a, N1, b, N2), want_w)
    reduction(rec, "colsum", runs[0][1].view[:, 0], emu_colsum(a, N1), want_b)
    if mode == "workspace":
        same = torch.equal(runs[0][0].view, runs[1][0].view) and torch.equal(runs[0][1].view, runs[1][1].view)
        rec.line("deterministic workspace: two runs bit-identical: %s" % ("yes" if same else "NO"))
        assert same


# ======================================================================================================================== B. LayerNorm
LN_C, LN_EPS = 384, 1e-5


def ln_reference(x, gamma, beta):
    xd = x.double()
    mean, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    rstd = (var + LN_EPS).rsqrt()
    return (xd - mean) * rstd * gamma.double() + beta.double(), mean[:, 0], rstd[:, 0]


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8-emitting"])
def test_layernorm_forward(lib, rec, fp8):
    """x and y [M, 384] past 2^32 bytes; the fp8-emitting forward also writes y as e4m3 bytes past 2^31 elements.  mean / rstd: fp32 sums of
    384 values whose mean is 0.5 -- n * 2^-24 = 2.3e-5 in the worst case, held to 1e-4"""
    C, P = LN_C, P_ROWS
    M = BA.rows_past(C, BF, 32, tile=16)
    x0, gamma, beta = rnd(P, C, shift=0.5, seed=41), frand(C, seed=42, scale=0.2, shift=1.0), frand(C, seed=43, scale=0.2)
    gd, bd = dev(gamma), dev(beta)
    scale = dev(torch.tensor([16.0], dtype=F32))

    def go(rows, r):
        x = pin(r, "x", x0, rows)
        y, mean, rstd = pout(r, "y", rows, C), pvec(r, "mean", rows), pvec(r, "rstd", rows)
        y8, amax = None, None
        if fp8:
            y8, amax = pout(r, "y8", rows, C, dtype=U8), torch.zeros(1, dtype=F32, device="cuda")
            rc = lib.ap_layernorm_fwd_fp8(x.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.ptr(), y8.ptr(), scale.data_ptr(), amax.data_ptr(), mean.ptr(), rstd.ptr(),
                                          rows, C, LN_EPS, S())
        else:
            rc = lib.ap_layernorm_fwd(x.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.ptr(), mean.ptr(), rstd.ptr(), rows, C, LN_EPS, S())
        assert rc == 0, "ap_layernorm_fwd: code %d" % rc
        sync()
        return y, mean, rstd, y8, amax
    small = go(P, None)
    y_ref, mean_ref, rstd_ref = ln_reference(x0, gamma, beta)
    tiled(rec, "y", small[0].view, y_ref, TOL_BF16)
    vec_rel(rec, "mean", small[1].view[:, 0], mean_ref, 1e-4)
    vec_rel(rec, "rstd", small[2].view[:, 0], rstd_ref, 1e-4)
    if fp8:
        y_host = small[0].view.cpu().float()
        want8 = (y_host * 16.0).clamp(-448, 448).to(torch.float8_e4m3fn)
        assert torch.equal(small[3].view.cpu().view(torch.float8_e4m3fn).float(), want8.float()), "y8 is not sat(y * scale) as e4m3"
        assert float(small[4]) == float(y_host.abs().max())
    big = go(M, rec)
    verify(rec, "y", big[0], small[0], P)
    verify(rec, "mean", big[1], small[1], P)
    verify(rec, "rstd", big[2], small[2], P)
    if fp8:
        verify(rec, "y8", big[3], small[3], P, sentinel_ok=True)
        assert torch.equal(big[4], small[4]), "amax of the big launch differs from the period's"


@pytest.mark.parametrize("reduce", ["in-launch", "batched"])
def test_layernorm_backward(lib, rec, reduce):
    """dy, x, dres and dx [M, 384] past 2^32 bytes; dgamma / dbeta over ~5.6 M rows against the exact fp64 value of the analytic per-row
    terms dy * xhat and dy; `batched`: ap_layernorm_bwd_partial + ap_layernorm_bwd_reduce_batched"""
    from autoprog_amd._lib import LnReduce
    C, P = LN_C, P_ROWS
    M = BA.rows_past(C, BF, 32, tile=16)
    x0, dy0, dres0 = rnd(P, C, shift=0.5, seed=41), rnd(P, C, scale=0.05, seed=44), rnd(P, C, scale=0.05, seed=45)
    gamma = frand(C, seed=42, scale=0.2, shift=1.0)
    _, mean_ref, rstd_ref = ln_reference(x0, gamma, torch.zeros(C))
    mean0, rstd0 = mean_ref.float()[:, None], rstd_ref.float()[:, None]
    gd = dev(gamma)

    def go(rows, r):
        x, dy, dres = pin(r, "x", x0, rows), pin(r, "dy", dy0, rows), pin(r, "dres", dres0, rows)
        mean, rstd = pin(r, "mean", mean0, rows), pin(r, "rstd", rstd0, rows)
        dx = pout(r, "dx", rows, C)
        dg, db = pvec(r, "dgamma", C), pvec(r, "dbeta", C)
        dg.view.zero_()
        db.view.zero_()
        ws_bytes = lib.ap_layernorm_bwd_workspace(rows, C)
        ws = BA.BigOut(1, ws_bytes // 4, dtype=F32, device="cuda", pre=1, post=1, what="workspace")
        args = (dy.data_ptr(), x.data_ptr(), gd.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dres.data_ptr(), dx.ptr())
        if reduce == "in-launch":
            rc = lib.ap_layernorm_bwd(*args, dg.ptr(), db.ptr(), rows, C, ws.ptr(), ws_bytes, S())
            assert rc == 0, "ap_layernorm_bwd: code %d" % rc
        else:
            n = ctypes.c_int(0)
            rc = lib.ap_layernorm_bwd_partial(*args, rows, C, ws.ptr(), ws_bytes, ctypes.byref(n), S())
            assert rc == 0 and n.value > 0, "ap_layernorm_bwd_partial: code %d, %d partial rows" % (rc, n.value)
            item = LnReduce(partial=ws.ptr(), n_partial=n.value, C=C, dgamma=dg.ptr(), dbeta=db.ptr())
            rc = lib.ap_layernorm_bwd_reduce_batched(ctypes.addressof(item), 1, S())
            assert rc == 0, "ap_layernorm_bwd_reduce_batched: code %d" % rc
        sync()
        ws.check_guards()
        dg.check_guards()
        db.check_guards()
        return [dx, dg, db, (x, dy, mean, rstd)]
    small = go(P, None)
    # fp64 on the statistics the kernel was given (fp32 mean / rstd of the period)
    xd, dyd = x0.double().requires_grad_(True), dy0.double()
    xhat = (xd - mean0.double()) * rstd0.double()
    mu, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    (((xd - mu) * (var + LN_EPS).rsqrt() * gamma.double()) * dyd).sum().backward()
    tiled(rec, "dx", small[0].view, xd.grad + dres0.double(), TOL_BF16)
    terms_g, terms_b = (dyd * xhat).detach(), dyd
    vec_rel(rec, "dgamma (period)", small[1].view[:, 0], terms_g.sum(0), TOL_F32)
    vec_rel(rec, "dbeta (period)", small[2].view[:, 0], terms_b.sum(0), TOL_F32)
    del small[3:]
    big = go(M, rec)
    verify(rec, "dx", big[0], small[0], P)
    x, dy, mean, rstd = big[3]
    emu_g = torch.zeros(C, dtype=F32, device="cuda")
    for s in range(0, M, 65536):
        e = slice(s, s + 65536)
        emu_g += (dy[e].float() * ((x[e].float() - mean[e]) * rstd[e])).sum(0)
    reduction(rec, "dgamma", big[1].view[:, 0], emu_g, BA.periodic_sum(terms_g, M))
    reduction(rec, "dbeta", big[2].view[:, 0], emu_colsum(dy, C), BA.periodic_sum(terms_b, M))


# ======================================================================================================================== B. elementwise
EW_C = 384


def test_cast_f32_bf16(lib, rec):
    """n past 2^31 elements: the fp32 source passes 2^33 bytes, the bf16 destination 2^32"""
    P = P_ROWS
    M = BA.rows_past(EW_C, BF, 32, tile=16)
    s0 = frand(P, EW_C, seed=51)

    def go(rows, r):
        src = pin(r, "src", s0, rows, powers=(31, 32, 33))
        dst = pout(r, "dst", rows, EW_C)
        rc = lib.ap_cast_f32_bf16(src.data_ptr(), dst.ptr(), rows * EW_C, S())
        assert rc == 0
        sync()
        return dst
    small = go(P, None)
    assert torch.equal(small.view.cpu(), s0.to(BF)), "the cast is not round-to-nearest-even"
    big = go(M, rec)
    assert M * EW_C > 2 ** 31
    verify(rec, "dst", big, small, P)


def test_cast_bf16_f32(lib, rec):
    """the bf16 source passes 2^32 bytes, the fp32 destination 2^33"""
    P = P_ROWS
    M = BA.rows_past(EW_C, BF, 32, tile=16)
    s0 = rnd(P, EW_C, seed=52)

    def go(rows, r):
        src = pin(r, "src", s0, rows)
        dst = pout(r, "dst", rows, EW_C, dtype=F32, powers=(31, 32, 33))
        rc = lib.ap_cast_bf16_f32(src.data_ptr(), dst.ptr(), rows * EW_C, S())
        assert rc == 0
        sync()
        return dst
    small = go(P, None)
    assert torch.equal(small.view.cpu(), s0.float())
    big = go(M, rec)
    verify(rec, "dst", big, small, P)


def test_quantize_fp8(lib, rec):
    """x past 2^32 bytes, the e4m3 bytes past 2^31 elements; amax of the big launch equals the period's"""
    P = P_ROWS
    M = BA.rows_past(EW_C, BF, 32, tile=16)
    x0 = rnd(P, EW_C, scale=3.0, seed=53)
    scale = dev(torch.tensor([8.0], dtype=F32))

    def go(rows, r):
        x = pin(r, "x", x0, rows)
        y = pout(r, "y8", rows, EW_C, dtype=U8)
        amax = torch.zeros(1, dtype=F32, device="cuda")
        rc = lib.ap_quantize_fp8(x.data_ptr(), y.ptr(), rows * EW_C, scale.data_ptr(), amax.data_ptr(), S())
        assert rc == 0
        sync()
        return y, amax
    y_s, amax_s = go(P, None)
    want = (x0.float() * 8.0).clamp(-448, 448).to(torch.float8_e4m3fn)
    assert torch.equal(y_s.view.cpu().view(torch.float8_e4m3fn).float(), want.float())
    assert float(amax_s) == float(x0.float().abs().max())
    y_b, amax_b = go(M, rec)
    verify(rec, "y8", y_b, y_s, P, sentinel_ok=True)
    assert torch.equal(amax_b, amax_s)


def test_quantize_bf8_with_colsum(lib, rec):
    """g [rows, 384] past 2^32 bytes -> e5m2 bytes past 2^31 elements, amax, and the fused bias gradient over ~5.6 M rows"""
    P, C = P_ROWS, EW_C
    M = BA.rows_past(C, BF, 32, tile=16)
    g0 = rnd(P, C, scale=0.05, seed=54)
    scale = dev(torch.tensor([4096.0], dtype=F32))

    def go(rows, r):
        g = pin(r, "g", g0, rows)
        y = pout(r, "y8", rows, C, dtype=U8)
        amax = torch.zeros(1, dtype=F32, device="cuda")
        cs = pvec(r, "colsum", C)
        cs.view.zero_()
        rc = lib.ap_quantize_bf8(g.data_ptr(), y.ptr(), rows * C, scale.data_ptr(), amax.data_ptr(), cs.ptr(), rows, C, None, 1.0, None, S())
        assert rc == 0
        sync()
        cs.check_guards()
        return y, amax, cs, g
    y_s, amax_s, cs_s, _ = go(P, None)
    want = (g0.float() * 4096.0).clamp(-57344, 57344).to(torch.float8_e5m2)
    assert torch.equal(y_s.view.cpu().view(torch.float8_e5m2).float(), want.float())
    vec_rel(rec, "colsum (period)", cs_s.view[:, 0], g0.double().sum(0), TOL_F32)
    y_b, amax_b, cs_b, g = go(M, rec)
    verify(rec, "y8", y_b, y_s, P, sentinel_ok=True)
    assert torch.equal(amax_b, amax_s)
    reduction(rec, "colsum", cs_b.view[:, 0], emu_colsum(g, C), BA.periodic_sum(g0.double(), M))


def test_row_scale(lib, rec):
    """x and y past 2^32 bytes, one scale per row (the scale vector is periodic as well)"""
    P = P_ROWS
    M = BA.rows_past(EW_C, BF, 32, tile=16)
    x0 = rnd(P, EW_C, seed=55)
    s0 = (torch.rand(P, 1, generator=torch.Generator().manual_seed(56)) > 0.2).float() / 0.8

    def go(rows, r):
        x, sc = pin(r, "x", x0, rows), pin(r, "scale", s0, rows)
        y = pout(r, "y", rows, EW_C)
        rc = lib.ap_row_scale(x.data_ptr(), sc.data_ptr(), y.ptr(), rows, EW_C, 1, S())
        assert rc == 0
        sync()
        return y
    small = go(P, None)
    tiled(rec, "y", small.view, x0.double() * s0.double(), TOL_BF16)
    big = go(M, rec)
    verify(rec, "y", big, small, P)


def test_add_bcast(lib, rec):
    """y = a + b, b one row broadcast over all rows: a and y past 2^32 bytes"""
    P = P_ROWS
    M = BA.rows_past(EW_C, BF, 32, tile=16)
    a0, b = rnd(P, EW_C, seed=57), rnd(1, EW_C, seed=58)
    bd = dev(b)

    def go(rows, r):
        a = pin(r, "a", a0, rows)
        y = pout(r, "y", rows, EW_C)
        rc = lib.ap_add_bcast(a.data_ptr(), bd.data_ptr(), y.ptr(), rows * EW_C, EW_C, S())
        assert rc == 0
        sync()
        return y
    small = go(P, None)
    tiled(rec, "y", small.view, a0.double() + b.double(), TOL_BF16)
    big = go(M, rec)
    verify(rec, "y", big, small, P)


def test_sum_reps_acc(lib, rec):
    """out[i] += sum_r x[r, i] over reps repetitions of n = 393 216 elements: x past 2^32 bytes, periodic in r with period 13"""
    n, P = 1024 * EW_C, 13
    reps = BA.rows_past(n, BF, 32, tile=16)
    x0 = rnd(P, n, scale=0.5, seed=59)
    x = pin(rec, "x", x0, reps)
    out = pout(rec, "out", 1, n, dtype=F32)
    out.view.zero_()
    rc = lib.ap_sum_reps_acc(x.data_ptr(), out.ptr(), n, reps, S())
    assert rc == 0
    sync()
    out.check_guards()
    emu = torch.zeros(n, dtype=F32, device="cuda")
    for s in range(0, reps, 512):
        emu += x[s:s + 512].float().sum(0)
    reduction(rec, "out", out.view[0], emu, BA.periodic_sum(x0.double(), reps))


def test_sum_reps_acc_at_its_repetition_limit(lib, rec):
    """AP_SUM_REPS_MAX = 16 * 65 535 repetitions (the grid's y axis) of n = 8 elements pass; one more is refused before any launch"""
    n, P, reps = 8, 13, 16 * 65535
    x0 = rnd(P, n, scale=0.5, seed=59)
    x = pin(rec, "x", x0, reps + 1)
    out = pout(rec, "out", 1, n, dtype=F32)
    out.view.zero_()
    assert lib.ap_sum_reps_acc(x.data_ptr(), out.ptr(), n, reps + 1, S()) == -1
    sync()
    assert bool((out.view == 0).all())
    assert lib.ap_sum_reps_acc(x.data_ptr(), out.ptr(), n, reps, S()) == 0
    sync()
    out.check_guards()
    emu = torch.zeros(n, dtype=F32, device="cuda")
    for s0 in range(0, reps, 65536):
        emu += x[s0:min(reps, s0 + 65536)].float().sum(0)
    reduction(rec, "out", out.view[0], emu, BA.periodic_sum(x0.double(), reps))


def test_colsum_acc(lib, rec):
    """out[n] += sum_m A[m, n] over ~5.6 M rows, A past 2^32 bytes"""
    P, C = P_ROWS, EW_C
    M = BA.rows_past(C, BF, 32, tile=256)
    a0 = rnd(P, C, scale=0.05, seed=60)
    a = pin(rec, "A", a0, M)
    out = pvec(rec, "out", C)
    out.view.zero_()
    rc = lib.ap_colsum_acc(a.data_ptr(), C, out.ptr(), M, C, S())
    assert rc == 0
    sync()
    out.check_guards()
    reduction(rec, "out", out.view[:, 0], emu_colsum(a, C), BA.periodic_sum(a0.double(), M))


# ======================================================================================================================== B. narrow losses
NC = 1000                            # classes of the narrow (register) kernels; ld = C


def test_narrow_sparse_ce(lib, rec):
    """ap_soft_ce_sparse_fwd_bwd at 1000 classes (one wave per row): logits and dlogits past 2^32 bytes; rows_per_batch = 1"""
    K, smoothing, P = 8, 0.1, P_ROWS
    M = BA.rows_past(NC, BF, 32, tile=16)
    gs = 0.5 / M
    g = torch.Generator().manual_seed(61)
    l0 = rnd(P, NC, scale=2.0, seed=62)
    i0 = torch.randint(0, NC, (P, K), generator=g, dtype=I32)
    i0[0] = torch.tensor([0, 1, NC - 2, NC - 1, 5, 5, -1, NC], dtype=I32)
    v0 = torch.rand(P, K, generator=g) + 0.05

    def go(rows, r):
        x, idx, val = pin(r, "logits", l0, rows), pin(r, "idx", i0, rows), pin(r, "val", v0, rows)
        loss, dl = pvec(r, "row_loss", rows), pout(r, "dlogits", rows, NC)
        rc = lib.ap_soft_ce_sparse_fwd_bwd(x.data_ptr(), NC, idx.data_ptr(), val.data_ptr(), K, K, K, 1, smoothing, loss.ptr(), dl.ptr(), gs, rows, NC, 1.0, 0, S())
        assert rc == 0, "code %d" % rc
        sync()
        return loss, dl
    loss_s, dl_s = go(P, None)
    t = torch.full((P, NC), smoothing / NC, dtype=torch.float64)
    ok = (i0 >= 0) & (i0 < NC)
    t.scatter_add_(1, i0.clamp(0, NC - 1).long(), (1 - smoothing) * v0.double() * ok)
    rows_ref, grad_ref = ce_reference(l0, t, gs)
    vec_rel(rec, "row_loss", loss_s.view[:, 0], rows_ref, 1e-4)
    tiled(rec, "dlogits", dl_s.view, grad_ref, TOL_BF16)
    loss_b, dl_b = go(M, rec)
    verify(rec, "row_loss", loss_b, loss_s, P)
    verify(rec, "dlogits", dl_b, dl_s, P)


def test_narrow_dense_ce(lib, rec):
    """ap_soft_ce_fwd_bwd at 1000 classes with a row-major fp32 target [M, C] (rows_per_batch = 1): the target passes 2^33 bytes"""
    P = P_ROWS
    M = BA.rows_past(NC, BF, 32, tile=16)
    gs = 0.5 / M
    g = torch.Generator().manual_seed(63)
    l0 = rnd(P, NC, scale=2.0, seed=64)
    t0 = torch.rand(P, NC, generator=g) * (torch.rand(P, NC, generator=g) < 0.05) + 0.1 / NC

    def go(rows, r):
        x, t = pin(r, "logits", l0, rows), pin(r, "target", t0, rows, powers=(31, 32, 33))
        loss, dl = pvec(r, "row_loss", rows), pout(r, "dlogits", rows, NC)
        rc = lib.ap_soft_ce_fwd_bwd(x.data_ptr(), NC, t.data_ptr(), NC, 1, NC, 1, loss.ptr(), dl.ptr(), gs, rows, NC, 1.0, 0, S())
        assert rc == 0, "code %d" % rc
        sync()
        return loss, dl
    loss_s, dl_s = go(P, None)
    rows_ref, grad_ref = ce_reference(l0, t0.double(), gs)
    vec_rel(rec, "row_loss", loss_s.view[:, 0], rows_ref, 1e-4)
    tiled(rec, "dlogits", dl_s.view, grad_ref, TOL_BF16)
    loss_b, dl_b = go(M, rec)
    verify(rec, "row_loss", loss_b, loss_s, P)
    verify(rec, "dlogits", dl_b, dl_s, P)


def test_narrow_softmax_topk(lib, rec):
    """ap_softmax_topk_rows at 1000 classes, K = 5: logits past 2^32 bytes"""
    K, P = 5, P_ROWS
    M = BA.rows_past(NC, BF, 32, tile=16)
    l0 = rnd(P, NC, scale=2.0, seed=65)

    def go(rows, r):
        x = pin(r, "logits", l0, rows)
        idx, val = pout(r, "idx", rows, K, dtype=I32), pout(r, "val", rows, K, dtype=F32)
        rc = lib.ap_softmax_topk_rows(x.data_ptr(), NC, NC, K, 1.0, idx.ptr(), val.ptr(), K, K, 1, rows, S())
        assert rc == 0, "code %d" % rc
        sync()
        return idx, val
    idx_s, val_s = go(P, None)
    check_pairs(idx_s.view, val_s.view, *topk_ref(l0, K), rec.name)
    idx_b, val_b = go(M, rec)
    verify(rec, "idx", idx_b, idx_s, P)
    verify(rec, "val", val_b, val_s, P)


def test_classify_stats(lib, rec):
    """ap_classify_stats at 1000 classes: logits past 2^32 bytes; one label of the period lies outside the classes (loss 0, rank -1)"""
    P = P_ROWS
    M = BA.rows_past(NC, BF, 32, tile=4)
    l0 = rnd(P, NC, scale=2.0, seed=66)
    lab0 = torch.randint(0, NC, (P,), generator=torch.Generator().manual_seed(67))
    lab0[7] = -1

    def go(rows, r):
        x = pin(r, "logits", l0, rows)
        labels = lab0.cuda().repeat((rows + P - 1) // P)[:rows].contiguous()              # (int64 [rows]: 45 MB, far from any boundary)
        loss, rank = pvec(r, "loss", rows), pvec(r, "rank", rows, I32)
        rc = lib.ap_classify_stats(x.data_ptr(), NC, NC, labels.data_ptr(), loss.ptr(), rank.ptr(), rows, S())
        assert rc == 0, "code %d" % rc
        sync()
        return loss, rank
    loss_s, rank_s = go(P, None)
    z = l0.double()
    valid = lab0 >= 0
    want = torch.where(valid, torch.logsumexp(z, 1) - z.gather(1, lab0.clamp(min=0)[:, None])[:, 0], torch.zeros(P, dtype=torch.float64))
    want_rank = torch.where(valid, (z > z.gather(1, lab0.clamp(min=0)[:, None])).sum(1), torch.full((P,), -1))
    vec_rel(rec, "loss", loss_s.view[:, 0], want, 1e-4)
    assert torch.equal(rank_s.view[:, 0].cpu().long(), want_rank), "ranks differ from the reference"
    loss_b, rank_b = go(M, rec)
    verify(rec, "loss", loss_b, loss_s, P)
    verify(rec, "rank", rank_b, rank_s, P)


@pytest.mark.parametrize("mode", [0, 1], ids=["soft", "hard"])
def test_distill(lib, rec, mode):
    """ap_distill_fwd_bwd at 1000 classes: student, teacher and dstudent past 2^32 bytes"""
    P, T = P_ROWS, 2.0
    M = BA.rows_past(NC, BF, 32, tile=8)
    gs = 0.5 / M
    s0, t0 = rnd(P, NC, scale=2.0, seed=68), rnd(P, NC, scale=2.0, seed=69)

    def go(rows, r):
        s, t = pin(r, "student", s0, rows), pin(r, "teacher", t0, rows)
        loss, ds = pvec(r, "row_loss", rows), pout(r, "dstudent", rows, NC)
        rc = lib.ap_distill_fwd_bwd(s.data_ptr(), NC, t.data_ptr(), NC, NC, mode, 1.0 / T, loss.ptr(), ds.ptr(), gs, rows, S())
        assert rc == 0, "code %d" % rc
        sync()
        return loss, ds
    loss_s, ds_s = go(P, None)
    xs, xt = s0.double().requires_grad_(True), t0.double()
    if mode == 0:
        rows_ref = T * T * (F.softmax(xt / T, 1) * (F.log_softmax(xt / T, 1) - F.log_softmax(xs / T, 1))).sum(1)
    else:
        rows_ref = F.cross_entropy(xs, xt.argmax(1), reduction="none")
    (rows_ref.sum() * gs).backward()
    vec_rel(rec, "row_loss", loss_s.view[:, 0], rows_ref.detach(), 1e-4)
    tiled(rec, "dstudent", ds_s.view, xs.grad, TOL_BF16)
    loss_b, ds_b = go(M, rec)
    verify(rec, "row_loss", loss_b, loss_s, P)
    verify(rec, "dstudent", ds_b, ds_s, P)


# ======================================================================================================================== B. per-image kernels
# P counts IMAGES here (13): an operand is [images, elements per image], so the period in rows keeps the odd factor 13.  The guard "rows" of an
# output are three whole images.
P_IMAGES = 13


def images_past(image_elems, dtype, k=32):
    """the smallest batch that puts three whole images and one more behind the image that holds byte 2^k"""
    return BA.rows_past(image_elems, dtype, k, tile=1)


MHSA_CASES = [pytest.param(196, 2, 32, False, id="resident-persistent-196x2x32"), pytest.param(257, 1, 48, False, id="blocked-257x1x48"),
              pytest.param(257, 1, 48, True, id="blocked-fp8-257x1x48")]


@pytest.mark.parametrize("N,heads,hd,fp8", MHSA_CASES)
def test_mhsa(lib, rec, N, heads, hd, fp8):
    """ap_mhsa_fwd / ap_mhsa_bwd (fp8: ap_mhsa_fwd_fp8, forward only) with qkv and dqkv past 2^32 bytes; out_row_scale drops one phase of the
    period -- an image of that phase lies behind the boundary -- and its dout is zero, as the backward's contract says"""
    from oracle import ref_cpu as R
    Pi, C = P_IMAGES, heads * hd
    img = N * 3 * C
    B = images_past(img, BF)
    scale = hd ** -0.5
    dropped = (B - 2) % Pi
    assert B - 2 > BA.boundary_row(img, BF, 32)
    qkv0, do0 = rnd(Pi * N, 3 * C, seed=71), rnd(Pi * N, C, seed=72).reshape(Pi, N * C).clone()
    rs0 = torch.ones(Pi, 1)
    rs0[dropped] = 0.0
    do0[dropped] = 0
    q_scale = dev(torch.tensor([24.0], dtype=F32))

    def go(images, r):
        qkv, do, rs = pin(r, "qkv", qkv0.reshape(Pi, img), images), pin(r, "dout", do0, images), pin(r, "out_row_scale", rs0, images)
        out, lse = pout(r, "out", images, N * C), pout(r, "lse", images, heads * N, dtype=F32)
        if fp8:
            out8, amax = pout(r, "out8", images, N * C, dtype=U8), torch.zeros(1, dtype=F32, device="cuda")
            rc = lib.ap_mhsa_fwd_fp8(qkv.data_ptr(), out.ptr(), out8.ptr(), q_scale.data_ptr(), amax.data_ptr(), lse.ptr(), images, N, heads, hd, scale, rs.data_ptr(), S())
            assert rc == 0, "ap_mhsa_fwd_fp8: code %d" % rc
            sync()
            return [out, lse, out8, amax]
        rc = lib.ap_mhsa_fwd(qkv.data_ptr(), out.ptr(), lse.ptr(), images, N, heads, hd, scale, rs.data_ptr(), S())
        assert rc == 0, "ap_mhsa_fwd: code %d" % rc
        dqkv = pout(r, "dqkv", images, img)
        ws_bytes = lib.ap_mhsa_bwd_workspace(images, N, heads, hd)
        ws = BA.BigOut(1, max(ws_bytes // 4, 1), dtype=F32, device="cuda", pre=1, post=1, what="workspace")
        rc = lib.ap_mhsa_bwd(qkv.data_ptr(), out.ptr(), do.data_ptr(), lse.ptr(), dqkv.ptr(), images, N, heads, hd, scale, ws.ptr() if ws_bytes else None, ws_bytes, S())
        assert rc == 0, "ap_mhsa_bwd: code %d" % rc
        sync()
        ws.check_guards()
        return [out, lse, dqkv]
    small = go(Pi, None)
    qr = qkv0.double().reshape(Pi, N, 3 * C).requires_grad_(True)
    orf = R.mhsa_core(qr, heads)
    orf.backward(do0.double().reshape(Pi, N, C))
    tiled(rec, "out", small[0].view.reshape(Pi * N, C), (orf.detach() * rs0.double()[:, :, None]).reshape(Pi * N, C), TOL_BF16)
    q, k, _ = qkv0.double().reshape(Pi, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    lse_err = float((small[1].view.cpu().double().reshape(Pi, heads, N) - torch.logsumexp(q @ k.transpose(-1, -2) * scale, dim=-1)).abs().max())
    rec.line("lse | period against fp64: max |error| %.3e (bound 2e-3)" % lse_err)
    assert lse_err < 2e-3
    if fp8:
        o_host = small[0].view.cpu().float()
        want8 = (o_host * 24.0).clamp(-448, 448).to(torch.float8_e4m3fn)
        assert torch.equal(small[2].view.cpu().view(torch.float8_e4m3fn).float(), want8.float()), "out8 is not sat(out * scale) as e4m3"
        assert float(small[3]) == float(o_host.abs().max())
    else:
        gr, dg = qr.grad.reshape(Pi * N, 3, C), small[2].view.reshape(Pi * N, 3, C)
        for i, nm in enumerate("qkv"):
            tiled(rec, "d" + nm, dg[:, i], gr[:, i], 1.5e-2)
    big = go(B, rec)
    verify(rec, "out", big[0], small[0], Pi)
    verify(rec, "lse", big[1], small[1], Pi)
    if fp8:
        verify(rec, "out8", big[2], small[2], Pi, sentinel_ok=True)
        assert torch.equal(big[3], small[3])
    else:
        verify(rec, "dqkv", big[2], small[2], Pi)


def test_class_attention(lib, rec):
    """ap_class_attn_fwd / ap_class_attn_bwd, N = 65 keys, 2 heads of 32: kv and dkv past 2^32 bytes"""
    Pi, N, heads, hd = P_IMAGES, 65, 2, 32
    C = heads * hd
    img = N * 2 * C
    B = images_past(img, BF)
    scale = hd ** -0.5
    q0, kv0, do0 = rnd(Pi, C, seed=73), rnd(Pi * N, 2 * C, seed=74), rnd(Pi, C, seed=75)

    def go(images, r):
        q, kv, do = pin(r, "q", q0, images), pin(r, "kv", kv0.reshape(Pi, img), images), pin(r, "dout", do0, images)
        out, probs = pout(r, "out", images, C), pout(r, "probs", images, heads * N, dtype=F32)
        dq, dkv = pout(r, "dq", images, C), pout(r, "dkv", images, img)
        rc = lib.ap_class_attn_fwd(q.data_ptr(), kv.data_ptr(), None, out.ptr(), probs.ptr(), images, N, heads, hd, scale, S())
        assert rc == 0, "ap_class_attn_fwd: code %d" % rc
        rc = lib.ap_class_attn_bwd(q.data_ptr(), kv.data_ptr(), None, probs.ptr(), do.data_ptr(), dq.ptr(), dkv.ptr(), None, images, N, heads, hd, scale, S())
        assert rc == 0, "ap_class_attn_bwd: code %d" % rc
        sync()
        return [out, probs, dq, dkv]
    small = go(Pi, None)
    qr = q0.double().requires_grad_(True)
    kvr = kv0.double().reshape(Pi, N, 2, heads, hd).requires_grad_(True)
    kk, vv = kvr[:, :, 0].transpose(1, 2), kvr[:, :, 1].transpose(1, 2)
    att = torch.softmax((qr.reshape(Pi, heads, 1, hd) * scale) @ kk.transpose(-1, -2), dim=-1)
    orf = (att @ vv).transpose(1, 2).reshape(Pi, C)
    orf.backward(do0.double())
    tiled(rec, "out", small[0].view, orf.detach(), TOL_BF16)
    vec_rel(rec, "probs", small[1].view, att.detach().reshape(Pi, heads * N), 1e-3)
    tiled(rec, "dq", small[2].view, qr.grad, TOL_BF16)
    tiled(rec, "dkv", small[3].view.reshape(Pi * N, 2 * C), kvr.grad.reshape(Pi * N, 2 * C), TOL_BF16)
    big = go(B, rec)
    for i, nm in enumerate(("out", "probs", "dq", "dkv")):
        verify(rec, nm, big[i], small[i], Pi)


@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_outlook(lib, rec, direction):
    """ap_outlook_fwd / ap_outlook_bwd on 14 x 14 maps with 6 heads (C = 192, 486 logits in ldl = 488): v, y, dy and dv past 2^32 bytes, the
    logits and dlogits past 2^31; the columns 486 .. 487 of dlogits are zeroed"""
    from oracle import ref_cpu as R
    Pi, H, W, heads, hd = P_IMAGES, 14, 14, 6, 32
    C, h, w, nl, ldl = heads * hd, 7, 7, heads * 81, 488
    img, limg = H * W * C, h * w * ldl
    B = images_past(img, BF)
    scale = hd ** -0.5
    v0, dy0 = rnd(Pi, H, W, C, seed=76), rnd(Pi, H, W, C, seed=77)
    lg0 = rnd(Pi * h * w, nl, scale=2.0, seed=78)
    lgp = torch.empty(Pi * h * w, ldl, dtype=BF)
    BA.fill_bits(lgp, 0x7FA5)
    lgp[:, :nl] = lg0

    def go(images, r):
        v, lg = pin(r, "v", v0.reshape(Pi, img), images), pin(r, "logits", lgp.reshape(Pi, limg), images)
        if direction == "forward":
            y = pout(r, "y", images, img)
            rc = lib.ap_outlook_fwd(v.data_ptr(), lg.data_ptr(), ldl, y.ptr(), images, H, W, heads, hd, scale, S())
            assert rc == 0, "ap_outlook_fwd: code %d" % rc
            sync()
            return [y]
        dy = pin(r, "dy", dy0.reshape(Pi, img), images)
        dv, dl = pout(r, "dv", images, img), pout(r, "dlogits", images, limg)
        rc = lib.ap_outlook_bwd(v.data_ptr(), lg.data_ptr(), ldl, dy.data_ptr(), dv.ptr(), dl.ptr(), images, H, W, heads, hd, scale, S())
        assert rc == 0, "ap_outlook_bwd: code %d" % rc
        sync()
        return [dv, dl]
    small = go(Pi, None)
    vr = v0.double().requires_grad_(True)
    lr = lg0.double().reshape(Pi, h, w, nl).requires_grad_(True)
    yr = R.outlook_core(vr, lr, heads)
    if direction == "forward":
        tiled(rec, "y", small[0].view.reshape(-1, C), yr.detach().reshape(-1, C), TOL_BF16)
    else:
        yr.backward(dy0.double())
        tiled(rec, "dv", small[0].view.reshape(-1, C), vr.grad.reshape(-1, C), TOL_BF16)
        dl = small[1].view.reshape(-1, ldl)
        tiled(rec, "dlogits", dl[:, :nl], lr.grad.reshape(-1, nl), TOL_BF16)
        assert bool((dl[:, nl:].view(torch.int16) == 0).all()), "the columns heads * 81 .. ldl-1 of dlogits are not zero bits"
    big = go(B, rec)
    for i, nm in enumerate(("y",) if direction == "forward" else ("dv", "dlogits")):
        verify(rec, nm, big[i], small[i], Pi)


def test_avgpool2_forward(lib, rec):
    """ap_avgpool2_fwd on 13 x 13 x 384 maps (ceil mode: the last row and column pool one pixel): x past 2^32 bytes"""
    Pi, H, W, C = P_IMAGES, 13, 13, 384
    h, w = 7, 7
    B = images_past(H * W * C, BF)
    x0 = rnd(Pi, H, W, C, seed=79)

    def go(images, r):
        x = pin(r, "x", x0.reshape(Pi, -1), images)
        y = pout(r, "y", images, h * w * C)
        rc = lib.ap_avgpool2_fwd(x.data_ptr(), y.ptr(), images, H, W, C, S())
        assert rc == 0
        sync()
        return y
    small = go(Pi, None)
    ref = F.avg_pool2d(x0.double().permute(0, 3, 1, 2), 2, 2, ceil_mode=True, count_include_pad=False).permute(0, 2, 3, 1)
    tiled(rec, "y", small.view.reshape(-1, C), ref.reshape(-1, C), TOL_BF16)
    big = go(B, rec)
    verify(rec, "y", big, small, Pi)


def test_avgpool2_backward(lib, rec):
    """ap_avgpool2_bwd_acc: dx += the pooled gradient, dx past 2^32 bytes (read and written in place: it starts from a periodic base)"""
    Pi, H, W, C = P_IMAGES, 13, 13, 384
    h, w = 7, 7
    B = images_past(H * W * C, BF)
    dp0, dx0 = rnd(Pi, h, w, C, seed=80), rnd(Pi, H, W, C, seed=81)

    def go(images, r):
        dp = pin(r, "dpooled", dp0.reshape(Pi, -1), images)
        dx = pout(r, "dx", images, H * W * C)
        BA.fill_periodic(dx.view, dev(dx0.reshape(Pi, -1)))
        BA.check_bands(dx.view, dx0.reshape(Pi, -1), [b for b, _ in BA.boundaries(H * W * C, BF, images)], "dx base")
        rc = lib.ap_avgpool2_bwd_acc(dp.data_ptr(), dx.ptr(), images, H, W, C, S())
        assert rc == 0
        sync()
        return dx
    small = go(Pi, None)
    xr = torch.zeros(Pi, H, W, C, dtype=torch.float64, requires_grad=True)
    F.avg_pool2d(xr.permute(0, 3, 1, 2), 2, 2, ceil_mode=True, count_include_pad=False).permute(0, 2, 3, 1).backward(dp0.double())
    tiled(rec, "dx", small.view.reshape(-1, C), (dx0.double() + xr.grad).reshape(-1, C), TOL_BF16)
    big = go(B, rec)
    verify(rec, "dx", big, small, Pi)


def test_mix_token_swap(lib, rec):
    """ap_mix_token_swap on 14 x 14 x 384 maps: the box of image b comes from image B-1-b, whose phase is (B-1-b) % 13 -- the small launch
    has Bs = 13 + B % 13 images, so that its first 13 images meet partners of the same phases"""
    Pi, H, W, C = P_IMAGES, 14, 14, 384
    img = H * W * C
    B = images_past(img, BF)
    Bs = Pi + B % Pi
    assert Bs % Pi == B % Pi and Bs >= Pi
    r0, r1, c0, c1 = 3, 10, 5, 14
    x0 = rnd(Pi, H, W, C, seed=82)

    def go(images, r):
        x = pin(r, "x", x0.reshape(Pi, img), images)
        y = pout(r, "y", images, img)
        rc = lib.ap_mix_token_swap(x.data_ptr(), y.ptr(), images, H, W, C, r0, r1, c0, c1, S())
        assert rc == 0
        sync()
        return y
    small = go(Bs, None)
    xs = x0[torch.arange(Bs) % Pi]
    ref = xs.clone()
    ref[:, r0:r1, c0:c1] = xs.flip(0)[:, r0:r1, c0:c1]
    assert torch.equal(small.view.cpu().reshape(Bs, H, W, C), ref), "the swap of the small launch differs from the reference"
    big = go(B, rec)
    verify(rec, "y", big, small, Pi)


# ======================================================================================================================== B. BatchNorm + ReLU
BN_C, BN_EPS = 64, 1e-5


def bn_apply_ref(x, gamma, beta, mean, rstd):
    return torch.relu((x.double() - mean.double()) * rstd.double() * gamma.double() + beta.double())


def test_bn_relu_forward(lib, rec):
    """ap_bn_relu_fwd at C = 64, ~33.6 M rows, x and y past 2^32 bytes.  eval: mean / rstd are inputs and every row is its own -- bit-identical to
    the period.  training: the batch statistics over all rows against the exact fp64 value; y then depends on those statistics, so it is
    compared bit for bit with an EVAL launch on the period that is given the statistics the big launch produced."""
    C, P = BN_C, P_ROWS
    M = BA.rows_past(C, BF, 32, tile=64)
    x0 = rnd(P, C, shift=0.3, seed=83)
    gamma, beta = frand(C, seed=84, scale=0.2, shift=1.0), frand(C, seed=85, scale=0.2)
    gd, bd = dev(gamma), dev(beta)
    mean_in, rstd_in = frand(C, seed=86, scale=0.1, shift=0.3), frand(C, seed=87, scale=0.05, shift=1.0)

    def go(rows, r, training, mean, rstd):
        x = pin(r, "x", x0, rows)
        y = pout(r, "y", rows, C)
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        ws_bytes = lib.ap_bn_relu_workspace(rows, C)
        ws = BA.BigOut(1, ws_bytes // 4, dtype=F32, device="cuda", pre=1, post=1, what="workspace")
        rc = lib.ap_bn_relu_fwd(x.data_ptr(), gd.data_ptr(), bd.data_ptr(), rm.data_ptr(), rv.data_ptr(), 1 if training else 0, 0.1, BN_EPS, y.ptr(),
                                mean.ptr(), rstd.ptr(), rows, C, ws.ptr(), ws_bytes, S())
        assert rc == 0, "ap_bn_relu_fwd: code %d" % rc
        sync()
        ws.check_guards()
        mean.check_guards()
        rstd.check_guards()
        return y, x, rm, rv

    def stats(values_mean, values_rstd):
        m, s = pvec(None, "mean", C), pvec(None, "rstd", C)
        m.view[:, 0] = values_mean.cuda()
        s.view[:, 0] = values_rstd.cuda()
        return m, s
    # eval
    m_s, s_s = stats(mean_in, rstd_in)
    y_s, _, _, _ = go(P, None, False, m_s, s_s)
    tiled(rec, "y (eval)", y_s.view, bn_apply_ref(x0, gamma, beta, mean_in, rstd_in), TOL_BF16)
    m_b, s_b = stats(mean_in, rstd_in)
    y_b, _, _, _ = go(M, rec, False, m_b, s_b)
    verify(rec, "y (eval)", y_b, y_s, P)
    del y_b, y_s
    # training
    m_t, s_t = pvec(rec, "mean", C), pvec(rec, "rstd", C)
    y_t, x, rm, rv = go(M, rec, True, m_t, s_t)
    sum1, sum2 = BA.periodic_sum(x0.double(), M), BA.periodic_sum(x0.double() ** 2, M)
    mean_ref = sum1 / M
    var_ref = sum2 / M - mean_ref ** 2
    emu1 = emu_colsum(x, C)
    reduction(rec, "batch mean", m_t.view[:, 0], emu1 / M, mean_ref)
    got_var = 1.0 / s_t.view[:, 0].cpu().double() ** 2 - BN_EPS
    emu2 = torch.zeros(C, dtype=F32, device="cuda")
    for s0 in range(0, M, 65536):
        emu2 += x[s0:s0 + 65536].float().square().sum(0)
    reduction(rec, "batch variance (from rstd)", got_var, emu2 / M - (emu1 / M) ** 2, var_ref)
    vec_rel(rec, "running_mean", rm, 0.1 * mean_ref, TOL_F32)
    vec_rel(rec, "running_var", rv, 0.9 + 0.1 * var_ref * M / (M - 1), TOL_F32)
    m_e, s_e = stats(m_t.view[:, 0].cpu(), s_t.view[:, 0].cpu())
    y_e, _, _, _ = go(P, None, False, m_e, s_e)
    tiled(rec, "y (training)", y_e.view, bn_apply_ref(x0, gamma, beta, mean_ref, (var_ref + BN_EPS).rsqrt()), TOL_BF16)
    verify(rec, "y (training) against an eval launch on the period with the same statistics", y_t, y_e, P)


def test_bn_relu_backward(lib, rec):
    """ap_bn_relu_bwd at C = 64, ~33.6 M rows: dgamma / dbeta against the exact fp64 value; dx depends on those sums, so bit identity with a
    launch on the period cannot hold -- the big dx must instead repeat ITSELF with the period, bit for bit (every row sees the same sums), and its
    first period is held against fp64"""
    C, P = BN_C, P_ROWS
    M = BA.rows_past(C, BF, 32, tile=64)
    x0, dy0 = rnd(P, C, shift=0.3, seed=83), rnd(P, C, scale=0.05, seed=88)
    gamma, beta = frand(C, seed=84, scale=0.2, shift=1.0), frand(C, seed=85, scale=0.2)
    sum1, sum2 = BA.periodic_sum(x0.double(), M), BA.periodic_sum(x0.double() ** 2, M)
    mean64 = sum1 / M
    rstd64 = (sum2 / M - mean64 ** 2 + BN_EPS).rsqrt()
    mean, rstd = mean64.float(), rstd64.float()
    x, dy = pin(rec, "x", x0, M), pin(rec, "dy", dy0, M)
    dx = pout(rec, "dx", M, C)
    dg, db = pvec(rec, "dgamma", C), pvec(rec, "dbeta", C)
    dg.view.zero_()
    db.view.zero_()
    ws_bytes = lib.ap_bn_relu_workspace(M, C)
    ws = BA.BigOut(1, ws_bytes // 4, dtype=F32, device="cuda", pre=1, post=1, what="workspace")
    gd, bd, md, sd = dev(gamma), dev(beta), dev(mean), dev(rstd)
    rc = lib.ap_bn_relu_bwd(dy.data_ptr(), x.data_ptr(), gd.data_ptr(), bd.data_ptr(), md.data_ptr(), sd.data_ptr(), dx.ptr(), dg.ptr(), db.ptr(), M, C,
                            ws.ptr(), ws_bytes, S())
    assert rc == 0, "ap_bn_relu_bwd: code %d" % rc
    sync()
    for o in (ws, dg, db, dx):
        o.check_guards()
    xhat = (x0.double() - mean.double()) * rstd.double()
    dz = dy0.double() * ((xhat * gamma.double() + beta.double()) > 0)
    want_g, want_b = BA.periodic_sum(dz * xhat, M), BA.periodic_sum(dz, M)
    emu_g, emu_b = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    for s in range(0, M, 65536):
        e = slice(s, s + 65536)
        xh = (x[e].float() - md) * sd
        z = dy[e].float() * ((xh * gd + bd) > 0)
        emu_g += (z * xh).sum(0)
        emu_b += z.sum(0)
    reduction(rec, "dgamma", dg.view[:, 0], emu_g, want_g)
    reduction(rec, "dbeta", db.view[:, 0], emu_b, want_b)
    dx_ref = gamma.double() * rstd.double() * (dz - want_b / M - xhat * want_g / M)
    tiled(rec, "dx (first period)", dx.view[:P], dx_ref, TOL_BF16)
    n = BA.compare_periodic(dx.view, dx.view[:P], C, "%s dx" % rec.name)
    rec.line("dx | %d rows bit-identical to the output's own first period: yes (a launch on the period has other sums: no exact comparison with it)" % n)


# ======================================================================================================================== B. the fused MLP
def mlp_args(**kw):
    from autoprog_amd._lib import MlpFusedArgs
    a = MlpFusedArgs()
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("mode", ["forward", "forward-layernorm", "infer", "infer-layernorm", "backward"])
def test_mlp_fused(lib, rec, mode):
    """ap_mlp_fused / ap_mlp_fused_infer at c = 384, m % 128 == 0, m such that x (and out, the residual) pass 2^31 bytes and hidden_out 2^32
    (its code bytes 2^31): one 128-row block per workgroup at any m, so the comparison launch runs on round_up(P, 128) rows"""
    from autoprog_amd import ops
    C, Hd, P = 384, 1152, P_ROWS
    M = max(BA.rows_past(C, BF, 31, tile=128, multiple=128), BA.rows_past(Hd, BF, 32, tile=128, multiple=128))
    Ms = BA.round_up(P, 128)
    ln, infer, bwd = mode.endswith("layernorm"), mode.startswith("infer"), mode == "backward"
    x0 = rnd(P, C, seed=91) if not ln else (rnd(P, C, seed=91).float() * 2.5 + 1.5).to(BF)
    w1, w2 = rnd(Hd, C, scale=C ** -0.5, seed=92), rnd(C, Hd, scale=Hd ** -0.5, seed=93)
    b1, b2 = frand(Hd, seed=94, scale=0.3), frand(C, seed=95, scale=0.3)
    res0 = rnd(P, C, seed=96)
    keep0 = (torch.rand(P, 1, generator=torch.Generator().manual_seed(97)) > 0.2).float()
    keep0[0] = 0.0
    lg, lb = frand(C, seed=98, scale=0.3, shift=1.0), frand(C, seed=99, scale=0.2)
    c0 = torch.randint(0, 256, (P, Hd), dtype=U8, generator=torch.Generator().manual_seed(100))
    dw1, dw2, db1, db2, dlg, dlb = dev(w1), dev(w2), dev(b1), dev(b2), dev(lg), dev(lb)
    w2t, w1t = dev(w2.t().contiguous()), dev(w1.t().contiguous())

    def go(rows, r):
        x = pin(r, "x", x0, rows)
        out = pout(r, "out", rows, C)
        keep, rs = pin(r, "row_scale_hidden", keep0, rows), pin(r, "row_scale_out", keep0 / 0.8, rows)
        outs = {"out": out}
        if bwd:
            codes = pin(r, "codes", c0, rows)
            outs["hidden_out"] = hid = pout(r, "hidden_out", rows, Hd)
            a = mlp_args(x=x.data_ptr(), ldx=C, wa=w2t.data_ptr(), ldwa=C, wb=w1t.data_ptr(), ldwb=Hd, out=out.ptr(), ldo=C, hidden_out=hid.ptr(), ldh=Hd,
                         codes=codes.data_ptr(), row_scale_hidden=rs.data_ptr(), rows_per_scale=1, m=rows, c=C, hidden=Hd, backward=1)
            rc = lib.ap_mlp_fused(ctypes.byref(a), S())
        else:
            res = x if ln else pin(r, "residual", res0, rows)                     # (with the LayerNorm the residual is its input, as in the block)
            a = mlp_args(wa=dw1.data_ptr(), ldwa=C, wb=dw2.data_ptr(), ldwb=Hd, out=out.ptr(), ldo=C, ldh=Hd, bias1=db1.data_ptr(), bias2=db2.data_ptr(),
                         row_scale_hidden=keep.data_ptr(), row_scale_out=rs.data_ptr(), rows_per_scale=1, residual=res.data_ptr(), ldr=C,
                         m=rows, c=C, hidden=Hd, backward=0)
            if ln:
                a.ln_in, a.ld_ln, a.ln_gamma, a.ln_beta, a.ln_eps = x.data_ptr(), C, dlg.data_ptr(), dlb.data_ptr(), 1e-5
            else:
                a.x, a.ldx = x.data_ptr(), C
            if not infer:
                outs["hidden_out"], outs["codes"] = pout(r, "hidden_out", rows, Hd), pout(r, "codes", rows, Hd, dtype=U8)
                a.hidden_out, a.codes = outs["hidden_out"].ptr(), outs["codes"].ptr()
                if ln:
                    outs["ln_out"], outs["ln_mean"], outs["ln_rstd"] = pout(r, "ln_out", rows, C), pvec(r, "ln_mean", rows), pvec(r, "ln_rstd", rows)
                    a.ln_out, a.ld_lno, a.ln_mean, a.ln_rstd = outs["ln_out"].ptr(), C, outs["ln_mean"].ptr(), outs["ln_rstd"].ptr()
            rc = (lib.ap_mlp_fused_infer if infer else lib.ap_mlp_fused)(ctypes.byref(a), S())
        assert rc == 0, "ap_mlp_fused (%s): code %d" % (mode, rc)
        sync()
        return outs
    small = go(Ms, None)
    kk = keep0.double()
    if bwd:
        gp = (c0.double() - ops.GELU_CODE_ZERO) / ops.GELU_CODE_SCALE
        tiled(rec, "dL/dh", small["hidden_out"].view[:P], (x0.double() @ w2.double()) * gp * (kk / 0.8), TOL_BF16)
        tiled(rec, "dL/dx", small["out"].view[:P], small["hidden_out"].view[:P].double().cpu() @ w1.double(), TOL_BF16)
    else:
        fc1_in = x0.double()
        if ln:
            y_ref, mean_ref, rstd_ref = ln_reference(x0, lg, lb)
            fc1_in = y_ref.to(BF).double()
            if not infer:
                tiled(rec, "ln_out", small["ln_out"].view[:P], y_ref, TOL_BF16)
                vec_rel(rec, "ln_mean", small["ln_mean"].view[:P, 0], mean_ref, 1e-4)
                vec_rel(rec, "ln_rstd", small["ln_rstd"].view[:P, 0], rstd_ref, 1e-4)
                fc1_in = small["ln_out"].view[:P].double().cpu()
        hid_ref, dref = gelu_refs(fc1_in @ w1.double().t() + b1.double())
        hid = (hid_ref * kk).to(BF).double()
        if not infer:
            tiled(rec, "hidden_out", small["hidden_out"].view[:P], hid_ref * kk, TOL_BF16)
            codes_check(rec, small["codes"].view[:P], dref)
            hid = small["hidden_out"].view[:P].double().cpu()
        tiled(rec, "out", small["out"].view[:P], (hid @ w2.double().t() + b2.double()) * (kk / 0.8) + (x0 if ln else res0).double(), TOL_BF16)
    big = go(M, rec)
    for name in big:
        verify(rec, name, big[name], small[name], P, sentinel_ok=name == "codes")


# ======================================================================================================================== B. convolutions
def conv_entry(lib, C, what):
    return getattr(lib, "ap_conv3x3_c%d%s" % (C, what))


@pytest.mark.parametrize("op", ["forward", "input-gradient", "weight-gradient"])
@pytest.mark.parametrize("C", [64, 128])
def test_conv3x3(lib, rec, C, op):
    """the stem's 3 x 3 convolutions on 33 x 33 maps (odd: ragged tiles on both axes), 64 and 128 channels, maps past 2^32 bytes.  Forward and
    input gradient (the same kernel on the flipped, transposed weights) are per image; the weight gradient is reduced over all images in a
    fixed order and held against the exact fp64 value, an fp32 emulation (one matmul per tap, 60 images = 65 340 rows at a time) beside it"""
    Pi, H, W = P_IMAGES, 33, 33
    img = H * W * C
    B = images_past(img, BF)
    x0, dy0 = rnd(Pi, H, W, C, seed=101), rnd(Pi, H, W, C, scale=0.05, seed=102)
    w = frand(C, C, 3, 3, seed=103, scale=0.05)
    w16 = w.to(BF).double()
    wd = dev(w)
    wf, wb = torch.empty(9 * C * C, dtype=BF, device="cuda"), torch.empty(9 * C * C, dtype=BF, device="cuda")
    assert conv_entry(lib, C, "_pack")(wd.data_ptr(), wf.data_ptr(), wb.data_ptr(), S()) == 0
    if op != "weight-gradient":
        src0, wp = (x0, wf) if op == "forward" else (dy0, wb)

        def go(images, r):
            x = pin(r, "x" if op == "forward" else "dy", src0.reshape(Pi, img), images)
            y = pout(r, "y" if op == "forward" else "dx", images, img)
            rc = conv_entry(lib, C, "")(x.data_ptr(), wp.data_ptr(), y.ptr(), images, H, W, None, S())
            assert rc == 0, "ap_conv3x3_c%d: code %d" % (C, rc)
            sync()
            return y
        small = go(Pi, None)
        nchw = src0.double().permute(0, 3, 1, 2)
        ref = F.conv2d(nchw, w16, None, 1, 1) if op == "forward" else F.conv_transpose2d(nchw, w16, None, 1, 1)
        tiled(rec, "output", small.view.reshape(-1, C), ref.permute(0, 2, 3, 1).reshape(-1, C), TOL_BF16)
        big = go(B, rec)
        verify(rec, "output", big, small, Pi)
        return
    x, dy = pin(rec, "x", x0.reshape(Pi, img), B), pin(rec, "dy", dy0.reshape(Pi, img), B)
    dw = pout(rec, "dw", C, C * 9, dtype=F32)
    dw.view.zero_()
    ws_bytes = conv_entry(lib, C, "_wgrad_workspace")(B, H, W)
    ws = BA.BigOut(1, ws_bytes // 4, dtype=F32, device="cuda", pre=1, post=1, what="workspace")
    rc = conv_entry(lib, C, "_wgrad")(x.data_ptr(), dy.data_ptr(), dw.ptr(), B, H, W, ws.ptr(), ws_bytes, S())
    assert rc == 0, "ap_conv3x3_c%d_wgrad: code %d" % (C, rc)
    sync()
    dw.check_guards()
    ws.check_guards()
    terms = torch.stack([torch.nn.grad.conv2d_weight(x0[i:i + 1].double().permute(0, 3, 1, 2), (C, C, 3, 3), dy0[i:i + 1].double().permute(0, 3, 1, 2), stride=1, padding=1)
                         for i in range(Pi)]).reshape(Pi, C, C * 9)
    emu = torch.zeros(C, C, 3, 3, dtype=F32, device="cuda")
    for s in range(0, B, 60):
        xp = F.pad(x[s:s + 60].reshape(-1, H, W, C).float(), (0, 0, 1, 1, 1, 1))
        g = dy[s:s + 60].reshape(-1, C).float()
        for ky in range(3):
            for kx in range(3):
                emu[:, :, ky, kx] += g.t() @ xp[:, ky:ky + H, kx:kx + W].reshape(-1, C)
    reduction(rec, "dw", dw.view, emu.reshape(C, C * 9), BA.periodic_sum(terms, B))


def test_conv7_s2d_forward(lib, rec):
    """ap_conv7_s2d (7 x 7 / stride 2 / pad 3, 3 -> 64 channels on the space-to-depth image): 33 x 33 output maps past 2^32 bytes"""
    Pi, R = P_IMAGES, 33
    B = images_past(R * R * 64, BF)
    g = torch.Generator().manual_seed(104)
    image = torch.randn(Pi, 3, 2 * R, 2 * R, generator=g).to(BF)
    xs0 = torch.zeros(Pi, R, R, 16, dtype=BF)
    xs0[..., :12] = image.reshape(Pi, 3, R, 2, R, 2).permute(0, 2, 4, 3, 5, 1).reshape(Pi, R, R, 12)      # channel = ((oy & 1) * 2 + (ox & 1)) * 3 + c
    w = frand(64, 3, 7, 7, seed=105, scale=0.1)
    wd, wp = dev(w), torch.empty(16 * 64 * 16, dtype=BF, device="cuda")
    assert lib.ap_conv7_pack(wd.data_ptr(), wp.data_ptr(), S()) == 0

    def go(images, r):
        xs = pin(r, "xs", xs0.reshape(Pi, -1), images)
        y = pout(r, "y", images, R * R * 64)
        rc = lib.ap_conv7_s2d(xs.data_ptr(), wp.data_ptr(), y.ptr(), images, R, R, None, S())
        assert rc == 0, "ap_conv7_s2d: code %d" % rc
        sync()
        return y
    small = go(Pi, None)
    ref = F.conv2d(image.double(), w.to(BF).double(), None, 2, 3).permute(0, 2, 3, 1)
    tiled(rec, "y", small.view.reshape(-1, 64), ref.reshape(-1, 64), TOL_BF16)
    big = go(B, rec)
    verify(rec, "y", big, small, Pi)


# ======================================================================================================================== B. fp8 weight gradients
@pytest.mark.parametrize("mode", ["atomics", "workspace"])
def test_gemm_tn8_acc_grouped(lib, rec, mode):
    """ap_gemm_tn8_acc_grouped, A [M, 1152] e5m2 bytes past 2^32 (and 2^31 elements), B [M, 384] e4m3 bytes; the workspace form twice,
    bit-identical"""
    from autoprog_amd._lib import Tn8Problem
    N1, N2, P = 1152, 384, P_ROWS
    M = BA.rows_past(N1, U8, 32, tile=64)
    g = torch.Generator().manual_seed(106)
    a8 = (torch.randn(P, N1, generator=g) * 0.05 * 256).to(torch.float8_e5m2)
    b8 = torch.randn(P, N2, generator=g).to(torch.float8_e4m3fn)
    dq = dev(torch.tensor([1.0 / 256, 1.0], dtype=F32))
    a, b = pin(rec, "A", a8.view(U8), M), pin(rec, "B", b8.view(U8), M)
    want = BA.periodic_matmul_tn(a8.float().double() / 256, b8.float().double(), M)
    emu = torch.zeros(N1, N2, dtype=F32, device="cuda")
    for s in range(0, M, 65536):
        emu += (a[s:s + 65536].view(torch.float8_e5m2).float() / 256).t() @ b[s:s + 65536].view(torch.float8_e4m3fn).float()
    runs = []
    for _ in range(2 if mode == "workspace" else 1):
        dw = pout(rec, "dW", N1, N2, dtype=F32)
        dw.view.zero_()
        prob = Tn8Problem(A=a.data_ptr(), lda=N1, B=b.data_ptr(), ldb=N2, C=dw.ptr(), ldc=N2, M=M, N1=N1, N2=N2, a_fmt=1, alpha=1.0,
                          dq_a=dq.data_ptr(), dq_b=dq.data_ptr() + 4)
        ws, ws_bytes = None, 0
        if mode == "workspace":
            ws_bytes = lib.ap_gemm_tn8_grouped_workspace(ctypes.addressof(prob), 1)
            assert ws_bytes > 0
            ws = BA.BigOut(1, ws_bytes // 4, dtype=F32, device="cuda", pre=1, post=1, what="workspace")
        rc = lib.ap_gemm_tn8_acc_grouped(ctypes.addressof(prob), 1, ws.ptr() if ws is not None else None, ws_bytes, S())
        assert rc == 0, "ap_gemm_tn8_acc_grouped: code %d" % rc
        sync()
        dw.check_guards()
        if ws is not None:
            ws.check_guards()
        runs.append(dw)
    reduction(rec, "dW", runs[0].view, emu, want)
    if mode == "workspace":
        same = torch.equal(runs[0].view, runs[1].view)
        rec.line("deterministic workspace: two runs bit-identical: %s" % ("yes" if same else "NO"))
        assert same
