"""The later work items of the persistent and grid-capped kernels.

A launch of these kernels starts at most N workgroups and each walks the items t, t + gridDim.x, ...; on a later item it runs code the first
never reaches: the operands prefetched during the previous item, the previous tile's output stored under the PREVIOUS tile's edge masks
(csrc/conv.hip: out_prev, nrow_prev, col_ok_prev), the weight-slab ring that runs across tiles (csrc/conv128.hip), the statistics row
added up over all of a workgroup's tiles.  The other kernel tests stay below one item per workgroup for this family; here every case

  * asserts FIRST, on the grid the library itself reports (or, where it reports none, on the largest cap in the launch code), that every
    workgroup runs at least two items, some run three, and the items are no multiple of the grid (tests/_multi_item.py::trips) -- with
    images that hold a full and a ragged tile in each direction, so that a workgroup's consecutive items differ in their edge masks and lie
    in different images.  That last part is asserted too: the items of an image must not divide the grid (tests/_multi_item.py::masks_change),
    or a workgroup would sit at one place of every image it visits and see one set of masks;
  * holds every 16 x 8 tile of the output to twice the tolerance the kernel tests use for the same output (tests/_tilecheck.py), against
    plain torch in fp64;
  * launches the SAME kernel on contiguous sub-batches small enough for one item per workgroup -- the first images, images whose tiles are
    second items of the big launch, the last images -- and wants the big launch's slice bit for bit (torch.equal): the other tests hold the
    single-item path to the reference, so any difference is the later-item path;
  * checks the reductions (statistics rows, weight gradients onto a non-zero base and bit-equal on a second run, dgamma / dbeta);
  * keeps every output inside sentinel rows and every input between NaN rows, and wants every element finite.

Each checked output prints one `MULTI` line; profiles/multi_item.txt is that output.
"""
import ctypes
import struct

import pytest
import torch

from oracle import ref_cpu as R
from tests import _multi_item as MI
from tests._tilecheck import SENTINEL, assert_tiled, guarded, nan_padded, rel, round_up

pytestmark = pytest.mark.gpu
TOL_BF16 = 1e-2
TOL_F32 = 3e-3
TOL_CONV = 5e-3          # tests/test_gpu_kernels.py: outputs and input gradients of the convolutions
TOL_SUMS = 1e-5          # ... their statistics rows and fp32 weight gradients
TOL_BN_STATS = 1e-4      # ... mean / rstd / running_* of the BatchNorm
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from autoprog_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib(ops):
    from autoprog_amd._lib import lib as _lib
    return _lib


@pytest.fixture
def case(request):
    return request.node.name


def P(t):
    return t.data_ptr() if t is not None else None


def stream():
    return torch.cuda.current_stream().cuda_stream


def din(t):
    """an input on the device between NaN guard rows, as [rows, C]"""
    return nan_padded(t.reshape(-1, t.shape[-1]), t.shape[-1], device="cuda")


def gbuf(rows, cols, dtype=BF16, what=""):
    return guarded(rows, cols, cols, dtype, device="cuda", what=what)


def gflat(n, what=""):
    view, g = guarded(1, n, round_up(n, 64) + 64, torch.float32, pre=1, post=1, device="cuda", what=what)
    return view[0, :n], g


def dvec(t):
    """an fp32 input vector on the device with a row of NaNs directly in front of it and one behind it"""
    return nan_padded(t.reshape(1, -1).float(), t.numel(), pre=1, post=1, device="cuda")[0]


def need_masks(classes, grid, what):
    ok, share = MI.masks_change(classes, grid)
    assert ok, "%s: %d items per image on %d workgroups: a workgroup's next item has other edge masks at only %.0f %% of the places" % (what, len(classes), grid, 100 * share)


def gacc(base, what=""):
    """a guarded fp32 accumulator that starts from `base` (the contract of the weight gradients and dgamma / dbeta is +=)"""
    b2 = base.reshape(base.shape[0], -1)
    view, g = gbuf(b2.shape[0], b2.shape[1], torch.float32, what)
    view.copy_(b2)
    g.before = g.whole.detach().cpu().view(g.before.dtype).clone()          # the base was written through the view
    return view, g


class FlatGuard:
    """a long vector between two bands of 1024 sentinel elements (a Guard would copy the whole allocation to the host twice)"""
    PAD = 1024

    def __init__(self, n, dtype, what):
        self.n, self.what = n, what
        self.bits = {torch.float32: torch.int32, BF16: torch.int16, torch.uint8: torch.uint8}[dtype]
        self.whole = torch.empty(n + 2 * self.PAD, dtype=dtype, device="cuda")
        pat = SENTINEL[dtype]
        top = {torch.int32: 1 << 31, torch.int16: 1 << 15, torch.uint8: 1 << 8}[self.bits]
        self.pat = pat if (pat < top or self.bits is torch.uint8) else pat - 2 * top
        self.whole.view(self.bits).fill_(self.pat)
        self.view = self.whole[self.PAD:self.PAD + n]

    def check(self):
        raw = self.whole.view(self.bits)
        assert bool((raw[:self.PAD] == self.pat).all()) and bool((raw[self.PAD + self.n:] == self.pat).all()), "%s: the sentinels around the vector changed" % self.what


def finite(*ts):
    for t in ts:
        assert bool(torch.isfinite(t.float()).all())


def need(t, what):
    assert t.ok, "%s: %d items on %d workgroups are %d .. %d trips: the case does not reach a second and a third item everywhere it should" % (
        what, t.items, t.grid, t.fewest, t.most)
    return t


def report(case, what, t, rep=None, equal=None, extra=""):
    print("MULTI %s | %s | items %d grid %d trips %d..%d | %s | sub-batches %s%s" % (
        case, what, t.items, t.grid, t.fewest, t.most,
        "whole %.3e worst tile %.3e at (%d, %d)" % (rep.whole, rep.worst, rep[2], rep[3]) if rep is not None else "reduction",
        {None: "n/a", True: "equal", False: "DIFFER"}[equal], extra and " | " + extra))


def sub_batches(B, n, second):
    """(first images, images whose items are second items of the big launch, last images)"""
    assert second + n <= B
    return [(0, n), (second, min(second + n, B)), (B - n, B)]


def bn_input(mean, rstd, gamma, beta):
    from autoprog_amd._lib import BnInput
    b = BnInput()
    b.mean, b.rstd, b.gamma, b.beta = mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr()
    return b


def stats_sums(st, C):
    return st.reshape(-1, 2, C).double().sum(0).cpu()


# ================================================================================= the 64-channel 3 x 3 family and the BatchNorm
class C64:
    """ONE set of tensors for ap_conv3x3_c64 (plain, stats, _bn), _bwd_stats, _wgrad(_bn) and the ap_bn_relu_* launches"""
    _it = None

    @classmethod
    def get(cls, ops):
        if cls._it is None:
            cls._it = cls(ops)
        return cls._it

    def __init__(self, ops):
        B, H, W = self.shape = MI.C64_SHAPE
        self.T = B * H * W
        self.x, self.dy = MI.rnd(B, H, W, 64, scale=1.5, shift=0.3, seed=1), MI.rnd(B, H, W, 64, seed=2)
        self.w = MI.frand(64, 64, 3, 3, seed=3, scale=0.05)
        self.w16 = self.w.to(BF16).double()
        self.gamma = MI.frand(64, seed=4, scale=0.3, shift=1.0)
        self.beta, margin = MI.bn_beta_between_inputs(self.x.reshape(-1, 64), self.gamma, MI.frand(64, seed=5, scale=0.3))
        assert margin > 1e-5
        x2 = self.x.reshape(-1, 64).double()
        self.mean, self.rstd = x2.mean(0).float(), (x2.var(0, unbiased=False) + 1e-5).rsqrt().float()
        self.xd, self.dyd = din(self.x), din(self.dy)
        self.wf, self.wb = ops.conv3x3_pack(self.w.cuda())
        self.bn_dev = [dvec(t) for t in (self.mean, self.rstd, self.gamma, self.beta)]
        self.bn = bn_input(*self.bn_dev)
        self._act = None

    @property
    def act(self):
        """relu(bn(x)) in fp64 from the fp32 statistics the kernels are given, rounded to bf16 like the operand the kernels stage"""
        if self._act is None:
            sc = self.rstd.double() * self.gamma.double()
            self._act = torch.relu((self.x.double() - self.mean.double()) * sc + self.beta.double()).to(BF16)
        return self._act


def conv64_launch(lib, c, x, wp, B, stats_rows=0, bn=None, guard=True, what="y"):
    _, H, W = c.shape
    rows = B * H * W
    if guard:
        y, gy = gbuf(rows, 64, what=what)
        st, gs = gbuf(stats_rows, 128, torch.float32, what + " statistics") if stats_rows else (None, None)
    else:
        y, gy, gs = torch.empty(rows, 64, dtype=BF16, device="cuda"), None, None
        st = torch.empty(stats_rows, 128, device="cuda") if stats_rows else None
    rc = lib.ap_conv3x3_c64_bn(P(x), ctypes.byref(bn) if bn is not None else None, P(wp), P(y), B, H, W, P(st), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for g in (gy, gs):
        if g is not None:
            g.check(pad="untouched")
    return y, st


def test_conv3x3_c64_forward_second_and_third_tiles(ops, lib, case):
    c = C64.get(ops)
    B, H, W = c.shape
    HW = H * W
    grid = lib.ap_conv3x3_c64_stat_rows(B, H, W)
    t = need(MI.trips(MI.tiles(B, H, W, 32, 16), grid), "ap_conv3x3_c64")
    assert MI.full_and_ragged(H, 32) and MI.full_and_ragged(W, 16)
    need_masks(MI.tile_classes(MI.cdiv(H, 32), MI.cdiv(W, 16)), grid, "ap_conv3x3_c64")
    n = grid // MI.tiles(1, H, W, 32, 16)                                     # images of a launch with one tile per workgroup
    subs = sub_batches(B, n, n + 1)
    for bn, xin, tag in ((None, c.x, "plain"), (c.bn, c.act, "bn_in")):
        ref = MI.conv3x3(xin.double(), c.w16).reshape(-1, 64)
        y, st = conv64_launch(lib, c, c.xd, c.wf, B, grid, bn, what="y " + tag)
        y0, _ = conv64_launch(lib, c, c.xd, c.wf, B, 0, bn, what="y without statistics " + tag)
        assert torch.equal(y, y0)
        finite(y, st)
        rep = assert_tiled(y, ref, TOL_CONV, "%s %s" % (case, tag))
        sums, yd = stats_sums(st, 64), y.double().cpu()
        e0, e1 = rel(sums[0], yd.sum(0)), rel(sums[1], yd.pow(2).sum(0))
        equal = True
        for b0, b1 in subs:
            assert MI.tiles(b1 - b0, H, W, 32, 16) <= grid
            ys, _ = conv64_launch(lib, c, c.xd[b0 * HW:], c.wf, b1 - b0, 0, bn, guard=False)
            equal &= torch.equal(ys, y[b0 * HW:b1 * HW])
        report(case, "ap_conv3x3_c64 " + tag, t, rep, equal, "statistics rows %.1e %.1e" % (e0, e1))
        assert e0 < TOL_SUMS and e1 < TOL_SUMS, (e0, e1)
        assert equal, "%s: a sub-batch launch with one tile per workgroup differs from the big launch" % tag


def test_conv3x3_c64_input_gradient_with_statistics_second_and_third_tiles(ops, lib, case):
    c = C64.get(ops)
    B, H, W = c.shape
    HW = H * W
    grid = lib.ap_conv3x3_c64_stat_rows(B, H, W)
    t = need(MI.trips(MI.tiles(B, H, W, 32, 16), grid), "ap_conv3x3_c64_bwd_stats")
    need_masks(MI.tile_classes(MI.cdiv(H, 32), MI.cdiv(W, 16)), grid, "ap_conv3x3_c64_bwd_stats")

    def launch(b0, b1, guard):
        rows = (b1 - b0) * HW
        if guard:
            da, g0 = gbuf(rows, 64, what="da")
            st, g1 = gbuf(grid, 128, torch.float32, "partial sums")
        else:
            da, st, g0, g1 = torch.empty(rows, 64, dtype=BF16, device="cuda"), torch.empty(grid, 128, device="cuda"), None, None
        rc = lib.ap_conv3x3_c64_bwd_stats(P(c.dyd[b0 * HW:]), P(c.wb), P(da), b1 - b0, H, W, P(c.xd[b0 * HW:]), ctypes.byref(c.bn), P(st), stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        for g in (g0, g1):
            if g is not None:
                g.check(pad="untouched")
        return da, st
    da, st = launch(0, B, True)
    finite(da, st)
    plain, _ = conv64_launch(lib, c, c.dyd, c.wb, B, 0, None, what="plain input gradient")
    assert torch.equal(da, plain)                                             # the epilogue does not change the map
    rep = assert_tiled(da, MI.conv3x3_dgrad(c.dy.double(), c.w16).reshape(-1, 64), TOL_CONV, case)
    x2 = c.x.reshape(-1, 64)
    xh = (x2.double() - c.mean.double()) * c.rstd.double()
    m = ((x2.float() - c.mean) * c.rstd * c.gamma + c.beta > 0).double()      # the kernels' mask; bn_beta_between_inputs: any arithmetic agrees
    assert torch.equal(m, (xh * c.gamma.double() + c.beta.double() > 0).double())
    dzm = da.double().cpu() * m
    sums = stats_sums(st, 64)
    e0, e1 = rel(sums[0], dzm.sum(0)), rel(sums[1], (dzm * xh).sum(0))
    n = grid // MI.tiles(1, H, W, 32, 16)
    equal = True
    for b0, b1 in sub_batches(B, n, n + 1):
        equal &= torch.equal(launch(b0, b1, False)[0], da[b0 * HW:b1 * HW])
    report(case, "ap_conv3x3_c64_bwd_stats", t, rep, equal, "partial sums %.1e %.1e" % (e0, e1))
    assert e0 < TOL_SUMS and e1 < TOL_SUMS, (e0, e1)
    assert equal


def test_conv3x3_c64_weight_gradient_many_tiles_per_workgroup(ops, lib, case):
    """no query for the grid: csrc/conv.hip, ap_conv3x3_c64_wgrad_bn -- the prefetching kernel (the default, and the only one with the
    BatchNorm input) starts at most 256 workgroups on 16 x 16 tiles, k_conv3x3_c64_wgrad (AP_CONV_WGRAD_P=0) at most cw_grid = 512, which is
    what the workspace query sizes"""
    c = C64.get(ops)
    B, H, W = c.shape
    ws_bytes = lib.ap_conv3x3_c64_wgrad_workspace(B, H, W)
    cap = ws_bytes // (9 * 64 * 64 * 4)
    items = MI.tiles(B, H, W, 16, 16)
    assert cap >= 256 and MI.full_and_ragged(H, 16) and MI.full_and_ragged(W, 16)
    t = need(MI.trips(items, 256), "k_conv3x3_c64_wgrad_p")
    need(MI.trips(items, cap), "k_conv3x3_c64_wgrad")
    for g_ in (256, cap):
        need_masks(MI.tile_classes(MI.cdiv(H, 16), MI.cdiv(W, 16)), g_, "ap_conv3x3_c64_wgrad")
    ws = torch.empty(ws_bytes // 4, device="cuda")
    base = MI.frand(64, 64, 3, 3, seed=9)
    for bn, xin, tag in ((None, c.x, "plain"), (c.bn, c.act, "bn_in")):
        ref = base.double() + MI.conv3x3_wgrad(xin.double(), c.dy.double())
        runs = []
        for _ in range(2):
            dw, g = gacc(base, "dw " + tag)
            ws.fill_(float("nan"))
            rc = lib.ap_conv3x3_c64_wgrad_bn(P(c.xd), ctypes.byref(bn) if bn is not None else None, P(c.dyd), P(dw), B, H, W, P(ws), ws_bytes, stream())
            assert rc == 0, rc
            torch.cuda.synchronize()
            g.check(pad="untouched")
            runs.append(dw)
        finite(runs[0])
        e = rel(runs[0].reshape(64, 64, 3, 3), ref)
        report(case, "ap_conv3x3_c64_wgrad " + tag, t, extra="rel to fp64 %.2e, second run %s" % (e, "bit-equal" if torch.equal(*runs) else "DIFFERS"))
        assert e < TOL_SUMS, e
        assert torch.equal(*runs)


def test_bn_relu_more_than_two_sweeps(ops, lib, case):
    """ap_bn_relu_fwd (own statistics; eval-mode apply), _fwd_partials (with and without the apply pass), _bwd and _bwd_partials at
    T = 135036 rows of 64 channels: more than two sweeps of 2048 blocks x 32 rows.  The BatchNorm normalises the convolution's own output
    (its statistics rows are the `partials`); the backward-with-partials pair runs on the layer below, as in the stem."""
    c = C64.get(ops)
    B, H, W = c.shape
    T, C, HW = c.T, 64, H * W
    ws_bytes = lib.ap_bn_relu_workspace(T, C)
    grid = ws_bytes // (2 * C * 4) - 1          # the workspace holds one partial row of 2 C floats per block and one more row, the finalized sums (bn_grid: 2048)
    t = need(MI.trips(MI.cdiv(T, 256 // (C // 8)), grid), "ap_bn_relu_*")
    assert T > 2 * 65536
    ws = torch.empty(ws_bytes // 4, device="cuda")
    cgrid = lib.ap_conv3x3_c64_stat_rows(B, H, W)
    z, part = conv64_launch(lib, c, c.xd, c.wf, B, cgrid, None, guard=False)
    zh = z.cpu()
    gamma = c.gamma
    beta, margin = MI.bn_beta_between_inputs(zh, gamma, MI.frand(64, seed=6, scale=0.3))
    assert margin > 1e-5
    zd, gd, bd = din(zh), dvec(gamma), dvec(beta)
    zr = zh.double().requires_grad_(True)
    yr, mr, rr, var_u = MI.bn_relu(zr, gamma.double(), beta.double())
    yr.backward(c.dy.reshape(-1, 64).double())
    rm0, rv0, mom = MI.frand(64, seed=7, scale=0.3), torch.rand(64, generator=torch.Generator().manual_seed(8)) + 0.5, 0.1
    # ---- forward, own statistics
    y, g0 = gbuf(T, C, what="y")
    mean, g1 = gflat(C, "mean")
    rstd, g2 = gflat(C, "rstd")
    (rm, g3), (rv, g4) = gacc(rm0[None], "running_mean"), gacc(rv0[None], "running_var")
    rm, rv = rm[0], rv[0]
    assert lib.ap_bn_relu_fwd(P(zd), P(gd), P(bd), P(rm), P(rv), 1, mom, 1e-5, P(y), P(mean), P(rstd), T, C, P(ws), ws_bytes, stream()) == 0
    torch.cuda.synchronize()
    for g in (g0, g1, g2, g3, g4):
        g.check(pad="untouched")
    finite(y, mean, rstd, rm, rv)
    rep = assert_tiled(y, yr.detach(), TOL_BF16, case + " y")
    es = [rel(mean, mr.detach()), rel(rstd, rr.detach()), rel(rm, (1 - mom) * rm0.double() + mom * mr.detach()), rel(rv, (1 - mom) * rv0.double() + mom * var_u.detach())]
    # ---- the same from the convolution's statistics rows; then statistics only
    y2, g0 = gbuf(T, C, what="y from partials")
    (mean2, g1), (rstd2, g2), (mean3, g3), (rstd3, g4) = (gflat(C, nm) for nm in ("mean from partials", "rstd from partials", "mean, statistics only", "rstd, statistics only"))
    (rm2, g5), (rv2, g6) = gacc(rm0[None], "running_mean"), gacc(rv0[None], "running_var")
    rm2, rv2 = rm2[0], rv2[0]
    assert lib.ap_bn_relu_fwd_partials(P(zd), P(part), cgrid, P(gd), P(bd), P(rm2), P(rv2), mom, 1e-5, P(y2), P(mean2), P(rstd2), T, C, stream()) == 0
    assert lib.ap_bn_relu_fwd_partials(P(zd), P(part), cgrid, P(gd), P(bd), None, None, mom, 1e-5, None, P(mean3), P(rstd3), T, C, stream()) == 0
    torch.cuda.synchronize()
    for g in (g0, g1, g2, g3, g4, g5, g6):
        g.check(pad="untouched")
    assert_tiled(y2, yr.detach(), TOL_BF16, case + " y from partials")
    es += [rel(mean2, mr.detach()), rel(rstd2, rr.detach()), rel(rm2, rm), rel(rv2, rv)]
    assert torch.equal(mean2, mean3) and torch.equal(rstd2, rstd3)
    # ---- the apply pass alone (eval mode: mean / rstd as given), the big launch against one-sweep sub-batches
    ye, g0 = gbuf(T, C, what="y eval")
    assert lib.ap_bn_relu_fwd(P(zd), P(gd), P(bd), None, None, 0, mom, 1e-5, P(ye), P(mean), P(rstd), T, C, P(ws), ws_bytes, stream()) == 0
    torch.cuda.synchronize()
    g0.check(pad="untouched")
    assert torch.equal(ye, y)
    equal, n = True, 40                                                           # 43560 rows: inside one sweep of 2048 blocks x 32 rows
    assert n * HW <= 2048 * 32
    for b0, b1 in sub_batches(B, n, MI.cdiv(2048 * 32, HW)):                      # (the first image that lies wholly in the second sweep)
        ys = torch.empty((b1 - b0) * HW, C, dtype=BF16, device="cuda")
        assert lib.ap_bn_relu_fwd(P(zd[b0 * HW:]), P(gd), P(bd), None, None, 0, mom, 1e-5, P(ys), P(mean), P(rstd), (b1 - b0) * HW, C, P(ws), ws_bytes, stream()) == 0
        equal &= torch.equal(ys, ye[b0 * HW:b1 * HW])
    report(case, "ap_bn_relu_fwd", t, rep, equal, "mean rstd running: %s" % " ".join("%.1e" % e for e in es))
    assert max(es) < TOL_BN_STATS, es
    assert equal
    # ---- backward
    dg0, db0 = MI.frand(C, seed=10), MI.frand(C, seed=11)
    dx, g0 = gbuf(T, C, what="dx")
    dg, g1 = gacc(dg0[None], "dgamma")
    db, g2 = gacc(db0[None], "dbeta")
    assert lib.ap_bn_relu_bwd(P(c.dyd), P(zd), P(gd), P(bd), P(mean), P(rstd), P(dx), P(dg), P(db), T, C, P(ws), ws_bytes, stream()) == 0
    torch.cuda.synchronize()
    for g in (g0, g1, g2):
        g.check(pad="untouched")
    finite(dx, dg, db)
    rep = assert_tiled(dx, zr.grad, 1.5e-2, case + " dx")
    xh = ((zh.double() - mr.detach()) * rr.detach())
    dym = c.dy.reshape(-1, 64).double() * (yr.detach() > 0)
    eg, eb = rel(dg[0], dg0.double() + (dym * xh).sum(0)), rel(db[0], db0.double() + dym.sum(0))
    report(case, "ap_bn_relu_bwd", t, rep, None, "dgamma %.1e dbeta %.1e" % (eg, eb))
    assert eg < TOL_F32 and eb < TOL_F32, (eg, eb)
    # ---- backward whose first pass ran in the input-gradient convolution: the layer below (x, its BatchNorm), dy = that convolution's map
    da, g0 = gbuf(T, C, what="da")
    part2, g4 = gbuf(cgrid, 128, torch.float32, "partial sums")
    assert lib.ap_conv3x3_c64_bwd_stats(P(c.dyd), P(c.wb), P(da), B, H, W, P(c.xd), ctypes.byref(c.bn), P(part2), stream()) == 0
    dx2, g1 = gbuf(T, C, what="dx from partials")
    dg, g2 = gacc(dg0[None], "dgamma")
    db, g3 = gacc(db0[None], "dbeta")
    mean0, rstd0, gam0, bet0 = c.bn_dev
    assert lib.ap_bn_relu_bwd_partials(P(da), P(c.xd), P(gam0), P(bet0), P(mean0), P(rstd0), P(part2), cgrid, P(dx2), P(dg), P(db), T, C, P(ws), ws_bytes, stream()) == 0
    torch.cuda.synchronize()
    for g in (g0, g1, g2, g3, g4):
        g.check(pad="untouched")
    finite(dx2, dg, db)
    xr = c.x.reshape(-1, 64).double().requires_grad_(True)
    y0, _, _, _ = MI.bn_relu(xr, c.gamma.double(), c.beta.double())
    dah = da.double().cpu()
    y0.backward(dah)
    rep = assert_tiled(dx2, xr.grad, 1.5e-2, case + " dx from partials")
    xh0 = (xr.detach() - c.mean.double()) * c.rstd.double()
    dam = dah * (y0.detach() > 0)
    eg, eb = rel(dg[0], dg0.double() + (dam * xh0).sum(0)), rel(db[0], db0.double() + dam.sum(0))
    report(case, "ap_bn_relu_bwd_partials", t, rep, None, "dgamma %.1e dbeta %.1e" % (eg, eb))
    assert eg < TOL_F32 and eb < TOL_F32, (eg, eb)


# ===================================================================================================== 128 channels (csrc/conv128.hip)
def test_conv3x3_c128_second_and_third_tiles(ops, lib, case):
    """forward, statistics, input gradient, and the four-quadrant weight gradient (csrc/conv.hip, ap_conv3x3_c128_wgrad: the prefetching
    64-channel kernel per quadrant on at most 256 workgroups -- no query; 16 x 16 tiles like the forward)"""
    B, H, W = MI.C128_SHAPE
    HW, T, C = H * W, B * H * W, 128
    grid = lib.ap_conv3x3_c128_stat_rows(B, H, W)
    items = MI.tiles(B, H, W, 16, 16)
    t = need(MI.trips(items, grid), "ap_conv3x3_c128")
    need(MI.trips(items, 256), "ap_conv3x3_c128_wgrad")
    for g_ in (grid, 256):
        need_masks(MI.tile_classes(MI.cdiv(H, 16), MI.cdiv(W, 16)), g_, "ap_conv3x3_c128")
    assert MI.full_and_ragged(H, 16) and MI.full_and_ragged(W, 16)
    x, dy = MI.rnd(B, H, W, C, seed=1), MI.rnd(B, H, W, C, seed=2)
    w = MI.frand(C, C, 3, 3, seed=3, scale=0.04)
    w16 = w.to(BF16).double()
    wf, wb = ops.conv3x3_pack(w.cuda())
    xd, dyd = din(x), din(dy)

    def launch(src, wp, b0, b1, stats, guard, what=""):
        rows = (b1 - b0) * HW
        if guard:
            y, g0 = gbuf(rows, C, what=what)
            st, g1 = gbuf(grid, 2 * C, torch.float32, what + " statistics") if stats else (None, None)
        else:
            y, st, g0, g1 = torch.empty(rows, C, dtype=BF16, device="cuda"), None, None, None
        rc = lib.ap_conv3x3_c128(P(src[b0 * HW:]), P(wp), P(y), b1 - b0, H, W, P(st), stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        for g in (g0, g1):
            if g is not None:
                g.check(pad="untouched")
        return y, st
    n = grid // MI.tiles(1, H, W, 16, 16)
    subs = sub_batches(B, n, n + 1)
    for src, srch, wp, ref, tag in ((xd, x, wf, MI.conv3x3(x.double(), w16), "forward"), (dyd, dy, wb, MI.conv3x3_dgrad(dy.double(), w16), "input gradient")):
        y, st = launch(src, wp, 0, B, True, True, tag)
        assert torch.equal(y, launch(src, wp, 0, B, False, True, tag)[0])
        finite(y, st)
        rep = assert_tiled(y, ref.reshape(-1, C), TOL_CONV, "%s %s" % (case, tag))
        sums, yd = stats_sums(st, C), y.double().cpu()
        e0, e1 = rel(sums[0], yd.sum(0)), rel(sums[1], yd.pow(2).sum(0))
        equal = True
        for b0, b1 in subs:
            assert MI.tiles(b1 - b0, H, W, 16, 16) <= grid
            equal &= torch.equal(launch(src, wp, b0, b1, False, False)[0], y[b0 * HW:b1 * HW])
        report(case, "ap_conv3x3_c128 " + tag, t, rep, equal, "statistics rows %.1e %.1e" % (e0, e1))
        assert e0 < TOL_SUMS and e1 < TOL_SUMS, (e0, e1)
        assert equal
    ws_bytes = lib.ap_conv3x3_c128_wgrad_workspace(B, H, W)
    ws = torch.empty(ws_bytes // 4, device="cuda")
    base = MI.frand(C, C, 3, 3, seed=9)
    runs = []
    for _ in range(2):
        dw, g = gacc(base, "dw")
        ws.fill_(float("nan"))
        assert lib.ap_conv3x3_c128_wgrad(P(xd), P(dyd), P(dw), B, H, W, P(ws), ws_bytes, stream()) == 0
        torch.cuda.synchronize()
        g.check(pad="untouched")
        runs.append(dw)
    finite(runs[0])
    e = rel(runs[0].reshape(C, C, 3, 3), base.double() + MI.conv3x3_wgrad(x.double(), dy.double()))
    report(case, "ap_conv3x3_c128_wgrad", MI.trips(items, 256), extra="rel to fp64 %.2e, second run %s" % (e, "bit-equal" if torch.equal(*runs) else "DIFFERS"))
    assert e < TOL_SUMS, e
    assert torch.equal(*runs)


# ============================================================================================================= csrc/conv7.hip
@pytest.mark.parametrize("Co", [64, 128], ids=["64-channels", "128-channels-ld-entry-points"])
def test_conv7_s2d_second_and_third_tiles(ops, lib, case, Co):
    """the first stem convolution on a 66 x 66 image (output map 33 x 33): forward and statistics on 32 x 16 tiles, the weight gradient on
    16 x 16 tiles (its grid: the workspace query, one slab of 16 * 64 * 16 floats per workgroup).  128 output channels: the 64-channel
    kernels once per half through ap_conv7_s2d_ld / ap_conv7_s2d_wgrad_ld with a pixel stride of 128, as ops.conv7_s2d does."""
    B, H, W = MI.CONV7_SHAPE
    HW, T = H * W, B * H * W
    grid = lib.ap_conv7_s2d_stat_rows(B, H, W)
    t = need(MI.trips(MI.tiles(B, H, W, 32, 16), grid), "ap_conv7_s2d")
    ws_bytes = lib.ap_conv7_s2d_wgrad_workspace(B, H, W)
    tw = need(MI.trips(MI.tiles(B, H, W, 16, 16), ws_bytes // (16 * 64 * 16 * 4)), "ap_conv7_s2d_wgrad")
    assert MI.full_and_ragged(H, 32) and MI.full_and_ragged(W, 16) and MI.full_and_ragged(H, 16)
    need_masks(MI.tile_classes(MI.cdiv(H, 32), MI.cdiv(W, 16)), t.grid, "ap_conv7_s2d")
    need_masks(MI.tile_classes(MI.cdiv(H, 16), MI.cdiv(W, 16)), tw.grid, "ap_conv7_s2d_wgrad")
    xs = torch.cat([MI.rnd(B, H, W, 12, seed=1), torch.zeros(B, H, W, 4, dtype=BF16)], -1)
    w = MI.frand(Co, 3, 7, 7, seed=2, scale=0.1)
    dz = MI.rnd(B, H, W, Co, seed=3)
    wp = ops.conv7_pack(w.cuda())
    xd, dzd = din(xs), din(dz)
    halves = Co // 64

    def launch(b0, b1, stats, guard):
        rows = (b1 - b0) * HW
        if guard:
            y, g0 = gbuf(rows, Co, what="y")
        else:
            y, g0 = torch.empty(rows, Co, dtype=BF16, device="cuda"), None
        sts, gs = [], [g0]
        for h in range(halves):
            st, g1 = gbuf(grid, 128, torch.float32, "statistics") if stats else (None, None)
            rc = lib.ap_conv7_s2d_ld(P(xd[b0 * HW:]), wp.data_ptr() + h * 16 * 64 * 16 * 2, y.data_ptr() + h * 64 * 2, Co, b1 - b0, H, W, P(st), stream())
            assert rc == 0, rc
            sts.append(st)
            gs.append(g1)
        torch.cuda.synchronize()
        for g in gs:
            if g is not None:
                g.check(pad="untouched")
        return y, sts
    y, sts = launch(0, B, True, True)
    assert torch.equal(y, launch(0, B, False, True)[0])
    finite(y, *sts)
    if Co == 64:                                 # the entry point without the stride is the same launch
        y1, g1 = gbuf(T, Co, what="y of ap_conv7_s2d")
        assert lib.ap_conv7_s2d(P(xd), P(wp), P(y1), B, H, W, None, stream()) == 0
        torch.cuda.synchronize()
        g1.check(pad="untouched")
        assert torch.equal(y, y1)
    rep = assert_tiled(y, MI.conv7(xs.double(), w.to(BF16).double()).reshape(-1, Co), TOL_CONV, case)
    yd = y.double().cpu()
    es = []
    for h in range(halves):
        sums = stats_sums(sts[h], 64)
        es += [rel(sums[0], yd[:, 64 * h:64 * h + 64].sum(0)), rel(sums[1], yd[:, 64 * h:64 * h + 64].pow(2).sum(0))]
    n = grid // MI.tiles(1, H, W, 32, 16)
    equal = True
    for b0, b1 in sub_batches(B, n, n + 1):
        assert MI.tiles(b1 - b0, H, W, 32, 16) <= grid
        equal &= torch.equal(launch(b0, b1, False, False)[0], y[b0 * HW:b1 * HW])
    report(case, "ap_conv7_s2d_ld" if Co == 128 else "ap_conv7_s2d", t, rep, equal, "statistics rows %s" % " ".join("%.1e" % e for e in es))
    assert max(es) < TOL_SUMS, es
    assert equal
    ws = torch.empty(ws_bytes // 4, device="cuda")
    base = MI.frand(Co, 3, 7, 7, seed=9)
    runs = []
    for _ in range(2):
        dw, g = gacc(base, "dw")
        ws.fill_(float("nan"))
        for h in range(halves):
            rc = lib.ap_conv7_s2d_wgrad_ld(P(xd), dzd.data_ptr() + h * 64 * 2, Co, dw.data_ptr() + h * 64 * 147 * 4, B, H, W, P(ws), ws_bytes, stream())
            assert rc == 0, rc
        torch.cuda.synchronize()
        g.check(pad="untouched")
        runs.append(dw)
    finite(runs[0])
    e = rel(runs[0].reshape(Co, 3, 7, 7), base.double() + MI.conv7_wgrad(xs.double(), dz.double()))
    report(case, "ap_conv7_s2d_wgrad" + ("_ld" if Co == 128 else ""), tw, extra="rel to fp64 %.2e, second run %s" % (e, "bit-equal" if torch.equal(*runs) else "DIFFERS"))
    assert e < TOL_SUMS, e
    assert torch.equal(*runs)


# ============================================================================================================ csrc/outlook.hip
def test_outlook_persistent_second_and_third_items(ops, lib, case):
    """k_outlook_p through ap_outlook_fwd / ap_outlook_bwd.  No query for the grid: csrc/outlook.hip, olk_launch -- min(items, ncu * per_cu)
    rounded down to a multiple of 8, per_cu = min(160 KiB / lds, 2048 / T) with T = 512 or 256 threads, so at most 8 per CU; an item is
    (image, strip of <= 3 window rows, head) (olk_pick).  At 7 x 7 the LDS image of an item is 15.2 KiB (forward) / 23.3 KiB (backward) by
    olk_pick's formula, so the default 512-thread instantiation runs 4 workgroups per CU: the trips are asserted for that grid, ncu * 4, and
    for the largest any instantiation can use, ncu * 8; the MULTI lines print both.  (The library does not report which kernel it
    launched; the one-item-per-workgroup kernels would pass this case as well.)  3 heads: the 6 items of an image do not divide a grid
    of ncu * 4 or ncu * 8 workgroups, so a workgroup alternates between full and ragged strips and between heads."""
    B, H, W, heads = MI.OUTLOOK_SHAPE
    C, hd, h, w = heads * 32, 32, (H + 1) // 2, (W + 1) // 2
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    strips = MI.cdiv(h, 3)
    items = B * strips * heads
    assert strips >= 2 and h % 3 != 0                                            # a full strip and a ragged one
    t = need(MI.trips(items, ncu * 4), "k_outlook_p at 4 workgroups per CU")
    t8 = need(MI.trips(items, ncu * 8), "k_outlook_p at 8 workgroups per CU")
    for g_ in (t.grid, t8.grid):
        assert g_ % 8 == 0
        need_masks(MI.strip_classes(strips, heads), g_, "k_outlook_p")
    nl, ldl, scale = heads * 81, round_up(heads * 81, 8), hd ** -0.5
    v, dy = MI.rnd(B, H, W, C, seed=1), MI.rnd(B, H, W, C, seed=3)
    lg = MI.rnd(B * h * w, nl, scale=2.0, seed=2)
    vr = v.double().requires_grad_(True)
    lr = lg.double().reshape(B, h, w, nl).requires_grad_(True)
    yr = R.outlook_core(vr, lr, heads)
    yr.backward(dy.double())
    vd, dyd, lgd = din(v), din(dy), nan_padded(lg, ldl, device="cuda")
    HW, hw = H * W, h * w

    def launch(b0, b1, guard):
        n = b1 - b0
        mk = (lambda rows, cols, what: gbuf(rows, cols, what=what)) if guard else (lambda rows, cols, what: (torch.empty(rows, cols, dtype=BF16, device="cuda"), None))
        (y, g0), (dv, g1), (dl, g2) = mk(n * HW, C, "y"), mk(n * HW, C, "dv"), mk(n * hw, ldl, "dlogits")
        st = stream()
        assert lib.ap_outlook_fwd(P(vd[b0 * HW:]), P(lgd[b0 * hw:]), ldl, P(y), n, H, W, heads, hd, scale, st) == 0
        assert lib.ap_outlook_bwd(P(vd[b0 * HW:]), P(lgd[b0 * hw:]), ldl, P(dyd[b0 * HW:]), P(dv), P(dl), n, H, W, heads, hd, scale, st) == 0
        torch.cuda.synchronize()
        for g in (g0, g1, g2):
            if g is not None:
                g.check(pad="untouched")
        return y, dv, dl
    y, dv, dl = launch(0, B, True)
    finite(y, dv, dl)
    reps = [assert_tiled(y, yr.detach().reshape(-1, C), TOL_BF16, case + " y"), assert_tiled(dv, vr.grad.reshape(-1, C), TOL_BF16, case + " dv"),
            assert_tiled(dl[:, :nl], lr.grad.reshape(-1, nl), TOL_BF16, case + " dlogits")]
    assert bool((dl[:, nl:].view(torch.int16) == 0).all())                       # the padding columns of dlogits are zeroed (include/autoprog_hip.h)
    ipi = strips * heads
    n = max(k for k in range(1, ncu // ipi + 1) if k * ipi % 8 == 0)             # <= ncu items and a multiple of 8 (olk_launch rounds the grid down to one): one per workgroup
    equal = [True, True, True]
    for b0, b1 in sub_batches(B, n, 2 * ncu) + [(B // 2, B // 2 + n)]:           # (image 2 * ncu: a second item even at 8 workgroups per CU)
        sub = launch(b0, b1, False)
        for i, (big, rows) in enumerate(((y, HW), (dv, HW), (dl, hw))):
            equal[i] &= torch.equal(sub[i], big[b0 * rows:b1 * rows])
    for nm, rep, eq in zip(("y", "dv", "dlogits"), reps, equal):
        report(case, "k_outlook_p " + nm, t, rep, eq, "grid: the default instantiation's ncu x 4, not reported by the library; at the largest cap %d: trips %d..%d" % (t8.grid, t8.fewest, t8.most))
    assert all(equal), equal


# ======================================================================================================== csrc/layernorm.hip
@pytest.mark.parametrize("C", [384, 768], ids=["C384-768-workgroups", "C768-512-workgroups"])
def test_layernorm_backward_three_trips(ops, lib, case, C):
    """k_ln_bwd_pf through ap_layernorm_bwd (plain), ap_layernorm_bwd_partial (defer=) and, at C <= 512, ap_layernorm_bwd_partial_pool
    (pool=).  The grid is the n_partial a launch returns; a first launch on as many rows as the workspace has partial rows for reads the
    cap, the case's row count follows from it and from the kernel's rows per trip (tests/_multi_item.py::ln_bwd_geometry, ln_rows)."""
    from autoprog_amd.ops import LnRider
    H, W = MI.LN_TOKENS
    gpb, U = MI.ln_bwd_geometry(C)
    ws_bytes = lib.ap_layernorm_bwd_workspace(1, C)
    st = stream()

    def partial_launch(dy, x, gamma, mean, rstd, dres, dx, rows, ws, pool=None):
        n = ctypes.c_int(0)
        if pool is None:
            rc = lib.ap_layernorm_bwd_partial(P(dy), P(x), P(gamma), P(mean), P(rstd), P(dres), P(dx), rows, C, P(ws), ws_bytes, ctypes.byref(n), st)
        else:
            rc = lib.ap_layernorm_bwd_partial_pool(P(dy), P(pool), rows // (H * W), H, W, P(x), P(gamma), P(mean), P(rstd), P(dres), P(dx), C, P(ws), ws_bytes, ctypes.byref(n), st)
        assert rc == 0, rc
        return n.value
    probe_rows = 1024 * gpb
    pz = torch.zeros(probe_rows, C, dtype=BF16, device="cuda")
    pf = torch.ones(probe_rows, device="cuda")
    cap = partial_launch(pz, pz, torch.ones(C, device="cuda"), pf, pf, None, torch.empty_like(pz), probe_rows, torch.empty(ws_bytes // 4, device="cuda"))
    B = MI.cdiv(MI.ln_rows(cap, gpb, U), H * W)
    rows, HW, h, w = B * H * W, H * W, (H + 1) // 2, (W + 1) // 2
    x, dy, dres = MI.rnd(B, H, W, C, scale=2.0, shift=0.5, seed=1), MI.rnd(B, H, W, C, seed=2), MI.rnd(B, H, W, C, seed=3)
    dp = MI.rnd(B, h, w, C, seed=4)
    gamma = MI.frand(C, seed=5, scale=0.3, shift=1.0)
    dg0, db0 = MI.frand(C, seed=6), MI.frand(C, seed=7)
    x2 = x.reshape(-1, C).double()
    mean, rstd = dvec(x2.mean(1)), dvec((x2.var(1, unbiased=False) + 1e-5).rsqrt())       # (the kernel clamps its prefetched rows to the last one)
    xd, dyd, dresd, dpd, gd = din(x), din(dy), din(dres), din(dp), dvec(gamma)
    n_sub = 2048 // HW                                                            # <= 512 x 4 rows: one row per lane group at either cap
    assert n_sub * HW <= min(cap, 512) * gpb
    for form in ("plain", "defer", "pool"):
        if form == "pool" and C > 512:
            n = ctypes.c_int(0)
            assert lib.ap_layernorm_bwd_partial_pool(P(dyd), P(dpd), B, H, W, P(xd), P(gd), P(mean), P(rstd), P(dresd), P(torch.empty(rows, C, dtype=BF16, device="cuda")),
                                                     C, P(torch.empty(ws_bytes // 4, device="cuda")), ws_bytes, ctypes.byref(n), st) == -2
            continue                                                              # (AP_ERR_UNSUPPORTED: two chunks per lane)
        dx, g0 = gbuf(rows, C, what="dx")
        dg, g1 = gacc(dg0[None], "dgamma")
        db, g2 = gacc(db0[None], "dbeta")
        ws = torch.full((ws_bytes // 4,), float("nan"), device="cuda")
        if form == "plain":
            assert lib.ap_layernorm_bwd(P(dyd), P(xd), P(gd), P(mean), P(rstd), P(dresd), P(dx), P(dg), P(db), rows, C, P(ws), ws_bytes, st) == 0
            n_partial = partial_launch(dyd, xd, gd, mean, rstd, dresd, torch.empty(rows, C, dtype=BF16, device="cuda"), rows, torch.empty_like(ws))
        else:
            n_partial = partial_launch(dyd, xd, gd, mean, rstd, dresd, dx, rows, ws, dpd if form == "pool" else None)
            ops.layernorm_bwd_reduce_batched([LnRider(ws, n_partial, C, dg, db)])
        torch.cuda.synchronize()
        assert n_partial == cap
        t = need(MI.ln_trips(rows, n_partial, gpb, U), "k_ln_bwd_pf")
        assert t.most == 3 and (U == 1 or t.fewest == 3)
        for g in (g0, g1, g2):
            g.check(pad="untouched")
        finite(dx, dg, db)
        d64 = dy.double() + (MI.pool_grad(dp.double(), H, W) if form == "pool" else 0)
        rdx, rdg, rdb = MI.layernorm_bwd(x2, d64.reshape(-1, C), gamma.double())
        rep = assert_tiled(dx, rdx + dres.reshape(-1, C).double(), TOL_BF16, "%s %s" % (case, form))
        eg, eb = rel(dg[0], dg0.double() + rdg), rel(db[0], db0.double() + rdb)
        trip_images = MI.cdiv(n_partial * gpb * U, HW)                            # the first image that lies wholly in the second trip
        equal = True
        for b0, b1 in sub_batches(B, n_sub, trip_images):
            dxs = torch.empty((b1 - b0) * HW, C, dtype=BF16, device="cuda")
            args = (dyd[b0 * HW:], xd[b0 * HW:], gd, mean[b0 * HW:], rstd[b0 * HW:], dresd[b0 * HW:], dxs, (b1 - b0) * HW, torch.empty_like(ws))
            partial_launch(*args, pool=dpd[b0 * h * w:] if form == "pool" else None)
            torch.cuda.synchronize()
            equal &= torch.equal(dxs, dx[b0 * HW:b1 * HW])
        report(case, "k_ln_bwd_pf " + form, t, rep, equal, "dgamma %.1e dbeta %.1e" % (eg, eb))
        assert eg < TOL_F32 and eb < TOL_F32, (eg, eb)
        assert equal


# ============================================================================================================== csrc/optim.hip
def _f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def test_adamw_ema_and_sumsq_beyond_two_sweeps(ops, lib, case):
    """ap_adamw_ema_step, _guarded and ap_sumsq_f32 on a slab of two sweeps and an odd number of float4s more (no query for the grids:
    csrc/optim.hip, adamw_ema_launch -- at most 256 * 16 workgroups of 256 lanes, one float4 each per sweep; ap_sumsq_f32 -- at most 1024):
    weight-decay mask, two EMA copies, the bf16 copy and value clipping, against an fp64 elementwise AdamW (tests/_multi_item.py::adamw_ema)
    at the tolerance of tests/test_gpu_kernels.py::test_fused_adamw_ema_matches_torch."""
    n = MI.ADAM_N
    t = need(MI.trips(n // 4, MI.ADAM_SWEEP_F4), "k_adamw_ema")
    ts = need(MI.trips((n - 1) // 4, MI.SUMSQ_SWEEP_F4), "k_sumsq_partial")
    assert (n // 4) % 2 == 1
    gen = torch.Generator().manual_seed(1)
    p0, g0, m0 = (torch.randn(n, generator=gen) for _ in range(3))
    m0 *= 0.1
    v0 = torch.rand(n, generator=gen) * 0.01
    e0 = [p0 + 0.01 * torch.randn(n, generator=gen) for _ in range(2)]
    mask = (torch.rand(n, generator=gen) < 0.7).to(torch.uint8)
    decays = [0.998, 0.9996]
    lr, b1, b2, eps, wd, step, gscale, clip = 1.6e-3, 0.9, 0.999, 1e-8, 0.05, 3, 0.5, 0.3
    b1f, b2f, decf = _f32(b1), _f32(b2), [_f32(d) for d in decays]
    ref = MI.adamw_ema(p0.double(), g0.double(), m0.double(), v0.double(), mask, [e.double() for e in e0], decf, _f32(lr), b1f, b2f, _f32(eps), _f32(wd), step, _f32(gscale), _f32(clip))
    gd, maskd = g0.cuda(), mask.cuda()
    dec_arr = (ctypes.c_float * 2)(*decays)

    def run(guard_state):
        bufs = [FlatGuard(n, torch.float32, nm) for nm in ("p", "m", "v", "ema 0", "ema 1")] + [FlatGuard(n, BF16, "bf16 copy")]
        for b, src in zip(bufs, (p0, m0, v0, e0[0], e0[1])):
            b.view.copy_(src)
        p, m, v, ea, eb, p16 = (b.view for b in bufs)
        ema_arr = (ctypes.c_void_p * 2)(ea.data_ptr(), eb.data_ptr())
        args = (P(p), P(gd), P(m), P(v), P(maskd), n, lr, b1, b2, eps, wd, step, gscale, None, 0.0, clip, None, ema_arr, dec_arr, 2, P(p16))
        rc = lib.ap_adamw_ema_step(*args, stream()) if guard_state is None else lib.ap_adamw_ema_step_guarded(*args, P(guard_state), stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        for b in bufs:
            b.check()
        return p, m, v, ea, eb, p16

    def state(nonfinite):
        bc1, bc2 = _f32(1.0 - b1f ** step), _f32((1.0 - b2f ** step) ** 0.5)
        words = struct.unpack("8i", struct.pack("4i2f2i", nonfinite, step, 0, 0, bc1, bc2, 0, 0))
        return torch.tensor(words, dtype=torch.int32).cuda()
    out = run(None)
    finite(*out)
    errs = []
    for nm, got, want in zip(("p", "m", "v", "ema 0", "ema 1"), out, (ref[0], ref[1], ref[2], ref[3][0], ref[3][1])):
        d = (got.double().cpu() - want).abs()
        errs.append(float((d / (2e-6 + 1e-5 * want.abs())).max()))
        assert errs[-1] <= 1.0, "%s: |got - fp64| exceeds 2e-6 + 1e-5 |fp64| by a factor %.2f at element %d" % (nm, errs[-1], int(torch.argmax(d)))
    assert torch.equal(out[5], out[0].to(BF16))
    guarded_out = run(state(0))
    same = all(torch.equal(a, b) for a, b in zip(out, guarded_out))
    skipped = run(state(1))                       # a skipped step: p, m, v untouched (the bf16 copy not written), the EMA copies lerp to the old p
    for got, src in zip(skipped[:3], (p0, m0, v0)):
        assert torch.equal(got.cpu(), src)
    for got, e, d in zip(skipped[3:5], e0, decf):
        assert torch.allclose(got.cpu().double(), d * e.double() + (1.0 - d) * p0.double(), rtol=1e-5, atol=2e-6)
    report(case, "ap_adamw_ema_step", t, extra="(items and grid in float4s: one sweep is the cap of 4096 workgroups x 256 lanes) worst |err| / (2e-6 + 1e-5 |ref|): %s; guarded step %s" % (" ".join("%.2f" % e for e in errs), "bit-equal" if same else "DIFFERS"))
    assert same
    sq = FlatGuard(1, torch.float32, "sum of squares")
    ws = torch.full((lib.ap_sumsq_workspace() // 8,), float("nan"), dtype=torch.float64, device="cuda")
    assert lib.ap_sumsq_f32(P(gd), n - 1, P(sq.view), P(ws), ws.numel() * 8, stream()) == 0        # n - 1: a tail of three elements behind the last float4
    torch.cuda.synchronize()
    sq.check()
    want = float(g0[:n - 1].double().pow(2).sum())
    e = abs(float(sq.view[0]) - want) / want
    report(case, "ap_sumsq_f32", ts, extra="(items and grid in float4s: one sweep is the cap of 1024 workgroups x 256 lanes) rel to fp64 %.2e" % e)
    # fp32 fma chains of at most 9 terms per lane and component (9 x 6e-8 at worst, random in sign), fp64 from there, one rounding to fp32
    assert e < 1e-6, e
