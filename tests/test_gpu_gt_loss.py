"""TokenLabelGTCrossEntropy on the sparse target: ap_soft_ce_sparse_gt_fwd_bwd through ops (the class rows: argmaxes, ratio and both blends
formed by the kernel), the loss class on a SparseTokenLabelTarget with nothing densified, and the loss inside GraphedStep and
AutoProgDriver(use_graphs=True).

The class counts take every path of the launcher: 24 / 1000 (a row in one wave's registers), 1001 (ld 1008: seven padding columns),
1100 (k_soft_ce_wide, one wave per row), 4100 (four waves per row), 21 843 (few cases).  The reference is tests/_gt_ref.py in fp64 on the
same bf16 logits (tests/test_gt_loss_host.py holds it against the oracle).  Bounds:
  row loss   1e-6 relative, per row (what tests/test_gpu_loss.py allows the sparse kernel against its densified target)
  gradient   the bf16 rounding of the reference gradient, per element: bf16 keeps 8 significant bits, so round-to-nearest moves a value by at
             most half an ulp = 2^-8 |ref|; on top of it the fp32 evaluation of grad_scale * (p * sum t - t), 1e-5 * grad_scale on a
             probability p <= 1.  (The rel-L2 of a tensor held to that is at most 2^-8 = 3.9e-3: printed, implied, not asserted twice.  The
             2e-3 of tests/test_gpu_loss.py is between two kernels that round the same fp32 value and does not apply to an fp64 reference.)
  loss level 2e-4 absolute on the loss, 6e-3 rel-L2 on both gradients (tests/test_gpu_loss.py)"""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests import _gt_ref as G
from tests._tilecheck import guarded, nan_padded, round_up

pytestmark = pytest.mark.gpu
N_TOK, SMOOTHING = 4, 0.1
WIDTHS = [24, 1000, 1001, 1100, 4100]
KERNEL_CASES = [(B, K, C) for C in WIDTHS for B in (5, 6) for K in (1, 5, 8)] + [(5, 5, 21843), (6, 8, 21843)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from autoprog_amd import ops as _ops
    return _ops


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _need_sparse_route():
    """the tests below hand the loss targets with -1 fillers in slot 0 (what SparseTokenLabelTarget.from_logits writes): only the sparse route
    may see them -- SparseTokenLabelTarget.dense scatters every index it is given"""
    from autoprog_amd import functional as AF
    assert hasattr(AF, "SparseTokenLabelGTCEFn"), "TokenLabelGTCrossEntropy has no sparse route: a target with -1 fillers would be densified"


def _pairs(B, K, C):
    idx, val, want = G.make_case(B, N_TOK, C, K, seed=B * 100 + K)
    if K >= 2:
        idx[B - 1, 1, K - 1] = C + 3                     # an index past the last class adds nothing (the smallest score of its slot)
    for s in (0, 1):
        assert float(G.score_gap(idx[:, s], val[:, s], C).min()) >= 1e-3
    assert torch.equal(G.ratios(idx, val, C), want)
    return idx, val


# ================================================================================================================ 1. the kernel through ops
@pytest.mark.parametrize("B,K,C", KERNEL_CASES)
def test_class_rows_kernel(ops, B, K, C):
    from autoprog_amd._lib import lib
    idx, val = _pairs(B, K, C)
    ld = round_up(C, 8)
    gen = torch.Generator().manual_seed(C + B)
    logits = (torch.randn(B, C, generator=gen) * 2).to(torch.bfloat16)
    x_c = torch.zeros(B, ld, dtype=torch.bfloat16)
    x_c[:, :C] = logits
    x_c = x_c.cuda()
    x_g = nan_padded(logits, ld, device="cuda")          # NaN in the columns C .. ld-1 and in the guard rows around the operand
    idev, vdev = idx.cuda(), val.cuda()
    p_sb = (2 + N_TOK) * K
    gs = 0.7 / B
    st = torch.cuda.current_stream().cuda_stream
    lam37 = torch.tensor([0.37], dtype=torch.float32, device="cuda")
    lam1 = torch.tensor([1.0], dtype=torch.float32, device="cuda")

    def run(lam, mix, ptr=None, x=x_c):
        return ops.soft_ce_sparse_gt_fwd_bwd(x, C, idev, vdev, p_sb, 0, K, SMOOTHING, gs, mix_lam=lam, mix_batches=mix, mix_lam_ptr=ptr)

    for lam, mix in ((1.0, 0), (0.37, B)):
        loss, dl = run(lam, mix)
        loss2, dl2 = run(lam, mix, x=x_g)                 # NaN padding in the logits changes nothing
        rows_ref, grad_ref = G.soft_ce_rows(logits, G.class_target(idx, val, C, SMOOTHING, lam), gs)
        e_loss = float(((loss.double().cpu() - rows_ref).abs() / rows_ref.abs()).max())
        d = dl[:, :C].double().cpu()
        e_grad = rel(d, grad_ref)
        e_elem = float(((d - grad_ref).abs() - 2.0 ** -8 * grad_ref.abs()).max())
        print("GT rows B %d K %d C %d lam %.2f | row loss %.3e | gradient rel %.3e | element excess over half an ulp %.3e (allowed %.1e)"
              % (B, K, C, lam, e_loss, e_grad, e_elem, 1e-5 * gs))
        assert e_loss <= 1e-6, e_loss
        assert e_elem <= 1e-5 * gs, e_elem
        assert bool((dl[:, C:].view(torch.int16) == 0).all()), "padding columns of dlogits must be zero bits"
        assert torch.equal(loss, loss2) and torch.equal(dl, dl2), "two runs (the second with NaN padding) must be bit-identical"
        # the guarded launch through the C ABI: sentinel rows around both outputs
        g_loss, guard_l = guarded(1, B, round_up(B, 64) + 64, torch.float32, pre=1, post=1, device="cuda", what="row_loss")
        g_dl, guard_d = guarded(B, C, ld, device="cuda", what="dlogits")
        rc = lib.ap_soft_ce_sparse_gt_fwd_bwd(x_g.data_ptr(), ld, idev.data_ptr(), vdev.data_ptr(), K, p_sb, 0, K, SMOOTHING, g_loss.data_ptr(), g_dl.data_ptr(),
                                              gs, B, C, lam, mix, None, st)
        assert rc == 0
        torch.cuda.synchronize()
        guard_l.check(pad="untouched")
        guard_d.check(pad="zero")
        assert torch.equal(g_loss[0, :B], loss) and torch.equal(g_dl, dl)
        # lam from device memory
        if mix == 0:
            for other in (run(1.0, 0, lam37.data_ptr()), run(1.0, B), run(0.0, B, lam1.data_ptr())):
                assert torch.equal(other[0], loss) and torch.equal(other[1], dl), "mix_batches = 0 / lam = 1: host and device lam give the same bits"
        else:
            other = run(1.0, B, lam37.data_ptr())
            assert torch.equal(other[0], loss) and torch.equal(other[1], dl)


def test_argument_refusals(ops):
    from autoprog_amd.ops import AutoProgHipError
    B, C = 4, 1100
    x = torch.zeros(B, 1104, dtype=torch.bfloat16, device="cuda")
    idx9 = torch.zeros(B, 2 + N_TOK, 9, dtype=torch.int32, device="cuda")
    with pytest.raises(AutoProgHipError, match=r"code -1"):                                   # K = 9
        ops.soft_ce_sparse_gt_fwd_bwd(x, C, idx9, idx9.float(), (2 + N_TOK) * 9, 0, 9, 0.1, 1.0)
    idx5 = torch.zeros(B, 2 + N_TOK, 5, dtype=torch.int32, device="cuda")
    flat = torch.zeros(B * 1104 + 8, dtype=torch.bfloat16, device="cuda")
    off = flat[1:1 + B * 1104].view(B, 1104)                                                  # a wide row 2 bytes off the 16-byte grid
    assert off.data_ptr() % 16 == 2
    with pytest.raises(AutoProgHipError, match=r"code -1"):
        ops.soft_ce_sparse_gt_fwd_bwd(off, C, idx5, idx5.float(), (2 + N_TOK) * 5, 0, 5, 0.1, 1.0)
    with pytest.raises(AutoProgHipError, match=r"code -1"):                                   # mix_batches not in {0, B}
        ops.soft_ce_sparse_gt_fwd_bwd(x, C, idx5, idx5.float(), (2 + N_TOK) * 5, 0, 5, 0.1, 1.0, mix_lam=0.5, mix_batches=B - 1)
    with pytest.raises(AutoProgHipError):                                                     # the slots would leave the pair arrays
        ops.soft_ce_sparse_gt_fwd_bwd(x, C, idx5, idx5.float(), (2 + N_TOK) * 5, 0, (1 + N_TOK) * 5 + 1, 0.1, 1.0)
    torch.cuda.synchronize()


# ================================================================================================================ 2. the loss class
LOSS_CASES = [(5, 24, 5), (6, 1001, 8), (5, 1100, 5), (6, 4100, 1), (5, 21843, 5)]


def _loss_inputs(B, C, K, fillers):
    from autoprog_amd.loss import SparseTokenLabelTarget
    idx, val = _pairs(B, K, C)
    if not fillers:
        # every index inside [0, C): the -1 fillers of slot 0 become classes of score 0 (they add nothing either), so that
        # SparseTokenLabelTarget.dense, which scatters every index, can serve as the reference
        idx = idx.clone()
        idx[idx < 0] = 0
        idx[idx >= C] = 0
        for sl in (0, 1):
            assert float(G.score_gap(idx[:, sl], val[:, sl], C).min()) >= 1e-3
    g = torch.Generator().manual_seed(B + C)
    x_cls = (torch.randn(B, C, generator=g) * 2).to(torch.bfloat16)
    x_aux = (torch.randn(B, N_TOK, C, generator=g) * 2).to(torch.bfloat16)
    return idx, val, x_cls, x_aux, SparseTokenLabelTarget(idx.cuda(), val.cuda(), smoothing=SMOOTHING)


@pytest.mark.parametrize("fillers", [False, True])
@pytest.mark.parametrize("B,C,K", LOSS_CASES)
def test_loss_on_a_sparse_target_equals_the_oracle_on_the_densified_one(ops, monkeypatch, B, C, K, fillers):
    """without a box and with one (lam = 0.5), from host lam and from a DeviceBox; then the same calls with SparseTokenLabelTarget.dense
    made to raise: the sparse route densifies nothing.  (A target with -1 fillers runs only with dense() disabled.)"""
    from autoprog_amd.graph import DeviceBox, StepScalars
    from autoprog_amd.loss import SparseTokenLabelTarget, TokenLabelGTCrossEntropy
    if fillers:
        _need_sparse_route()
    idx, val, x_cls, x_aux, target = _loss_inputs(B, C, K, fillers)
    # the reference's input: target.dense(C) where every index is a class; with -1 fillers the same tensor built on the CPU without them
    dense = G.densify(idx, val, C, SMOOTHING) if fillers else target.dense(C).cpu()
    if not fillers:
        assert torch.allclose(dense, G.densify(idx, val, C, SMOOTHING), atol=1e-7)
    loss_fn = TokenLabelGTCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=C)
    scalars = StepScalars(torch.device("cuda"))

    def run(bb):
        xc, xa = x_cls.cuda().requires_grad_(True), x_aux.cuda().requires_grad_(True)
        loss = loss_fn((xc, xa, bb), target)
        loss.backward()
        return loss.detach().clone(), xc.grad.clone(), xa.grad.clone()

    def check_all(outs):
        for bb in ((0, 0, 0, 0), (0, 0, 1, 2)):
            got = run(bb)
            if bb in outs:
                assert all(torch.equal(a, b) for a, b in zip(outs[bb], got))
            outs[bb] = got
            cr, ar = x_cls.double().requires_grad_(True), x_aux.double().requires_grad_(True)
            ref = R.token_label_gt_ce((cr, ar, bb), dense.double(), 0.5, 1.0)
            ref.backward()
            e = (abs(float(got[0]) - float(ref.detach())), rel(got[1], cr.grad), rel(got[2], ar.grad))
            print("GT loss B %d C %d K %d fillers %s box %s | loss %.7f (oracle %.7f, diff %.3e) | d cls %.3e d aux %.3e" % (B, C, K, fillers, bb, float(got[0]), float(ref.detach()), *e))
            assert e[0] < 2e-4 and e[1] < 6e-3 and e[2] < 6e-3, e
            # the step's box in device memory: the same bits
            scalars.begin()
            scalars.set_box(bb, N_TOK)
            scalars.push()
            dev = run(DeviceBox(scalars))
            assert all(torch.equal(a, b) for a, b in zip(got, dev)), "host lam and device lam must give the same bits"

    outs = {}
    if not fillers:
        check_all(outs)

    def refuse(self, classes):
        raise AssertionError("SparseTokenLabelTarget.dense was called: the sparse route must not densify")
    monkeypatch.setattr(SparseTokenLabelTarget, "dense", refuse)
    check_all(outs)


def test_a_subclass_with_its_own_adjust_cls_keeps_the_dense_route(ops, monkeypatch):
    from autoprog_amd.loss import SparseTokenLabelTarget, TokenLabelGTCrossEntropy

    class Mine(TokenLabelGTCrossEntropy):
        def _adjust_cls(self, target_cls, target):
            return target_cls

    idx, val, x_cls, x_aux, target = _loss_inputs(5, 24, 5, False)
    called = []
    real = SparseTokenLabelTarget.dense
    monkeypatch.setattr(SparseTokenLabelTarget, "dense", lambda self, classes: (called.append(classes), real(self, classes))[1])
    loss = Mine(dense_weight=0.5, cls_weight=1.0, classes=24)((x_cls.cuda(), x_aux.cuda(), (0, 0, 0, 0)), target)
    assert called == [24] and np.isfinite(float(loss))


# ================================================================================================================ 3. graph
BOX_SEED = 3          # the first numpy seed whose three mix-token draws on the 4 x 4 grid differ in area and include an empty box:
                      # (0, 2, 2, 4), (0, 0, 0, 0), (0, 1, 1, 3) -> lam = 0.75, 1, 0.875 (all exact in fp32)


def _step_setup(kind, stem=16, loss="TokenLabelGTCrossEntropy"):
    import autoprog_amd.loss as L
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import FlatAdamWEma
    torch.manual_seed(0)
    model = create_model("model_variant", variant="volo_h2_l3", num_classes=24, img_size=64, stem_hidden_dim=stem, drop_path_rate=0.0).cuda().train()
    red = GradientBucketReducer(list(model.parameters()), world_size=1, defer_mean=True)
    red.install_sink(model)
    opt = FlatAdamWEma(model, red, lr=2e-3, weight_decay=0.05, ema_decays=[0.9, 0.99])
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(1)).cuda()
    idx, val, _ = G.make_case(4, 16, 24, 5, seed=9)
    idx[idx < 0] = 0                           # (score 0: adds nothing) every index is a class, so the dense form of the same target exists
    target = L.SparseTokenLabelTarget(idx.cuda(), val.cuda(), smoothing=SMOOTHING) if kind == "sparse" else G.densify(idx, val, 24, SMOOTHING).cuda()
    return model, red, opt, getattr(L, loss)(dense_weight=0.5, cls_weight=1.0, classes=24), x, target


def _named(model):
    return {n: p.detach().clone() for n, p in model.named_parameters()}


def _eager_steps(kind, steps, **kw):
    model, red, opt, loss_fn, x, target = _step_setup(kind, **kw)
    try:
        np.random.seed(BOX_SEED)
        torch.manual_seed(5)
        losses, boxes = [], []
        for s in range(steps):
            red.zero_grad()
            out = model(x)
            boxes.append(tuple(int(v) for v in out[2]))
            loss = loss_fn(out, target)
            loss.backward()
            red.finish()
            opt.step()
            losses.append(float(loss.detach()))
        return losses, boxes, opt.p.clone(), _named(model)
    finally:
        red.remove()


def _graphed_steps(kind, steps, **kw):
    from autoprog_amd.graph import GraphedStep
    model, red, opt, loss_fn, x, target = _step_setup(kind, **kw)
    try:
        gs = GraphedStep(model, loss_fn, red, opt, x, target)
        p0, m0, v0 = opt.p.clone(), opt.m.clone(), opt.v.clone()
        ema0 = [e.clone() for e in opt.ema]
        bufs0 = [b.detach().clone() for b in opt._buffers]
        ebufs0 = [[b.clone() for b in bs] for bs in opt.ema_buffers]
        gs.capture(warmup=2)                       # warm-up steps are real steps: rewind what they moved (tests/test_gpu_graph.py)
        with torch.no_grad():
            opt.p.copy_(p0); opt.m.copy_(m0); opt.v.copy_(v0)
            for e, e0 in zip(opt.ema, ema0):
                e.copy_(e0)
            for b, b0 in zip(opt._buffers, bufs0):
                b.copy_(b0)
            for bs, bs0 in zip(opt.ema_buffers, ebufs0):
                for b, b0 in zip(bs, bs0):
                    b.copy_(b0)
            for m in model.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.num_batches_tracked.zero_()
        opt.step_count = 0
        opt.resync()
        np.random.seed(BOX_SEED)
        torch.manual_seed(5)
        losses, boxes = [], []
        for s in range(steps):
            loss = gs.step()
            boxes.append(gs.scalars.box)
            losses.append(float(loss.detach()))
        return losses, boxes, opt.p.clone(), _named(model)
    finally:
        red.remove()


@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_graph_replays_are_the_eager_steps(ops, monkeypatch, kind):
    """a one-block volo_h2_l3 with TokenLabelGTCrossEntropy in GraphedStep, DropPath off: three replays give the losses and the weights of
    three eager steps with the same seeds, bit for bit"""
    monkeypatch.setattr(ops, "deterministic", True)
    # the 16-channel stem runs on the vendor convolution, whose default weight-gradient algorithm is not reproducible from run to run
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    le, be, pe, _ = _eager_steps(kind, 3)
    lg, bg, pg, _ = _graphed_steps(kind, 3)
    print("GT graph %s | boxes %s | eager %s | graph %s" % (kind, be, le, lg))
    assert be == bg == [(0, 2, 2, 4), (0, 0, 0, 0), (0, 1, 1, 3)] and all(np.isfinite(v) for v in le)
    assert le == lg, (le, lg)
    assert torch.equal(pe, pg)


# ================================================================================================================ 4. driver
def test_driver_with_a_teacher_eager_and_graphed(ops, monkeypatch):
    """AutoProgDriver(teacher=labeler, use_graphs=True) with TokenLabelGTCrossEntropy, two epochs of three steps at one configuration,
    DropPath 0, same seeds: the losses, weights and EMA copies of the eager driver, bit for bit (as tests/test_gpu_token_label_topk.py
    checks the plain loss)"""
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import SparseTokenLabelTarget, TokenLabelGTCrossEntropy
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import FlatAdamWEma
    from autoprog_amd.prog.driver import AutoProgDriver
    from autoprog_amd.prog.teacher import TeacherLabeler
    monkeypatch.setattr(ops, "deterministic", True)
    _need_sparse_route()

    def volo(seed, variant):
        torch.manual_seed(seed)
        return create_model("model_variant", variant=variant, num_classes=24, img_size=64, stem_hidden_dim=64).cuda()
    teacher = volo(0, "volo_h2_l3").eval()
    out = {}
    for use_graphs in (False, True):
        student = volo(4, "volo_h2_l6").train()
        red = GradientBucketReducer(list(student.parameters()), world_size=1, defer_mean=True)
        red.install_sink(student)
        opt = FlatAdamWEma(student, red, lr=1e-3, weight_decay=0.05, ema_decays=[0.9, 0.99])
        g = torch.Generator().manual_seed(1)
        seen = []

        def get_batch(r):
            return torch.randn(8, 3, 96, 96, generator=g).cuda(), torch.randint(0, 24, (8,), generator=g).cuda()

        def loss_fn(outputs, target, _ce=TokenLabelGTCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=24)):
            seen.append(type(target))
            return _ce(outputs, target)

        drv = AutoProgDriver(student, loss_fn, opt, red, get_batch, r_list=[64], l_list=[6], dp_list=[0.0], grow_epochs=[0], steps_per_epoch=3,
                             auto_grow=False, use_graphs=use_graphs, graph_after=2, teacher=TeacherLabeler(teacher, k=5, num_classes=24))
        steps, real = [], drv._train_step
        monkeypatch.setattr(drv, "_train_step", lambda *a, **k: (steps.append(real(*a, **k)), steps[-1])[1])
        try:
            np.random.seed(3)
            drv.run(2)
            out[use_graphs] = ([float(s) for s in steps], opt.p.clone(), [e.clone() for e in opt.ema], len(drv._graphs))
            assert seen and all(t is SparseTokenLabelTarget for t in seen)
        finally:
            red.remove()
    le, pe, ee, _ = out[False]
    lg, pg, eg, live = out[True]
    print("GT driver eager:", le)
    print("GT driver graph:", lg)
    assert len(le) == 6 and all(np.isfinite(v) for v in le) and live == 1
    assert le == lg, (le, lg)
    assert torch.equal(pe, pg) and all(torch.equal(a, b) for a, b in zip(ee, eg))
