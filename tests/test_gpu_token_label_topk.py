"""Token-label targets from a teacher network: ap_softmax_topk_rows (csrc/topk.hip) through the C ABI, SparseTokenLabelTarget.from_logits,
VOLO.forward_dense, prog.teacher.TeacherLabeler and AutoProgDriver(teacher=...).

The launcher takes one of three kernels by the row stride: ld <= 1024 k_softmax_topk (a row in one wave's registers, two 16-byte chunks per
lane -- the second one is all padding up to ld = 512), 1024 < ld <= 4096 k_softmax_topk_wide<1> (a wave per row, the row in LDS) and beyond
k_softmax_topk_wide<4> (four waves per row).  The row cases stand on both sides of each of these widths: 512 | 520, 1024 | 1032, 4096 | 4104.
All three are PLAIN grids -- one workgroup per group of 16, 4 or 1 rows, no workgroup takes a second item -- so there is no later-trip case.

The reference is tests/_topk_ref.py: fp64 softmax of inv_temp * x on the same bf16 logits and torch's stable descending sort.  Bounds: idx exact,
|val - ref| <= 1e-4 ref + 1e-37, val non-increasing along k."""
import functools

import numpy as np
import pytest
import torch

from tests._topk_ref import check_pairs, topk_ref
from tests.test_gpu_localized import P, case, dev, ops, stream  # noqa: F401  (ops, case: fixtures)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
M_ROWS, RPB = 37, 8                 # 37 rows in batches of 8: five batches, the last one with five rows
IDX_SENTINEL, VAL_SENTINEL = -7777, -123.25
ROW_CASES = [(5, 8, 5), (16, 16, 16), (512, 512, 16), (513, 520, 5), (1000, 1000, 5), (1001, 1008, 8), (1024, 1024, 16), (1025, 1032, 5),
             (4096, 4096, 16), (4097, 4104, 5), (21843, 21848, 8), (65536, 65536, 16)]
# the end of a row one chunk either side of a batch of the staging walk (4 chunks per thread in flight: 256 chunks = 2048 columns for a team of
# one wave, 1024 chunks = 8192 columns for a team of four): 255 chunks, 256 with the last partly masked, 257 (a second batch of one chunk and
# three clamped loads); 1024 and 1025
ROW_CASES += [(2040, 2040, 5), (2041, 2048, 16), (2049, 2056, 5), (8185, 8192, 16), (8193, 8200, 5)]


@functools.lru_cache(maxsize=None)
def _rows(C, ld, K):
    """-> (logits bf16 [37, ld] on the CPU with NaN / +inf in columns C .. ld-1, the reference order [37, K]); built once, never modified"""
    g = torch.Generator().manual_seed(1000 * K + C)
    x = (torch.randn(M_ROWS, C, generator=g) * 3).to(BF16)
    x[1] = 1.5                                                          # all equal: idx = 0 .. K-1
    x[2, 0] = x[2, C - 1] = 40.0                                        # the same peak at both ends: [0, C-1]
    x[3] = (x[3].float() + 300).to(BF16)                                # a missing maximum subtraction overflows / underflows
    x[4] = (x[4].float() - 300).to(BF16)
    x[5, ::3] = float("-inf")
    full = torch.full((M_ROWS, ld), float("nan"), dtype=BF16)
    full[:, C + 1::2] = float("inf")
    full[:, :C] = x
    order = topk_ref(x, K)[0]
    assert order[1].tolist() == list(range(K)) and order[2, :2].tolist() == [0, C - 1]
    return full, order


def _launch_rows(lib, xd, C, ld, K, inv_temp):
    """one launch into slots 2.. of a sentinel-filled [B, 2 + RPB, K] pair -> (idx [37, K], val [37, K]) after checking the rest is untouched"""
    B = -(-M_ROWS // RPB)
    idx = torch.full((B, 2 + RPB, K), IDX_SENTINEL, dtype=torch.int32, device="cuda")
    val = torch.full((B, 2 + RPB, K), VAL_SENTINEL, dtype=torch.float32, device="cuda")
    rc = lib.ap_softmax_topk_rows(P(xd), ld, C, K, inv_temp, idx[:, 2:].data_ptr(), val[:, 2:].data_ptr(), (2 + RPB) * K, K, RPB, M_ROWS, stream())
    assert rc == 0, "ap_softmax_topk_rows(C = %d, ld = %d, K = %d): code %d" % (C, ld, K, rc)
    torch.cuda.synchronize()
    written = torch.zeros(B, 2 + RPB, dtype=torch.bool)
    for r in range(M_ROWS):
        written[r // RPB, 2 + r % RPB] = True
    ic, vc = idx.cpu(), val.cpu()
    assert bool((ic[~written] == IDX_SENTINEL).all()) and bool((vc[~written] == VAL_SENTINEL).all()), "elements outside the addressed slots were written"
    return ic[written], vc[written]


# ================================================================================================================ 1. rows against fp64
@pytest.mark.parametrize("C,ld,K", ROW_CASES)
def test_rows_against_fp64(ops, case, C, ld, K):
    """37 rows (N(0, 3) rounded to bf16: ties abound; an all-equal row, a row with its peak in column 0 and C-1, rows shifted by +300 and
    -300, a row with -inf in every third column), columns C .. ld-1 NaN and +inf, inv_temp 2, 1 and 0.25, written through the strides into
    slots 2.. of a sentinel-filled [5, 2 + 8, K] buffer whose last batch has five rows: every element outside the addressed slots comes
    back untouched, idx is the stable descending order, val inside 1e-4 ref + 1e-37 of the fp64 softmax and non-increasing.
    Widths either side of the launcher's thresholds: 512 | 520 (second chunk of a lane all padding), 1024 | 1032 (registers | LDS, one
    wave per row), 4096 | 4104 (one | four waves per row)."""
    from autoprog_amd._lib import lib
    x, order = _rows(C, ld, K)
    xd = dev(x)
    for inv_temp in (2.0, 1.0, 0.25):
        ref_val = torch.softmax(inv_temp * x[:, :C].double(), dim=1).gather(1, order)
        idx, val = _launch_rows(lib, xd, C, ld, K, inv_temp)
        check_pairs(idx, val, order, ref_val, "%s inv_temp %.2f" % (case, inv_temp))


# ================================================================================================================ 2. every column can win
def _planted_columns(C):
    if C <= 4097:
        return list(range(C))
    return sorted(set(range(64)) | set(range(0, C, 509)) | set(range(C - 64, C)))


@pytest.mark.parametrize("C,ld", [(1001, 1008), (4097, 4104), (21843, 21848), (65536, 65536)])
def test_every_column_can_win(ops, case, C, ld):
    """background N(0, 1), row i has +12 planted in its own column: idx[i, 0] is that column for every column (1001, 4097) or for columns
    0 .. 63, every 509th and the last 64 (21 843, 65 536) -- a dropped chunk, lane or tail column cannot pass -- and the pairs hold the bounds"""
    from autoprog_amd._lib import lib
    K = 5
    cols = _planted_columns(C)
    M = len(cols)
    g = torch.Generator().manual_seed(C)
    x = torch.zeros(M, ld)
    x[:, :C] = torch.randn(M, C, generator=g)
    x[torch.arange(M), torch.tensor(cols)] += 12.0
    x = x.to(BF16)
    idx = torch.empty(M, K, dtype=torch.int32, device="cuda")
    val = torch.empty(M, K, dtype=torch.float32, device="cuda")
    rc = lib.ap_softmax_topk_rows(P(dev(x)), ld, C, K, 1.0, P(idx), P(val), K, 0, 1, M, stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert idx[:, 0].cpu().tolist() == cols, "a planted column did not win its row"
    ref_idx, ref_val = topk_ref(x[:, :C], K)
    check_pairs(idx, val, ref_idx, ref_val, case)


# ================================================================================================================ 4. poisoned LDS
@pytest.mark.parametrize("C,ld,K", [(1001, 1008, 8), (4097, 4104, 5), (21843, 21848, 8)])
def test_same_bits_after_poisoned_lds(ops, case, C, ld, K):
    """the three kernels once more behind ops.poison_lds(): same bits (nothing is read from LDS that the launch did not write)"""
    from autoprog_amd._lib import lib
    xd = dev(_rows(C, ld, K)[0])
    i0, v0 = _launch_rows(lib, xd, C, ld, K, 1.0)
    ops.poison_lds()
    i1, v1 = _launch_rows(lib, xd, C, ld, K, 1.0)
    assert torch.equal(i0, i1) and torch.equal(v0.view(torch.int32), v1.view(torch.int32))


# ================================================================================================================ 5. graph capture
def _teacher_like_logits(B, N, C, seed):
    """(labels, cls_logits [B, C], aux_logits [B, N, C]) as padded views, the way functional.linear returns them at C % 8 != 0"""
    g = torch.Generator().manual_seed(seed)
    ld = (C + 7) // 8 * 8
    cls = torch.zeros(B, ld, dtype=BF16)
    aux = torch.zeros(B, N, ld, dtype=BF16)
    cls[:, :C] = (torch.randn(B, C, generator=g) * 3).to(BF16)
    aux[..., :C] = (torch.randn(B, N, C, generator=g) * 3).to(BF16)
    return torch.randint(0, C, (B,), generator=g), cls, aux


def _check_target(t, labels, cls, aux, k, inv_temp, what):
    B, N, C = aux.shape
    assert tuple(t.idx.shape) == (B, 2 + N, k) and t.idx.dtype == torch.int32 and t.val.dtype == torch.float32
    want_i = torch.full((B, k), -1, dtype=torch.int32)
    want_i[:, 0] = labels.cpu().int()
    want_v = torch.zeros(B, k)
    want_v[:, 0] = 1.0
    assert torch.equal(t.idx[:, 0].cpu(), want_i) and torch.equal(t.val[:, 0].cpu(), want_v), "%s: slot 0 is not (label, 1.0), (-1, 0.0).." % what
    x = torch.cat([cls.cpu().reshape(B, 1, C), aux.cpu()], dim=1).reshape(B * (1 + N), C)
    ref_idx, ref_val = topk_ref(x, k, inv_temp)
    check_pairs(t.idx[:, 1:].reshape(-1, k), t.val[:, 1:].reshape(-1, k), ref_idx, ref_val, what)


def test_from_logits_graph_capture(ops, case):
    """from_logits(..., out=target) captured on one stream (1001 classes: padded views, the register kernel; 1100: the LDS kernel), new logits
    copied into the static inputs, one replay: the eager call on those logits bit for bit -- and the pairs hold the bounds"""
    from autoprog_amd.loss import SparseTokenLabelTarget
    for C in (1001, 1100):
        B, N, k = 3, 5, 5
        lab0, cls0, aux0 = _teacher_like_logits(B, N, C, 1)
        lab1, cls1, aux1 = _teacher_like_logits(B, N, C, 2)
        s_lab, s_cls, s_aux = lab0.cuda(), cls0.cuda(), aux0.cuda()
        target = SparseTokenLabelTarget.from_logits(s_lab, s_cls[:, :C], s_aux[..., :C], k=k, temperature=2.0)         # (eager first: lazy initialisations)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                   # (one capture stream)
            SparseTokenLabelTarget.from_logits(s_lab, s_cls[:, :C], s_aux[..., :C], k=k, temperature=2.0, out=target)
        s_lab.copy_(lab1); s_cls.copy_(cls1); s_aux.copy_(aux1)
        target.idx.fill_(IDX_SENTINEL); target.val.fill_(VAL_SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        eager = SparseTokenLabelTarget.from_logits(lab1.cuda(), cls1.cuda()[:, :C], aux1.cuda()[..., :C], k=k, temperature=2.0)
        assert torch.equal(target.idx, eager.idx) and torch.equal(target.val.view(torch.int32), eager.val.view(torch.int32))
        _check_target(target, lab1, cls1[:, :C], aux1[..., :C], k, 0.5, "%s C %d" % (case, C))


# ================================================================================================================ 6. error codes
def test_error_codes(ops):
    from autoprog_amd._lib import AutoProgHipError, lib
    from autoprog_amd.loss import SparseTokenLabelTarget
    x = torch.zeros(4, 16, dtype=BF16, device="cuda")
    idx = torch.full((4, 16), IDX_SENTINEL, dtype=torch.int32, device="cuda")
    val = torch.full((4, 16), VAL_SENTINEL, dtype=torch.float32, device="cuda")

    def call(ptr=None, ld=16, C=16, K=5, M=4, idx_ptr=None, val_ptr=None):
        return lib.ap_softmax_topk_rows(P(x) if ptr is None else ptr, ld, C, K, 1.0, P(idx) if idx_ptr is None else idx_ptr,
                                        P(val) if val_ptr is None else val_ptr, 16, 0, 1, M, stream())
    assert call(K=0) == -1 and call(K=17) == -1 and call(C=5, K=6) == -1                 # AP_ERR_SHAPE: K outside 1 .. min(16, C)
    assert call(ld=12, C=12) == -1 and call(ld=8, C=16) == -1                             # ld % 8, ld < C
    assert call(ptr=P(x) + 2, ld=8, C=8) == -1                                            # rows are not 16-byte aligned
    assert call(ld=65544, C=16) == -2                                                     # AP_ERR_UNSUPPORTED
    assert call(ptr=0) == -4 and call(idx_ptr=0) == -4 and call(val_ptr=0) == -4          # AP_ERR_NULL
    assert call(M=0) == 0 and call(ptr=0, idx_ptr=0, val_ptr=0, M=0) == 0                 # no rows: success without a launch
    torch.cuda.synchronize()
    assert bool((idx == IDX_SENTINEL).all()) and bool((val == VAL_SENTINEL).all()), "a refused call wrote something"
    with pytest.raises(AutoProgHipError):
        ops.softmax_topk(x.cpu(), 16, 5, 1.0, idx.view(-1), val.view(-1), 16, 0, 1)
    with pytest.raises(AutoProgHipError):                                                 # the strides would leave the outputs
        ops.softmax_topk(x, 16, 5, 1.0, idx.view(-1)[:20], val.view(-1)[:20], 16, 0, 1)
    lab = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        SparseTokenLabelTarget.from_logits(lab, x, x.view(4, 1, 16), k=9)


# ================================================================================================================ 7. forward_dense
def _small_volo(classes=24, seed=0, variant="volo_h2_l3"):
    from autoprog_amd.models import create_model
    torch.manual_seed(seed)
    return create_model("model_variant", variant=variant, num_classes=classes, img_size=64, stem_hidden_dim=64).cuda()


@pytest.fixture(scope="module")
def teacher24(ops):
    return _small_volo().eval()


def test_forward_dense(ops, teacher24):
    """eval() under no_grad: x_cls + 0.5 * x_aux.max(1)[0] is model(x) bit for bit; train mode: the unmixed (x_cls, x_aux) -- what forward()
    returns once mix_token is off -- of shape [4, 24] and [4, 16, 24]"""
    model = teacher24
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()
    try:
        with torch.no_grad():
            y = model(x)
            x_cls, x_aux = model.forward_dense(x)
        assert tuple(x_cls.shape) == (4, 24) and tuple(x_aux.shape) == (4, 16, 24)
        assert torch.equal(x_cls + 0.5 * x_aux.max(1)[0], y)
        model.train()
        np.random.seed(11)
        t_cls, t_aux = model.forward_dense(x)
        assert tuple(t_cls.shape) == (4, 24) and tuple(t_aux.shape) == (4, 16, 24) and t_cls.requires_grad and t_aux.requires_grad
        model.mix_token = False
        p_cls, p_aux, box = model(x)
        assert tuple(box) == (0, 0, 0, 0) and torch.equal(t_cls, p_cls) and torch.equal(t_aux, p_aux)
    finally:
        model.mix_token = True
        model.eval()


# ================================================================================================================ 8. the labeler
@pytest.mark.parametrize("r", [64, 96])
@pytest.mark.parametrize("kind", ["fp32", "prepared"])
def test_labeler(ops, case, teacher24, kind, r):
    """96-px images (fp32, and a PreparedBatch with RandomErasing and no mix) at the student's stage resolution r: the target is
    [B, 2 + (r // 16)^2, 5], slot 0 the ground truth, slots 1.. the reference's pairs of forward_dense's logits at that resolution, and a
    second call fills the same buffers"""
    from autoprog_amd.data import DeviceBatchPrep
    from autoprog_amd.prog.teacher import TeacherLabeler
    B, k = 4, 5
    g = torch.Generator().manual_seed(r)
    labels = torch.randint(0, 24, (B,), generator=g).cuda()
    if kind == "fp32":
        images = torch.randn(B, 3, 96, 96, generator=g).cuda()
    else:
        prep = DeviceBatchPrep((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), re_prob=0.9, re_mode="pixel", num_classes=24, seed=5)
        images = prep.prep(torch.randint(0, 256, (B, 3, 96, 96), dtype=torch.uint8, generator=g).cuda())
    labeler = TeacherLabeler(teacher24, k=k, temperature=1.0, smoothing=0.1, num_classes=24)
    t = labeler(images, labels, r)
    N = (r // 16) ** 2
    assert tuple(t.idx.shape) == (B, 2 + N, k) and t.smoothing == 0.1 and not teacher24.training
    with torch.no_grad():
        x_cls, x_aux = teacher24.forward_dense(images)                  # (the labeler left resize_to = r, resize_in_eval = True)
    assert tuple(x_aux.shape) == (B, N, 24)
    _check_target(t, labels, x_cls, x_aux, k, 1.0, case)
    ptrs = (t.idx.data_ptr(), t.val.data_ptr())
    t2 = labeler(images, labels.flip(0), r)
    assert t2 is t and (t2.idx.data_ptr(), t2.val.data_ptr()) == ptrs and torch.equal(t2.idx[:, 0, 0].cpu(), labels.flip(0).cpu().int())


def test_labeler_refuses_a_batch_that_may_be_mixed(ops, teacher24):
    from autoprog_amd.data import DeviceBatchPrep
    from autoprog_amd.prog.teacher import TeacherLabeler
    prep = DeviceBatchPrep((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), cutmix_alpha=1.0, num_classes=24, seed=5)
    images = prep.prep(torch.zeros(4, 3, 96, 96, dtype=torch.uint8).cuda())
    with pytest.raises(NotImplementedError):
        TeacherLabeler(teacher24)(images, torch.zeros(4, dtype=torch.int64).cuda(), 64)


# ================================================================================================================ 9. wide head
def test_wide_head_step_on_the_labeler_target(ops, case):
    """21 843 classes, B = 2, r = 64: the labeler's target goes into TokenLabelCrossEntropy on a student of the same shape; its loss equals
    (1e-4 relative) the loss on the target rebuilt from the reference's pairs, and one training step stays finite"""
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import SparseTokenLabelTarget, TokenLabelCrossEntropy
    from autoprog_amd.optim import FlatAdamWEma
    from autoprog_amd.prog.teacher import TeacherLabeler
    C, B, r, k = 21843, 2, 64, 5
    teacher = _small_volo(C, seed=1).eval()
    student = _small_volo(C, seed=2).train()
    red = GradientBucketReducer(list(student.parameters()), world_size=1, defer_mean=True)
    red.install_sink(student)
    opt = FlatAdamWEma(student, red, lr=1e-3, weight_decay=0.05, ema_decays=[0.9])
    try:
        x = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()
        labels = torch.tensor([C - 1, 7]).cuda()
        target = TeacherLabeler(teacher, k=k, num_classes=C)(x, labels, r)
        with torch.no_grad():
            x_cls, x_aux = teacher.forward_dense(x)
        _check_target(target, labels, x_cls, x_aux, k, 1.0, case)
        ref_idx, ref_val = topk_ref(torch.cat([x_cls.cpu().reshape(B, 1, C), x_aux.cpu()], dim=1).reshape(-1, C), k)
        rebuilt_i, rebuilt_v = target.idx.cpu().clone(), target.val.cpu().clone()
        rebuilt_i[:, 1:] = ref_idx.reshape(B, -1, k).int()
        rebuilt_v[:, 1:] = ref_val.reshape(B, -1, k).float()
        rebuilt = SparseTokenLabelTarget(rebuilt_i.cuda(), rebuilt_v.cuda(), smoothing=0.1)
        loss_fn = TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=C)
        red.zero_grad()
        np.random.seed(3)
        out = student(x)
        loss = loss_fn(out, target)
        with torch.no_grad():
            want = float(loss_fn((out[0].detach(), out[1].detach(), out[2]), rebuilt))
        loss.backward()
        red.finish()
        opt.step()
        got = float(loss.detach())
        print("TOPK %s | loss %.7f on the labeler's target, %.7f on the reference's pairs" % (case, got, want))
        assert np.isfinite(got) and abs(got - want) <= 1e-4 * abs(want)
        assert bool(torch.isfinite(opt.p).all())
    finally:
        red.remove()


# ================================================================================================================ 10. driver
def test_driver_with_a_teacher_eager_and_graphed(ops, monkeypatch, teacher24):
    """AutoProgDriver(teacher=labeler) with integer labels from get_batch, six steps at one configuration, DropPath 0, same seeds: the run
    with use_graphs (two eager steps, then replays with the labeler running eagerly in front of each) gives the eager run's losses, weights
    and EMA copies bit for bit"""
    from autoprog_amd import ops as _ops
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import SparseTokenLabelTarget, TokenLabelCrossEntropy
    from autoprog_amd.optim import FlatAdamWEma
    from autoprog_amd.prog.driver import AutoProgDriver
    from autoprog_amd.prog.teacher import TeacherLabeler
    monkeypatch.setattr(_ops, "deterministic", True)
    out = {}
    for use_graphs in (False, True):
        student = _small_volo(24, seed=4, variant="volo_h2_l6").train()
        red = GradientBucketReducer(list(student.parameters()), world_size=1, defer_mean=True)
        red.install_sink(student)
        opt = FlatAdamWEma(student, red, lr=1e-3, weight_decay=0.05, ema_decays=[0.9, 0.99])
        g = torch.Generator().manual_seed(1)
        seen = []

        def get_batch(r):
            return torch.randn(8, 3, 96, 96, generator=g).cuda(), torch.randint(0, 24, (8,), generator=g).cuda()

        def loss_fn(outputs, target, _ce=TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=24)):
            seen.append(type(target))
            return _ce(outputs, target)

        drv = AutoProgDriver(student, loss_fn, opt, red, get_batch, r_list=[64], l_list=[6], dp_list=[0.0], grow_epochs=[0], steps_per_epoch=6,
                             auto_grow=False, use_graphs=use_graphs, graph_after=2, teacher=TeacherLabeler(teacher24, k=5, num_classes=24))
        steps, real = [], drv._train_step
        monkeypatch.setattr(drv, "_train_step", lambda *a, **k: (steps.append(real(*a, **k)), steps[-1])[1])
        try:
            np.random.seed(3)
            drv.run(1)
            out[use_graphs] = ([float(s) for s in steps], opt.p.clone(), [e.clone() for e in opt.ema], len(drv._graphs))
            assert seen and all(t is SparseTokenLabelTarget for t in seen)
        finally:
            red.remove()
    le, pe, ee, _ = out[False]
    lg, pg, eg, live = out[True]
    print("TOPK driver eager:", le)
    print("TOPK driver graph:", lg)
    assert len(le) == 6 and all(np.isfinite(v) for v in le) and live == 1
    assert le == lg, (le, lg)
    assert torch.equal(pe, pg) and all(torch.equal(a, b) for a, b in zip(ee, eg))
