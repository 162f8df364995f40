"""The Python in front of the loss kernels (autoprog_amd/functional.py: SoftTargetCEFn, TokenLabelCEFn, SparseTokenLabelCEFn,
SparseTokenLabelGTCEFn, MixedLabelCEFn, DistillCEFn), pinned call for call.  A recorder stands in for ops.lib and notes, for every library
call of one forward + backward, the entry point, every integer and float argument and, for every pointer, whether it lies in one of the
caller's tensors (its name and the byte offset from that tensor's first element) or in memory the Function allocated ("fresh"); the
record is compared with the one written out here.  The loss and the gradients (values, shape and strides) are compared bit for bit
with the same launches composed by hand from ops.*.

  class counts  16 (ld == C: the rows go to the library as they are), 20 (copied into rows of 24), 1032 (past 64 * 2 * CE_MAXV: the wide
                kernels, as they are), 1100 (wide, rows of 1104)
  sizes         B = 4, N = 6, K = 3: a batch is no whole 16-token tile and the mix partner B-1-b is never b
  lam           host 1.0 (nothing blended), host 0.625 (exact in fp32), and 0.625 in device memory behind an object with `lam_ptr`, which
                must give the host case's bits
  padded views  what functional.linear returns at C = 20 (row stride 24): the CE Functions copy it (the CE wrappers of ops take contiguous
                rows only); the distillation teacher and the logits of SparseTokenLabelTarget.from_logits go to the library in place"""
import ctypes
from contextlib import contextmanager

import pytest
import torch

pytestmark = pytest.mark.gpu
B, N, K = 4, 6, 3
BF16 = torch.bfloat16
WIDTHS = [16, 20, 1032, 1100]
FORMS = [(C, False) for C in WIDTHS] + [(20, True)]          # (class count, logits handed over as a padded view)
FRESH = "fresh"
SMOOTHING, CLS_W, DENSE_W = 0.1, 0.75, 0.5
S = (2 + N) * K                                              # pair elements per image
LAMS = ["host 1.0", "host 0.625", "device 0.625"]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from autoprog_amd import ops as _ops
    return _ops


def round_up(v, m):
    return (v + m - 1) // m * m


class Recorder:
    """ops.lib for the length of one `recording`: every call goes on to the library and is noted without its last argument (the stream)"""

    def __init__(self, lib, named):
        self._lib, self._named, self.calls = lib, named, []

    def _pointer(self, p):
        if p is None:
            return None
        for name, t in self._named.items():
            st = t.untyped_storage()
            if st.data_ptr() <= p < st.data_ptr() + st.nbytes():
                return (name, p - t.data_ptr())
        return FRESH

    def __getattr__(self, entry):
        fn = getattr(self._lib, entry)

        def call(*args):
            assert len(args) == len(fn.argtypes), entry
            self.calls.append((entry, tuple(self._pointer(a) if ty is ctypes.c_void_p else a for a, ty in zip(args[:-1], fn.argtypes))))
            return fn(*args)
        return call


@contextmanager
def recording(ops, named):
    rec, real = Recorder(ops.lib, named), ops.lib
    ops.lib = rec
    try:
        yield rec
    finally:
        ops.lib = real


def check_record(got, want):
    assert len(got) == len(want), "library calls: %s, expected %s" % ([c[0] for c in got], [c[0] for c in want])
    for i, ((g_entry, g_args), (w_entry, w_args)) in enumerate(zip(got, want)):
        assert g_entry == w_entry, "call %d is %s, expected %s" % (i, g_entry, w_entry)
        assert len(g_args) == len(w_args), (g_entry, g_args, w_args)
        for j, (a, w) in enumerate(zip(g_args, w_args)):
            assert type(a) is type(w) and a == w, "call %d (%s) argument %d: %r, expected %r" % (i, g_entry, j, a, w)


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def same_tensor(got, want, what):
    assert got.shape == want.shape and got.stride() == want.stride(), "%s: shape %s strides %s, by hand %s %s" % (
        what, tuple(got.shape), got.stride(), tuple(want.shape), want.stride())
    assert bits_equal(got, want), "%s differs from the launches composed by hand" % what


def make_logits(shape, C, view, seed):
    """bf16 logits [*shape, C] on the GPU, a leaf: contiguous, or the first C columns of rows of round_up(C, 8) (functional.linear's output)"""
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(*shape, C, generator=gen) * 2).to(BF16)
    if view:
        buf = torch.zeros(*shape, round_up(C, 8), dtype=BF16)
        buf[..., :C] = x
        x = buf.cuda()[..., :C]
        assert not x.is_contiguous()
    else:
        x = x.cuda()
    return x.requires_grad_()


def make_pairs(C, seed):
    gen = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, C, (B, 2 + N, K), generator=gen).to(torch.int32)
    val = torch.rand(B, 2 + N, K, generator=gen) + 0.05
    return idx.cuda(), val.cuda()


class DeviceLam:
    """what graph.StepScalars and data.MixedLabelTarget are to the loss: an object whose `lam_ptr` is the device address of lam"""

    def __init__(self, word):
        self.word = word

    @property
    def lam_ptr(self):
        return self.word.data_ptr()


def lam_cases(word):
    """name -> (the lam a Function is given, the (mix_lam, mix_batches, mix_lam_ptr) its class-row launch takes, the pointer's record)"""
    return {"host 1.0": (1.0, (1.0, 0, None), None),
            "host 0.625": (0.625, (0.625, B, None), None),
            "device 0.625": (DeviceLam(word), (1.0, B, word.data_ptr()), ("lam_word", 0))}


def ce_rows(x2d, C):
    """the rows a CE wrapper of ops is given: as they are when contiguous with ld == C, else a zero-filled copy [M, round_up(C, 8)]"""
    ld = round_up(C, 8)
    if ld == C and x2d.is_contiguous():
        return x2d
    xp = torch.zeros((x2d.shape[0], ld), dtype=BF16, device=x2d.device)
    xp[:, :C] = x2d
    return xp


def scaled(ops, d, g, C):
    out = ops.row_scale(d, g.reshape(1), d.shape[0])
    return out if out.shape[1] == C else out[:, :C]


def grad_scalar():
    return torch.tensor(0.5, dtype=torch.float32, device="cuda")


def row_scale_record(rows, ld):
    return ("ap_row_scale", (FRESH, ("g", 0), FRESH, rows, ld, rows))


# ================================================================================================================ the three token-label losses
def _token_label_case(ops, kind, C, view):
    from autoprog_amd import functional as AF
    ld = round_up(C, 8)
    copied = ld != C or view
    x_cls, x_aux = make_logits((B,), C, view, 1), make_logits((B, N), C, view, 2)
    word = torch.tensor([0.625], dtype=torch.float32, device="cuda")
    g = grad_scalar()
    named = {"x_cls": x_cls, "x_aux": x_aux, "lam_word": word, "g": g}
    if kind == "dense":
        target = torch.softmax(torch.randn(B, C, 2 + N, generator=torch.Generator().manual_seed(3)), dim=1).cuda()
        named["target"] = target
        sb, sc, sn = target.stride()
    else:
        idx, val = make_pairs(C, 3)
        named["idx"], named["val"] = idx, val
    p_cls = FRESH if copied else ("x_cls", 0)
    p_aux = FRESH if copied else ("x_aux", 0)
    gs_cls, gs_aux = CLS_W / B, DENSE_W / (B * N)
    results = {}
    for name, (lam, (mix_lam, mix_batches, mix_ptr), ptr_rec) in lam_cases(word).items():
        with recording(ops, named) as rec:
            if kind == "dense":
                loss = AF.TokenLabelCEFn.apply(x_cls, x_aux, target, lam, CLS_W, DENSE_W)
            elif kind == "sparse":
                loss = AF.SparseTokenLabelCEFn.apply(x_cls, x_aux, idx, val, SMOOTHING, lam, CLS_W, DENSE_W)
            else:
                loss = AF.SparseTokenLabelGTCEFn.apply(x_cls, x_aux, idx, val, SMOOTHING, lam, CLS_W, DENSE_W)
            d_cls, d_aux = torch.autograd.grad(loss, [x_cls, x_aux], g)
        mix = (mix_lam, mix_batches, ptr_rec)
        if kind == "dense":
            want = [("ap_soft_ce_fwd_bwd_dev", (p_aux, ld, ("target", 8), sb, sc, sn, N, FRESH, FRESH, gs_aux, B * N, C, 1.0, 0, None)),
                    ("ap_soft_ce_fwd_bwd_dev", (p_cls, ld, ("target", 4), sb, sc, 0, 1, FRESH, FRESH, gs_cls, B, C) + mix)]
        else:
            want = [("ap_soft_ce_sparse_fwd_bwd_dev", (p_aux, ld, ("idx", 8 * K), ("val", 8 * K), K, S, K, N, SMOOTHING, FRESH, FRESH, gs_aux,
                                                       B * N, C, 1.0, 0, None))]
            if kind == "sparse":        # slot 1 of every image, in place
                want.append(("ap_soft_ce_sparse_fwd_bwd_dev", (p_cls, ld, ("idx", 4 * K), ("val", 4 * K), K, S, 0, 1, SMOOTHING, FRESH, FRESH,
                                                               gs_cls, B, C) + mix))
            else:                       # slot 0 at offset 0 and slot 1 at offset K of every image, in place
                want.append(("ap_soft_ce_sparse_gt_fwd_bwd", (p_cls, ld, ("idx", 0), ("val", 0), K, S, 0, K, SMOOTHING, FRESH, FRESH, gs_cls,
                                                              B, C) + mix))
        want += [("ap_loss_combine", (FRESH, B, gs_cls, FRESH, B * N, gs_aux, FRESH)), row_scale_record(B, ld), row_scale_record(B * N, ld)]
        check_record(rec.calls, want)

        # the same launches by hand
        aux2d, cls2d = ce_rows(x_aux.detach().reshape(B * N, C), C), ce_rows(x_cls.detach().reshape(B, C), C)
        kw = dict(mix_lam=mix_lam, mix_batches=mix_batches, mix_lam_ptr=mix_ptr)
        if kind == "dense":
            rl_aux, h_aux = ops.soft_ce_fwd_bwd(aux2d, C, target[:, :, 2:], sb, sc, sn, N, gs_aux)
            rl_cls, h_cls = ops.soft_ce_fwd_bwd(cls2d, C, target[:, :, 1], sb, sc, 0, 1, gs_cls, **kw)
        else:
            rl_aux, h_aux = ops.soft_ce_sparse_fwd_bwd(aux2d, C, idx[:, 2:], val[:, 2:], S, K, N, SMOOTHING, gs_aux)
            if kind == "sparse":
                rl_cls, h_cls = ops.soft_ce_sparse_fwd_bwd(cls2d, C, idx[:, 1], val[:, 1], S, 0, 1, SMOOTHING, gs_cls, **kw)
            else:
                rl_cls, h_cls = ops.soft_ce_sparse_gt_fwd_bwd(cls2d, C, idx, val, S, 0, K, SMOOTHING, gs_cls, **kw)
        h_loss = ops.loss_combine(rl_cls, gs_cls, rl_aux, gs_aux)
        h_dc, h_da = scaled(ops, h_cls, g, C), scaled(ops, h_aux, g, C).reshape(B, N, C)
        assert h_dc.stride() == (ld, 1) and h_da.stride() == (N * ld, ld, 1)
        same_tensor(loss.detach(), h_loss, "%s: loss" % name)
        same_tensor(d_cls, h_dc, "%s: d x_cls" % name)
        same_tensor(d_aux, h_da, "%s: d x_aux" % name)
        assert bool(torch.isfinite(loss)) and float(d_cls.float().abs().max()) > 0 and float(d_aux.float().abs().max()) > 0
        results[name] = (loss.detach(), d_cls, d_aux)
    for a, b in zip(results["device 0.625"], results["host 0.625"]):
        assert bits_equal(a, b), "lam from device memory and the same lam from the host differ"
    assert not bits_equal(results["host 1.0"][1], results["host 0.625"][1])             # (the blend does reach the class rows)


@pytest.mark.parametrize("C,view", FORMS)
def test_token_label_ce(ops, C, view):
    _token_label_case(ops, "dense", C, view)


@pytest.mark.parametrize("C,view", FORMS)
def test_sparse_token_label_ce(ops, C, view):
    _token_label_case(ops, "sparse", C, view)


@pytest.mark.parametrize("C,view", FORMS)
def test_sparse_token_label_gt_ce(ops, C, view):
    _token_label_case(ops, "gt", C, view)


# ================================================================================================================ the one-tensor losses
@pytest.mark.parametrize("C,view", FORMS)
def test_soft_target_ce(ops, C, view):
    from autoprog_amd import functional as AF
    ld, M = round_up(C, 8), B * N
    x = make_logits((M,), C, view, 4)
    target = torch.softmax(torch.randn(B, C, 2 + N, generator=torch.Generator().manual_seed(5)), dim=1).cuda()
    g = grad_scalar()
    sb, sc, sn = target.stride()
    with recording(ops, {"x": x, "target": target, "g": g}) as rec:
        loss = AF.SoftTargetCEFn.apply(x, target[:, :, 2:], sb, sc, sn, N)
        (dx,) = torch.autograd.grad(loss, [x], g)
    p_x = FRESH if (ld != C or view) else ("x", 0)
    check_record(rec.calls, [("ap_soft_ce_fwd_bwd_dev", (p_x, ld, ("target", 8), sb, sc, sn, N, FRESH, FRESH, 1.0 / M, M, C, 1.0, 0, None)),
                             row_scale_record(M, ld)])
    rl, h = ops.soft_ce_fwd_bwd(ce_rows(x.detach(), C), C, target[:, :, 2:], sb, sc, sn, N, 1.0 / M)
    h_dx = scaled(ops, h, g, C)
    assert h_dx.stride() == (ld, 1)
    same_tensor(loss.detach(), rl.mean(), "loss")
    same_tensor(dx, h_dx, "d logits")
    assert bool(torch.isfinite(loss)) and float(dx.float().abs().max()) > 0


@pytest.mark.parametrize("C,view", FORMS)
def test_mixed_label_ce(ops, C, view):
    from autoprog_amd import functional as AF
    ld = round_up(C, 8)
    x = make_logits((B,), C, view, 6)
    labels = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(7)).to(torch.int32).cuda()
    ones = torch.ones(B, dtype=torch.float32, device="cuda")
    word = torch.tensor([0.625], dtype=torch.float32, device="cuda")
    g = grad_scalar()
    p_x = FRESH if (ld != C or view) else ("x", 0)
    results = {}
    for name, (lam, (mix_lam, mix_batches, mix_ptr), ptr_rec) in lam_cases(word).items():
        with recording(ops, {"x": x, "labels": labels, "ones": ones, "lam_word": word, "g": g}) as rec:
            loss = AF.MixedLabelCEFn.apply(x, labels, ones, SMOOTHING, lam)
            (dx,) = torch.autograd.grad(loss, [x], g)
        check_record(rec.calls, [("ap_soft_ce_sparse_fwd_bwd_dev", (p_x, ld, ("labels", 0), ("ones", 0), 1, 1, 0, 1, SMOOTHING, FRESH, FRESH, 1.0 / B,
                                                                    B, C, mix_lam, mix_batches, ptr_rec)),
                                 row_scale_record(B, ld)])
        rl, h = ops.soft_ce_sparse_fwd_bwd(ce_rows(x.detach(), C), C, labels.view(B, 1), ones.view(B, 1), 1, 0, 1, SMOOTHING, 1.0 / B,
                                           mix_lam=mix_lam, mix_batches=mix_batches, mix_lam_ptr=mix_ptr)
        h_dx = scaled(ops, h, g, C)
        assert h_dx.stride() == (ld, 1)
        same_tensor(loss.detach(), rl.mean(), "%s: loss" % name)
        same_tensor(dx, h_dx, "%s: d logits" % name)
        assert bool(torch.isfinite(loss)) and float(dx.float().abs().max()) > 0
        results[name] = (loss.detach(), dx)
    for a, b in zip(results["device 0.625"], results["host 0.625"]):
        assert bits_equal(a, b), "lam from device memory and the same lam from the host differ"
    assert not bits_equal(results["host 1.0"][1], results["host 0.625"][1])


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("C,view", FORMS)
def test_distill_ce(ops, C, view, mode, with_base):
    """the student rows follow the CE rule (copied unless contiguous with ld == C); the teacher rows follow the other one: a padded view is
    read in place, anything else that is no aligned padded view (contiguous rows of 20 or 1100 columns) is copied"""
    from autoprog_amd import functional as AF
    ld, M = round_up(C, 8), B * N
    student = make_logits((M,), C, view, 8)
    teacher = make_logits((M,), C, view, 9).detach()
    base = torch.tensor(1.25, dtype=torch.float32, device="cuda", requires_grad=True) if with_base else None
    inv_temp, weight, base_weight = (0.5, 0.3 * 4.0 / M, 0.7) if mode == 0 else (1.0, 0.3 / M, 0.7)
    g = grad_scalar()
    named = {"student": student, "teacher": teacher, "g": g}
    if with_base:
        named["base"] = base
    with recording(ops, named) as rec:
        loss = AF.DistillCEFn.apply(student, teacher, mode, inv_temp, weight, base, base_weight)
        grads = torch.autograd.grad(loss, [student, base] if with_base else [student], g)
    p_s = FRESH if (ld != C or view) else ("student", 0)
    p_t = FRESH if (ld != C and not view) else ("teacher", 0)
    combine = (("base", 0), 1, base_weight, FRESH, M, weight, FRESH) if with_base else (FRESH, M, weight, None, 0, 0.0, FRESH)
    check_record(rec.calls, [("ap_distill_fwd_bwd", (p_s, ld, p_t, ld, C, mode, inv_temp, FRESH, FRESH, weight, M)),
                             ("ap_loss_combine", combine), row_scale_record(M, ld)])
    tp = teacher
    if ld != C and not view:
        tp = torch.zeros((M, ld), dtype=BF16, device="cuda")
        tp[:, :C] = teacher
        tp = tp[:, :C]
    rl, h = ops.distill_fwd_bwd(ce_rows(student.detach(), C), C, tp, mode, inv_temp, weight)
    h_loss = ops.loss_combine(base.detach().reshape(1), base_weight, rl, weight) if with_base else ops.loss_combine(rl, weight)
    h_ds = scaled(ops, h, g, C)
    assert h_ds.stride() == (ld, 1)
    same_tensor(loss.detach(), h_loss, "loss")
    same_tensor(grads[0], h_ds, "d student")
    if with_base:
        same_tensor(grads[1], g * base_weight, "d base")
    assert bool(torch.isfinite(loss)) and float(grads[0].float().abs().max()) > 0


# ================================================================================================================ the aligned-view rule
@pytest.mark.parametrize("view", [True, False])
def test_teacher_logits_reach_top_k_in_place(ops, view):
    """SparseTokenLabelTarget.from_logits at C = 20: a padded view (row stride 24) goes to ap_softmax_topk_rows as the caller's own storage;
    contiguous rows of 20 columns are no padded view and are copied into rows of 24"""
    from autoprog_amd.loss.cross_entropy import SparseTokenLabelTarget
    C, ld = 20, 24
    cls_logits, aux_logits = make_logits((B,), C, view, 10).detach(), make_logits((B, N), C, view, 11).detach()
    labels = torch.arange(B, device="cuda")
    out = SparseTokenLabelTarget(torch.zeros((B, 2 + N, K), dtype=torch.int32, device="cuda"), torch.zeros((B, 2 + N, K), device="cuda"))
    named = {"cls_logits": cls_logits, "aux_logits": aux_logits, "out_idx": out.idx, "out_val": out.val}
    with recording(ops, named) as rec:
        got = SparseTokenLabelTarget.from_logits(labels, cls_logits, aux_logits, k=K, temperature=2.0, out=out)
    assert got is out
    p_cls, p_aux = (("cls_logits", 0), ("aux_logits", 0)) if view else (FRESH, FRESH)
    check_record(rec.calls, [("ap_softmax_topk_rows", (p_aux, ld, C, K, 0.5, ("out_idx", 8 * K), ("out_val", 8 * K), S, K, N, B * N)),
                             ("ap_softmax_topk_rows", (p_cls, ld, C, K, 0.5, ("out_idx", 4 * K), ("out_val", 4 * K), S, 0, 1, B))])

    def rows(x2d):
        if view:
            return x2d
        xp = torch.zeros((x2d.shape[0], ld), dtype=BF16, device="cuda")
        xp[:, :C] = x2d
        return xp[:, :C]
    h_idx = torch.zeros((B, 2 + N, K), dtype=torch.int32, device="cuda")
    h_val = torch.zeros((B, 2 + N, K), device="cuda")
    ops.softmax_topk(rows(aux_logits.reshape(B * N, C)), C, K, 0.5, h_idx.view(-1)[2 * K:], h_val.view(-1)[2 * K:], S, K, N)
    ops.softmax_topk(rows(cls_logits), C, K, 0.5, h_idx.view(-1)[K:], h_val.view(-1)[K:], S, 0, 1)
    assert bits_equal(out.idx[:, 1:], h_idx[:, 1:]) and bits_equal(out.val[:, 1:], h_val[:, 1:])
    assert int(out.idx[:, 1:].min()) >= 0 and int(out.idx[:, 1:].max()) < C and float(out.val[:, 1:].min()) > 0
