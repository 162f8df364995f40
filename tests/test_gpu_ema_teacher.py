"""An EMA copy of the student as a network to compute with -- and so as its own teacher (FlatAdamWEma.ema_model; the reference keeps its EMA
copies as ModelEmaV2 modules, main_prog.py:1030-1033).  The shadow module's parameters are views of the EMA slab, its bf16 weights the
slab ap_adamw_ema_step_ema16 writes in the optimizer's own pass.  The yardstick everywhere is the route that existed before: the student
itself in eval() inside `with opt.ema_weights(i)`.  Everything is bit for bit (torch.equal); small models only."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DECAYS = [0.5, 0.6, 0.7, 0.8]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ---------------------------------------------------------------------------------------------------------------------- helpers
def _volo(variant, classes=16, seed=0):
    from autoprog_amd.models import create_model
    torch.manual_seed(seed)
    return create_model("model_variant", variant=variant, num_classes=classes, img_size=64, stem_hidden_dim=64, drop_path_rate=0.0).cuda().train()


def _deit(classes=16, seed=0):
    """deit_tiny_distilled_patch16_224 at 64 px, cut to two blocks"""
    from autoprog_amd.models import create_model
    torch.manual_seed(seed)
    model = create_model("deit_tiny_distilled_patch16_224", num_classes=classes, img_size=64)
    model.blocks = torch.nn.ModuleList(list(model.blocks)[:2])
    return model.cuda().train()


def _optim(model, **kw):
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.optim import FlatAdamWEma
    red = GradientBucketReducer(list(model.parameters()), world_size=1, defer_mean=True)
    red.install_sink(model)
    return red, FlatAdamWEma(model, red, lr=2e-3, weight_decay=0.05, ema_decays=DECAYS, **kw)


def _batch(classes=16, r=64, B=4, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, r, r, generator=g).cuda()
    target = torch.softmax(torch.randn(B, classes, 2 + (r // 16) ** 2, generator=g) * 2, dim=1).cuda()
    labels = torch.randint(0, classes, (B,), generator=g).cuda()
    return x, target, labels


def _volo_step(model, red, opt, x, target, classes=16, **step_kw):
    from autoprog_amd.loss import TokenLabelCrossEntropy
    red.zero_grad()
    loss = TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=classes)(model(x), target)
    loss.backward()
    red.finish()
    opt.step(**step_kw)
    return float(loss.detach())


def _deit_step(model, red, opt, x, labels):
    red.zero_grad()
    y, yd = model(x)
    loss = torch.nn.functional.cross_entropy(y.float(), labels) + torch.nn.functional.cross_entropy(yd.float(), labels)
    loss.backward()
    red.finish()
    opt.step()
    return float(loss.detach())


def _swap_route(model, opt, i, x, dense):
    """what a user could do before: the student in eval() with the slabs of EMA copy i swapped in"""
    was = model.training
    model.eval()
    try:
        with opt.ema_weights(i), torch.no_grad():
            return model.forward_dense(x) if dense else model(x)
    finally:
        model.train(was)


def _assert_shadow(model, opt, i, x, dense=True, what=""):
    """the shadow of copy i against the swap route on x, and where its tensors live.  The shadow runs FIRST: the swap route refreshes the
    bf16 slab on its way in and out, and must not repair what the optimizer's kernel should have written."""
    from autoprog_amd import functional as AF
    shadow = opt.ema_model(i)
    assert shadow is opt.ema_model(i) and not shadow.training and shadow is not model
    assert all(not p.requires_grad and p.grad is None for p in shadow.parameters())
    assert torch.equal(opt.ema16[i].view(torch.int16), opt.ema[i].to(BF16).view(torch.int16)), "%s: ema16[%d] is not the cast of ema[%d]" % (what, i, i)
    lo = opt.ema[i].data_ptr()
    hi = lo + opt.ema[i].numel() * 4
    names = dict(model.named_parameters())
    for name, p in shadow.named_parameters():
        assert lo <= p.data_ptr() and p.data_ptr() + p.numel() * 4 <= hi, "%s lives outside ema[%d]" % (name, i)
        assert p.data_ptr() - lo == names[name].data_ptr() - opt.p.data_ptr(), "%s sits at another offset than the student's" % name
        if p.dim() >= 2:
            lo16 = opt.ema16[i].data_ptr()
            flat = p._ap_flat16
            assert flat[1].data_ptr() - lo16 == (p.data_ptr() - lo) // 2 and tuple(flat[1].shape) == (p.shape[0], p.numel() // p.shape[0]) and flat[2] is None
            assert AF.bank.get(p) is flat[1], "%s: the weight bank does not hand out the bf16 slab's view" % name
    floats = [b for b in shadow.buffers() if b.dtype.is_floating_point]
    assert len(floats) == len(opt.ema_buffers[i]) and all(a is b for a, b in zip(floats, opt.ema_buffers[i]))
    real_get_t = AF.bank.get_t

    def no_get_t(p):
        raise AssertionError("a transposed weight copy was asked for in a shadow module's forward")
    AF.bank.get_t = no_get_t
    try:
        with torch.no_grad():
            got_dense = shadow.forward_dense(x) if dense else None
            got = shadow(x)
    finally:
        AF.bank.get_t = real_get_t
    want = _swap_route(model, opt, i, x, False)
    assert torch.equal(got, want), "%s: the eval() forward of shadow %d differs from the swap route" % (what, i)
    if dense:
        want_dense = _swap_route(model, opt, i, x, True)
        assert torch.equal(got_dense[0], want_dense[0]) and torch.equal(got_dense[1], want_dense[1]), "%s: forward_dense of shadow %d" % (what, i)
    return got_dense if dense else got


# ---------------------------------------------------------------------------------------------------------------------- 1. shadow = swap
@pytest.mark.parametrize("kind", ["volo_h2_l3", "deit2"])
def test_shadow_equals_swap_route(kind):
    """three training steps with the shadows of copies 0 and 3 alive: each shadow's forward_dense and eval() forward are the student's under
    ema_weights(i), the parameters lie in ema[i], the float buffers are ema_buffers[i]'s tensors, ema16[i] is the cast of ema[i]"""
    volo = kind != "deit2"
    model = _volo(kind) if volo else _deit()
    red, opt = _optim(model)
    x, target, labels = _batch()
    try:
        first = {i: opt.ema_model(i) for i in (0, 3)}
        assert opt.ema16[1] is None and opt.ema16[2] is None and [i for i, _ in opt.live_ema_models()] == [0, 3]
        hooks = [m for m in first[0].modules() if m._load_state_dict_post_hooks or m._forward_hooks or m._backward_hooks]
        assert not hooks and model._load_state_dict_post_hooks                # the student keeps its resync hook, the shadow has none
        np.random.seed(0)
        for step in range(3):
            _volo_step(model, red, opt, x, target) if volo else _deit_step(model, red, opt, x, labels)
            for i in (0, 3):
                out = _assert_shadow(model, opt, i, x, dense=volo, what="step %d" % step)
        assert opt.ema_model(0) is first[0] and not torch.equal(opt.ema[0], opt.ema[3])
        if volo:
            assert tuple(out[1].shape[:2]) == (4, 16)
    finally:
        red.remove()


# ---------------------------------------------------------------------------------------------------------------------- 2. outside writes
def test_shadow_follows_writes_from_outside_the_kernel():
    """grow, model.load_state_dict, opt.load_state_dict from a differently stepped twin and a completed ema_weights block: after each, and
    after one more step, the shadows are the swap route"""
    from autoprog_amd.prog import elastic
    x, target, _ = _batch()
    cfg3, cfg6 = dict(layer_num=3, min_layer_num=3, max_layer_num=6), dict(layer_num=6, min_layer_num=3, max_layer_num=6)
    twin = _volo("volo_h2_l6", seed=5)                                          # (first: one gradient sink at a time)
    red2, opt2 = _optim(twin)
    try:
        twin.set_sample_config(cfg6)
        np.random.seed(1)
        for _ in range(4):
            _volo_step(twin, red2, opt2, x.flip(0), target)
        saved = opt2.state_dict()
    finally:
        red2.remove()
    del twin, red2, opt2
    model = _volo("volo_h2_l6")
    red, opt = _optim(model)
    try:
        shadows = [opt.ema_model(i) for i in (0, 3)]
        old_mask = model.set_sample_config(cfg3)
        for s in shadows:
            s.set_sample_config(cfg3)
        np.random.seed(0)
        for _ in range(2):
            _volo_step(model, red, opt, x, target)

        def check(what):
            for i in (0, 3):
                _assert_shadow(model, opt, i, x, what=what)
            _volo_step(model, red, opt, x, target)
            for i in (0, 3):
                _assert_shadow(model, opt, i, x, what=what + ", one step later")
        check("before any outside write")
        opt.grow(old_mask, elastic.make_mask(6, 3, 6))
        model.set_sample_config(cfg6)
        for s in shadows:
            s.set_sample_config(cfg6)
        check("grow")
        sd = {k: (v + 0.01 * torch.randn_like(v) if v.dtype.is_floating_point and v.dim() > 1 else v.clone()) for k, v in model.state_dict().items()}
        model.load_state_dict(sd)
        check("model.load_state_dict")
        opt.load_state_dict(saved)
        assert all(torch.equal(a, b) for a, b in zip(opt.ema, saved["ema"]))
        check("opt.load_state_dict")
        with opt.ema_weights(3):
            pass
        with opt.ema_weights(0):
            pass
        check("a completed ema_weights block")
    finally:
        red.remove()


# ---------------------------------------------------------------------------------------------------------------------- 3. elastic
def test_driver_keeps_the_shadow_at_the_students_configuration():
    """AutoProgDriver._activate(l, r, dp) at two configurations: the shadow gives [B, (r // 16)^2, C] token logits, the swap route's"""
    from autoprog_amd.loss import TokenLabelCrossEntropy
    from autoprog_amd.prog.driver import AutoProgDriver
    model = _volo("volo_h2_l6")
    red, opt = _optim(model)
    try:
        shadow = opt.ema_model(3)
        drv = AutoProgDriver(model, TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=16), opt, red, lambda r: None,
                             r_list=[64, 96], l_list=[3, 6], dp_list=[0.0, 0.0], grow_epochs=[0, 1], steps_per_epoch=1, auto_grow=False)
        np.random.seed(0)
        for l, r in ((3, 64), (6, 96)):
            drv._activate(l, r, 0.0)
            x, target, _ = _batch(r=r, seed=r)
            _volo_step(model, red, opt, x, target)
            active = [sum(not b.is_identity_layer for b in st) for st in shadow.network if isinstance(st, torch.nn.Sequential)]
            assert active == [sum(not b.is_identity_layer for b in st) for st in model.network if isinstance(st, torch.nn.Sequential)]
            assert shadow.patch_embed.resize_to == r
            x_cls, x_aux = _assert_shadow(model, opt, 3, x, what="(l, r) = (%d, %d)" % (l, r))
            assert tuple(x_aux.shape[:2]) == (4, (r // 16) ** 2) and tuple(x_cls.shape[:1]) == (4,)
            shadow.patch_embed.resize_in_eval = True                            # as a teacher runs it: a 128 px batch resized to the stage's r
            with torch.no_grad():
                assert tuple(shadow.forward_dense(torch.randn(4, 3, 128, 128, device="cuda"))[1].shape[:2]) == (4, (r // 16) ** 2)
            shadow.patch_embed.resize_in_eval = False
    finally:
        red.remove()


# ---------------------------------------------------------------------------------------------------------------------- 4. guarded steps
def test_shadow_after_a_skipped_guarded_step():
    """skip_nonfinite=True and a NaN in one gradient element: the parameters stay, the EMA copies move, the shadow is the swap route"""
    from autoprog_amd.loss import TokenLabelCrossEntropy
    model = _volo("volo_h2_l3")
    red, opt = _optim(model)
    x, target, _ = _batch()
    try:
        opt.ema_model(3)
        np.random.seed(0)
        _volo_step(model, red, opt, x, target, skip_nonfinite=True)
        _assert_shadow(model, opt, 3, x, what="applied guarded step")
        p0, e0 = opt.p.clone(), opt.ema[3].clone()
        red.zero_grad()
        TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=16)(model(x), target).backward()
        red.finish()
        red.flat[red.flat.numel() // 2] = float("nan")
        opt.step(skip_nonfinite=True)
        assert opt.guard_counts()["skipped"] == 1 and torch.equal(opt.p, p0) and not torch.equal(opt.ema[3], e0)
        _assert_shadow(model, opt, 3, x, what="skipped guarded step")
    finally:
        red.remove()


# ---------------------------------------------------------------------------------------------------------------------- 5. release
def test_release_goes_back_to_the_old_entry_point(monkeypatch):
    """after release_ema_model a step is the step of a twin optimizer that never had a shadow, and step() calls ap_adamw_ema_step again"""
    from autoprog_amd import optim as O
    x, target, _ = _batch()
    calls = []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(O_lib, name)
            if name.startswith("ap_adamw_ema_step"):
                return lambda *a: (calls.append(name), fn(*a))[1]
            return fn
    O_lib = O.lib
    monkeypatch.setattr(O, "lib", Counting())
    out = []
    for with_shadow in (False, True):
        model = _volo("volo_h2_l3")
        red, opt = _optim(model)
        try:
            np.random.seed(0)
            if with_shadow:
                opt.ema_model(1)
            _volo_step(model, red, opt, x, target)
            if with_shadow:
                assert calls[-1] == "ap_adamw_ema_step_ema16"
                opt.release_ema_model(1)
                assert opt.ema16 == [None] * 4 and not opt.live_ema_models()
                with pytest.raises(KeyError):
                    opt.release_ema_model(1)
            _volo_step(model, red, opt, x, target)
            assert calls[-1] == "ap_adamw_ema_step"
            _volo_step(model, red, opt, x, target, skip_nonfinite=True)
            assert calls[-1] == "ap_adamw_ema_step_guarded"
            out.append([opt.p.clone(), opt.m.clone(), opt.v.clone(), opt.p16.clone().view(torch.int16)] + [e.clone() for e in opt.ema])
        finally:
            red.remove()
    assert calls.count("ap_adamw_ema_step_ema16") == 1
    for name, a, b in zip(("p", "m", "v", "p16", "ema0", "ema1", "ema2", "ema3"), *out):
        assert torch.equal(a, b), name


def test_first_call_is_refused_during_capture(monkeypatch):
    """(the capture is pretended: the refusal must come before anything is allocated or launched)"""
    model = _volo("volo_h2_l3")
    red, opt = _optim(model)
    try:
        first = opt.ema_model(0)
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        assert opt.ema_model(0) is first                                        # an existing shadow is simply returned
        with pytest.raises(RuntimeError, match="captured"):
            opt.ema_model(1)
        assert opt.ema16[1] is None and [i for i, _ in opt.live_ema_models()] == [0]
    finally:
        red.remove()


# ---------------------------------------------------------------------------------------------------------------------- 6. self-taught runs
def _self_taught(use_graphs, monkeypatch, intercept=None):
    from autoprog_amd.loss import TokenLabelGTCrossEntropy
    from autoprog_amd.prog.driver import AutoProgDriver
    from autoprog_amd.prog.teacher import TeacherLabeler
    model = _volo("volo_h2_l6", classes=24, seed=4)
    red, opt = _optim(model)
    g = torch.Generator().manual_seed(1)
    batches, targets = [], []

    def get_batch(r):
        batches.append((torch.randn(4, 3, 96, 96, generator=g).cuda(), torch.randint(0, 24, (4,), generator=g).cuda()))
        return batches[-1]
    labeler = TeacherLabeler(opt.ema_model(3), k=5, num_classes=24)
    if intercept is not None:
        class Watching(TeacherLabeler):
            def __call__(self, images, labels, r):
                if len(batches) == intercept:                                   # the swap route FIRST: it leaves the slabs as it found them
                    want = _swap_dense_at(model, opt, 3, images, r)
                out = TeacherLabeler.__call__(self, images, labels, r)
                if len(batches) == intercept:
                    targets.append((out.idx.clone(), out.val.clone(), want, labels, r))
                return out
        labeler.__class__ = Watching
    drv = AutoProgDriver(model, TokenLabelGTCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=24), opt, red, get_batch, r_list=[64, 96],
                         l_list=[3, 6], dp_list=[0.0, 0.0], grow_epochs=[0, 1], steps_per_epoch=3, auto_grow=False, use_graphs=use_graphs,
                         graph_after=1, teacher=labeler)
    steps, real_step = [], drv._train_step
    monkeypatch.setattr(drv, "_train_step", lambda *a, **k: (steps.append(real_step(*a, **k)), steps[-1])[1])
    try:
        np.random.seed(3)
        hist = drv.run(2)
        return [float(s) for s in steps], hist, targets, opt.p.clone()
    finally:
        red.remove()


def _swap_dense_at(model, opt, i, images, r):
    """the swap route's logits on a batch resized to r, as a teacher resizes it"""
    pe = model.patch_embed
    keep = (pe.resize_to, pe.resize_in_eval)
    pe.resize_to, pe.resize_in_eval = int(r), True
    try:
        return _swap_route(model, opt, i, images, True)
    finally:
        pe.resize_to, pe.resize_in_eval = keep


def test_self_taught_two_stages_eager_and_graphed(monkeypatch):
    """volo_h2_l6 taught by its own EMA copy 3 through the driver, stages (l 3, r 64) -> (l 6, r 96), three steps each, DropPath 0: finite
    losses, the target of the fifth step is from_logits of the swap route's logits on that batch, and the graphed run (graph_after=1)
    reads the eager run's losses digit for digit"""
    from autoprog_amd import ops
    from autoprog_amd.loss import SparseTokenLabelTarget
    monkeypatch.setattr(ops, "deterministic", True)
    eager, hist, targets, p_eager = _self_taught(False, monkeypatch, intercept=5)
    print("EMA teacher eager:", eager)
    assert len(eager) == 6 and all(np.isfinite(v) for v in eager) and len(set(eager)) == 6
    assert [(h["l"], h["r"]) for h in hist] == [(3, 64), (6, 96)]
    (idx, val, (w_cls, w_aux), labels, r), = targets
    want = SparseTokenLabelTarget.from_logits(labels, w_cls, w_aux, 5, 1.0, 0.1)
    assert r == 96 and tuple(idx.shape) == (4, 2 + 36, 5)
    assert torch.equal(idx, want.idx) and torch.equal(val, want.val)
    graphed, _, _, p_graphed = _self_taught(True, monkeypatch)
    print("EMA teacher graph:", graphed)
    assert graphed == eager, (eager, graphed)
    assert torch.equal(p_eager, p_graphed)


def _deit_driver(teacher_of, batch_prep=None, seen=None, uint8=False):
    from autoprog_amd.loss import DistillationLoss, SoftTargetCrossEntropy
    from autoprog_amd.prog.driver import AutoProgDriver
    model = _deit()
    red, opt = _optim(model)
    g = torch.Generator().manual_seed(2)
    dl = DistillationLoss(SoftTargetCrossEntropy(), "soft", alpha=0.5, tau=3.0)
    steps = []

    def get_batch(r):
        labels = torch.randint(0, 16, (6,), generator=g).cuda()
        if uint8:
            return torch.randint(0, 256, (6, 3, r, r), dtype=torch.uint8, generator=g).cuda(), labels
        return torch.randn(6, 3, r, r, generator=g).cuda(), labels

    def loss_fn(outputs, target):
        if seen is not None:
            seen.append(target)
        loss = dl(outputs, target)
        steps.append(loss.detach())
        return loss
    drv = AutoProgDriver(model, loss_fn, opt, red, get_batch, r_list=[64], l_list=[2], dp_list=[0.0], grow_epochs=[0], steps_per_epoch=3,
                         auto_grow=False, teacher=teacher_of(opt), batch_prep=batch_prep)
    return drv, red, steps


def test_distilled_deit_taught_by_its_ema_copy():
    from autoprog_amd.loss import DistillTarget
    from autoprog_amd.prog.teacher import TeacherLogits
    seen = []
    drv, red, steps = _deit_driver(lambda opt: TeacherLogits(opt.ema_model(0), num_classes=16), seen=seen)
    try:
        drv.run(1)
        losses = [float(s) for s in steps]
        print("EMA teacher DeiT:", losses)
        assert len(losses) == 3 and all(np.isfinite(v) for v in losses) and len(set(losses)) == 3
        assert all(isinstance(t, DistillTarget) for t in seen)
    finally:
        red.remove()


# ---------------------------------------------------------------------------------------------------------------------- 7. TeacherLogits + CutMix
def test_teacher_logits_beside_cutmix_through_the_driver():
    """the driver accepts TeacherLogits beside DeviceBatchPrep(cutmix_alpha=1.0) and runs three steps; the DistillTarget's base is the
    batch's MixedLabelTarget"""
    from autoprog_amd.data import DeviceBatchPrep, MixedLabelTarget
    from autoprog_amd.loss import DistillTarget
    from autoprog_amd.prog.teacher import TeacherLogits
    seen = []
    prep = DeviceBatchPrep(MEAN, STD, cutmix_alpha=1.0, num_classes=16, seed=4)
    drv, red, steps = _deit_driver(lambda opt: TeacherLogits(opt.ema_model(0), num_classes=16), batch_prep=prep, seen=seen, uint8=True)
    try:
        drv.run(1)
        losses = [float(s) for s in steps]
        assert len(losses) == 3 and all(np.isfinite(v) for v in losses)
        assert len(seen) == 3 and all(isinstance(t, DistillTarget) and isinstance(t.base, MixedLabelTarget) for t in seen)
        assert any(0.0 < t.base.lam < 1.0 for t in seen)
    finally:
        red.remove()
