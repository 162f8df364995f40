"""Per-group learning rates and weight decays in the fused AdamW + EMA step (ap_adamw_ema_step_groups; FlatAdamWEma(param_groups=),
optim.layer_decay_param_groups).  Yardsticks: the launch without a group table, bit for bit, wherever it can express the groups;
torch.optim.AdamW with groups at the tolerance tests/test_gpu_optim.py::test_gradient_clipping_inside_the_flat_slab_step uses for the same
kernel, oracle, step count and largest rate; a torch restatement of the kernel's formula for the later trips of the grid-capped loop; the
eager step for a step replayed from a graph."""
import copy
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR, WD = 1e-2, 0.05


class _Net(torch.nn.Module):
    def __init__(self, extra):
        super().__init__()
        self.body = torch.nn.Sequential(torch.nn.Linear(24, 32), torch.nn.GELU(), torch.nn.Linear(32, 16))
        self.extra = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(k) * 0.1) for k in extra])

    def forward(self, x):
        return self.body(x)


def _net(extra):
    """the net of the clipping test plus 1-D parameters of the given lengths, registered behind it.  The slab holds the parameters in
    REVERSED order, so the extras come first and every tensor behind an odd one starts inside a float4"""
    torch.manual_seed(0)
    return _Net(extra).cuda()


def _loss(net, x):
    out = net(x).pow(2).mean()
    for n, p in net.named_parameters():
        if n.startswith("extra"):
            out = out + p.pow(2).sum()
    return out


def _grads(net, red, step, world=4):
    """the gradients of the clipping test: the slab as an all-reduce over `world` ranks leaves it (the SUM), the mean deferred to the update"""
    torch.manual_seed(10 + step)
    x = torch.randn(8, 24, device="cuda")
    red.zero_grad()
    (_loss(net, x) * world).backward()
    red._pending_scale = 1.0 / world
    return x


def _optimizer(net, groups=None, ema=(0.9, 0.99), **kw):
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.optim import FlatAdamWEma
    red = GradientBucketReducer(list(net.parameters()), world_size=1, defer_mean=True)
    return red, FlatAdamWEma(net, red, lr=LR, weight_decay=WD, ema_decays=list(ema), param_groups=groups, **kw)


def _two_groups(net, **kw):
    """the default groups, written out: decayed, then un-decayed parameters"""
    named = list(net.named_parameters())
    return [dict(params=[p for n, p in named if p.dim() > 1], weight_decay=WD, **kw), dict(params=[p for n, p in named if p.dim() <= 1], weight_decay=0.0, **kw)]


def _state(opt):
    out = {"p": opt.p, "m": opt.m, "v": opt.v, "p16": opt.p16, "p16_t": opt.p16_t}
    out.update(("ema%d" % i, e) for i, e in enumerate(opt.ema))
    out.update(("ema16_%d" % i, e) for i, e in enumerate(opt.ema16) if e is not None)
    return out


def _assert_same_state(a, b, what):
    sa, sb = _state(a), _state(b)
    assert set(sa) == set(sb)
    for k in sa:
        assert torch.equal(sa[k].view(torch.int16 if sa[k].dtype == torch.bfloat16 else torch.int32),
                           sb[k].view(torch.int16 if sb[k].dtype == torch.bfloat16 else torch.int32)), (what, k)


@pytest.mark.parametrize("shadow", [False, True], ids=["no_shadow", "ema_model"])
@pytest.mark.parametrize("guard", [False, True], ids=["unguarded", "skip_nonfinite"])
@pytest.mark.parametrize("clip", [None, ("norm", 0.05), ("value", 0.01)], ids=["noclip", "norm", "value"])
def test_grouped_launch_restating_the_default_groups_is_the_default_launch_bit_for_bit(clip, guard, shadow):
    """one optimizer built the way it always was, one with the same two groups given explicitly (which always takes
    ap_adamw_ema_step_groups): p, m, v, p16, the transposed copies, both EMA slabs -- and the bf16 copy of EMA slab 1 while it is a
    network -- are equal after each of three steps on the same gradient slab.  The 5-element parameter puts every group boundary inside
    a float4 and makes the slab 1333 long (the padded-copy route).  With the guard the second step's gradient carries an inf: both skip."""
    net_a = _net((5,))
    net_b = copy.deepcopy(net_a)
    red_a, opt_a = _optimizer(net_a)
    red_b, opt_b = _optimizer(net_b, _two_groups(net_b))
    assert opt_a.grouped is False and opt_b.grouped is True and opt_a.n_pad == 1336 and opt_a.g is None
    assert [len(g["params"]) for g in opt_a.param_groups] == [len(g["params"]) for g in opt_b.param_groups] == [2, 3]
    if shadow:
        opt_a.ema_model(1), opt_b.ema_model(1)
    kw = dict(clip_grad=clip[1], clip_mode=clip[0]) if clip else {}
    for step in range(3):
        _grads(net_a, red_a, step)
        if guard and step == 1:
            red_a.flat[7] = float("inf")
        red_b.flat.copy_(red_a.flat)
        red_b._pending_scale = red_a._pending_scale
        before = opt_a.p.clone()
        opt_a.step(skip_nonfinite=guard, **kw)
        opt_b.step(skip_nonfinite=guard, **kw)
        _assert_same_state(opt_a, opt_b, step)
        assert torch.equal(opt_a.p, before) == (guard and step == 1)            # the step with the inf, and only that one, was skipped
    if guard:
        assert opt_a.guard_counts() == opt_b.guard_counts() == {"applied": 2, "skipped": 1, "consecutive": 0}
    ids = opt_b.group_id.cpu()
    assert ids.numel() == 1336 and ids[:5].eq(1).all() and ids[5:21].eq(1).all() and ids[21:533].eq(0).all() and ids[1333:].eq(0).all()
    assert opt_a.group_id is None                                               # allocated only where the grouped launch runs


def _oracle(ref, groups):
    """torch.optim.AdamW on the twin network: groups = [(names, lr, weight_decay)]"""
    named = dict(ref.named_parameters())
    return torch.optim.AdamW([{"params": [named[n] for n in names], "lr": lr, "weight_decay": wd} for names, lr, wd in groups], lr=LR)


def _against_oracle(net, ref, red, opt, ropt, steps=3, watch=None):
    """-> for the parameter named `watch`: (largest element of its mean gradient, largest difference between the optimizer's mean gradient
    and the oracle's own) over the steps -- the two networks' weights agree to the bound below, not bit for bit, so neither do their
    gradients"""
    gmax = gdiff = 0.0
    ref_named = dict(ref.named_parameters())
    for step in range(steps):
        x = _grads(net, red, step)
        ropt.zero_grad()
        _loss(ref, x).backward()
        if watch is not None:
            mine = dict(net.named_parameters())[watch].grad * red._pending_scale
            gmax = max(gmax, float(mine.abs().max()))
            gdiff = max(gdiff, float((mine - ref_named[watch].grad).abs().max()))
        ropt.step()
        opt.step()
        for (n, p), q in zip(net.named_parameters(), ref.parameters()):
            assert torch.allclose(p.detach(), q.detach(), atol=2e-6, rtol=1e-5), (step, n, float((p - q).abs().max()))
    return gmax, gdiff


def test_four_groups_against_torch_adamw():
    """four groups with their own rate and decay, one of them frozen by lr = 0, three steps on the clipping test's gradients with the
    deferred mean of world = 4 pending.  Slab (reversed parameter order): extra.2 [0, 2) extra.1 [2, 3) extra.0 [3, 9) body.2.bias [9, 25)
    body.2.weight [25, 537) body.0.bias [537, 569) body.0.weight [569, 1337): float4 0 holds THREE groups (1, 1, 2, 0), the float4s at 8, 24, 536 and 568
    two each."""
    net = _net((6, 1, 2))
    ref = copy.deepcopy(net)
    assign = [(["extra.0", "body.2.weight"], 1e-2, 0.05), (["extra.2", "body.0.bias"], 3e-3, 0.0), (["extra.1", "body.0.weight"], 1e-3, 0.2), (["body.2.bias"], 0.0, 0.05)]
    named = dict(net.named_parameters())
    red, opt = _optimizer(net, [{"params": [named[n] for n in names], "lr": lr, "weight_decay": wd} for names, lr, wd in assign])
    ropt = _oracle(ref, assign)
    start = {n: p.detach().clone() for n, p in net.named_parameters()}
    gmax, gdiff = _against_oracle(net, ref, red, opt, ropt, watch="body.2.bias")
    ids = opt.group_id.cpu().tolist()
    assert ids[:4] == [1, 1, 2, 0] and ids[8:12] == [0, 3, 3, 3] and ids[24:28] == [3, 0, 0, 0] and ids[536:540] == [0, 1, 1, 1] and ids[568:572] == [1, 2, 2, 2]
    assert ids[1337:] == [0, 0, 0]                                               # the tail padding: group 0
    # the frozen group: its weights never moved, its moments did -- as the oracle's.  The oracle's gradients are its own network's and
    # differ from the slab's by up to `gdiff` per element (measured above, on the inputs).  m is a convex combination of the gradients
    # (weights (1 - b1) b1^k, sum < 1): it inherits at most gdiff, plus fp32 rounding of terms of either sign, a few ulps of the largest
    # element (1e-6 gmax).  v is the same combination of g^2 >= 0: |g^2 - g'^2| <= 2 gmax gdiff + gdiff^2, plus relative rounding of three
    # steps of three roundings each (1e-6)
    assert torch.equal(named["body.2.bias"].detach(), start["body.2.bias"])
    off = [o for n, o, _ in opt._views if n == "body.2.bias"][0]
    st = ropt.state[dict(ref.named_parameters())["body.2.bias"]]
    m, v = opt.m[off:off + 16], opt.v[off:off + 16]
    assert float(m.abs().min()) > 0 and float(v.min()) > 0
    print("frozen group: gmax %.3e gdiff %.3e  |dm| %.3e  |dv| %.3e" % (gmax, gdiff, float((m - st["exp_avg"]).abs().max()), float((v - st["exp_avg_sq"]).abs().max())))
    assert gdiff < 1e-3 * gmax
    assert torch.allclose(m, st["exp_avg"], rtol=0.0, atol=gdiff + 1e-6 * gmax), float((m - st["exp_avg"]).abs().max())
    assert torch.allclose(v, st["exp_avg_sq"], rtol=1e-6, atol=2 * gmax * gdiff + gdiff * gdiff), float((v - st["exp_avg_sq"]).abs().max())
    assert not torch.equal(named["body.2.weight"].detach(), start["body.2.weight"])


@pytest.mark.parametrize("lr1,wd1", [(0.5 * LR, 0.0), (LR, 0.1), (0.5 * LR, 0.1)], ids=["lr", "wd", "both"])
def test_default_built_optimizer_honours_what_is_written_into_group_1(lr1, wd1):
    """a scheduler (or a user) writes another rate into param_groups[1]["lr"], or a decay into param_groups[1]["weight_decay"], of an
    optimizer built without param_groups=: the step runs -- it used to raise ValueError for the rate and to ignore the decay -- and is
    torch.optim.AdamW's with those groups"""
    net = _net((5,))
    ref = copy.deepcopy(net)
    red, opt = _optimizer(net)
    assert opt.grouped is False
    opt.param_groups[1]["lr"] = lr1
    opt.param_groups[1]["weight_decay"] = wd1
    assert opt.grouped is True
    dec = [n for n, p in net.named_parameters() if p.dim() > 1]
    nodec = [n for n, p in net.named_parameters() if p.dim() <= 1]
    _against_oracle(net, ref, red, opt, _oracle(ref, [(dec, LR, WD), (nodec, lr1, wd1)]))
    opt.param_groups[1]["lr"], opt.param_groups[1]["weight_decay"] = LR, 0.0
    assert opt.grouped is False                                                  # back to the launch without a table
    opt.lr = 3e-3
    assert [g["lr"] for g in opt.param_groups] == [3e-3, 3e-3] and opt.weight_decay == WD


def _f32(x):
    return float(np.float32(x))


def test_later_trips_of_the_grid_capped_loop_through_the_entry_point():
    """ap_adamw_ema_step_groups on synthetic slabs of 4096 * 1024 + 4 * 259 elements: the grid is capped at 4096 workgroups of 256 lanes
    x 4 elements, so 259 threads make a second trip.  Seven groups, the group byte changing every 1021 elements (inside float4s).
    Reference: the kernel's formula restated with torch in fp32 on the device, the same operations in the same order, every element of
    every output held to rtol 2e-7 (one fp32 ulp is at most 1.2e-7): the kernel contracts b * m + t and x - s * q into fused
    multiply-adds and torch rounds the product first, which moves a result by at most one ulp where the two terms have one sign -- so
    the slabs are built sign-coherent (g and m of one sign, p and the EMA copies of the other: the update then grows |p|), nothing
    cancels, and a relative bound with atol = 0 holds for every element.  Beside it: the two-group table that restates
    ap_adamw_ema_step's arguments, against ap_adamw_ema_step on the same slabs, bit for bit."""
    from autoprog_amd import ops
    from autoprog_amd._lib import lib
    n = 4096 * 1024 + 4 * 259
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(3)

    def rand(lo, hi):
        return torch.rand(n, device=dev, generator=gen) * (hi - lo) + lo
    sign = torch.where(torch.rand(n, device=dev, generator=gen) < 0.5, -1.0, 1.0)
    p0, g0, m0, v0 = -sign * rand(0.5, 2.0), sign * rand(0.04, 0.4), sign * rand(0.01, 0.1), rand(1e-4, 1e-2)
    e0 = [-sign * rand(0.5, 2.0) for _ in range(2)]
    del sign
    b1, b2, eps, step, gscale, cv = _f32(0.9), _f32(0.999), _f32(1e-8), 3, 0.25, _f32(0.08)
    decays = [_f32(0.9), _f32(0.99)]
    bc1 = _f32(1.0 - b1 ** step)
    bc2 = _f32(np.sqrt(1.0 - b2 ** step))
    dec_arr = (ctypes.c_float * 4)(decays[0], decays[1], 0.0, 0.0)

    def run(entry, byte_slab, lr, wd, table=None):
        s = [t.clone() for t in (p0, g0, m0, v0, e0[0], e0[1])]
        p16 = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        ema_arr = (ctypes.c_void_p * 4)(s[4].data_ptr(), s[5].data_ptr(), None, None)
        args = (s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), s[3].data_ptr(), byte_slab.data_ptr(), n, lr, b1, b2, eps, wd, step, gscale,
                None, 0.0, cv, None, ema_arr, dec_arr, 2, p16.data_ptr())
        if table is None:
            rc = entry(*args, ops._stream())
        else:
            rc = entry(*args, None, None, table.data_ptr(), table.shape[0], ops._stream())
        assert rc == 0
        return {"p": s[0], "m": s[2], "v": s[3], "ema0": s[4], "ema1": s[5], "p16": p16}

    # ---- seven groups against the restated formula (the float arguments lr / weight_decay are not read: poison them)
    gid = ((torch.arange(n, device=dev) // 1021) % 7).to(torch.uint8)
    table = torch.tensor([[1e-2, 0.05], [3e-3, 0.0], [1e-3, 0.2], [0.0, 0.05], [5e-3, 0.1], [2e-3, 0.0], [1e-2, 0.3]], dtype=torch.float32)
    got = run(lib.ap_adamw_ema_step_groups, gid, float("nan"), float("nan"), table.to(dev))
    factor = torch.tensor([_f32(1.0 - float(lr) * float(wd)) for lr, wd in table.tolist()], dtype=torch.float32, device=dev)   # one fma: the product is exact in fp64
    ssize = (table[:, 0] / torch.tensor(bc1, dtype=torch.float32)).to(dev)                                                  # IEEE fp32 division
    idx = gid.long()
    g = (g0 * gscale).clamp(-cv, cv)
    m = b1 * m0 + _f32(np.float32(1.0) - np.float32(b1)) * g
    v = b2 * v0 + _f32(np.float32(1.0) - np.float32(b2)) * g * g
    denom = v.sqrt() / bc2 + eps
    p = p0 * factor[idx] - ssize[idx] * (m / denom)
    want = {"p": p, "m": m, "v": v}
    for i, d in enumerate(decays):
        want["ema%d" % i] = d * e0[i] + _f32(np.float32(1.0) - np.float32(d)) * p
    assert float((g.abs() == cv).float().mean()) > 0.1 and float((g.abs() < cv).float().mean()) > 0.1      # the clamp acts on some, not on all
    for k, w in want.items():
        worst = float(((got[k] - w).abs() / w.abs()).max())
        print("later trips, %s: worst relative difference %.3e" % (k, worst))
        assert torch.allclose(got[k], w, atol=0.0, rtol=2e-7), (k, worst)
    assert torch.equal(got["p16"].view(torch.int16), got["p"].to(torch.bfloat16).view(torch.int16))
    frozen = idx == 3
    assert torch.equal(got["p"][frozen], p0[frozen]) and not torch.equal(got["m"][frozen], m0[frozen])
    del want, p, m, v, denom, g, idx, frozen

    # ---- the table that restates the ungrouped launch, against that launch
    mask = ((torch.arange(n, device=dev) // 1021) % 2).to(torch.uint8)
    lr, wd = _f32(1e-2), _f32(0.05)
    old = run(lib.ap_adamw_ema_step, mask, lr, wd)
    new = run(lib.ap_adamw_ema_step_groups, 1 - mask, float("nan"), float("nan"), torch.tensor([[lr, wd], [lr, 0.0]], dtype=torch.float32, device=dev))
    for k in old:
        view = torch.int16 if old[k].dtype == torch.bfloat16 else torch.int32
        assert torch.equal(old[k].view(view), new[k].view(view)), k
    assert not torch.equal(old["p"], got["p"])


# ---------------------------------------------------------------------------------------------------------------- graphs
def _volo_setup(groups, variant="volo_h2_l3", batch=4, img=64):
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import TokenLabelCrossEntropy
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import FlatAdamWEma, layer_decay_param_groups
    torch.manual_seed(0)
    model = create_model("model_variant", variant=variant, num_classes=16, img_size=img, stem_hidden_dim=64).cuda().train()
    red = GradientBucketReducer(list(model.parameters()), world_size=1, defer_mean=True)
    red.install_sink(model)
    opt = FlatAdamWEma(model, red, lr=2e-3, weight_decay=0.05, ema_decays=[0.9, 0.99],
                       param_groups=layer_decay_param_groups(model, 0.05, 0.75) if groups else None)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(batch, 3, img, img, generator=g).cuda()
    target = torch.softmax(torch.randn(batch, 16, 2 + (img // 16) ** 2, generator=g) * 2, dim=1).cuda()
    return model, red, opt, TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=16), x, target


def _schedule(opt, step, steps=5):
    lr = 2e-3 * 0.5 * (1.0 + np.cos(np.pi * step / steps))                       # what a cosine scheduler writes: ONE value into every group
    for g in opt.param_groups:
        g["lr"] = lr


def test_graph_replay_with_layer_decay_groups_is_the_eager_step(monkeypatch):
    """five steps of volo_h2_l3 under layer-wise decay groups and a schedule that writes a new "lr" into every group before each step:
    the run replayed from a HIP graph equals the eager run from the same seeds bit for bit (losses, weights, EMA copies) -- the
    table is sent in front of every replay, so a replay reads the rates of ITS step"""
    from autoprog_amd import ops
    from autoprog_amd.graph import GraphedStep
    monkeypatch.setattr(ops, "deterministic", True)
    out = []
    for graphed in (False, True):
        model, red, opt, loss_fn, x, target = _volo_setup(True)
        try:
            assert opt.grouped and 4 < len(opt.param_groups) <= 256
            if graphed:
                gs = GraphedStep(model, loss_fn, red, opt, x, target)
                # the warm-up steps of the capture are real steps: rewind what they moved (as tests/test_gpu_graph.py does)
                saved = [t.clone() for t in [opt.p, opt.m, opt.v] + opt.ema + [b.detach() for b in opt._buffers] + [b for bs in opt.ema_buffers for b in bs]]
                _schedule(opt, 0)
                gs.capture(warmup=2)
                with torch.no_grad():
                    for t, s in zip([opt.p, opt.m, opt.v] + opt.ema + list(opt._buffers) + [b for bs in opt.ema_buffers for b in bs], saved):
                        t.copy_(s)
                    for mod in model.modules():
                        if isinstance(mod, torch.nn.BatchNorm2d):
                            mod.num_batches_tracked.zero_()
                opt.step_count = 0
                opt.resync()
            np.random.seed(11)
            torch.manual_seed(5)
            losses = []
            for s in range(5):
                _schedule(opt, s)
                if graphed:
                    losses.append(float(gs.step().detach()))
                else:
                    red.zero_grad()
                    loss = loss_fn(model(x), target)
                    loss.backward()
                    red.finish()
                    opt.step()
                    losses.append(float(loss.detach()))
            out.append((losses, opt.p.clone(), [e.clone() for e in opt.ema], opt.group_table()))
        finally:
            red.remove()
    (le, pe, ee, te), (lg, pg, eg, tg) = out
    print("eager :", le)
    print("graph :", lg)
    assert torch.equal(te, tg) and float(te[:, 0].max()) / float(te[:, 0].min()) > 3          # the groups really are apart
    assert le == lg, (le, lg)
    assert torch.equal(pe, pg) and all(torch.equal(a, b) for a, b in zip(ee, eg))


def test_graph_of_a_default_optimizer_refuses_to_replay_once_its_groups_diverge():
    from autoprog_amd.graph import GraphedStep
    model, red, opt, loss_fn, x, target = _volo_setup(False)
    try:
        gs = GraphedStep(model, loss_fn, red, opt, x, target).capture(warmup=0)
        gs.step()
        opt.param_groups[1]["lr"] = 0.5 * opt.param_groups[0]["lr"]
        with pytest.raises(RuntimeError, match="recapture"):
            gs.step()
        opt.param_groups[1]["lr"] = opt.param_groups[0]["lr"]
        assert np.isfinite(float(gs.step().detach()))                                   # in agreement again: the graph is good again
    finally:
        red.remove()


def test_driver_crosses_a_stage_transition_with_layer_decay_groups(monkeypatch):
    """AutoProgDriver on volo_h2_l6, depth 3 then 6, steps replayed from graphs, the optimizer built from layer_decay_param_groups: the
    transition (grow, graphs released and captured again) goes through, training goes on with a finite loss that falls within each
    stage (one fixed batch), and the group map is what it was: it follows the parameter, not the elastic configuration"""
    from autoprog_amd import graph as G
    from autoprog_amd.prog.driver import AutoProgDriver
    replays = []
    real_step = G.GraphedStep.step
    monkeypatch.setattr(G.GraphedStep, "step", lambda self, *a, **k: (replays.append(self._grouped), real_step(self, *a, **k))[1])
    np.random.seed(3)
    model, red, opt, loss_fn, x, target = _volo_setup(True, variant="volo_h2_l6")
    try:
        ids0 = opt._group_workspace(x.device)["group_id"].clone()
        assert int(ids0.max()) == len(opt.param_groups) - 1
        drv = AutoProgDriver(model, loss_fn, opt, red, lambda r: (x, target), r_list=[64, 64], l_list=[3, 6], dp_list=[0.0, 0.0], grow_epochs=[0, 2],
                             steps_per_epoch=4, auto_grow=False, use_graphs=True, graph_after=1)
        hist = drv.run(4)
        losses = [h["loss"] for h in hist]
        print("driver losses:", losses, [h["l"] for h in hist])
        assert [h["l"] for h in hist] == [3, 3, 6, 6] and all(np.isfinite(losses))
        assert losses[1] < losses[0] and losses[3] < losses[2]
        assert len(replays) == 2 * (2 * 4 - 1) and all(replays) and len(drv._graphs) == 1
        assert torch.equal(opt.group_id, ids0) and opt.grouped
    finally:
        red.remove()


def test_checkpoint_round_trip_of_a_grouped_optimizer():
    """state_dict() of a four-group optimizer into a fresh one built on a copy of the model: the next step is the original's next step
    bit for bit, lr_scale and every other group entry survive, and a state with another number of groups is refused"""
    net = _net((6, 1, 2))
    named = dict(net.named_parameters())
    split = [["extra.0", "body.2.weight"], ["extra.2", "body.0.bias"], ["extra.1", "body.0.weight"], ["body.2.bias"]]

    def groups(of, scale):
        return [{"params": [of[n] for n in names], "weight_decay": 0.1 * i, "lr_scale": scale ** i, "name": "g%d" % i} for i, names in enumerate(split)]
    red, opt = _optimizer(net, groups(named, 0.5))
    for step in range(2):
        _grads(net, red, step)
        opt.step()
    for g in opt.param_groups:
        g["lr"] = 4e-3                                                           # a scheduler has been here
    sd = copy.deepcopy(opt.state_dict())
    assert [g["lr_scale"] for g in sd["param_groups"]] == [1.0, 0.5, 0.25, 0.125] and [g["name"] for g in sd["param_groups"]] == ["g0", "g1", "g2", "g3"]
    twin = copy.deepcopy(net)
    red_t, opt_t = _optimizer(twin, groups(dict(twin.named_parameters()), 1.0))
    assert torch.equal(opt_t.p, opt.p) and float(opt_t.m.abs().sum()) == 0.0
    opt_t.load_state_dict(sd)
    assert len(opt_t.param_groups) == 4 and [g["lr_scale"] for g in opt_t.param_groups] == [1.0, 0.5, 0.25, 0.125]
    assert all(g["lr"] == 4e-3 for g in opt_t.param_groups) and opt_t.step_count == 2
    assert torch.equal(opt_t.group_table(), opt.group_table())
    _grads(net, red, 2)
    red_t.flat.copy_(red.flat)
    red_t._pending_scale = red._pending_scale
    opt.step()
    opt_t.step()
    _assert_same_state(opt, opt_t, "after the load")
    other = copy.deepcopy(net)
    _, opt_o = _optimizer(other)                                                 # the two default groups
    with pytest.raises(ValueError, match="4 parameter groups"):
        opt_o.load_state_dict(sd)
