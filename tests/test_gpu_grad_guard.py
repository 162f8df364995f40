"""The non-finite gradient guard of the fused optimizer step (FlatAdamWEma.step(skip_nonfinite=True); csrc/optim.hip ap_grad_health,
ap_adamw_ema_step_guarded).  The reference trains under apex's dynamic loss scaler, which skips optimizer.step() for an iteration whose
gradients hold an inf or a NaN (prog/scaler.py:20-26) while ModelEmaV2.update still runs (main_prog.py:1030-1033): the twin here is
torch.optim.AdamW whose step() is simply not called on those iterations.  Non-finite values are DATA in these tests: written into the
gradient slab after backward(), or into a batch's target scores."""
import copy
import os
import socket

import numpy as np
import pytest
import torch

from ._tilecheck import guarded

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
LENS = [1, 3, 5, 4, 7, 1, 1030, 2, 262147, 6]          # odd offsets, a tail that is no multiple of 4, one segment over many workgroups
CHUNK, MAX_GRID = 8192, 2048                             # csrc/optim.hip GH_CHUNK / GH_MAX_GRID: what one sweep of the kernel's grid covers


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel alone
def _typed_guarded(count, dtype, what):
    """`count` elements of `dtype` inside a guarded BYTE buffer (tests/_tilecheck.py knows bf16, fp32 and bytes) -> (typed view, Guard)"""
    size = count * torch.empty(0, dtype=dtype).element_size()
    view, guard = guarded(1, size, dtype=torch.uint8, device="cuda", what=what)
    return view.view(-1)[:size].view(dtype), guard


def _reference(slab, offsets):
    """the fp64 loop over the same table: per segment the sum of squares of the finite elements and the number of the others"""
    x = slab.astype(np.float64)
    sums, counts = [], []
    for lo, hi in zip(offsets, offsets[1:]):
        seg = x[lo:hi]
        fin = np.isfinite(seg)
        sums.append(float(np.sum(np.square(seg[fin]))))
        counts.append(int((~fin).sum()))
    return np.array(sums), np.array(counts)


def _run_health(slab, offsets, launches=1, state0=(0, 0, 0, 0), betas=(0.9, 0.999), pre=3, post=3):
    """slab (host fp32) -> per launch (seg_sumsq, seg_nonfinite, state) as host arrays.  The slab sits in a guarded allocation whose padding is
    fp32 NaN; the table, both outputs and the state record in guarded byte buffers; all of them are checked after the launches."""
    from autoprog_amd import ops
    n, n_seg = slab.size, len(offsets) - 1
    g_row, g_guard = guarded(1, n, dtype=torch.float32, pre=pre, post=post, device="cuda", what="gradient slab")
    g = g_row[0, :n]
    g.copy_(torch.from_numpy(slab))
    assert g.data_ptr() % 16 == 0 and g.is_contiguous()
    table, t_guard = _typed_guarded(n_seg + 1, torch.int64, "segment table")
    table.copy_(torch.tensor([int(o) for o in offsets], dtype=torch.int64))
    sumsq, s_guard = _typed_guarded(n_seg, torch.float64, "seg_sumsq")
    count, c_guard = _typed_guarded(n_seg, torch.int32, "seg_nonfinite")
    state, st_guard = _typed_guarded(8, torch.int32, "ap_guard_state")
    state.zero_()
    state[:4] = torch.tensor(state0, dtype=torch.int32)
    ws_bytes = ops.grad_health_workspace(n, n_seg)
    ws, w_guard = _typed_guarded(ws_bytes // 8, torch.float64, "workspace")
    out = []
    for _ in range(launches):
        ops.grad_health(g, table, sumsq, count, state, ws, beta1=betas[0], beta2=betas[1])
        torch.cuda.synchronize()
        out.append((sumsq.cpu().numpy().copy(), count.cpu().numpy().copy(), state.cpu().clone()))
    for gd in (g_guard, t_guard, s_guard, c_guard, st_guard, w_guard):      # nothing written before, behind or right of any buffer
        gd.check(pad="untouched")
    assert g.cpu().numpy().tobytes() == slab.tobytes(), "the pass wrote into the gradient slab"
    assert table.cpu().tolist() == [int(o) for o in offsets], "the pass wrote into the segment table"
    return out


def _offsets(lens):
    return [0] + [int(v) for v in np.cumsum(lens)]


def _base_slab(lens, seed=0):
    rng = np.random.RandomState(seed)
    return (rng.standard_normal(int(sum(lens))) * 0.02).astype(np.float32)


def _plant_finite_oddities(slab, off):
    slab[off[1]:off[2]] = np.array([1e-40, -3e-42, 1.4e-45], dtype=np.float32)     # a segment of denormals only
    slab[off[2]] = 3.0e38                                                          # finite: its square overflows fp32, not fp64
    slab[off[2] + 1] = -0.0
    slab[off[8] + 70001] = 3.0e38
    slab[off[8] + 70002] = -1e-39
    return slab


def _assert_matches(got_s, got_c, slab, off):
    ref_s, ref_c = _reference(slab, off)
    assert np.array_equal(got_c, ref_c), (got_c.tolist(), ref_c.tolist())
    err = np.abs(got_s - ref_s)
    print("seg_sumsq: worst relative difference to the fp64 loop %.3e" % float(np.max(err / np.maximum(ref_s, 1e-300))))
    assert np.all(err <= 1e-12 * ref_s), (got_s.tolist(), ref_s.tolist())
    assert np.all(np.isfinite(got_s))


def _bias_corrections(t, betas=(0.9, 0.999)):
    b1, b2 = float(np.float32(betas[0])), float(np.float32(betas[1]))
    return np.float32(1.0 - b1 ** t), np.float32(np.sqrt(1.0 - b2 ** t))


@pytest.mark.parametrize("rot", [0, 1, 2])
def test_health_kernel_counts_and_sums_per_segment(rot):
    """+inf, -inf and NaN (rotated over the positions) at the first element of the slab -- a 1-element segment --, at the last element, at
    the last element of one segment and the first of the next, and in another 1-element segment; a finite 3.0e38, -0.0 and denormals
    elsewhere.  Counts exact, sums within 1e-12 of the fp64 loop (x^2 is exact in fp64, only the order of the additions differs), two
    launches bit-identical, nothing outside the outputs written."""
    off = _offsets(LENS)
    slab = _plant_finite_oddities(_base_slab(LENS), off)
    bad = [INF, -INF, NAN]
    for k, pos in enumerate([0, off[-1] - 1, off[7] - 1, off[7], off[5], off[8] + 8191, off[8] + 8192, off[8] + 200000]):
        slab[pos] = bad[(k + rot) % 3]
    (s1, c1, st1), (s2, c2, st2) = _run_health(slab, off, launches=2, state0=(0, 6, 1, 0))
    _assert_matches(s1, c1, slab, off)
    assert s1.tobytes() == s2.tobytes() and c1.tobytes() == c2.tobytes()          # run to run: the same bits
    assert c1.tolist() == [1, 0, 0, 0, 0, 1, 1, 1, 3, 1]
    bc1, bc2 = _bias_corrections(6)
    assert st1[:4].tolist() == [8, 6, 2, 1] and st2[:4].tolist() == [8, 6, 3, 2]  # nonfinite, applied, skipped, consecutive
    assert st1[4:6].view(torch.float32).tolist() == [float(bc1), float(bc2)]      # t = applied, unchanged by a skipped step


def test_health_kernel_clean_slab_applies():
    off = _offsets(LENS)
    slab = _plant_finite_oddities(_base_slab(LENS, seed=1), off)
    (s1, c1, st1), (s2, c2, st2) = _run_health(slab, off, launches=2, state0=(5, 2, 4, 3))
    _assert_matches(s1, c1, slab, off)
    assert int(c1.sum()) == 0 and s1.tobytes() == s2.tobytes()
    assert st1[:4].tolist() == [0, 3, 4, 0] and st2[:4].tolist() == [0, 4, 4, 0]
    for st, t in ((st1, 3), (st2, 4)):
        bc1, bc2 = _bias_corrections(t)
        assert st[4:6].view(torch.float32).tolist() == [float(bc1), float(bc2)]


@pytest.mark.parametrize("lens", [[1100003], [MAX_GRID * CHUNK + 4099, 3, 2 * CHUNK + 1]], ids=["one_segment_1100003", "beyond_one_sweep"])
def test_health_kernel_long_segments(lens):
    """one segment of 1 100 003 elements, and a slab longer than one sweep of the kernel's grid (GH_MAX_GRID chunks of GH_CHUNK): the
    workgroups come round to a second chunk, with segment bounds in the second sweep"""
    off = _offsets(lens)
    slab = _base_slab(lens, seed=2)
    n = off[-1]
    for pos, v in ((0, NAN), (n - 1, -INF), (n // 2, INF), (7, 3.0e38), (n - 2, 1e-41)):
        slab[pos] = v
    wide = n > 4 * 1100003
    (s1, c1, st1), (s2, c2, _) = _run_health(slab, off, launches=2, pre=1 if wide else 3, post=1 if wide else 3)
    _assert_matches(s1, c1, slab, off)
    assert s1.tobytes() == s2.tobytes() and c1.tobytes() == c2.tobytes()
    assert int(c1.sum()) == 3 and st1[:4].tolist() == [3, 0, 1, 1]


# ------------------------------------------------------------------------------------------------------------------ 2. / 3. skip semantics
def _mlp_pair():
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(24, 32), torch.nn.GELU(), torch.nn.Linear(32, 16)).cuda()
    return net, copy.deepcopy(net)


def _twin_adamw(ref):
    dec = [p for n, p in ref.named_parameters() if p.dim() > 1]
    nodec = [p for n, p in ref.named_parameters() if p.dim() <= 1]
    return torch.optim.AdamW([{"params": dec, "weight_decay": 0.05}, {"params": nodec, "weight_decay": 0.0}], lr=1e-2)


def _snapshot(opt):
    return {"p": opt.p.clone(), "m": opt.m.clone(), "v": opt.v.clone(), "p16": opt.p16.clone(), "p16_t": opt.p16_t.clone(),
            "ema": [e.clone() for e in opt.ema]}


@pytest.mark.parametrize("variant", ["plain", "deferred_mean", "clip_norm"])
def test_skipped_steps_leave_the_weights_and_move_the_emas(variant):
    """six guarded steps; an inf in a bias gradient before step 3 and a NaN in a weight gradient before step 4.  Across a skipped step p,
    m, v and both bf16 copies are unchanged bit for bit and every EMA slab is d * e + (1 - d) * p; after the six steps the parameters
    equal the twin's, whose step() was not called on those two iterations -- which holds only if step 5 used the bias corrections of
    t = 3.  deferred_mean: the slab holds the all-reduced SUM of 4 ranks; clip_norm: clip_grad_norm_ inside the step."""
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.optim import FlatAdamWEma
    net, ref = _mlp_pair()
    world = 4 if variant == "deferred_mean" else 1
    clip = 0.05 if variant == "clip_norm" else None
    decays = [0.9, 0.99]
    red = GradientBucketReducer(list(net.parameters()), world_size=1, defer_mean=(world > 1))
    opt = FlatAdamWEma(net, red, lr=1e-2, weight_decay=0.05, ema_decays=decays)
    ropt = _twin_adamw(ref)
    poison = {2: ("0.bias", lambda: net[0].bias.grad.__setitem__(5, INF)), 3: ("2.weight", lambda: net[2].weight.grad.__setitem__((3, 7), NAN))}
    for step in range(6):
        torch.manual_seed(10 + step)
        x = torch.randn(8, 24, device="cuda")
        red.zero_grad()
        (net(x).pow(2).mean() * world).backward()
        if world > 1:
            red._pending_scale = 1.0 / world              # as finish() sets it under a deferred mean
        ropt.zero_grad()
        ref(x).pow(2).mean().backward()
        twin_norms = {n: float(p.grad.norm()) for n, p in ref.named_parameters()}
        if step in poison:
            poison[step][1]()
        before = _snapshot(opt)
        opt.step(clip_grad=clip, clip_mode="norm", skip_nonfinite=True)
        if step in poison:
            for k in ("p", "m", "v", "p16", "p16_t"):
                assert torch.equal(getattr(opt, k), before[k]), (step, k)
            for d, e, e0 in zip(decays, opt.ema, before["ema"]):
                d32 = float(np.float32(d))
                want = (d32 * e0.double() + float(np.float32(1.0) - np.float32(d)) * opt.p.double()).float()
                torch.testing.assert_close(e, want, rtol=1e-6, atol=0.0)
            if clip is not None:
                assert not np.isfinite(float(opt.last_grad_norm))
        else:
            if clip is not None:
                total = torch.nn.utils.clip_grad_norm_(ref.parameters(), clip)
                assert abs(float(opt.last_grad_norm) - float(total)) < 1e-5 * max(1.0, float(total))
            ropt.step()
            assert not torch.equal(opt.p, before["p"])
        if step == 2:
            health = opt.grad_health()
            assert [h[0] for h in health] == ["2.bias", "2.weight", "0.bias", "0.weight"]          # slab order: reversed parameters
            assert {h[0]: h[2] for h in health} == {"0.bias": 1, "0.weight": 0, "2.bias": 0, "2.weight": 0}
            for name, norm, count in health:
                assert np.isfinite(norm), name
                if count == 0:
                    assert abs(norm - twin_norms[name]) <= 1e-5 * twin_norms[name], (name, norm, twin_norms[name])
    for (n, p), q in zip(net.named_parameters(), ref.parameters()):
        assert torch.allclose(p.detach(), q.detach(), atol=2e-6, rtol=1e-5), (n, float((p - q).abs().max()))
    assert opt.guard_counts() == {"applied": 4, "skipped": 2, "consecutive": 0}
    assert float(opt.state_dict()["state"][0]["step"]) == 4.0 and opt.step_count == 6


def test_guard_changes_nothing_while_gradients_are_finite():
    """two copies of the net on the same gradients, one stepped with the guard: p, m, v, the EMAs and the bf16 copy are equal bit for bit
    after each of 20 steps (the bias corrections formed on the device are the host's); a finite 3.0e38 is applied like any gradient"""
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.optim import FlatAdamWEma
    a, b = _mlp_pair()
    reds = [GradientBucketReducer(list(net.parameters()), world_size=1) for net in (a, b)]
    opts = [FlatAdamWEma(net, red, lr=1e-2, weight_decay=0.05, ema_decays=[0.9, 0.99]) for net, red in zip((a, b), reds)]

    def both_equal(step):
        for k in ("p", "m", "v", "p16", "p16_t"):
            assert torch.equal(getattr(opts[0], k), getattr(opts[1], k)), (step, k)
        for e0, e1 in zip(opts[0].ema, opts[1].ema):
            assert torch.equal(e0, e1), step

    for step in range(21):
        torch.manual_seed(30 + step)
        x = torch.randn(8, 24, device="cuda")
        reds[0].zero_grad()
        a(x).pow(2).mean().backward()
        if step == 20:
            a[0].weight.grad[1, 2] = 3.0e38               # finite: its square is not
        reds[1].flat.copy_(reds[0].flat)                  # the same gradients, bit for bit
        opts[0].step(skip_nonfinite=True)
        opts[1].step()
        both_equal(step)
    assert opts[0].guard_counts() == {"applied": 21, "skipped": 0, "consecutive": 0}
    assert opts[0].grad_health()[-1][2] == 0


# ------------------------------------------------------------------------------------------------------------------ 4. whole model
def _tiny():
    from autoprog_amd.models import create_model
    torch.manual_seed(0)
    return create_model("model_variant", variant="volo_h2_l3", num_classes=16, img_size=64, stem_hidden_dim=16).cuda().train()


def _setup(**kw):
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import TokenLabelCrossEntropy
    from autoprog_amd.optim import FlatAdamWEma
    model = _tiny()
    red = GradientBucketReducer(list(model.parameters()), world_size=kw.pop("world_size", 1), **kw)
    red.install_sink(model)
    opt = FlatAdamWEma(model, red, lr=1e-3, weight_decay=0.05, ema_decays=[0.9, 0.99])
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4, 3, 64, 64, generator=g).cuda()
    target = torch.softmax(torch.randn(4, 16, 18, generator=g) * 2, dim=1).cuda()
    return model, red, opt, TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=16), x, target


def test_whole_model_skips_one_step_and_trains_on():
    model, red, opt, loss_fn, x, target = _setup()
    try:
        np.random.seed(0)
        params, losses = [], []
        for step in range(3):
            red.zero_grad()
            loss = loss_fn(model(x), target)
            loss.backward()
            red.finish()
            if step == 1:
                red.flat[red.flat.numel() // 3] = INF
            opt.step(skip_nonfinite=True)
            losses.append(float(loss.detach()))
            params.append({n: p.detach().clone() for n, p in model.named_parameters()})
        assert all(torch.equal(params[1][n], params[0][n]) for n in params[0])                 # the second step left every parameter alone
        assert any(not torch.equal(params[2][n], params[1][n]) for n in params[0]) and all(np.isfinite(losses))
        assert all(bool(torch.isfinite(p).all()) for p in params[2].values())
        assert opt.guard_counts() == {"applied": 2, "skipped": 1, "consecutive": 0}
        sd = copy.deepcopy(opt.state_dict())
        assert float(sd["state"][0]["step"]) == 2.0
        opt.load_state_dict(sd)
        assert opt.guard_counts()["applied"] == 2 and opt.step_count == 2
        opt.resync(reset_moments=True)
        assert opt.guard_counts() == {"applied": 0, "skipped": 0, "consecutive": 0}
    finally:
        red.remove()


# ------------------------------------------------------------------------------------------------------------------ 5. graph
def _graph_setup():
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import TokenLabelCrossEntropy
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import FlatAdamWEma
    torch.manual_seed(0)
    model = create_model("model_variant", variant="volo_h2_l3", num_classes=16, img_size=64, stem_hidden_dim=64, drop_path_rate=0.0).cuda().train()
    red = GradientBucketReducer(list(model.parameters()), world_size=1, defer_mean=True)
    red.install_sink(model)
    opt = FlatAdamWEma(model, red, lr=2e-3, weight_decay=0.05, ema_decays=[0.9, 0.99])
    g = torch.Generator().manual_seed(1)
    x = torch.randn(8, 3, 64, 64, generator=g).cuda()
    target = torch.softmax(torch.randn(8, 16, 18, generator=g) * 2, dim=1).cuda()
    bad = target.clone()
    bad[2, 5, 7] = INF
    return model, red, opt, TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=16), x, [target, bad, target]


def _final(opt):
    return {"p": opt.p.clone(), "m": opt.m.clone(), "v": opt.v.clone(), "ema": [e.clone() for e in opt.ema], "counts": opt.guard_counts()}


def test_guarded_graph_replay_is_the_guarded_eager_step(monkeypatch):
    """three replays of GraphedStep(skip_nonfinite=True), the second fed a target whose scores hold an inf, against the same three guarded
    steps run eagerly with the same seeds: bit-identical weights, moments and EMA copies, the same counters"""
    from autoprog_amd import ops
    from autoprog_amd.graph import GraphedStep
    monkeypatch.setattr(ops, "deterministic", True)
    model, red, opt, loss_fn, x, targets = _graph_setup()
    try:
        np.random.seed(11)
        for t in targets:
            red.zero_grad()
            loss_fn(model(x), t).backward()
            red.finish()
            opt.step(skip_nonfinite=True)
        eager = _final(opt)
    finally:
        red.remove()
    model, red, opt, loss_fn, x, targets = _graph_setup()
    try:
        gs = GraphedStep(model, loss_fn, red, opt, x, targets[0], skip_nonfinite=True)
        p0, ema0 = opt.p.clone(), [e.clone() for e in opt.ema]
        bufs0 = [b.detach().clone() for b in opt._buffers]
        ebufs0 = [[b.clone() for b in bs] for bs in opt.ema_buffers]
        gs.capture(warmup=2)                       # warm-up steps are real steps: rewind what they moved (tests/test_gpu_graph.py)
        with torch.no_grad():
            opt.p.copy_(p0)
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
        opt.resync(reset_moments=True)             # moments, step count and the guard's device record back to zero
        assert opt.guard_counts() == {"applied": 0, "skipped": 0, "consecutive": 0}
        np.random.seed(11)
        losses = [float(gs.step(x, t).detach()) for t in targets]
        graphed = _final(opt)
    finally:
        red.remove()
    assert graphed["counts"] == eager["counts"] == {"applied": 2, "skipped": 1, "consecutive": 0}
    assert np.isfinite(losses[0]) and not np.isfinite(losses[1]) and np.isfinite(losses[2])
    for k in ("p", "m", "v"):
        assert torch.equal(graphed[k], eager[k]), k
    assert all(torch.equal(a, b) for a, b in zip(graphed["ema"], eager["ema"]))


# ------------------------------------------------------------------------------------------------------------------ 6. two ranks, one device
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        model, red, opt, loss_fn, _, _ = _setup(world_size=world, bucket_bytes=64 << 10, defer_mean=True)
        g = torch.Generator().manual_seed(100 + rank)      # every rank its own batch
        x = torch.randn(4, 3, 64, 64, generator=g).cuda()
        target = torch.softmax(torch.randn(4, 16, 18, generator=g) * 2, dim=1).cuda()
        moved = []
        np.random.seed(5)                                   # the same mix-token boxes on both ranks
        for step in range(3):
            t = target
            if step == 1 and rank == 1:                     # rank 1's batch alone is bad; the all-reduce carries it to rank 0
                t = target.clone()
                t[1, 3, 4] = float("nan")
            before = opt.p.clone()
            red.zero_grad()
            loss_fn(model(x), t).backward()
            red.finish()
            opt.step(skip_nonfinite=True)
            moved.append(not torch.equal(before, opt.p))
        torch.cuda.synchronize()
        q.put((rank, {"p": opt.p.cpu().numpy(), "moved": moved, "counts": opt.guard_counts()}))
        red.remove()
    except Exception as e:                                  # pragma: no cover
        import traceback
        q.put((rank, "fail: %r\n%s" % (e, traceback.format_exc())))
    finally:
        dist.destroy_process_group()


def test_two_ranks_skip_the_same_step():
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        out = dict(q.get(timeout=300) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(isinstance(v, dict) for v in out.values()), out
    assert out[0]["moved"] == out[1]["moved"] == [True, False, True]
    assert out[0]["counts"] == out[1]["counts"] == {"applied": 2, "skipped": 1, "consecutive": 0}
    assert np.array_equal(out[0]["p"], out[1]["p"]) and np.all(np.isfinite(out[0]["p"]))
