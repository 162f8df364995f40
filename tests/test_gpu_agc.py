"""Adaptive gradient clipping on the flat gradient slab (csrc/agc.hip, ap_agc_clip; FlatAdamWEma.adaptive_clip_grad; the reference's
`--clip-mode agc`, main_prog.py:129-132, 1019-1027) against the fp64 statements of the rule in tests/_agc_ref.py.

Kernel cases go through ops.agc_clip on synthetic slabs; g and p each sit in a larger buffer with NaN guard bands on both sides, which are
checked afterwards.  In every case p is unchanged bit for bit, elements of units the kernel reports factor 1 for are unchanged bit for bit,
and clipped elements and unit_factor are within 1e-6 relative of the fp64 reference (absolute floor: one fp32 denormal step).  The bound is
derived, not measured: with exact fp64 sums an fp32 result passes through at most five roundings of 2^-24 ~ 6e-8 (two norms, the bound, the
quotient, the product), 3e-7 in all; 1e-6 leaves a factor of three.  (The kernel forms the bound and the quotient in fp64, so it uses two of
the five.)  clip_factor, eps and grad_scale are given as fp32-representable numbers, so kernel and reference decide from the same values."""
import copy

import numpy as np
import pytest
import torch

from tests._agc_ref import agc_flat, agc_per_parameter

pytestmark = pytest.mark.gpu

CF = float(np.float32(0.01))
EPS = float(np.float32(1e-3))
GUARD = 64                                   # elements of NaN on either side (a multiple of 4: the slab stays 16-byte aligned)
DENORM = float(np.float32(1e-45))


def _embed(values):
    """a 1-D fp32 array on the device inside NaN guard bands: -> (the whole buffer, the view that is the slab)"""
    buf = torch.full((GUARD + values.size + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[GUARD:GUARD + values.size]
    view.copy_(torch.from_numpy(values))
    assert view.data_ptr() % 16 == 0
    return buf, view


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _run(g, p, lens, skip, cf=CF, eps=EPS, scale=1.0):
    """one launch on fresh device copies -> dict with everything the checks read (host arrays)"""
    from autoprog_amd import ops
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    gbuf, gv = _embed(g)
    pbuf, pv = _embed(p)
    table = torch.from_numpy(off).cuda()
    skip_d = torch.from_numpy(np.asarray(skip, dtype=np.uint8)).cuda()
    factor = torch.full((len(lens),), -7.0, dtype=torch.float32, device="cuda")
    counts = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    ops.agc_clip(gv, pv, table, skip_d, cf, eps=eps, grad_scale=scale, unit_factor=factor, counts=counts)
    torch.cuda.synchronize()
    return {"off": off, "gbuf": gbuf.cpu().numpy(), "pbuf": pbuf.cpu().numpy(), "factor": factor.cpu().numpy(), "counts": counts.cpu().numpy()}


def _check(g, p, lens, skip, res, cf=CF, eps=EPS, scale=1.0, ref=None):
    off, lens = res["off"], np.asarray(lens)
    n = g.size
    want, f_ref, clipped, nonfinite = ref if ref is not None else agc_flat(g, p, off, skip, cf, eps, grad_scale=scale)
    got, f = res["gbuf"][GUARD:GUARD + n], res["factor"]
    # guard bands and p
    for buf in (res["gbuf"], res["pbuf"]):
        assert np.isnan(buf[:GUARD]).all() and np.isnan(buf[GUARD + n:]).all(), "a guard band was written"
    assert np.array_equal(_bits(res["pbuf"][GUARD:GUARD + n]), _bits(p)), "p was written"
    # factors, decisions and tallies
    assert np.all(np.abs(f.astype(np.float64) - f_ref) <= 1e-6 * f_ref), np.abs(f - f_ref).max()
    assert np.all(f[~clipped] == 1.0) and np.all(f <= 1.0)
    assert int(res["counts"][0]) == int(clipped.sum()) and int(res["counts"][1]) == int(nonfinite.sum()), (res["counts"], clipped.sum(), nonfinite.sum())
    # untouched elements keep their bits; clipped ones are within the bound
    el_same = np.repeat(f == 1.0, lens)
    assert np.array_equal(_bits(got)[el_same], _bits(g)[el_same]), "an element of an unclipped unit changed"
    el = np.repeat(clipped, lens)
    err = np.abs(got[el].astype(np.float64) - want[el])
    assert np.all(err <= 1e-6 * np.abs(want[el]) + DENORM), (err.max(), np.abs(want[el]).max())
    return f_ref, clipped, nonfinite


def _random_slab(lens, seed, spread=1.0):
    """p ~ N(0, 1); g ~ N(0, 1) times a per-unit log-normal scale around clip_factor, so that about half the units clip"""
    rng = np.random.RandomState(seed)
    n = int(np.sum(lens))
    p = rng.standard_normal(n).astype(np.float32)
    scale = (CF * np.exp(spread * rng.standard_normal(len(lens)))).astype(np.float32)
    g = (rng.standard_normal(n).astype(np.float32) * np.repeat(scale, lens)).astype(np.float32)
    return g, p


@pytest.fixture(scope="module")
def geometry():
    """the unit-geometry slab, its launch and its fp64 reference, computed once (tests 1, 4 and 5 read them, none writes them)"""
    from autoprog_amd import ops
    T = ops.agc_short_max()
    lens = [3, 63, 1, T + 1, 5, 255, 4, 3 * T + 7, 65, 257, 64, 75265, 1023, T - 1, 256, T, 384, 1000]
    assert sorted(lens) == sorted([1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 384, 1000, 1023, T - 1, T, T + 1, 3 * T + 7, 75265])
    g, p = _random_slab(lens, seed=0)
    skip = np.zeros(len(lens), dtype=np.uint8)
    res = _run(g, p, lens, skip)
    ref = agc_flat(g, p, res["off"], skip, CF, EPS)
    return {"T": T, "lens": lens, "g": g, "p": p, "skip": skip, "res": res, "ref": ref}


def test_unit_geometry(geometry):
    """units of 1 .. 75 265 elements around every boundary of the kernel -- one lane, one float4, one wave's sweep, the short path's limit T
    = ap_agc_short_max() and just past it, a long unit of many workgroup sweeps -- laid so that unit starts fall on all four residues mod
    4, the three long units on three different ones"""
    d = geometry
    off, lens, T = d["res"]["off"], np.asarray(d["lens"]), d["T"]
    assert {int(s) % 4 for s in off[:-1]} == {0, 1, 2, 3}
    assert len({int(s) % 4 for s, l in zip(off[:-1], lens) if l > T}) == 3
    f_ref, clipped, nonfinite = _check(d["g"], d["p"], lens, d["skip"], d["res"], ref=d["ref"])
    share = (f_ref < 1.0).mean()
    assert 0.3 <= share <= 0.7, share                                              # (a condition on the input, read from the reference)
    assert clipped[lens > T].any() and (~clipped[lens > T]).any()                  # long units with and without the second walk
    assert not nonfinite.any()


def test_many_units():
    """70 001 units of lengths 1 .. 13 in rotation.  The grid is capped at 4096 workgroups of four waves, one unit per wave and sweep:
    16 384 units per sweep, so this exceeds the cap 4.27 times -- every wave takes later units, the last sweep is a partial one, and one
    group of four holds a single unit (70 001 = 4 x 17 500 + 1)."""
    lens = [1 + (i % 13) for i in range(70001)]
    g, p = _random_slab(lens, seed=5)
    skip = np.zeros(len(lens), dtype=np.uint8)
    res = _run(g, p, lens, skip)
    f_ref, clipped, _ = _check(g, p, lens, skip, res)
    assert 0.3 <= clipped.mean() <= 0.7, clipped.mean()


def test_special_units():
    """in one slab: an all-zero gradient (untouched, factor 1); an all-zero parameter unit (the bound is eps * clip_factor); a unit with one
    inf and -- a long one -- a unit with one NaN (bit-identical afterwards, counted, factor 1); a skipped unit whose gradient is 1e6 times
    the bound (bit-identical); a plainly clipped and a plainly unclipped unit between them"""
    from autoprog_amd import ops
    T = ops.agc_short_max()
    lens = [37, 50, 300, T + 452, 129, 200, 77]
    rng = np.random.RandomState(9)
    n = int(np.sum(lens))
    off = np.concatenate([[0], np.cumsum(lens)])
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * CF * 0.1).astype(np.float32)                    # (gn = 0.1 of the bound: unclipped unless changed below)
    sl = [slice(int(a), int(b)) for a, b in zip(off[:-1], off[1:])]
    g[sl[0]] = 0.0
    p[sl[1]] = 0.0
    g[sl[1]] = (rng.standard_normal(lens[1]) * 1e-3).astype(np.float32)           # gn ~ 7e-3 against a bound of 1e-5
    g[sl[2]] *= 100.0
    g[sl[2]][17] = np.inf
    g[sl[3]] *= 100.0
    g[sl[3]][T + 100] = np.nan
    g[sl[4]] *= 1e7                                                                # 1e6 times the bound, skipped
    g[sl[5]] *= 100.0                                                              # clipped
    skip = np.array([0, 0, 0, 0, 1, 0, 0], dtype=np.uint8)
    res = _run(g, p, lens, skip)
    f_ref, clipped, nonfinite = _check(g, p, lens, skip, res)
    assert list(clipped) == [False, True, False, False, False, True, False] and list(nonfinite) == [False, False, True, True, False, False, False]
    f = res["factor"]
    assert f[0] == 1.0 and f[2] == 1.0 and f[3] == 1.0 and f[4] == 1.0 and f[6] == 1.0 and int(res["counts"][1]) == 2
    gn1 = np.sqrt((g[sl[1]].astype(np.float64) ** 2).sum())
    assert abs(f[1] - EPS * CF / gn1) <= 1e-6 * EPS * CF / gn1                     # the bound of a zero parameter unit is eps * clip_factor
    got = res["gbuf"][GUARD:GUARD + n]
    for u in (0, 2, 3, 4, 6):
        assert np.array_equal(_bits(got[sl[u]]), _bits(g[sl[u]])), u
    assert np.isinf(got[sl[2]][17]) and np.isnan(got[sl[3]][T + 100])


def test_deferred_mean(geometry):
    """grad_scale = 0.25 (a pending 1/world): the reference's result for the slab scaled by 0.25, then clipped, then divided by 0.25 -- the
    slab stays the SUM"""
    d = geometry
    g4 = (d["g"] * np.float32(4.0)).astype(np.float32)                             # (exact: a power of two) the SUM over four ranks
    res = _run(g4, d["p"], d["lens"], d["skip"], scale=0.25)
    want, f_ref, clipped, nonfinite = agc_flat(g4.astype(np.float64) * 0.25, d["p"], res["off"], d["skip"], CF, EPS, grad_scale=1.0)
    _check(g4, d["p"], d["lens"], d["skip"], res, scale=0.25, ref=(want / 0.25, f_ref, clipped, nonfinite))
    assert np.array_equal(clipped, d["ref"][2]) and 0 < clipped.sum() < clipped.size
    # without the scale four times as loud: more units clip
    res1 = _run(g4, d["p"], d["lens"], d["skip"], scale=1.0)
    assert int(res1["counts"][0]) > int(res["counts"][0])


def test_two_launches_write_the_same_bits(geometry):
    d = geometry
    again = _run(d["g"], d["p"], d["lens"], d["skip"])
    assert np.array_equal(_bits(again["gbuf"][GUARD:-GUARD]), _bits(d["res"]["gbuf"][GUARD:-GUARD]))
    assert np.array_equal(_bits(again["factor"]), _bits(d["res"]["factor"])) and np.array_equal(again["counts"], d["res"]["counts"])


@pytest.mark.parametrize("exclude", [None, ()])
def test_against_torch_adamw(exclude):
    """the network of test_gradient_clipping_inside_the_flat_slab_step, three steps under a deferred mean of world = 4:
    adaptive_clip_grad + step against the per-parameter form of tests/_agc_ref.py on a deep copy followed by torch.optim.AdamW, to that
    test's atol 2e-6 / rtol 1e-5.  Default exclusion: the last two parameters (the last Linear) stay unclipped; exclude=(): everything
    clips.  clip_factor 0.02 sits in the middle of the units' gradient-to-weight ratios (0.002 .. 0.2): some but not all units clip."""
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.optim import FlatAdamWEma
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(24, 32), torch.nn.GELU(), torch.nn.Linear(32, 16)).cuda()
    ref = copy.deepcopy(net)
    red = GradientBucketReducer(list(net.parameters()), world_size=1, defer_mean=True)
    opt = FlatAdamWEma(net, red, lr=1e-2, weight_decay=0.05)
    dec = [p for n, p in ref.named_parameters() if p.dim() > 1]
    nodec = [p for n, p in ref.named_parameters() if p.dim() <= 1]
    ropt = torch.optim.AdamW([{"params": dec, "weight_decay": 0.05}, {"params": nodec, "weight_decay": 0.0}], lr=1e-2)
    world, cf = 4, 0.02
    for step in range(3):
        torch.manual_seed(10 + step)
        x = torch.randn(8, 24, device="cuda")
        red.zero_grad()
        (net(x).pow(2).mean() * world).backward()            # the slab as an all-reduce over 4 ranks would leave it: the SUM
        red._pending_scale = 1.0 / world                      # ... with the mean deferred (finish() sets this)
        ropt.zero_grad()
        ref(x).pow(2).mean().backward()
        clipped_ps = list(ref.parameters()) if exclude == () else list(ref.parameters())[:-2]
        for q, gq in zip(clipped_ps, agc_per_parameter(clipped_ps, [q.grad for q in clipped_ps], cf, 1e-3)):
            q.grad.copy_(gq.float())
        ropt.step()
        opt.adaptive_clip_grad(cf, exclude=exclude)
        assert red.grad_scale == 1.0 / world                  # the pass read the pending scale and did not take it
        rep = opt.agc_report()
        assert rep["units"] == (32 + 1 + 16 + 1 if exclude == () else 32 + 1 + 1 + 1) and rep["nonfinite"] == 0
        assert 0 < rep["clipped"] < rep["units"], rep
        assert len(rep["worst"]) == 3 and rep["worst"][0][1] < 1.0 and rep["worst"][0][1] <= rep["worst"][1][1] <= rep["worst"][2][1]
        assert rep["worst"][0][0].split("[")[0] in ("0.weight", "0.bias", "2.weight", "2.bias")
        if exclude is None:
            assert all(not name.startswith("2.") for name, f in rep["worst"] if f < 1.0)
        opt.step()
        for (n, p), q in zip(net.named_parameters(), ref.parameters()):
            assert torch.allclose(p.detach(), q.detach(), atol=2e-6, rtol=1e-5), (step, n, float((p - q).abs().max()))
    with pytest.raises(NotImplementedError, match="adaptive_clip_grad"):
        opt.step(clip_grad=0.1, clip_mode="agc")


def _volo_setup():
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import TokenLabelCrossEntropy
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import FlatAdamWEma
    torch.manual_seed(0)
    model = create_model("model_variant", variant="volo_h2_l3", num_classes=16, img_size=64, stem_hidden_dim=64, drop_path_rate=0.0).cuda().train()
    red = GradientBucketReducer(list(model.parameters()), world_size=1, defer_mean=True)
    red.install_sink(model)
    opt = FlatAdamWEma(model, red, lr=2e-3, weight_decay=0.05, ema_decays=[0.9])
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4, 3, 64, 64, generator=g).cuda()
    target = torch.softmax(torch.randn(4, 16, 18, generator=g) * 2, dim=1).cuda()
    return model, red, opt, TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=16), x, target


def test_graph_replays_are_the_eager_steps(monkeypatch):
    """GraphedStep(clip_grad=0.01, clip_mode='agc') on volo_h2_l3 at 64 px, batch 4, DropPath off, deterministic weight gradients: three
    replays against three eager steps of adaptive_clip_grad followed by step -- losses, weights and the EMA copy bit for bit, and the pass
    really clipped.  Asking for the workspace for the first time during a capture raises (the capture is pretended: the refusal comes
    before anything is allocated)."""
    from autoprog_amd import ops
    from autoprog_amd.graph import GraphedStep
    monkeypatch.setattr(ops, "deterministic", True)
    steps = 3
    model, red, opt, loss_fn, x, target = _volo_setup()
    try:
        np.random.seed(11)
        torch.manual_seed(5)
        le = []
        for s in range(steps):
            red.zero_grad()
            loss = loss_fn(model(x), target)
            loss.backward()
            red.finish()
            opt.adaptive_clip_grad(0.01)
            opt.step()
            le.append(float(loss.detach()))
        rep_e = opt.agc_report()
        pe, ee = opt.p.clone(), opt.ema[0].clone()
    finally:
        red.remove()
    assert 0 < rep_e["clipped"] < rep_e["units"] and rep_e["nonfinite"] == 0, rep_e
    model, red, opt, loss_fn, x, target = _volo_setup()
    try:
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
            with pytest.raises(RuntimeError, match="captured"):
                opt._agc_workspace(x.device)
            assert opt._agc is None
        gs = GraphedStep(model, loss_fn, red, opt, x, target, clip_grad=0.01, clip_mode="agc")
        # the capture's warm-up steps are real steps: weights, moments, the EMA copy and the BatchNorm statistics are rewound afterwards
        # (as tests/test_gpu_graph.py does)
        p0, m0, v0, ema0 = opt.p.clone(), opt.m.clone(), opt.v.clone(), opt.ema[0].clone()
        bufs0 = [b.detach().clone() for b in opt._buffers]
        ebufs0 = [b.clone() for b in opt.ema_buffers[0]]
        gs.capture(warmup=2)
        assert opt._agc is not None
        with torch.no_grad():
            opt.p.copy_(p0); opt.m.copy_(m0); opt.v.copy_(v0); opt.ema[0].copy_(ema0)
            for b, b0 in zip(opt._buffers, bufs0):
                b.copy_(b0)
            for b, b0 in zip(opt.ema_buffers[0], ebufs0):
                b.copy_(b0)
            for m in model.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.num_batches_tracked.zero_()
        opt.step_count = 0
        opt.resync()
        np.random.seed(11)
        torch.manual_seed(5)
        lg = [float(gs.step().detach()) for _ in range(steps)]
        rep_g = opt.agc_report()
        assert lg == le, (le, lg)
        assert torch.equal(pe, opt.p) and torch.equal(ee, opt.ema[0])
        assert rep_g == rep_e
    finally:
        red.remove()


def test_a_nan_passes_through_to_the_guard():
    """one NaN written into one gradient element: adaptive_clip_grad leaves that unit's gradient with its original bits, and
    step(skip_nonfinite=True) then skips -- the parameters are unchanged and guard_counts()['skipped'] == 1"""
    model, red, opt, loss_fn, x, target = _volo_setup()
    try:
        np.random.seed(11)
        red.zero_grad()
        loss_fn(model(x), target).backward()
        red.finish()
        ws = opt._agc_workspace(x.device)
        off = ws["table"].cpu().numpy()
        names = ws["names"]
        u = next(i for i, n in enumerate(names) if n.endswith("mlp.fc1.weight[5]"))
        b, e = int(off[u]), int(off[u + 1])
        red.flat[b + (e - b) // 2] = float("nan")
        before = red.flat.clone()
        p0 = opt.p.clone()
        opt.adaptive_clip_grad(0.01)
        rep = opt.agc_report()
        assert rep["nonfinite"] == 1 and rep["clipped"] > 0
        after = red.flat.clone()
        assert torch.equal(after[b:e].view(torch.int32), before[b:e].view(torch.int32))
        assert not torch.equal(after.view(torch.int32), before.view(torch.int32))          # (other units were clipped)
        opt.step(skip_nonfinite=True)
        assert torch.equal(opt.p, p0)
        assert opt.guard_counts()["skipped"] == 1
        assert torch.equal(red.flat[b:e].view(torch.int32), before[b:e].view(torch.int32))
    finally:
        red.remove()
