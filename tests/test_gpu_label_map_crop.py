"""Token labels from stored top-k maps: ap_label_map_crop (csrc/labelmap.hip) through the C ABI, ops.label_map_crop,
data.DeviceLabelMapCrop on a seeded DeviceRandomResizedCrop and AutoProgDriver(label_maps=...).

The reference is tests/_labelmap_ref.py, the fp64 sample loop over a dense row per bin.  The comparison rule (check_row) skips no row: val
non-increasing with equal values in ascending class order, every kept pair within 1e-4 ref + 1e-37, no class left out above the smallest
kept value * (1 + 1e-4), dropped within 1e-4 of the reference's sum over the classes that were not kept.  The 1e-4 is derived, not tuned:
all terms are non-negative, so a bin's relative error stays below (terms + weight roundings) * 2^-24, under 1e-4 at 4096 candidates.

Shapes: 18 x 18 x 5 maps (tlt's), a non-square 7 x 5 x 3 and 32 x 16 x 8, the 4096-candidate limit of the class slot's workgroup; P = 1
(a token bin as large as the box: the workgroup body from a token workgroup), 8 and 14 (wave-sized bins; at Kin = 8 the bins of P = 8
cross the 128-candidate threshold between the two bodies)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests._labelmap_ref import check_row, label_map_ref, topk_row
from tests.test_gpu_localized import P as PTR, case, ops, stream  # noqa: F401  (ops, case: fixtures)

pytestmark = pytest.mark.gpu
IDX_SENTINEL, VAL_SENTINEL = -7777, -123.25
SHAPES = [(18, 18, 5), (7, 5, 3), (32, 16, 8)]            # Hm, Wm, Kin
GRIDS = [1, 8, 14]
KS = [1, 5, 8]
# (map kind, class form): float classes live in the scores' dtype with C = 1000, int32 classes with C = 65536
KINDS = [("random", "float"), ("random", "int"), ("shared", "float"), ("differ", "int"), ("zero", "float")]
B = 5


def boxes_for(Hm, Wm):
    """one of each per batch, fp32 [5, 8]: the whole extent; a box narrower than one map pixel (the max(.., 1) clamp); a box against the
    bottom-right edge (the xl >= Wm - 1 branch); a flipped box; a flipped box on a ragged extent, formed as DeviceLabelMapCrop forms it"""
    eh, ew, top, left, h, w = 150, 200, 13, 21, 90, 131
    rec = np.zeros((B, 8), dtype=np.float32)
    rec[0, :5] = (0, 0, Wm, Hm, 0)
    rec[1, :5] = (Wm * 0.37, Hm * 0.52, Wm * 0.37 + 0.4, Hm * 0.52 + 0.3, 0)
    rec[2, :5] = (Wm * 0.55, Hm * 0.6, Wm, Hm, 0)
    rec[3, :5] = (Wm * 0.1 + 0.3, Hm * 0.2, Wm * 0.8, Hm * 0.9 + 0.05, 1)
    rec[4, :5] = (left * Wm / ew, top * Hm / eh, (left + w) * Wm / ew, (top + h) * Hm / eh, 1)
    return rec


@functools.lru_cache(maxsize=None)
def maps_for(Hm, Wm, Kin, kind, form):
    """-> (scores fp64 [B, Kin, Hm, Wm] with fp16-exact values, classes int64, C); built once, never modified"""
    g = np.random.RandomState(Hm * 1000 + Wm * 10 + Kin + len(kind))
    n = Kin * Hm * Wm
    scores = (g.randint(1, 1025, (B, Kin, Hm, Wm)) / 1024.0)                    # multiples of 2^-10 in (0, 1]: exact in fp16
    if form == "float":
        C, pool = 1000, np.array([0, 1, 7, 44, 45, 300, 301, 512, 998, 999, 1500, 2047])       # 1500 and 2047 >= C: they vanish
    else:
        C, pool = 65536, np.array([0, 3, 21842, 21843, 40000, 65534, 65535, 65536, 70000, -3, 1 << 20, 12])   # the last five but 12 vanish
    if kind == "random":
        classes = pool[g.randint(0, len(pool), (B, Kin, Hm, Wm))]
    elif kind == "shared":                                                      # every pixel carries the same Kin classes: exactly Kin pairs
        classes = np.broadcast_to(pool[:Kin].reshape(1, Kin, 1, 1), (B, Kin, Hm, Wm)).copy()
    elif kind == "differ":                                                      # every candidate its own class: truncation, dropped > 0
        classes = np.stack([g.permutation(C)[:n].reshape(Kin, Hm, Wm) for _ in range(B)])
    else:
        classes = pool[g.randint(0, len(pool), (B, Kin, Hm, Wm))]
        scores = np.zeros_like(scores)
    return scores, classes.astype(np.int64), C


@functools.lru_cache(maxsize=None)
def reference(Hm, Wm, Kin, kind, form, P):
    scores, classes, C = maps_for(Hm, Wm, Kin, kind, form)
    return label_map_ref(scores, classes, boxes_for(Hm, Wm), P, C)


def device_maps(scores, classes, form, dtype):
    """float form: tlt's [B, 2, Kin, Hm, Wm] tensor, passed as two views of it; int form: separate scores and int32 classes"""
    if form == "float":
        both = torch.stack([torch.from_numpy(scores), torch.from_numpy(classes.astype(np.float64))], dim=1).to(dtype).cuda()
        return both[:, 0], both[:, 1]
    return torch.from_numpy(scores).to(dtype).cuda(), torch.from_numpy(classes.astype(np.int32)).cuda()


def launch(lib, sc, cl, labels, rec, P, K, C, want_dropped=True):
    """one launch through the C ABI into sentinel-filled outputs with a guard image in front and behind -> (rc, idx, val, dropped) on the CPU,
    after checking that nothing outside the target was written"""
    from autoprog_amd._lib import LabelMapCropArgs
    Bn, Kin, Hm, Wm = sc.shape
    slots = 2 + P * P
    idx = torch.full((Bn + 2, slots, K), IDX_SENTINEL, dtype=torch.int32, device="cuda")
    val = torch.full((Bn + 2, slots, K), VAL_SENTINEL, dtype=torch.float32, device="cuda")
    drp = torch.full((Bn + 2, slots - 1), VAL_SENTINEL, dtype=torch.float32, device="cuda")
    boxes = torch.from_numpy(rec).cuda()
    a = LabelMapCropArgs()
    a.scores, a.score_dtype, a.score_stride = sc.data_ptr(), int(sc.dtype == torch.float32), sc.stride(0)
    a.classes, a.class_dtype, a.class_stride = cl.data_ptr(), int(cl.dtype == torch.int32), cl.stride(0)
    a.labels, a.boxes, a.boxes_host = labels.data_ptr(), boxes.data_ptr(), rec.ctypes.data
    a.idx, a.val = idx[1:].data_ptr(), val[1:].data_ptr()
    a.dropped = drp[1:].data_ptr() if want_dropped else None
    a.B, a.Kin, a.Hm, a.Wm, a.P, a.K, a.C = Bn, Kin, Hm, Wm, P, K, C
    rc = lib.ap_label_map_crop(ctypes.byref(a), stream())
    torch.cuda.synchronize()
    ic, vc, dc = idx.cpu(), val.cpu(), drp.cpu()
    for g in (0, Bn + 1):
        assert bool((ic[g] == IDX_SENTINEL).all()) and bool((vc[g] == VAL_SENTINEL).all()) and bool((dc[g] == VAL_SENTINEL).all()), "a guard image was written"
    if not want_dropped:
        assert bool((dc == VAL_SENTINEL).all())
    return rc, ic[1:-1], vc[1:-1], (dc[1:-1] if want_dropped else None)


def check_target(idx, val, dropped, labels, ref, K, what):
    """slot 0 exactly, every other row under the comparison rule"""
    Bn, slots, _ = idx.shape
    want_i = torch.full((Bn, K), -1, dtype=torch.int32)
    want_i[:, 0] = labels.cpu().int()
    want_v = torch.zeros(Bn, K)
    want_v[:, 0] = 1.0
    assert torch.equal(idx[:, 0], want_i) and torch.equal(val[:, 0], want_v), "%s: slot 0 is not (label, 1.0), (-1, 0.0).." % what
    inp, vnp = idx.numpy(), val.numpy()
    for b in range(Bn):
        assert len(ref[b]) == slots - 1
        for s in range(1, slots):
            check_row(inp[b, s], vnp[b, s], None if dropped is None else dropped[b, s - 1].item(), ref[b][s - 1], K, "%s image %d slot %d" % (what, b, s))


# ================================================================================================================ 1. bins against fp64
@pytest.mark.parametrize("kind,form", KINDS)
@pytest.mark.parametrize("P", GRIDS)
@pytest.mark.parametrize("Hm,Wm,Kin", SHAPES)
def test_bins_against_fp64(ops, case, Hm, Wm, Kin, P, kind, form):
    """five boxes (whole extent, narrower than a pixel, bottom-right edge, flipped, flipped on a ragged extent) on one kind of map, K = 1, 5
    and 8, fp16 and fp32 storage: every row under the comparison rule, slot 0 exactly, nothing written outside the target.  shared: exactly
    Kin pairs per bin that sees anything; differ: more classes than K, dropped > 0; zero: all fillers and dropped = 0."""
    from autoprog_amd._lib import lib
    scores, classes, C = maps_for(Hm, Wm, Kin, kind, form)
    ref = reference(Hm, Wm, Kin, kind, form, P)
    rec = boxes_for(Hm, Wm)
    labels = torch.tensor([0, C - 1, 5, 2, 1], dtype=torch.int64).cuda()
    for dtype in (torch.float16, torch.float32):
        sc, cl = device_maps(scores, classes, form, dtype)
        for K in KS:
            rc, idx, val, drp = launch(lib, sc, cl, labels, rec, P, K, C)
            assert rc == 0, "ap_label_map_crop: code %d" % rc
            what = "%s %s K %d" % (case, str(dtype)[6:], K)
            check_target(idx, val, drp, labels, ref, K, what)
            pairs = (idx[:, 1:] != -1).sum(-1)
            if kind == "shared":
                assert bool((pairs == min(K, Kin)).all()), "%s: a bin of a map that shares its classes must hold min(K, Kin) pairs" % what
                if K >= Kin:
                    assert bool((drp == 0).all())
            elif kind == "differ":                                      # the whole extent sees Hm Wm Kin classes
                assert int(pairs[0, 0]) == K and float(drp[0, 0]) > 0, "%s: the class slot of the whole extent must be truncated" % what
            elif kind == "zero":
                assert bool((pairs == 0).all()) and bool((drp == 0).all())
    # without `dropped` the same pairs, and nothing written to it
    rc, idx2, val2, _ = launch(lib, sc, cl, labels, rec, P, KS[-1], C, want_dropped=False)
    assert rc == 0 and torch.equal(idx, idx2) and torch.equal(val.view(torch.int32), val2.view(torch.int32))


# ================================================================================================================ 2. exact order
@pytest.mark.parametrize("P", [2, 4])
def test_dyadic_case_is_exact(ops, case, P):
    """scores in {0.25, 0.5, 1}, pixel-aligned boxes of 8 x 8 and 16 x 8 map pixels on 16 x 16 x 4 maps: P divides the box, every sample
    sits on a half pixel and every weight is a power of two, so any summation order is exact in fp32 -- idx and val equal the reference bit
    for bit at K = 4 (six classes: truncation, dropped exact too) and K = 8.  Image 0 has four constant planes of score 0.5, one class each:
    four equal sums in every bin, which must come out in ascending class order"""
    from autoprog_amd._lib import lib
    g = np.random.RandomState(P)
    Hm = Wm = 16
    Kin, C = 4, 1000
    scores = g.choice([0.25, 0.5, 1.0], (B, Kin, Hm, Wm))
    classes = g.choice([5, 9, 17, 33, 64, 900], (B, Kin, Hm, Wm)).astype(np.int64)
    scores[0], classes[0, 0], classes[0, 1], classes[0, 2], classes[0, 3] = 0.5, 40, 30, 20, 10      # four classes with equal sums everywhere
    rec = np.zeros((B, 8), dtype=np.float32)
    rec[:, :5] = [(0, 0, 8, 8, 0), (4, 4, 12, 12, 1), (0, 8, 16, 16, 0), (8, 0, 16, 16, 1), (0, 0, 16, 16, 1)]
    ref = label_map_ref(scores, classes, rec, P, C)
    labels = torch.arange(B, dtype=torch.int64).cuda()
    for dtype, form, K in ((torch.float16, "float", 4), (torch.float32, "int", 8)):
        sc, cl = device_maps(scores, classes, form, dtype)
        rc, idx, val, drp = launch(lib, sc, cl, labels, rec, P, K, C)
        assert rc == 0
        for b in range(B):
            for s in range(1, 2 + P * P):
                wi, wv, wd = topk_row(ref[b][s - 1], K)
                assert idx[b, s].tolist() == wi.tolist() and val[b, s].tolist() == wv.tolist(), "%s image %d slot %d: %s %s, reference %s %s" % (
                    case, b, s, idx[b, s].tolist(), val[b, s].tolist(), wi.tolist(), wv.tolist())
                assert drp[b, s - 1].item() == wd
        assert all(idx[0, s].tolist()[:4] == [10, 20, 30, 40] for s in range(1, 2 + P * P))


# ================================================================================================================ 3. same bits
@pytest.mark.parametrize("Hm,Wm,Kin,P", [(18, 18, 5, 14), (32, 16, 8, 8), (32, 16, 8, 1)])
def test_two_launches_give_the_same_bits(ops, Hm, Wm, Kin, P):
    from autoprog_amd._lib import lib
    scores, classes, C = maps_for(Hm, Wm, Kin, "random", "int")
    sc, cl = device_maps(scores, classes, "int", torch.float16)
    labels = torch.zeros(B, dtype=torch.int64).cuda()
    first = launch(lib, sc, cl, labels, boxes_for(Hm, Wm), P, 8, C)
    ops.poison_lds()                                                    # (nothing is read from LDS that the launch did not write)
    second = launch(lib, sc, cl, labels, boxes_for(Hm, Wm), P, 8, C)
    assert first[0] == 0 and second[0] == 0
    for x, y in zip(first[1:], second[1:]):
        assert np.array_equal(x.numpy().view(np.int32), y.numpy().view(np.int32))


# ================================================================================================================ 4. the data object
def _stored(Bn, Hm, Wm, Kin, seed, form="float", C=1000):
    from autoprog_amd.data import StoredLabelMaps
    g = np.random.RandomState(seed)
    scores = g.randint(1, 1025, (Bn, Kin, Hm, Wm)) / 1024.0
    classes = g.randint(0, C, (Bn, 1, Hm, Wm)) // 50 * 50 + g.randint(0, 3, (Bn, Kin, Hm, Wm))       # neighbouring pixels share classes
    labels = torch.from_numpy(g.randint(0, C, Bn))
    if form == "float":
        maps = torch.stack([torch.from_numpy(scores), torch.from_numpy(classes.astype(np.float64))], dim=1).half().cuda()
    else:
        maps = (torch.from_numpy(scores).float().cuda(), torch.from_numpy(classes.astype(np.int32)).cuda())
    return StoredLabelMaps(labels.cuda(), maps), scores, classes, labels


@pytest.mark.parametrize("r", [128, 224])
def test_target_follows_the_crop(ops, case, r):
    """DeviceLabelMapCrop.target on a seeded DeviceRandomResizedCrop over ragged extents: the SparseTokenLabelTarget [B, 2 + (r // 16)^2, 5]
    equals the reference on the records formed from crop.last (flip included) and crop.last_extents; a second call refills the same buffers"""
    from autoprog_amd.data import DeviceLabelMapCrop, DeviceRandomResizedCrop
    from autoprog_amd.loss import SparseTokenLabelTarget
    Bn, H, W, k = 6, 96, 128, 5
    crop = DeviceRandomResizedCrop(seed=r)
    g = torch.Generator().manual_seed(r)
    u8 = torch.randint(0, 256, (Bn, 3, H, W), dtype=torch.uint8, generator=g).cuda()
    ext = np.array([[96, 128], [96, 100], [50, 128], [77, 33], [96, 128], [64, 64]])
    stored, scores, classes, labels = _stored(Bn, 18, 18, 5, r)
    lm = DeviceLabelMapCrop(k=k, smoothing=0.1, num_classes=1000)
    crop.crop(u8, r, extents=ext)
    t = lm.target(stored, crop, r)
    torch.cuda.synchronize()
    P = r // 16
    assert isinstance(t, SparseTokenLabelTarget) and tuple(t.idx.shape) == (Bn, 2 + P * P, k) and t.smoothing == 0.1
    rec = np.zeros((Bn, 8), dtype=np.float32)
    for b, (top, left, h, w, flip) in enumerate(crop.last):
        eh, ew = ext[b]
        rec[b, :5] = (left * 18 / ew, top * 18 / eh, (left + w) * 18 / ew, (top + h) * 18 / eh, flip)
    assert crop.last_extents == [tuple(e) for e in ext.tolist()] and any(rr[4] for rr in crop.last) and not all(rr[4] for rr in crop.last)
    assert np.array_equal(np.array(lm.last, dtype=np.float32), rec[:, :5])
    ref = label_map_ref(scores, classes, rec, P, 1000)
    check_target(t.idx.cpu(), t.val.cpu(), None, labels, ref, k, case)
    ptrs = (t.idx.data_ptr(), t.val.data_ptr())
    crop.crop(u8, r, extents=ext)
    t2 = lm.target(stored, crop, r)
    assert t2 is t and (t2.idx.data_ptr(), t2.val.data_ptr()) == ptrs
    with pytest.raises(ValueError):                                     # crop.last belongs to six images
        lm.target(_stored(4, 18, 18, 5, 1)[0], crop, r)


def test_ops_wrapper(ops, case):
    """ops.label_map_crop with int32 classes, out= and dropped= buffers and host records; what it cannot run is refused"""
    from autoprog_amd._lib import AutoProgHipError
    Hm, Wm, Kin, P, K = 7, 5, 3, 8, 5
    scores, classes, C = maps_for(Hm, Wm, Kin, "random", "int")
    sc, cl = device_maps(scores, classes, "int", torch.float32)
    rec = torch.from_numpy(boxes_for(Hm, Wm)).reshape(-1)
    labels = torch.arange(B, dtype=torch.int64).cuda()
    idx = torch.empty(B, 2 + P * P, K, dtype=torch.int32, device="cuda")
    val = torch.empty(B, 2 + P * P, K, dtype=torch.float32, device="cuda")
    drp = torch.empty(B, 1 + P * P, dtype=torch.float32, device="cuda")
    got = ops.label_map_crop(sc, cl, labels, rec.cuda(), P, K, C, out=(idx, val), dropped=drp, host_records=rec)
    assert got[0] is idx and got[1] is val
    check_target(idx.cpu(), val.cpu(), drp.cpu(), labels, reference(Hm, Wm, Kin, "random", "int", P), K, case)
    with pytest.raises(AutoProgHipError):
        ops.label_map_crop(sc.cpu(), cl.cpu(), labels, rec.cuda(), P, K, C)
    with pytest.raises(AutoProgHipError):                               # K = 9
        ops.label_map_crop(sc, cl, labels, rec.cuda(), P, 9, C)
    bad = rec.clone()
    bad[2] = bad[0] - 1                                                 # x2 < x1
    with pytest.raises(AutoProgHipError):
        ops.label_map_crop(sc, cl, labels, rec.cuda(), P, K, C, host_records=bad)
    with pytest.raises(AutoProgHipError):                               # a transposed view: the images are not contiguous
        ops.label_map_crop(sc.transpose(2, 3), cl.transpose(2, 3), labels, rec.cuda(), P, K, C)


# ================================================================================================================ 5. the driver
def _small_volo(classes=24, seed=0, variant="volo_h2_l6"):
    from autoprog_amd.models import create_model
    torch.manual_seed(seed)
    return create_model("model_variant", variant=variant, num_classes=classes, img_size=96, stem_hidden_dim=64).cuda()


@pytest.mark.parametrize("loss_name", ["TokenLabelCrossEntropy", "TokenLabelGTCrossEntropy"])
def test_driver_with_label_maps_eager_and_graphed(ops, monkeypatch, loss_name):
    """AutoProgDriver(crop=, batch_prep=, label_maps=) with (canvases, StoredLabelMaps) from get_batch over a stage change (r 64 -> 96, depth
    3 -> 6), DropPath 0, same seeds: finite losses, every target a SparseTokenLabelTarget of the stage's token grid, and the run with
    use_graphs gives the eager run's losses, weights and EMA copies bit for bit"""
    from autoprog_amd import loss as L
    from autoprog_amd import ops as _ops
    from autoprog_amd.data import DeviceBatchPrep, DeviceLabelMapCrop, DeviceRandomResizedCrop
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.optim import FlatAdamWEma
    from autoprog_amd.prog.driver import AutoProgDriver
    monkeypatch.setattr(_ops, "deterministic", True)
    out = {}
    for use_graphs in (False, True):
        student = _small_volo(24, seed=4).train()
        red = GradientBucketReducer(list(student.parameters()), world_size=1, defer_mean=True)
        red.install_sink(student)
        opt = FlatAdamWEma(student, red, lr=1e-3, weight_decay=0.05, ema_decays=[0.9])
        g = torch.Generator().manual_seed(1)
        seen = []
        stored = [_stored(8, 18, 18, 5, s, C=24)[0] for s in range(3)]
        count = [0]

        def get_batch(r):
            count[0] += 1
            return torch.randint(0, 256, (8, 3, 112, 112), dtype=torch.uint8, generator=g).cuda(), stored[count[0] % 3]

        def loss_fn(outputs, target, _ce=getattr(L, loss_name)(dense_weight=0.5, cls_weight=1.0, classes=24)):
            seen.append((type(target), tuple(target.idx.shape)))
            return _ce(outputs, target)

        drv = AutoProgDriver(student, loss_fn, opt, red, get_batch, r_list=[64, 96], l_list=[3, 6], dp_list=[0.0, 0.0], grow_epochs=[0, 1],
                             steps_per_epoch=4, auto_grow=False, use_graphs=use_graphs, graph_after=2,
                             batch_prep=DeviceBatchPrep((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), re_prob=0.25, num_classes=24, seed=5),
                             crop=DeviceRandomResizedCrop(seed=7), label_maps=DeviceLabelMapCrop(k=5, num_classes=24))
        steps, real = [], drv._train_step
        monkeypatch.setattr(drv, "_train_step", lambda *a, **k: (steps.append(real(*a, **k)), steps[-1])[1])
        try:
            np.random.seed(3)
            drv.run(2)
            out[use_graphs] = ([float(s) for s in steps], opt.p.clone(), [e.clone() for e in opt.ema])
            calls = 3 if use_graphs else 4                              # (per stage two eager steps and the capture call the loss; replays do not)
            assert [s for _, s in seen] == [(8, 2 + 16, 5)] * calls + [(8, 2 + 36, 5)] * calls and all(t is L.SparseTokenLabelTarget for t, _ in seen)
        finally:
            red.remove()
    le, pe, ee = out[False]
    lg, pg, eg = out[True]
    print("LABELMAP driver eager:", le)
    print("LABELMAP driver graph:", lg)
    assert len(le) == 8 and all(np.isfinite(v) for v in le)
    assert le == lg, (le, lg)
    assert torch.equal(pe, pg) and all(torch.equal(a, b) for a, b in zip(ee, eg))
