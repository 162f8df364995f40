"""Token labels from stored maps without a GPU: the fp64 reference of the GPU tests (tests/_labelmap_ref.py) against hand-worked cases,
the new entry point's presence in the C ABI and its refusals before any launch, DeviceLabelMapCrop's host records against the formulas,
DeviceRandomResizedCrop.last_extents, and what AutoProgDriver(label_maps=...) refuses."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests._labelmap_ref import check_row, dense_bin, label_map_ref, topk_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "ap_label_map_crop"


# ================================================================================================================ 1. the reference
def test_whole_map_with_one_bin_per_pixel():
    """a 4 x 4 map, every pixel its own class, the box the whole map and P = 4: bin_w = 1, one sample per bin at p + 0.5, which is half of
    pixel p and half of pixel p + 1 -- and the last bin's sample, at 3.5, is clamped onto the edge pixel 3 entirely"""
    g = np.random.RandomState(0)
    s = g.rand(1, 1, 4, 4)
    c = np.arange(16).reshape(1, 1, 4, 4)
    rows = label_map_ref(s, c, [(0, 0, 4, 4, 0)], 4, 16)[0]
    assert len(rows) == 1 + 16
    half = lambda p: [(p, 0.5), (p + 1, 0.5)] if p < 3 else [(3, 1.0)]
    for ph in range(4):
        for pw in range(4):
            want = {y * 4 + x: wy * wx * s[0, 0, y, x] for y, wy in half(ph) for x, wx in half(pw)}
            cls, val = rows[1 + ph * 4 + pw]
            assert cls.tolist() == sorted(want) and np.allclose(val, [want[k] for k in sorted(want)], rtol=1e-15, atol=0)
    # the class slot: a 1 x 1 pooling with 4 x 4 samples at the same positions -> the mean of the sixteen token bins
    cls, val = rows[0]
    total = np.zeros(16)
    for r in rows[1:]:
        total[r[0]] += r[1]
    assert cls.tolist() == list(range(16)) and np.allclose(val, total / 16, rtol=1e-14, atol=0)


def test_one_class_map_merges_to_the_bilinear_blend():
    """every candidate carries class 7: each bin holds one merged pair, the sum over k of the bilinear blend of plane k at the sample"""
    g = np.random.RandomState(1)
    s = g.rand(1, 3, 5, 6)
    c = np.full((1, 3, 5, 6), 7)
    # a 2 x 2 box at (0.25, 0.75), P = 2: one sample per bin at (x, y) = (0.75 + pw, 1.25 + ph)
    rows = label_map_ref(s, c, [(0.25, 0.75, 2.25, 2.75, 0)], 2, 10)[0]
    for ph in range(2):
        for pw in range(2):
            x0, y0 = pw, 1 + ph
            blend = sum(0.75 * (0.25 * s[0, k, y0, x0] + 0.75 * s[0, k, y0, x0 + 1]) + 0.25 * (0.25 * s[0, k, y0 + 1, x0] + 0.75 * s[0, k, y0 + 1, x0 + 1])
                        for k in range(3))
            cls, val = rows[1 + ph * 2 + pw]
            assert cls.tolist() == [7] and abs(val[0] - blend) <= 1e-15 * blend
    idx, v, dropped = topk_row(rows[1], 5)
    assert idx.tolist() == [7, -1, -1, -1, -1] and v[1:].tolist() == [0.0] * 4 and dropped == 0.0
    # a sample on a pixel centre reads that pixel alone: box (0.5, 0.5) .. (2.5, 2.5), bin (0, 0) samples (1, 1)
    rows = label_map_ref(s, c, [(0.5, 0.5, 2.5, 2.5, 0)], 2, 10)[0]
    assert abs(rows[1][1][0] - s[0, :, 1, 1].sum()) <= 1e-14
    # a box narrower than a pixel is widened to one: roi = max(0.2, 1) = 1, the class slot's single sample sits at x1 + 0.5
    d = dense_bin(s[0], c[0], 10, (2.0, 1.0, 2.2, 1.1), 1, 0, 0)
    want = sum(0.25 * (s[0, k, 1, 2] + s[0, k, 1, 3] + s[0, k, 2, 2] + s[0, k, 2, 3]) for k in range(3))
    assert abs(d[7] - want) <= 1e-14 and d.sum() == d[7]
    # classes outside [0, C) and float classes: truncation, and nothing from class 12 at C = 10
    c2 = np.where(np.arange(6) % 2 == 0, 7.9, 12.0) * np.ones((1, 3, 5, 6))
    rows = label_map_ref(s, c2, [(0, 0, 6, 5, 0)], 1, 10)[0]
    assert rows[0][0].tolist() == [7] and rows[1][0].tolist() == [7]


def test_flip_reverses_the_columns_and_nothing_else():
    g = np.random.RandomState(2)
    s = g.rand(2, 4, 9, 7)
    c = g.randint(0, 30, (2, 4, 9, 7))
    box = (0.7, 1.1, 6.2, 8.4)
    plain = label_map_ref(s, c, [box + (0,)] * 2, 3, 30)
    flipped = label_map_ref(s, c, [box + (1,)] * 2, 3, 30)
    for b in range(2):
        assert np.array_equal(plain[b][0][0], flipped[b][0][0]) and np.array_equal(plain[b][0][1], flipped[b][0][1])      # the class slot
        for ph in range(3):
            for pw in range(3):
                p, f = plain[b][1 + ph * 3 + pw], flipped[b][1 + ph * 3 + (2 - pw)]
                assert np.array_equal(p[0], f[0]) and np.array_equal(p[1], f[1])
    assert not np.array_equal(plain[0][1][1], flipped[0][1][1])


def test_tie_rule_and_comparison_rule():
    row = (np.array([3, 5, 9, 11]), np.array([0.25, 0.5, 0.25, 0.125]))
    idx, val, dropped = topk_row(row, 3)
    assert idx.tolist() == [5, 3, 9] and val.tolist() == [0.5, 0.25, 0.25] and dropped == 0.125
    check_row(idx, val, dropped, row, 3, "exact")
    with pytest.raises(AssertionError):                                 # equal values in descending class order
        check_row([5, 9, 3], val, dropped, row, 3, "order")
    with pytest.raises(AssertionError):                                 # a larger class was left out
        check_row([5, 3, 11], [0.5, 0.25, 0.125], 0.25, row, 3, "left out")
    with pytest.raises(AssertionError):                                 # a value off by 2e-4
        check_row(idx, [0.5001, 0.25, 0.25], dropped, row, 3, "value")
    with pytest.raises(AssertionError):
        check_row(idx, val, 0.126, row, 3, "dropped")
    with pytest.raises(AssertionError):                                 # a filler in front of a class that exists
        check_row([5, 3, -1], [0.5, 0.25, 0.0], 0.375, row, 3, "filler")


# ================================================================================================================ 2. ABI
def _args(**kw):
    from autoprog_amd._lib import LabelMapCropArgs
    a = LabelMapCropArgs()
    a.scores, a.classes, a.labels, a.boxes, a.idx, a.val, a.dropped = 4096, 8192, 12288, 16384, 20480, 24576, 28672
    a.score_dtype, a.class_dtype, a.score_stride, a.class_stride = 0, 0, 2 * 1620, 2 * 1620
    a.B, a.Kin, a.Hm, a.Wm, a.P, a.K, a.C = 2, 5, 18, 18, 14, 5, 1000
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_entry_point_is_declared_exported_and_refuses_before_any_launch():
    from autoprog_amd._lib import _SIGNATURES, EXPORTED_SYMBOLS, LIB_PATH, lib
    header = open(os.path.join(ROOT, "include", "autoprog_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(\s*const\s+ap_label_map_crop_args\s*\*\s*args\s*,\s*ap_stream_t\s+stream\s*\)" % SYMBOL, header)
    assert SYMBOL in EXPORTED_SYMBOLS and SYMBOL in _SIGNATURES and hasattr(ctypes.CDLL(LIB_PATH), SYMBOL)
    assert lib.ap_abi_version() == 7
    f = getattr(lib, SYMBOL)
    assert f.restype is ctypes.c_int
    call = lambda **kw: f(ctypes.byref(_args(**kw)), None)
    assert f(None, None) == -4
    for name in ("scores", "classes", "labels", "boxes", "idx", "val"):                 # AP_ERR_NULL: a required pointer
        assert call(**{name: None}) == -4, name
    for kw in (dict(K=0), dict(K=9), dict(Kin=0), dict(Kin=9), dict(P=0), dict(Hm=0), dict(Wm=-1), dict(C=0), dict(C=65537), dict(B=-1),
               dict(score_dtype=2), dict(class_dtype=-1)):                               # AP_ERR_SHAPE
        assert call(**kw) == -1, kw
    assert call(Hm=32, Wm=17, Kin=8) == -2 and call(Hm=4097, Wm=1, Kin=1) == -2          # AP_ERR_UNSUPPORTED: Hm Wm Kin > 4096

    def host(*second):
        rec = (ctypes.c_float * 16)(0, 0, 18, 18, 0, 0, 0, 0, *second, 0, 0, 0)
        return call(boxes_host=ctypes.cast(rec, ctypes.c_void_p).value)
    assert host(5, 2, 4.5, 9, 0) == -1 and host(5, 2, 9, 1.5, 1) == -1                   # x2 < x1, y2 < y1
    assert host(float("nan"), 2, 9, 9, 0) == -1 and host(1, 2, float("inf"), 9, 0) == -1 and host(1, 2, 9, 9, float("nan")) == -1
    assert host(1, 2, 9, 9, 0.5) == -1 and host(1, 2, 9, 9, 2) == -1 and host(1, 2, 9, 9, -1) == -1      # a flip other than 0 or 1
    assert call(B=0) == 0                                                                # no launch
    assert call(B=0, scores=None, classes=None, labels=None, boxes=None, idx=None, val=None, dropped=None) == 0
    assert call(B=0, K=9) == -1                                                          # the shape checks come first


def test_ops_wrapper_refuses_what_it_cannot_run():
    from autoprog_amd import ops
    from autoprog_amd._lib import AutoProgHipError
    z = torch.zeros(2, 5, 18, 18)
    with pytest.raises(AutoProgHipError):                                                # CPU tensors
        ops.label_map_crop(z, z, torch.zeros(2, dtype=torch.int64), torch.zeros(16), 14, 5, 1000)


# ================================================================================================================ 3. the data objects
def _crop(**kw):
    from autoprog_amd.data import DeviceRandomResizedCrop
    return DeviceRandomResizedCrop(device="cpu", **kw)


def test_crop_records_its_extents():
    c = _crop(seed=3)
    assert c.last_extents is None
    ext = np.array([[40, 56], [33, 20], [40, 17]])
    c.draw(3, 40, 56, ext)
    assert c.last_extents == [(40, 56), (33, 20), (40, 17)] and len(c.last) == 3
    c.draw(2, 40, 56)
    assert c.last_extents == [(40, 56)] * 2
    c.center_records(3, 64, 64, 0.875, ext + 3)
    assert c.last_extents == [(43, 59), (36, 23), (43, 20)]
    c.center_records(1, 64, 48)
    assert c.last_extents == [(64, 48)]


@pytest.mark.parametrize("interpolation", [None, "random"])
def test_host_records_equal_the_formulas(interpolation):
    """a seeded crop over ragged extents, 18 x 18 and 7 x 5 maps: x1 = left Wm / ew, y1 = top Hm / eh, x2 = (left + w) Wm / ew,
    y2 = (top + h) Hm / eh in float64, rounded to fp32, then the flip and three zero words; more calls than ring slots"""
    from autoprog_amd.data import DeviceLabelMapCrop
    B, H, W = 7, 96, 128
    g = np.random.RandomState(5)
    ext = np.stack([g.randint(30, H + 1, B), g.randint(30, W + 1, B)], axis=1)
    c = _crop(seed=11, interpolation=interpolation)
    lm = DeviceLabelMapCrop(k=5)
    flips = set()
    for step in range(10):
        c.draw(B, H, W, ext)
        for Hm, Wm in ((18, 18), (7, 5)):
            rec = lm.records(c, B, Hm, Wm).numpy().reshape(-1, 8)[:B].copy()
            assert rec.dtype == np.float32 and not rec[:, 5:].any()
            for b in range(B):
                top, left, h, w, flip = c.last[b][:5]
                eh, ew = int(ext[b][0]), int(ext[b][1])
                want = np.array([left * Wm / ew, top * Hm / eh, (left + w) * Wm / ew, (top + h) * Hm / eh, flip], dtype=np.float64).astype(np.float32)
                assert np.array_equal(rec[b, :5], want), (b, rec[b], want)
                assert 0 <= rec[b, 0] <= rec[b, 2] <= Wm and 0 <= rec[b, 1] <= rec[b, 3] <= Hm
                flips.add(flip)
            assert lm.last == [tuple(float(v) for v in r[:5]) for r in rec]
    assert flips == {0, 1}
    c.center_records(B, H, W, 0.875, ext, interpolation="bilinear" if interpolation else None)      # a centre crop: no flip
    rec = lm.records(c, B, 18, 18).numpy().reshape(-1, 8)[:B]
    assert not rec[:, 4].any() and bool((rec[:, 2] > rec[:, 0]).all())
    with pytest.raises(ValueError):                                     # crop.last belongs to 7 images
        lm.records(c, B + 1, 18, 18)
    with pytest.raises(ValueError):                                     # nothing cropped yet
        lm.records(_crop(seed=1), B, 18, 18)


def test_holders_refuse_bad_arguments():
    from autoprog_amd.data import DeviceLabelMapCrop, StoredLabelMaps
    labels = torch.arange(3)
    tlt = torch.zeros(3, 2, 5, 18, 18, dtype=torch.float16)
    s = StoredLabelMaps(labels, tlt)
    assert s.labels.dtype == torch.int64 and tuple(s.scores.shape) == (3, 5, 18, 18)
    assert s.scores.data_ptr() == tlt.data_ptr() and s.classes.data_ptr() == tlt[:, 1].data_ptr()            # two views, no copy
    pair = StoredLabelMaps(labels.int(), (torch.zeros(3, 5, 18, 18), torch.zeros(3, 5, 18, 18, dtype=torch.int32)))
    assert pair.classes.dtype == torch.int32
    for bad in (lambda: StoredLabelMaps(labels, torch.zeros(3, 3, 5, 18, 18)), lambda: StoredLabelMaps(labels, tlt.double()),
                lambda: StoredLabelMaps(labels[:2], tlt), lambda: StoredLabelMaps(labels.float(), tlt),
                lambda: StoredLabelMaps(labels, (torch.zeros(3, 5, 18, 18), torch.zeros(3, 5, 18, 18, dtype=torch.int64))),
                lambda: StoredLabelMaps(labels, (torch.zeros(3, 5, 18, 18), torch.zeros(3, 5, 18, 17, dtype=torch.int32))),
                lambda: DeviceLabelMapCrop(k=9), lambda: DeviceLabelMapCrop(k=0), lambda: DeviceLabelMapCrop(num_classes=65537)):
        with pytest.raises(ValueError):
            bad()
    from autoprog_amd._lib import AutoProgHipError
    with pytest.raises(AutoProgHipError):                               # maps on the CPU: there is no fallback
        DeviceLabelMapCrop().target(s, _crop(), 224)
    with pytest.raises(ValueError):
        DeviceLabelMapCrop().target((labels, tlt), _crop(), 224)


# ================================================================================================================ 4. the driver
def test_driver_refusals_and_routing():
    from autoprog_amd.data import DeviceBatchPrep, DeviceLabelMapCrop, StoredLabelMaps
    from autoprog_amd.prog.driver import AutoProgDriver
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    base = dict(model=None, loss_fn=None, optimizer=None, reducer=None, get_batch=lambda r: None, r_list=[64, 96], l_list=[3, 6], dp_list=[0.0, 0.0],
                grow_epochs=[0, 2], steps_per_epoch=1)
    lm = DeviceLabelMapCrop(k=5, num_classes=24)
    prep = DeviceBatchPrep(mean, std, device="cpu", re_prob=0.25)
    assert AutoProgDriver(**base).label_maps is None                    # the default: nothing changes
    import inspect
    assert inspect.signature(AutoProgDriver.__init__).parameters["label_maps"].kind is inspect.Parameter.KEYWORD_ONLY
    with pytest.raises(ValueError, match="needs a crop"):
        AutoProgDriver(label_maps=lm, batch_prep=prep, **base)

    class Teacher:
        num_classes = 24
    with pytest.raises(ValueError, match="teacher"):
        AutoProgDriver(label_maps=lm, batch_prep=prep, crop=_crop(), teacher=Teacher(), **base)
    for kw in (dict(mixup_alpha=0.8), dict(cutmix_alpha=1.0)):          # the message a TeacherLabeler gets
        with pytest.raises(ValueError, match="token labels cannot follow Mixup / CutMix"):
            AutoProgDriver(label_maps=lm, batch_prep=DeviceBatchPrep(mean, std, device="cpu", **kw), crop=_crop(), **base)
    student = torch.nn.Linear(4, 4)
    student.num_classes = 25
    with pytest.raises(ValueError):
        AutoProgDriver(label_maps=lm, batch_prep=prep, crop=_crop(), **dict(base, model=student))
    student.num_classes = 24
    assert AutoProgDriver(label_maps=lm, batch_prep=prep, crop=_crop(), **dict(base, model=student)).label_maps is lm

    # routing: the maps become the target right behind the crop, at the r the crop was asked for
    log = []

    class Crop:
        layout, last, last_extents = "nchw", None, None

        def crop(self, images, size):
            log.append(("crop", size))
            return images

    class Maps:
        num_classes = 24

        def target(self, stored, crop, r):
            log.append(("target", r, type(stored).__name__, type(crop).__name__))
            return "sparse target"

    class Prep:
        layout, re_prob, mix_enabled = "nchw", 0.0, False

        def prep(self, u8):
            log.append(("prep",))
            return u8
    stored = StoredLabelMaps(torch.arange(2), torch.zeros(2, 2, 5, 18, 18, dtype=torch.float16))
    drv = AutoProgDriver(label_maps=Maps(), batch_prep=Prep(), crop=Crop(), **dict(base, get_batch=lambda r: (torch.zeros(2, 3, 8, 8, dtype=torch.uint8), stored)))
    images, target = drv.get_batch(96)
    assert target == "sparse target" and log == [("crop", 96), ("target", 96, "StoredLabelMaps", "Crop"), ("prep",)]
    drv._raw_get_batch = lambda r: (torch.zeros(2, 3, 8, 8, dtype=torch.uint8), torch.zeros(2, 4))
    assert drv.get_batch(64)[1].shape == (2, 4)                         # any other target passes as it is
