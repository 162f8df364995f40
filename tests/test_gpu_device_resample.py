"""ap_crop_resample_u8 / ops.crop_resample_u8 / data.DeviceRandomResizedCrop(interpolation=...) on the GPU, both layouts throughout.  The
criterion everywhere is np.array_equal with the numpy restatement of Pillow's 8-bit resize (tests/_resample_ref.py, held to Pillow's own
bytes by tests/test_device_resample_host.py): the coefficients are IEEE doubles and everything behind them is integer arithmetic, so
there is no tolerance."""
import numpy as np
import pytest
import torch

from tests import _resample_ref as RR
from tests.test_gpu_device_crop import BOXES_A, BOXES_B, MEAN, STD, _canvas, _hwc

pytestmark = pytest.mark.gpu
LAYOUTS = ["nchw", "nhwc"]
FILTERS = [1, 2]


def _records(recs):
    r = np.zeros((len(recs), 8), dtype=np.int32)
    r[:, :6] = recs
    return r


def _with(boxes, filters):
    """5-tuples (top, left, h, w, flip) + one filter code or one per box -> 6-tuples"""
    filters = [filters] * len(boxes) if isinstance(filters, int) else filters
    return [tuple(b) + (f,) for b, f in zip(boxes, filters)]


def _run(u8, S, recs, layout, out=None, host=True):
    from autoprog_amd import ops
    rec = torch.from_numpy(_records(recs))
    y = ops.crop_resample_u8(torch.from_numpy(u8).cuda(), S, rec.cuda(), layout=layout, out=out, host_records=rec if host else None)
    assert y.dtype == torch.uint8 and tuple(y.shape) == ((len(recs), 3, S, S) if layout == "nchw" else (len(recs), S, S, 3))
    return y.cpu().numpy()


def _equal(got, want, what):
    d = got != want
    assert not d.any(), "%s: %d of %d bytes differ from the restatement, largest difference %d, first at %s" % (
        what, int(d.sum()), d.size, int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max()), tuple(np.argwhere(d)[0]))


# ================================================================================================================ 1. exact known results
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_identity_and_flip_are_the_slice(layout, filt):
    u8 = _canvas(2, 32, 32, layout, 1)
    got = _hwc(_run(u8, 32, _with([(0, 0, 32, 32, 0), (0, 0, 32, 32, 1)], filt), layout), layout)
    src = _hwc(u8, layout)
    assert np.array_equal(got[0], src[0]) and np.array_equal(got[1], src[1][:, ::-1])
    u8 = _canvas(2, 40, 56, layout, 2)
    got = _hwc(_run(u8, 24, _with([(7, 13, 24, 24, 0), (7, 13, 24, 24, 1)], filt), layout), layout)
    sl = _hwc(u8, layout)[:, 7:31, 13:37]
    assert np.array_equal(got[0], sl[0]) and np.array_equal(got[1], sl[1][:, ::-1])
    # one 5 x 7 image: a batch of 105 bytes, more than 16 and no multiple of 16, and the box ends on its last byte -- the 16-byte load
    # that would cross the end of the batch is the one that goes byte by byte
    u8 = _canvas(1, 5, 7, layout, 3)
    src = _hwc(u8, layout)[0, 2:5, 4:7]
    for flip in (0, 1):
        got = _hwc(_run(u8, 3, [(2, 4, 3, 3, flip, filt)], layout), layout)[0]
        assert np.array_equal(got, src[:, ::-1] if flip else src), flip


@pytest.mark.parametrize("layout", LAYOUTS)
def test_integer_ratios_a_one_pixel_box_and_tiny_canvases(layout):
    u8 = _canvas(4, 50, 70, layout, 3)
    boxes = [(0, 0, 48, 32, 0), (2, 38, 48, 32, 1), (1, 3, 32, 64, 0), (34, 6, 16, 48, 1)]
    for filters in (1, 2, [2, 1, 1, 2]):
        recs = _with(boxes, filters)
        _equal(_run(u8, 16, recs, layout), RR.resample(u8, 16, recs, layout), "%s 48 x 32 -> 16 filters %s" % (layout, filters))
    # bilinear at ratio 2 along the width: taps 2 o - 1 .. 2 o + 2 weigh 1, 3, 3, 1 (eighths); the two border windows lose a tap
    src = _hwc(u8, layout)
    got = _hwc(_run(u8[:1], 16, [(0, 0, 16, 32, 0, 1)], layout), layout)[0]
    rows = src[0][0:16, 0:32].astype(np.int64)
    K = np.array([1 << 19, 3 << 19, 3 << 19, 1 << 19])
    inner = ((1 << 21) + sum(K[i] * rows[:, 1 + i:29 + i:2] for i in range(4))) >> 22
    assert np.array_equal(got[:, 1:15], inner)
    for S in (1, 5, 8):
        recs = _with([(3, 4, 1, 1, 0), (49, 69, 1, 1, 1), (0, 69, 1, 1, 0), (49, 0, 1, 1, 1)], [1, 2, 2, 1])
        got = _hwc(_run(u8, S, recs, layout), layout)
        for b, (y, x) in enumerate([(3, 4), (49, 69), (0, 69), (49, 0)]):
            assert np.array_equal(got[b], np.broadcast_to(src[b][y, x], (S, S, 3))), (S, b)
    # batches smaller than one 16-byte load: a 1 x 1 canvas (3 bytes) and a 2 x 2 one (12 bytes), read byte by byte
    for filt in FILTERS:
        tiny = _canvas(1, 1, 1, layout, 9)
        assert np.array_equal(_hwc(_run(tiny, 3, [(0, 0, 1, 1, 1, filt)], layout), layout)[0], np.broadcast_to(_hwc(tiny, layout)[0][0, 0], (3, 3, 3)))
        tiny = _canvas(1, 2, 2, layout, 10)
        assert np.array_equal(_run(tiny, 2, [(0, 0, 2, 2, 0, filt)], layout), tiny)
        _equal(_run(tiny, 4, [(0, 0, 2, 2, 1, filt)], layout), RR.resample(tiny, 4, [(0, 0, 2, 2, 1, filt)], layout), "2 x 2 -> 4")


# ================================================================================================================ 2. general boxes
@pytest.mark.parametrize("S", [16, 24, 31])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_general_boxes_equal_the_restatement(layout, S):
    u8 = _canvas(5, 40, 56, layout, 4)
    for name, boxes in (("A", BOXES_A), ("B", BOXES_B)):
        for filters in (1, 2, [1, 2, 2, 1, 2]):
            recs = _with(boxes, filters)
            _equal(_run(u8, S, recs, layout), RR.resample(u8, S, recs, layout), "%s 40x56 -> %d boxes %s filters %s" % (layout, S, name, filters))


# ================================================================================================================ 3. the feature
def _patterns(layout):
    """two 96 x 128 canvases of one-pixel patterns at 0 / 255.  0: vertical stripes above a checkerboard; 1: quadrants of vertical
    stripes, horizontal stripes, checkerboard and the inverted vertical stripes"""
    y, x = np.mgrid[0:96, 0:128]
    v, h, c = (x & 1) * 255, (y & 1) * 255, ((x ^ y) & 1) * 255
    a = np.where(y < 48, v, c)
    b = np.where(y < 48, np.where(x < 64, v, h), np.where(x < 64, c, 255 - v))
    hwc = np.repeat(np.stack([a, b])[..., None], 3, axis=3).astype(np.uint8)
    return np.ascontiguousarray(hwc.transpose(0, 3, 1, 2)) if layout == "nchw" else hwc


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_strong_downscale_is_antialiased(layout, filt):
    """the whole 96 x 128 canvas to 24: 4 x along the height, 5.33 x along the width.  The two-tap sample of ap_crop_resize_u8 reads 2 of
    5.33 columns at fractions 1/6, 1/2, 5/6 between a black and a white one: the vertical stripes come out as a pattern between 42 and
    212.  (Along the height, at the exact ratio 4, it lands midway between two rows and returns their mean, which hides horizontal stripes
    and the checkerboard by coincidence: the canvases carry vertical stripes in every image.)  The antialiased filters weigh all of them:
    grey, within a few levels"""
    from autoprog_amd import ops
    u8 = _patterns(layout)
    recs = _with([(0, 0, 96, 128, 0), (0, 0, 96, 128, 1)], filt)
    got = _run(u8, 24, recs, layout)
    _equal(got, RR.resample(u8, 24, recs, layout), "%s stripes 96 x 128 -> 24 filter %d" % (layout, filt))
    rec = torch.from_numpy(_records([r[:5] + (0,) for r in recs]))
    plain = ops.crop_resize_u8(torch.from_numpy(u8).cuda(), 24, rec.cuda(), layout=layout, host_records=rec).cpu().numpy()
    share = float((got != plain).mean())
    spread = [(int(a.max()) - int(a.min()), int(p.max()) - int(p.min())) for a, p in zip(got, plain)]
    print("RESAMPLE %s filter %d | %.1f %% of the bytes differ from the two-tap sample; spread (antialiased, two-tap) per image %s" % (layout, filt, 100 * share, spread))
    assert share > 0.005, "only %.3f %% of the bytes differ from the two-tap sample" % (100 * share)
    assert all(a < p for a, p in spread), "spread (antialiased, two-tap) per image: %s" % (spread,)


# ================================================================================================================ 4. several tiles per image
@pytest.mark.parametrize("S", [48, 33])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_vertical_supports_cross_tile_borders(layout, S):
    """160 x 144 -> 48 and -> 33: three tiles of 16 output rows whose vertical windows (up to 21 taps) reach into the neighbours' rows"""
    u8 = _canvas(2, 160, 144, layout, 11)
    for boxes in ([(0, 0, 160, 144, 0), (0, 0, 160, 144, 1)], [(0, 0, 77, 91, 1), (83, 53, 77, 91, 0)], [(101, 0, 59, 144, 0), (0, 99, 160, 45, 1)]):
        for filters in ([1, 2], [2, 1]):
            recs = _with(boxes, filters)
            _equal(_run(u8, S, recs, layout), RR.resample(u8, S, recs, layout), "%s 160x144 -> %d %s" % (layout, S, recs))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_drawn_batch_at_256_to_224_and_the_centre_crop(layout):
    from autoprog_amd.data import DeviceRandomResizedCrop
    u8 = _canvas(2, 256, 256, layout, 5)
    c = DeviceRandomResizedCrop(interpolation="random", seed=3, layout=layout)
    got = c.crop(torch.from_numpy(u8).cuda(), 224).cpu().numpy()
    assert len(c.last) == 2 and all(len(r) == 6 and r[5] in (1, 2) for r in c.last)
    _equal(got, RR.resample(u8, 224, c.last, layout), "%s 256 -> 224 drawn %s" % (layout, c.last))
    state = c._py.getstate()
    got = c.center(torch.from_numpy(u8).cuda(), 224, 0.96, interpolation="bicubic").cpu().numpy()
    assert c.last == [(5, 5, 246, 246, 0, 2)] * 2 and c._py.getstate() == state
    _equal(got, RR.resample(u8, 224, c.last, layout), "%s centre 0.96 bicubic" % layout)
    plain = DeviceRandomResizedCrop(seed=3, layout=layout)         # interpolation=None: the two-tap kernel, 5-tuples
    plain.crop(torch.from_numpy(u8).cuda(), 224)
    assert all(len(r) == 5 for r in plain.last)


# ================================================================================================================ 5. locality
@pytest.mark.parametrize("layout", LAYOUTS)
def test_bytes_outside_the_boxes_do_not_matter(layout):
    u8 = _canvas(5, 40, 56, layout, 6)
    recs = _with(BOXES_A, [2, 1, 2, 1, 2])
    ref = [_run(u8, S, recs, layout) for S in (16, 31)]
    g = np.random.RandomState(60)
    for trial in range(2):
        v = _hwc(u8.copy(), layout)                                # a view: writes land in the copy
        keep = np.zeros(v.shape[:3], dtype=bool)
        for b, (top, left, h, w, _) in enumerate(BOXES_A):
            keep[b, top:top + h, left:left + w] = True
        v[~keep] = g.randint(0, 256, v[~keep].shape)
        base = v.transpose(0, 3, 1, 2) if layout == "nchw" else v
        for S, r in zip((16, 31), ref):
            assert np.array_equal(_run(np.ascontiguousarray(base), S, recs, layout), r)


@pytest.mark.parametrize("lead", [64, 37])
@pytest.mark.parametrize("S", [24, 31])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_guard_bytes_around_the_output_stay(layout, S, lead):
    """the output as a view into a larger allocation (16-byte aligned, and at an odd address with an odd S: byte stores), sentinel bytes
    before and after"""
    u8 = _canvas(5, 40, 56, layout, 7)
    recs = _with(BOXES_B, [1, 2, 1, 2, 2])
    n = 5 * 3 * S * S
    buf = torch.full((lead + n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    view = buf[lead:lead + n].view((5, 3, S, S) if layout == "nchw" else (5, S, S, 3))
    got = _run(u8, S, recs, layout, out=view)
    _equal(got, RR.resample(u8, S, recs, layout), "%s -> %d into a view at byte %d" % (layout, S, lead))
    host = buf.cpu().numpy()
    assert (host[:lead] == 0xA5).all() and (host[lead + n:] == 0xA5).all()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_record_the_host_never_saw_is_clamped(layout):
    """no records_host: boxes that overhang the canvas and filter codes outside {1, 2} give the clamped box under bilinear"""
    u8 = _canvas(3, 40, 56, layout, 8)
    wild = [(30, 40, 20, 30, 1, 7), (-5, -3, 100, 100, 0, 7), (39, 55, 0, -4, 1, 0)]
    tame = [(20, 26, 20, 30, 1, 1), (0, 0, 40, 56, 0, 1), (39, 55, 1, 1, 1, 1)]
    _equal(_run(u8, 17, wild, layout, host=False), RR.resample(u8, 17, tame, layout), "%s clamped records" % layout)


def test_ops_wrapper_refusals():
    from autoprog_amd import ops
    from autoprog_amd._lib import AutoProgHipError
    u8 = torch.zeros(2, 3, 8, 8, dtype=torch.uint8).cuda()
    rec = torch.from_numpy(_records([(0, 0, 8, 8, 0, 1)] * 2)).cuda()
    for bad in (lambda: ops.crop_resample_u8(u8.float(), 8, rec), lambda: ops.crop_resample_u8(u8, 8, rec[:1]), lambda: ops.crop_resample_u8(u8, 0, rec),
                lambda: ops.crop_resample_u8(u8, 8, rec, layout="nhwc"),
                lambda: ops.crop_resample_u8(u8, 8, rec, out=torch.zeros(2, 3, 9, 9, dtype=torch.uint8).cuda()),
                lambda: ops.crop_resample_u8(u8, 8, rec, host_records=torch.from_numpy(_records([(0, 0, 8, 8, 0, 1), (0, 0, 8, 8, 0, 0)]))),
                lambda: ops.crop_resample_u8(u8, 8, rec, host_records=torch.from_numpy(_records([(0, 0, 8, 8, 0, 3), (0, 0, 8, 8, 0, 2)])))):
        with pytest.raises(AutoProgHipError):
            bad()
    assert tuple(ops.crop_resample_u8(u8[:0], 8, rec).shape) == (0, 3, 8, 8)


# ================================================================================================================ 6. pipeline
def _drive(monkeypatch, use_graphs, steps=4):
    from autoprog_amd import ops
    from autoprog_amd.data import DeviceBatchPrep, DeviceRandomResizedCrop
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import TokenLabelCrossEntropy
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import FlatAdamWEma
    from autoprog_amd.prog.driver import AutoProgDriver
    monkeypatch.setattr(ops, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)      # the 16-channel stem runs on the vendor convolution
    torch.manual_seed(0)
    model = create_model("model_variant", variant="volo_h2_l3", num_classes=16, img_size=64, stem_hidden_dim=16).cuda().train()
    red = GradientBucketReducer(list(model.parameters()), world_size=1, defer_mean=True)
    red.install_sink(model)
    opt = FlatAdamWEma(model, red, lr=1e-3, weight_decay=0.05, ema_decays=[0.9])
    prep = DeviceBatchPrep(MEAN, STD, num_classes=16, seed=5)
    crop = DeviceRandomResizedCrop(seed=7, interpolation="random")
    loss_fn = TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=16)
    g = torch.Generator().manual_seed(1)
    log = []

    def get_batch(r):
        u8 = torch.randint(0, 256, (8, 3, 80, 112), dtype=torch.uint8, generator=g).cuda()
        return u8, torch.softmax(torch.randn(8, 16, 2 + (r // 16) ** 2, generator=g) * 2, dim=1).cuda()

    real_prep = prep.prep
    monkeypatch.setattr(prep, "prep", lambda u8: (log.append((tuple(u8.shape), u8.dtype, list(crop.last))), real_prep(u8))[1])
    drv = AutoProgDriver(model, loss_fn, opt, red, get_batch, r_list=[64, 96], l_list=[3, 3], dp_list=[0.0, 0.0], grow_epochs=[0, 1],
                         steps_per_epoch=steps, auto_grow=False, use_graphs=use_graphs, graph_after=2, batch_prep=prep, crop=crop,
                         resize_list=[[0.35, 1.0], [0.08, 1.0]])
    losses, real = [], drv._train_step
    monkeypatch.setattr(drv, "_train_step", lambda *a, **k: (losses.append(real(*a, **k)), losses[-1])[1])
    try:
        np.random.seed(3)
        drv.run(2)
        return [float(v) for v in losses], log
    finally:
        red.remove()


def test_antialiased_random_crop_under_the_driver_eager_and_graphed(monkeypatch):
    """as the two-tap crop's driver test: two stages (r = 64, 96) on 80 x 112 canvases, the uint8 tensor handed to prep has side r, every
    record carries a filter and both filters occur, losses are finite, and with DropPath 0 and equal seeds the run from graphs gives the
    eager run's losses bit for bit"""
    le, log = _drive(monkeypatch, False)
    assert [p[0] for p in log] == [(8, 3, 64, 64)] * 4 + [(8, 3, 96, 96)] * 4 and all(p[1] == torch.uint8 for p in log)
    for _, _, recs in log:
        assert len(recs) == 8 and all(h >= 1 and w >= 1 and top >= 0 and left >= 0 and top + h <= 80 and left + w <= 112 and f in (1, 2)
                                      for top, left, h, w, _, f in recs)
    assert {r[5] for _, _, recs in log for r in recs} == {1, 2} and len({tuple(p[2]) for p in log}) == 8
    assert len(le) == 8 and all(np.isfinite(v) for v in le)
    lg, log_g = _drive(monkeypatch, True)
    print("RESAMPLE driver eager:", le)
    print("RESAMPLE driver graph:", lg)
    assert [p[2] for p in log_g] == [p[2] for p in log]
    assert le == lg, (le, lg)
