"""ap_crop_resize_u8 / ops.crop_resize_u8 / data.DeviceRandomResizedCrop on the GPU, both layouts throughout: boxes whose result is known
exactly (identity, flips, integer ratios, a 1 x 1 box) bit for bit; general boxes against the float64 restatement of tests/_crop_ref.py
under the cap tests/test_device_crop_host.py derives for float32 arithmetic (no byte off by more than 1, at most 0.5 % of the bytes off by
1); independence from every byte outside the boxes; guard bytes around the output; and the crop in front of DeviceBatchPrep under
AutoProgDriver, eager and from graphs."""
import numpy as np
import pytest
import torch

from tests import _crop_ref as CR

pytestmark = pytest.mark.gpu
LAYOUTS = ["nchw", "nhwc"]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _canvas(B, H, W, layout, seed):
    """uint8 numpy [B,3,H,W] / [B,H,W,3] of random bytes (the same pixels in both layouts)"""
    hwc = np.random.RandomState(seed).randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    return np.ascontiguousarray(hwc.transpose(0, 3, 1, 2)) if layout == "nchw" else hwc


def _hwc(a, layout):
    return a.transpose(0, 2, 3, 1) if layout == "nchw" else a


def _records(boxes):
    r = np.zeros((len(boxes), 8), dtype=np.int32)
    r[:, :5] = boxes
    return r


def _run(u8, S, boxes, layout, out=None):
    from autoprog_amd import ops
    rec = torch.from_numpy(_records(boxes))
    y = ops.crop_resize_u8(torch.from_numpy(u8).cuda(), S, rec.cuda(), layout=layout, out=out, host_records=rec)
    assert y.dtype == torch.uint8 and tuple(y.shape) == ((len(boxes), 3, S, S) if layout == "nchw" else (len(boxes), S, S, 3))
    return y.cpu().numpy()


def _within_cap(got, want, what):
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    off, worst = int((d > 0).sum()), int(d.max())
    print("CROP %s | %d of %d bytes differ from the float64 reference (%.3f %%), largest difference %d" % (what, off, d.size, 100.0 * off / d.size, worst))
    assert worst <= 1 and off <= 0.005 * d.size, (what, off, d.size, worst)


# ================================================================================================================ 1. exact cases
@pytest.mark.parametrize("layout", LAYOUTS)
def test_identity_and_flip_are_the_slice(layout):
    u8 = _canvas(2, 32, 32, layout, 1)
    got = _hwc(_run(u8, 32, [(0, 0, 32, 32, 0), (0, 0, 32, 32, 1)], layout), layout)
    src = _hwc(u8, layout)
    assert np.array_equal(got[0], src[0]) and np.array_equal(got[1], src[1][:, ::-1])
    u8 = _canvas(2, 40, 56, layout, 2)
    got = torch.from_numpy(_run(u8, 24, [(7, 13, 24, 24, 0), (7, 13, 24, 24, 1)], layout))
    t = torch.from_numpy(u8)
    sl = t[:, :, 7:31, 13:37] if layout == "nchw" else t[:, 7:31, 13:37]
    assert torch.equal(got[0], sl[0]) and torch.equal(got[1], sl[1].flip(2 if layout == "nchw" else 1))
    # one 5 x 7 image: a batch of 105 bytes, more than 16 and no multiple of 16, and the box ends on its last byte -- the 16-byte load
    # that would cross the end of the batch is the one that goes byte by byte
    u8 = _canvas(1, 5, 7, layout, 3)
    src = _hwc(u8, layout)[0, 2:5, 4:7]
    for flip in (0, 1):
        got = _hwc(_run(u8, 3, [(2, 4, 3, 3, flip)], layout), layout)[0]
        assert np.array_equal(got, src[:, ::-1] if flip else src), flip


@pytest.mark.parametrize("layout", LAYOUTS)
def test_integer_ratios_and_a_one_pixel_box(layout):
    """48 x 32 -> 16: the row ratio 3 picks row 3 o + 1, the column ratio 2 takes the half-even-rounded mean of two columns"""
    u8 = _canvas(4, 50, 70, layout, 3)
    boxes = [(0, 0, 48, 32, 0), (2, 38, 48, 32, 1), (1, 3, 32, 64, 0), (34, 6, 16, 48, 1)]
    got = _hwc(_run(u8, 16, boxes, layout), layout)
    src = _hwc(u8, layout)
    for b, box in enumerate(boxes):
        assert np.array_equal(got[b], CR.crop_resize_int(src[b], 16, box)), box
    rows = src[0][1:48:3, 0:32].astype(np.int64)                                # rows 3 o + 1; columns 2 o, 2 o + 1
    s = rows[:, 0::2] + rows[:, 1::2]
    assert np.array_equal(got[0], (s // 2 + ((s % 2 == 1) & ((s // 2) % 2 == 1))).astype(np.uint8))
    for S in (1, 5, 8):
        got = _hwc(_run(u8, S, [(3, 4, 1, 1, 0), (49, 69, 1, 1, 1), (0, 69, 1, 1, 0), (49, 0, 1, 1, 1)], layout), layout)
        for b, (y, x) in enumerate([(3, 4), (49, 69), (0, 69), (49, 0)]):
            assert np.array_equal(got[b], np.broadcast_to(src[b][y, x], (S, S, 3))), (S, b)
    # batches smaller than one 16-byte load: a 1 x 1 canvas (3 bytes) and a 2 x 2 one (12 bytes), read byte by byte
    tiny = _canvas(1, 1, 1, layout, 9)
    assert np.array_equal(_hwc(_run(tiny, 3, [(0, 0, 1, 1, 1)], layout), layout)[0], np.broadcast_to(_hwc(tiny, layout)[0][0, 0], (3, 3, 3)))
    tiny = _canvas(1, 2, 2, layout, 10)
    assert np.array_equal(_run(tiny, 2, [(0, 0, 2, 2, 0)], layout), tiny)
    assert np.array_equal(_hwc(_run(tiny, 4, [(0, 0, 2, 2, 1)], layout), layout)[0],
                          CR.crop_resize_one(_hwc(tiny, layout)[0], 4, (0, 0, 2, 2, 1), np.float32))      # (every weight is 0.25 or 0.75: exact)


# ================================================================================================================ 2. general cases
# whole image; a box in each corner; an upscale (h < S at every S), a downscale (h > S at every S); one-pixel-wide and one-pixel-high boxes
BOXES_A = [(0, 0, 40, 56, 0), (0, 0, 10, 12, 1), (0, 23, 37, 33, 0), (15, 0, 25, 40, 1), (31, 6, 9, 50, 0)]
BOXES_B = [(0, 0, 40, 56, 1), (3, 5, 33, 47, 0), (11, 2, 5, 51, 1), (0, 55, 40, 1, 0), (39, 0, 1, 56, 1)]


@pytest.mark.parametrize("S", [16, 24, 31])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_general_boxes_against_the_float64_reference(layout, S):
    u8 = _canvas(5, 40, 56, layout, 4)
    for name, boxes in (("A", BOXES_A), ("B", BOXES_B)):
        _within_cap(_run(u8, S, boxes, layout), CR.crop_resize(u8, S, boxes, layout, np.float64), "%s 40x56 -> %d boxes %s" % (layout, S, name))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_drawn_batch_at_256_to_224(layout):
    """more than one tile per image and the class's own draws, through DeviceRandomResizedCrop.crop; then the centre crop"""
    from autoprog_amd.data import DeviceRandomResizedCrop
    u8 = _canvas(2, 256, 256, layout, 5)
    c = DeviceRandomResizedCrop(seed=3, layout=layout, size=224)
    got = c.crop(torch.from_numpy(u8).cuda()).cpu().numpy()
    assert len(c.last) == 2 and got.shape == ((2, 3, 224, 224) if layout == "nchw" else (2, 224, 224, 3))
    _within_cap(got, CR.crop_resize(u8, 224, c.last, layout, np.float64), "%s 256 -> 224 drawn %s" % (layout, c.last))
    got = c.center(torch.from_numpy(u8).cuda(), 224).cpu().numpy()
    assert c.last == [(16, 16, 224, 224, 0)] * 2
    src = _hwc(u8, layout)[:, 16:240, 16:240]
    assert np.array_equal(_hwc(got, layout), src)


# ================================================================================================================ 3. dependence
@pytest.mark.parametrize("layout", LAYOUTS)
def test_bytes_outside_the_boxes_do_not_matter(layout):
    u8 = _canvas(5, 40, 56, layout, 6)
    outs = []
    for fill in (0, 255):
        v = _hwc(u8.copy(), layout)                                # a view: writes land in the copy
        keep = np.zeros(v.shape[:3], dtype=bool)
        for b, (top, left, h, w, _) in enumerate(BOXES_A):
            keep[b, top:top + h, left:left + w] = True
        v[~keep] = fill
        base = v.transpose(0, 3, 1, 2) if layout == "nchw" else v
        outs.append([_run(np.ascontiguousarray(base), S, BOXES_A, layout) for S in (16, 31)])
    ref = [_run(u8, S, BOXES_A, layout) for S in (16, 31)]
    for a, b, r in zip(outs[0], outs[1], ref):
        assert np.array_equal(a, b) and np.array_equal(a, r)


# ================================================================================================================ 4. guards
@pytest.mark.parametrize("lead", [64, 37])
@pytest.mark.parametrize("S", [24, 31])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_guard_bytes_around_the_output_stay(layout, S, lead):
    """the output as a view into a larger allocation (16-byte aligned, and at an odd address: byte stores), sentinel bytes before and
    after; a second call into the same buffers gives the same bytes"""
    u8 = _canvas(5, 40, 56, layout, 7)
    n = 5 * 3 * S * S
    buf = torch.full((lead + n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    view = buf[lead:lead + n].view((5, 3, S, S) if layout == "nchw" else (5, S, S, 3))
    first = _run(u8, S, BOXES_B, layout, out=view)
    assert np.array_equal(first, _run(u8, S, BOXES_B, layout))     # (the same bytes as into a fresh tensor)
    host = buf.cpu().numpy()
    assert (host[:lead] == 0xA5).all() and (host[lead + n:] == 0xA5).all()
    second = _run(u8, S, BOXES_B, layout, out=view)
    assert np.array_equal(first, second)
    host = buf.cpu().numpy()
    assert (host[:lead] == 0xA5).all() and (host[lead + n:] == 0xA5).all()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_offsets_past_2_gib(layout):
    """10 928 canvases of 256 x 256 (2.15 GB in) to S = 256 (2.15 GB out): the images whose input and output offsets lie past 2^31 bytes.
    Identity boxes come back as the canvas, flipped ones as its mirror (torch.equal on the device, every image); the last three images
    carry general boxes and are held to the float64 reference"""
    from autoprog_amd import ops
    B, H, S = 10928, 256, 256
    assert (B - 3) * 3 * H * H > 2 ** 31
    u8 = torch.randint(0, 256, (B, 3, H, H) if layout == "nchw" else (B, H, H, 3), dtype=torch.uint8, device="cuda",
                       generator=torch.Generator(device="cuda").manual_seed(8))
    boxes = [(0, 0, H, H, b & 1) for b in range(B - 3)] + [(10, 20, 200, 131, 1), (0, 0, 256, 256, 0), (101, 3, 77, 250, 0)]
    rec = torch.from_numpy(_records(boxes))
    out = ops.crop_resize_u8(u8, S, rec.cuda(), layout=layout, host_records=rec)
    wd = 3 if layout == "nchw" else 2
    assert torch.equal(out[0:B - 3:2], u8[0:B - 3:2]) and torch.equal(out[1:B - 3:2], u8[1:B - 3:2].flip(wd))
    tail = u8[B - 3:].cpu().numpy()
    _within_cap(out[B - 3:].cpu().numpy(), CR.crop_resize(tail, S, boxes[B - 3:], layout, np.float64), "%s past 2 GiB" % layout)


def test_ops_wrapper_refusals():
    from autoprog_amd import ops
    from autoprog_amd._lib import AutoProgHipError
    u8 = torch.zeros(2, 3, 8, 8, dtype=torch.uint8).cuda()
    rec = torch.from_numpy(_records([(0, 0, 8, 8, 0)] * 2)).cuda()
    for bad in (lambda: ops.crop_resize_u8(u8.float(), 8, rec), lambda: ops.crop_resize_u8(u8[0], 8, rec), lambda: ops.crop_resize_u8(u8, 8, rec[:1]),
                lambda: ops.crop_resize_u8(u8, 8, rec, layout="nhwc"), lambda: ops.crop_resize_u8(u8, 0, rec), lambda: ops.crop_resize_u8(u8, 8, rec.long()),
                lambda: ops.crop_resize_u8(u8, 8, rec, out=torch.zeros(2, 3, 9, 9, dtype=torch.uint8).cuda()),
                lambda: ops.crop_resize_u8(u8, 8, rec, host_records=torch.from_numpy(_records([(0, 0, 8, 8, 0), (1, 0, 8, 8, 0)])))):
        with pytest.raises(AutoProgHipError):
            bad()
    assert tuple(ops.crop_resize_u8(u8[:0], 8, rec).shape) == (0, 3, 8, 8)


# ================================================================================================================ 5. pipeline
def _drive(monkeypatch, use_graphs, with_teacher=False, steps=4):
    from autoprog_amd import ops
    from autoprog_amd.data import DeviceBatchPrep, DeviceRandomResizedCrop
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import TokenLabelCrossEntropy
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import FlatAdamWEma
    from autoprog_amd.prog.driver import AutoProgDriver
    from autoprog_amd.prog.teacher import TeacherLabeler
    monkeypatch.setattr(ops, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)      # the 16-channel stem runs on the vendor convolution
    torch.manual_seed(0)
    model = create_model("model_variant", variant="volo_h2_l3", num_classes=16, img_size=64, stem_hidden_dim=16).cuda().train()
    red = GradientBucketReducer(list(model.parameters()), world_size=1, defer_mean=True)
    red.install_sink(model)
    opt = FlatAdamWEma(model, red, lr=1e-3, weight_decay=0.05, ema_decays=[0.9])
    prep = DeviceBatchPrep(MEAN, STD, num_classes=16, seed=5)
    crop = DeviceRandomResizedCrop(seed=7)
    loss_fn = TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=16)
    g = torch.Generator().manual_seed(1)
    log = dict(prep=[], scale=[], taught=[])

    def get_batch(r):
        log["scale"].append(crop.scale)
        u8 = torch.randint(0, 256, (8, 3, 80, 112), dtype=torch.uint8, generator=g).cuda()
        if with_teacher:
            return u8, torch.randint(0, 16, (8,), generator=g).cuda()
        return u8, torch.softmax(torch.randn(8, 16, 2 + (r // 16) ** 2, generator=g) * 2, dim=1).cuda()

    real_prep = prep.prep
    monkeypatch.setattr(prep, "prep", lambda u8: (log["prep"].append((tuple(u8.shape), u8.dtype, list(crop.last))), real_prep(u8))[1])
    teacher = None
    if with_teacher:
        torch.manual_seed(9)
        labeler = TeacherLabeler(create_model("model_variant", variant="volo_h2_l3", num_classes=16, img_size=64, stem_hidden_dim=64).cuda().eval(),
                                 k=5, num_classes=16)

        def teacher(images, labels, r):
            t = labeler(images, labels, r)
            log["taught"].append((type(images).__name__, tuple(images.shape), r, tuple(t.idx.shape)))
            return t
        teacher.num_classes = 16
    drv = AutoProgDriver(model, loss_fn, opt, red, get_batch, r_list=[64, 96], l_list=[3, 3], dp_list=[0.0, 0.0], grow_epochs=[0, 1],
                         steps_per_epoch=steps, auto_grow=False, use_graphs=use_graphs, graph_after=2, batch_prep=prep, crop=crop,
                         resize_list=[[0.35, 1.0], [0.08, 1.0]], teacher=teacher)
    losses, real = [], drv._train_step
    monkeypatch.setattr(drv, "_train_step", lambda *a, **k: (losses.append(real(*a, **k)), losses[-1])[1])
    try:
        np.random.seed(3)
        drv.run(2)
        return [float(v) for v in losses], log, crop
    finally:
        red.remove()


def test_crop_in_front_of_the_preparation_under_the_driver_eager_and_graphed(monkeypatch):
    """two stages (r = 64, 96) on 80 x 112 canvases: the uint8 tensor handed to prep has side r, crop.scale follows resize_list from the
    first batch of each stage, every box lies in the canvas, losses are finite, and with DropPath 0 and equal seeds the run from graphs
    gives the eager run's losses bit for bit"""
    le, log, crop = _drive(monkeypatch, False)
    assert log["scale"] == [(0.35, 1.0)] * 4 + [(0.08, 1.0)] * 4 and crop.scale == (0.08, 1.0)
    assert [p[0] for p in log["prep"]] == [(8, 3, 64, 64)] * 4 + [(8, 3, 96, 96)] * 4 and all(p[1] == torch.uint8 for p in log["prep"])
    for _, _, boxes in log["prep"]:
        assert len(boxes) == 8 and all(h >= 1 and w >= 1 and top >= 0 and left >= 0 and top + h <= 80 and left + w <= 112 for top, left, h, w, _ in boxes)
    assert len({tuple(p[2]) for p in log["prep"]}) == 8            # a fresh draw per step
    assert len(le) == 8 and all(np.isfinite(v) for v in le)
    lg, log_g, _ = _drive(monkeypatch, True)
    print("CROP driver eager:", le)
    print("CROP driver graph:", lg)
    assert [p[2] for p in log_g["prep"]] == [p[2] for p in log["prep"]]
    assert le == lg, (le, lg)


def test_a_teacher_in_front_sees_the_cropped_batch(monkeypatch):
    _, log, _ = _drive(monkeypatch, False, with_teacher=True, steps=2)
    assert [t[:3] for t in log["taught"]] == [("PreparedBatch", (8, 3, 64, 64), 64)] * 2 + [("PreparedBatch", (8, 3, 96, 96), 96)] * 2
    assert [t[3] for t in log["taught"]] == [(8, 2 + 16, 5)] * 2 + [(8, 2 + 36, 5)] * 2
