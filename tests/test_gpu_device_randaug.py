"""ap_randaug_u8 / ops.randaug_u8 / data.DeviceRandAugment on the GPU, both layouts throughout.  The criterion everywhere is
np.array_equal with the numpy restatement of Pillow's pixel rules (tests/_randaug_ref.py, held to Pillow's own bytes by
tests/test_device_randaug_host.py): table ops are integer arithmetic on exact counts, the blends are single float32 operations and the
affine samples single float64 operations, each rounded on its own on both sides, so there is no tolerance."""
import functools

import numpy as np
import pytest
import torch

from tests import _randaug_ref as R

pytestmark = pytest.mark.gpu
LAYOUTS = ["nchw", "nhwc"]
FILL = (124, 116, 104)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
NAN = float("nan")


def _rec(op, filt=0, iarg=0, farg=0.0, m=R.NO_MATRIX):
    return (op, filt, iarg, float(np.float32(farg)), tuple(float(v) for v in m))


def _block(records):
    from autoprog_amd import ops
    from autoprog_amd.data import DeviceRandAugment
    n = len(records[0]) if records else 1
    block = np.zeros(max(len(records) * n, 1) * ops.RANDAUG_RECORD_WORDS, dtype=np.int32)
    DeviceRandAugment.pack(records, block)
    return torch.from_numpy(block)


def _layout(hwc, layout):
    return np.array(hwc.transpose(0, 3, 1, 2) if layout == "nchw" else hwc, order="C")      # (a writable copy either way)


def _run(hwc, records, layout, host=True, fill=FILL, **kw):
    """hwc: uint8 [B,S,S,3] -> the kernel's result, back in [B,S,S,3]; the input must come through unchanged"""
    from autoprog_amd import ops
    block = _block(records)
    src = torch.from_numpy(_layout(hwc, layout)).cuda()
    keep = src.clone()
    y = ops.randaug_u8(src, block.cuda(), len(records[0]) if records else 1, fill, layout=layout, host_records=block if host else None, **kw)
    assert y.dtype == torch.uint8 and y.shape == src.shape and y.data_ptr() != src.data_ptr() and torch.equal(src, keep)
    return R.hwc(y.cpu().numpy(), layout)


def _equal(got, want, what, records=None):
    d = got != want
    if d.any():
        b = int(np.argwhere(d)[0][0])
        raise AssertionError("%s: %d of %d bytes differ from the restatement, largest difference %d, first at %s%s" % (
            what, int(d.sum()), d.size, int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max()), tuple(np.argwhere(d)[0]),
            "" if records is None else ", record %s" % (records[b],)))


def catalogue(S):
    """every op code at its extremes and in between, every affine case: one record each"""
    out = [_rec(R.NONE), _rec(R.AUTOCONTRAST), _rec(R.EQUALIZE), _rec(R.INVERT)]
    out += [_rec(R.SOLARIZE, iarg=t) for t in (0, 77, 128, 256)] + [_rec(R.SOLARIZE_ADD, iarg=a) for a in (0, 55, 110)]
    out += [_rec(R.POSTERIZE, iarg=b) for b in (0, 1, 3, 4, 8)]
    out += [_rec(op, farg=f) for op in (R.BRIGHTNESS, R.CONTRAST, R.COLOR, R.SHARPNESS) for f in (0.0, 0.1, 0.55, 1.0, 1.45, 1.9)]
    for filt in (R.BILINEAR, R.BICUBIC):
        for s in (1, -1):
            out += [_rec(R.AFFINE, filt, m=(1, 0.3 * s, 0, 0, 1, 0)), _rec(R.AFFINE, filt, m=(1, 0, 0, 0.3 * s, 1, 0)),
                    _rec(R.AFFINE, filt, m=(1, 0, 0.45 * s * S, 0, 1, 0)), _rec(R.AFFINE, filt, m=(1, 0, 0, 0, 1, 0.45 * s * S)),
                    _rec(R.AFFINE, filt, m=R.rotate_matrix(30.0 * s, S)), _rec(R.AFFINE, filt, m=R.rotate_matrix(11.7 * s, S)),
                    _rec(R.AFFINE, filt, m=(1, 0, 1.5 * s * S, 0, 1, 0)), _rec(R.AFFINE, filt, m=(1, 0, 0, 0, 1, -2.0 * s * S))]      # all fill
        out += [_rec(R.AFFINE, filt, m=R.IDENTITY), _rec(R.AFFINE, filt, m=(1, 0, 0.5, 0, 1, 0.25)), _rec(R.AFFINE, filt, m=(0.7, 0.2, -0.4, -0.1, 1.3, 0.6)),
                _rec(R.AFFINE, filt, m=(NAN,) * 6), _rec(R.AFFINE, filt, m=(1, 0, NAN, 0, 1, 0)), _rec(R.AFFINE, filt, m=(1e300, 0, 0, 0, 1e300, 0)),
                _rec(R.AFFINE, filt, m=(1, 1e300, 0, 0, 1, -1e300)), _rec(R.AFFINE, filt, m=(1, 0, float("inf"), 0, 1, 0))]
    return out


KINDS = ("random", "constant", "two_valued", "extremes")


def image(kind, S, seed):
    g = np.random.RandomState(seed)
    if kind == "random":
        return g.randint(0, 256, (S, S, 3)).astype(np.uint8)
    if kind == "constant":                                         # the identity branches of AutoContrast and Equalize
        return np.full((S, S, 3), (0, 93, 255), dtype=np.uint8)
    if kind == "two_valued":                                       # per channel two values: Equalize's step from the smaller bin
        img = np.where(g.randint(0, 4, (S, S, 3)) > 0, np.array([200, 31, 255]), np.array([40, 30, 254])).astype(np.uint8)
        img[0, 0], img[-1, -1] = (40, 30, 254), (200, 31, 255)
        return img
    img = (g.randint(0, 2, (S, S, 3)) * 255).astype(np.uint8)       # values at 0 and 255: both clip branches of blend
    img[0, 0], img[-1, -1] = 0, 255
    return img


@functools.lru_cache(maxsize=None)
def expected(kind, S):
    """(input [N,S,S,3], records, restatement's result [N,S,S,3]) of the catalogue on one image kind: computed once for both layouts"""
    recs = catalogue(S)
    hwc = np.stack([image(kind, S, 100 + S)] * len(recs))
    want = R.apply(hwc, [[r] for r in recs], FILL, "nhwc")
    hwc.setflags(write=False); want.setflags(write=False)
    return hwc, recs, want


# ================================================================================================================ 1. every op, every shape
@pytest.mark.parametrize("S", [1, 2, 3, 7, 33, 64])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_op_and_filter_equals_the_restatement(layout, S):
    """S = 3: the smallest Sharpness interior, every bicubic tap clamps (1 and 2: Pillow accepts every op there, Sharpness copies);
    3 and 7: fewer than 255 pixels, Equalize's step is 0; 33: bands of 16, 16 and 1 rows, the affine ops' 8 x 8 tiles overhang; 64: four
    bands"""
    for kind in KINDS:
        hwc, recs, want = expected(kind, S)
        _equal(_run(hwc, [[r] for r in recs], layout), want, "%s S %d %s" % (layout, S, kind), recs)


def test_known_results():
    """what needs no restatement: copies, the inverse, black, all-fill, and that the enhancers moved something"""
    hwc, recs, want = expected("random", 33)
    got = _run(hwc, [[r] for r in recs], "nchw")
    fill = np.broadcast_to(np.asarray(FILL, dtype=np.uint8), (33, 33, 3))
    for b, (op, filt, iarg, farg, m) in enumerate(recs):
        if op == R.AUTOCONTRAST:                                   # (random bytes span 0 .. 255 or nearly: a copy or nearly one)
            continue
        if op == R.NONE or (op == R.AFFINE and m == R.IDENTITY) or (op >= R.BRIGHTNESS and op != R.AFFINE and farg == 1.0) \
                or (op, iarg) in ((R.SOLARIZE, 256), (R.POSTERIZE, 8), (R.SOLARIZE_ADD, 0)):
            assert np.array_equal(got[b], hwc[b]), recs[b]
        elif op == R.INVERT or (op, iarg) == (R.SOLARIZE, 0):
            assert np.array_equal(got[b], 255 - hwc[b]), recs[b]
        elif (op, iarg) == (R.POSTERIZE, 0):
            assert not got[b].any()
        elif op == R.AFFINE and (any(v != v or abs(v) > 1e6 for v in m) or abs(m[2]) > 33 or abs(m[5]) > 33):
            assert np.array_equal(got[b], fill), recs[b]
        else:
            assert not np.array_equal(got[b], hwc[b]), recs[b]


# ================================================================================================================ 2. layers and batches
def _chains(S, B, n, seed):
    g = np.random.RandomState(seed)
    cat = [r for r in catalogue(S) if r[0] != R.NONE]
    return [[cat[int(g.randint(len(cat)))] for _ in range(n)] for _ in range(B)]


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_layers_apply_in_order(layout, B, n):
    for S, seed in ((33, 1), (20, 2)):
        hwc = np.stack([image(KINDS[b % 4], S, 7 * b + seed) for b in range(B)])
        recs = _chains(S, B, n, 10 * n + B + seed)
        _equal(_run(hwc, recs, layout), R.apply(hwc, recs, FILL, "nhwc"), "%s S %d B %d n %d" % (layout, S, B, n), recs)
    if n == 2:                                                     # order matters: Solarize then a rotation is not the rotation then Solarize
        hwc = image("random", 16, 3)[None]
        a, b = _rec(R.SOLARIZE, iarg=100), _rec(R.AFFINE, 2, m=R.rotate_matrix(30.0, 16))
        ab, ba = _run(hwc, [[a, b]], layout), _run(hwc, [[b, a]], layout)
        _equal(ab, R.apply(hwc, [[a, b]], FILL, "nhwc"), "a then b")
        _equal(ba, R.apply(hwc, [[b, a]], FILL, "nhwc"), "b then a")
        assert not np.array_equal(ab, ba)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_object_end_to_end_at_224(layout):
    """the natural mix of rand-m9-mstd0.5-inc1 on 6 images of 224 x 224 through DeviceRandAugment: the result is the restatement applied
    to aug.last; a second call draws other records into the same output buffer; fill is timm's img_mean"""
    from autoprog_amd.data import DeviceRandAugment
    hwc = np.stack([image("random", 224, 40 + b) for b in range(6)])
    aug = DeviceRandAugment(seed=21, layout=layout)
    src = torch.from_numpy(_layout(hwc, layout)).cuda()
    keep = src.clone()
    y = aug(src)
    first = aug.last
    assert aug.fill == FILL and len(first) == 6 and all(len(image) == 2 for image in first) and torch.equal(src, keep)
    assert len({r[0] for image in first for r in image}) >= 4, first
    _equal(R.hwc(y.cpu().numpy(), layout), R.apply(hwc, first, FILL, "nhwc"), "%s 224 drawn" % layout, first)
    y2 = aug(src)
    assert y2.data_ptr() == y.data_ptr() and aug.last != first
    _equal(R.hwc(y2.cpu().numpy(), layout), R.apply(hwc, aug.last, FILL, "nhwc"), "%s 224 second draw" % layout, aug.last)
    # a first call at a new shape inside a graph capture would allocate: refused, and nothing is drawn
    state = aug._py.getstate()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError):
            aug(src[:2])
        assert aug._py.getstate() == state
        assert aug(src).data_ptr() == y.data_ptr()                  # the buffers of a known shape exist
    assert aug._py.getstate() != state
    aug.set_spec("")
    assert aug(src) is src
    with pytest.raises(ValueError):
        aug.set_spec("rand-m9-w0")
    with pytest.raises(ValueError):
        DeviceRandAugment(layout=layout)(src[:, :, :100] if layout == "nchw" else src[:, :100])      # not square


# ================================================================================================================ 3. locality and wild records
@pytest.mark.parametrize("lead", [64, 37])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_guard_bytes_around_out_and_scratch_stay(layout, lead):
    """out and scratch as views into larger allocations (aligned, and at an odd address with an odd S: the byte path of the table ops),
    sentinel bytes before and after both; n = 2 and n = 3 (the ping-pong starts in the other buffer)"""
    S, B = 33, 5
    hwc = np.stack([image(KINDS[b % 4], S, 60 + b) for b in range(B)])
    nbytes = B * 3 * S * S
    shape = (B, 3, S, S) if layout == "nchw" else (B, S, S, 3)
    for n in (2, 3):
        recs = _chains(S, B, n, 70 + n)
        bufs = [torch.full((lead + nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
        out, scratch = (b[lead:lead + nbytes].view(shape) for b in bufs)
        got = _run(hwc, recs, layout, out=out, scratch=scratch)
        _equal(got, R.apply(hwc, recs, FILL, "nhwc"), "%s n %d into views at byte %d" % (layout, n, lead), recs)
        for b in bufs:
            host = b.cpu().numpy()
            assert (host[:lead] == 0xA5).all() and (host[lead + nbytes:] == 0xA5).all()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_records_the_host_never_saw(layout):
    """no records_host: an unknown op code copies, any filter code but bicubic samples bilinearly; shown to the host they are refused"""
    from autoprog_amd._lib import AutoProgHipError
    S = 20
    hwc = np.stack([image("random", S, 80 + b) for b in range(5)])
    m = R.rotate_matrix(-17.0, S)
    wild = [[(12, 0, 5, 1.5, R.IDENTITY)], [(-1, 2, 0, 0.0, m)], [(1 << 30, 1, 0, 0.0, m)], [_rec(R.AFFINE, 7, m=m)], [_rec(R.AFFINE, 0, m=m)]]
    tame = [[_rec(R.NONE)]] * 3 + [[_rec(R.AFFINE, 1, m=m)]] * 2
    _equal(_run(hwc, wild, layout, host=False), R.apply(hwc, tame, FILL, "nhwc"), "%s wild records" % layout)
    for k in (0, 1, 3, 4):
        with pytest.raises(AutoProgHipError):
            _run(hwc[:1], [wild[k]], layout)


def test_ops_wrapper_refusals_and_an_empty_batch():
    from autoprog_amd import ops
    from autoprog_amd._lib import AutoProgHipError
    u8 = torch.zeros(2, 3, 8, 8, dtype=torch.uint8).cuda()
    rec = _block([[_rec(R.INVERT)] * 2] * 2)
    dev = rec.cuda()
    for bad in (lambda: ops.randaug_u8(u8.float(), dev, 2, FILL), lambda: ops.randaug_u8(u8, dev[:40], 2, FILL), lambda: ops.randaug_u8(u8, dev, 0, FILL),
                lambda: ops.randaug_u8(u8, dev, 9, FILL), lambda: ops.randaug_u8(u8, dev, 2, (1, 2)), lambda: ops.randaug_u8(u8, dev, 2, (1, 2, 256)),
                lambda: ops.randaug_u8(u8, dev, 2, FILL, layout="nhwc"), lambda: ops.randaug_u8(u8[:, :, :, :6].contiguous(), dev, 2, FILL),
                lambda: ops.randaug_u8(u8, dev, 2, FILL, out=torch.zeros(2, 3, 9, 9, dtype=torch.uint8).cuda()),
                lambda: ops.randaug_u8(u8, dev, 2, FILL, scratch=torch.zeros(2, 3, 8, 9, dtype=torch.uint8).cuda()),
                lambda: ops.randaug_u8(u8, dev, 2, FILL, out=u8), lambda: ops.randaug_u8(u8, dev, 2, FILL, scratch=u8),
                lambda: ops.randaug_u8(u8, dev, 2, FILL, host_records=rec[:40]), lambda: ops.randaug_u8(u8, rec, 2, FILL)):
        with pytest.raises(AutoProgHipError):
            bad()
    y = ops.randaug_u8(u8, dev, 2, FILL, host_records=rec)
    assert torch.equal(y, u8)                                      # inverted twice
    empty = ops.randaug_u8(u8[:0], dev, 2, FILL, host_records=rec)
    assert tuple(empty.shape) == (0, 3, 8, 8)


# ================================================================================================================ 4. pipeline
def _drive(monkeypatch, use_graphs, steps=3):
    from autoprog_amd import ops
    from autoprog_amd.data import DeviceBatchPrep, DeviceRandAugment, DeviceRandomResizedCrop
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
    aug = DeviceRandAugment(seed=9)
    loss_fn = TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=16)
    g = torch.Generator().manual_seed(1)
    log = []

    def get_batch(r):
        u8 = torch.randint(0, 256, (8, 3, 80, 112), dtype=torch.uint8, generator=g).cuda()
        return u8, torch.softmax(torch.randn(8, 16, 2 + (r // 16) ** 2, generator=g) * 2, dim=1).cuda()

    real_crop, real_prep = crop.crop, prep.prep
    cropped = []
    monkeypatch.setattr(crop, "crop", lambda u8, size: (cropped.append(real_crop(u8, size).clone()), cropped[-1])[1])
    monkeypatch.setattr(prep, "prep", lambda u8: (log.append((cropped[-1].cpu().numpy(), u8.cpu().numpy(), aug.enabled, aug.magnitude, aug.last)), real_prep(u8))[1])
    drv = AutoProgDriver(model, loss_fn, opt, red, get_batch, r_list=[64, 96], l_list=[3, 3], dp_list=[0.0, 0.0], grow_epochs=[0, 1],
                         steps_per_epoch=steps, auto_grow=False, use_graphs=use_graphs, graph_after=1, batch_prep=prep, crop=crop,
                         augment=aug, aa_list=["", "rand-m6-mstd0.5-inc1"])
    losses, real = [], drv._train_step
    monkeypatch.setattr(drv, "_train_step", lambda *a, **k: (losses.append(real(*a, **k)), losses[-1])[1])
    try:
        np.random.seed(3)
        drv.run(2)
        return [float(v) for v in losses], log
    finally:
        red.remove()


def test_augment_between_crop_and_prep_under_the_driver_eager_and_graphed(monkeypatch):
    """two stages with aa_list = ["", "rand-m6-mstd0.5-inc1"]: the first stage's batches reach prep as the crop made them, bit for bit, and
    nothing is drawn; the second stage's are the restatement applied to the crop's output at magnitude 6.  With DropPath 0 and equal seeds
    the run whose steps replay from graphs (GraphedStep copies the augmented batch into its static buffer) gives the eager run's losses
    bit for bit"""
    le, log = _drive(monkeypatch, False)
    assert len(log) == 6 and [p[0].shape for p in log] == [(8, 3, 64, 64)] * 3 + [(8, 3, 96, 96)] * 3
    for cropped, seen, enabled, magnitude, last in log[:3]:
        assert not enabled and last is None and np.array_equal(cropped, seen)
    changed = 0
    for cropped, seen, enabled, magnitude, last in log[3:]:
        assert enabled and magnitude == 6 and len(last) == 8
        _equal(seen, R.apply(cropped, last, FILL, "nchw"), "driver stage 2")
        changed += int((cropped != seen).sum())
    assert changed > 0 and len({str(p[4]) for p in log[3:]}) == 3
    assert len(le) == 6 and all(np.isfinite(v) for v in le)
    lg, log_g = _drive(monkeypatch, True)
    print("RANDAUG driver eager:", le)
    print("RANDAUG driver graph:", lg)
    assert [p[4] for p in log_g] == [p[4] for p in log] and all(np.array_equal(a[1], b[1]) for a, b in zip(log, log_g))
    assert le == lg, (le, lg)
