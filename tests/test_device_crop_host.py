"""The device crop without a GPU: DeviceRandomResizedCrop's draws against an independent restatement of timm's rule, the driver's
per-stage crop scale, the new entry point's presence in the C ABI and its refusals before any launch, and the cap the GPU tests hold the
kernel to (float32 arithmetic against float64: at most 1 grey level, on at most 0.5 % of the bytes)."""
import ctypes
import math
import os
import random
import re

import numpy as np
import pytest
import torch

from tests import _crop_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "ap_crop_resize_u8"


# ================================================================================================================ 1. draws
def rule(py, eh, ew, scale, ratio, hflip):
    """timm 0.4.5 RandomResizedCropAndInterpolation.get_params over an (eh, ew) extent, then one flip draw; written here independently
    of autoprog_amd.data"""
    box = None
    for _ in range(10):
        target = py.uniform(scale[0], scale[1]) * (eh * ew)
        aspect = math.exp(py.uniform(math.log(ratio[0]), math.log(ratio[1])))
        w = int(round(math.sqrt(target * aspect)))
        h = int(round(math.sqrt(target / aspect)))
        if 0 < w <= ew and 0 < h <= eh:
            top = py.randint(0, eh - h)
            left = py.randint(0, ew - w)
            box = (top, left, h, w)
            break
    if box is None:
        if ew / eh < ratio[0]:
            w = ew
            h = int(round(w / ratio[0]))
        elif ew / eh > ratio[1]:
            h = eh
            w = int(round(h * ratio[1]))
        else:
            h, w = eh, ew
        box = ((eh - h) // 2, (ew - w) // 2, h, w)
    return box + (int(py.random() < hflip),)


def _crop(**kw):
    from autoprog_amd.data import DeviceRandomResizedCrop
    return DeviceRandomResizedCrop(device="cpu", **kw)


def _records(host, B):
    return host.numpy().reshape(-1, 8)[:B]


@pytest.mark.parametrize("with_extents", [False, True])
@pytest.mark.parametrize("scale", [(0.08, 1.0), (0.35, 1.0)])
@pytest.mark.parametrize("H,W", [(40, 56), (256, 256)])
def test_draws_follow_the_rule(H, W, scale, with_extents):
    B = 16
    ext = None
    if with_extents:
        g = np.random.RandomState(H)
        ext = np.stack([g.randint(H // 3, H + 1, B), g.randint(W // 3, W + 1, B)], axis=1)
        ext[0] = (H, W)
    c = _crop(scale=scale, seed=11)
    py = random.Random(11)
    for step in range(12):                                        # (more steps than ring slots)
        rec = _records(c.draw(B, H, W, ext), B).copy()
        want = [rule(py, *((H, W) if ext is None else (int(ext[b][0]), int(ext[b][1]))), scale, (3 / 4, 4 / 3), 0.5) for b in range(B)]
        assert [tuple(r[:5]) for r in rec.tolist()] == want and c.last == want
        assert not rec[:, 5:].any()
        for b, (top, left, h, w, flip) in enumerate(want):
            eh, ew = (H, W) if ext is None else ext[b]
            assert h >= 1 and w >= 1 and top >= 0 and left >= 0 and top + h <= eh and left + w <= ew and flip in (0, 1)


def test_draws_are_reproducible_and_leave_the_global_streams_alone():
    random.seed(5); np.random.seed(5); torch.manual_seed(5)
    s_py, s_np, s_t = random.getstate(), np.random.get_state(), torch.get_rng_state()
    a, b, other = _crop(seed=3), _crop(seed=3), _crop(seed=4)
    ra = [_records(a.draw(8, 64, 48), 8).copy() for _ in range(3)]
    rb = [_records(b.draw(8, 64, 48), 8).copy() for _ in range(3)]
    ro = [_records(other.draw(8, 64, 48), 8).copy() for _ in range(3)]
    a.center_records(8, 64, 48)
    assert all(np.array_equal(x, y) for x, y in zip(ra, rb)) and not all(np.array_equal(x, y) for x, y in zip(ra, ro))
    assert random.getstate() == s_py and torch.equal(torch.get_rng_state(), s_t)
    now = np.random.get_state()
    assert now[0] == s_np[0] and np.array_equal(now[1], s_np[1]) and now[2:] == s_np[2:]


def test_fallback_is_the_central_crop_with_the_ratio_clamped():
    """scale = (4, 4) asks for four times the extent's area: no attempt is ever accepted.  An extent whose aspect lies inside the ratio
    range comes back whole -- 40 x 56 under ratio (3/4, 3/2), 48 x 56 under the default; 40 x 56 under the default ratio is wider than
    4/3 (56 / 40 = 1.4), so the rule clamps it: h = 40, w = round(40 * 4/3) = 53, centred"""
    c = _crop(scale=(4.0, 4.0), ratio=(3 / 4, 3 / 2), seed=0)
    c.draw(3, 40, 56)
    assert [r[:4] for r in c.last] == [(0, 0, 40, 56)] * 3
    c = _crop(scale=(4.0, 4.0), seed=0)
    c.draw(3, 64, 64, np.array([[48, 56]] * 3))
    assert [r[:4] for r in c.last] == [(0, 0, 48, 56)] * 3
    c.draw(3, 40, 56)
    assert [r[:4] for r in c.last] == [(0, 1, 40, 53)] * 3
    c.draw(2, 128, 128, np.array([[20, 100], [100, 20]]))
    w = int(round(20 * 4 / 3))
    assert c.last[0][:4] == (0, (100 - w) // 2, 20, w)
    h = int(round(20 / (3 / 4)))
    assert c.last[1][:4] == ((100 - h) // 2, 0, h, 20)


def test_hflip_zero_and_one_keep_the_boxes():
    recs = {}
    for p in (0.0, 0.5, 1.0):
        c = _crop(seed=9, hflip=p)
        recs[p] = np.concatenate([_records(c.draw(16, 40, 56), 16).copy() for _ in range(3)])
    assert not recs[0.0][:, 4].any() and recs[1.0][:, 4].all() and 0 < recs[0.5][:, 4].sum() < 48
    assert np.array_equal(recs[0.0][:, :4], recs[0.5][:, :4]) and np.array_equal(recs[1.0][:, :4], recs[0.5][:, :4])


def test_center_is_the_central_square():
    c = _crop(seed=1)
    state = c._py.getstate()
    rec = _records(c.center_records(2, 256, 320, 0.875, np.array([[256, 320], [100, 37]])), 2)
    assert c._py.getstate() == state                              # nothing drawn
    assert tuple(rec[0][:5]) == ((256 - 224) // 2, (320 - 224) // 2, 224, 224, 0)
    s = int(round(0.875 * 37))
    assert tuple(rec[1][:5]) == ((100 - s) // 2, (37 - s) // 2, s, s, 0)
    with pytest.raises(ValueError):
        c.draw(2, 40, 56, np.array([[41, 56], [40, 56]]))
    with pytest.raises(ValueError):
        c.draw(2, 40, 56, np.array([[40, 0], [40, 56]]))
    with pytest.raises(ValueError):
        c.crop(torch.zeros(2, 3, 8, 8, dtype=torch.uint8), 8)     # not on the device


# ================================================================================================================ 2. driver
def test_driver_sets_the_stage_crop_scale_and_refuses_bad_arguments():
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.prog.driver import AutoProgDriver

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = torch.nn.Linear(3, 4)

        def set_sample_config(self, cfg):
            pass

        def set_drop_path_rate(self, rate):
            pass

        def forward(self, x):
            return self.fc(x)

    class Opt:
        def __init__(self, red):
            self.red = red

        def step(self):
            self.red.take_pending_scale()

        def grow(self, *a, **k):
            pass

    class Crop:
        layout, scale = "nchw", (0.08, 1.0)

        def __init__(self):
            self.calls = []

        def crop(self, images, size):
            self.calls.append((self.scale, size, tuple(images.shape)))
            return images[:, :, :size // 16, :size // 16].contiguous()

    class Prep:
        layout, re_prob, mix_enabled = "nchw", 0.0, False

        def __init__(self):
            self.sides = []

        def prep(self, u8):
            self.sides.append(u8.shape[-1])
            return u8.float().mean((2, 3))

    assert AutoProgDriver(None, None, None, None, None, [64], [3], [0.0], [0], 1).crop is None
    from autoprog_amd.data import DeviceRandomResizedCrop
    real = DeviceRandomResizedCrop(device="cpu")
    real.scale = (0.3, 0.9)
    assert real.scale == (0.3, 0.9) and "scale" in vars(real)      # a plain attribute
    torch.manual_seed(0)
    model = Net()
    red = GradientBucketReducer(list(model.parameters()), world_size=1)
    crop, prep = Crop(), Prep()
    kw = dict(r_list=[64, 96], l_list=[3, 6], dp_list=[0.0, 0.0], grow_epochs=[0, 1], steps_per_epoch=2, auto_grow=False)

    def get_batch(r):
        return torch.randint(0, 256, (4, 3, 8, 8), dtype=torch.uint8), torch.randn(4, 4)
    drv = AutoProgDriver(model, lambda out, t: ((out - t) ** 2).mean(), Opt(red), red, get_batch, batch_prep=prep, crop=crop,
                         resize_list=[[0.35, 1.0], [0.08, 1.0]], **kw)
    hist = drv.run(2)
    assert [c[:2] for c in crop.calls] == [((0.35, 1.0), 64)] * 2 + [((0.08, 1.0), 96)] * 2
    assert all(c[2] == (4, 3, 8, 8) for c in crop.calls) and prep.sides == [4, 4, 6, 6]      # prep takes what the crop returned
    assert crop.scale == (0.08, 1.0) and all(np.isfinite(h["loss"]) for h in hist)
    with pytest.raises(ValueError):                                # a crop without a batch_prep
        AutoProgDriver(model, None, Opt(red), red, get_batch, crop=crop, **kw)
    with pytest.raises(ValueError):                                # a resize_list without a crop
        AutoProgDriver(model, None, Opt(red), red, get_batch, batch_prep=prep, resize_list=[[0.35, 1.0], [0.08, 1.0]], **kw)
    with pytest.raises(ValueError):                                # one entry per stage
        AutoProgDriver(model, None, Opt(red), red, get_batch, batch_prep=prep, crop=crop, resize_list=[[0.35, 1.0]], **kw)


# ================================================================================================================ 3. ABI
def _args(**kw):
    from autoprog_amd._lib import CropResizeArgs
    a = CropResizeArgs()
    a.u8, a.layout, a.B, a.Hi, a.Wi, a.out, a.S, a.records = 4096, 0, 2, 40, 56, 8192, 24, 12288
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_entry_point_is_declared_exported_and_refuses_before_any_launch():
    from autoprog_amd._lib import _SIGNATURES, EXPORTED_SYMBOLS, LIB_PATH, lib
    header = open(os.path.join(ROOT, "include", "autoprog_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(\s*const\s+ap_crop_resize_args\s*\*\s*args\s*,\s*ap_stream_t\s+stream\s*\)" % SYMBOL, header)
    assert SYMBOL in EXPORTED_SYMBOLS and SYMBOL in _SIGNATURES and hasattr(ctypes.CDLL(LIB_PATH), SYMBOL)
    assert lib.ap_abi_version() == 7
    f = getattr(lib, SYMBOL)
    assert f.argtypes is not None and f.restype is ctypes.c_int
    assert f(None, None) == -4
    for name in ("u8", "out", "records"):
        assert f(ctypes.byref(_args(**{name: None})), None) == -4, name
    assert f(ctypes.byref(_args(S=0)), None) == -1
    assert f(ctypes.byref(_args(Hi=0)), None) == -1 and f(ctypes.byref(_args(Wi=-3)), None) == -1 and f(ctypes.byref(_args(B=-1)), None) == -1
    assert f(ctypes.byref(_args(layout=2)), None) == -1
    assert f(ctypes.byref(_args(u8=4096 + 8)), None) == -1        # u8 not 16-byte aligned
    assert f(ctypes.byref(_args(B=1 << 30, Hi=1 << 10, Wi=1 << 10)), None) == -1      # 3 * 2^50 input bytes

    def host(*second):
        rec = (ctypes.c_int * 16)(0, 0, 40, 56, 0, 0, 0, 0, *second, 0, 0, 0)
        return f(ctypes.byref(_args(records_host=ctypes.cast(rec, ctypes.c_void_p).value)), None), rec
    assert host(20, 10, 21, 40, 1)[0] == -1                       # rows 20 .. 40 of 40
    assert host(0, 17, 40, 40, 0)[0] == -1                        # columns 17 .. 56 of 56
    assert host(-1, 0, 8, 8, 0)[0] == -1 and host(0, -1, 8, 8, 0)[0] == -1
    assert host(0, 0, 0, 8, 0)[0] == -1 and host(0, 0, 8, 0, 0)[0] == -1      # h = 0, w = 0
    assert host(0, 0, 8, 8, 2)[0] == -1 and host(0, 0, 8, 8, -1)[0] == -1     # flip outside {0, 1}
    assert f(ctypes.byref(_args(Hi=1 << 14, Wi=1 << 14, S=8)), None) == -2    # one output row reads more rows than the LDS budget holds
    assert f(ctypes.byref(_args(B=0)), None) == 0                  # no launch
    assert f(ctypes.byref(_args(B=0, u8=None, out=None, records=None)), None) == 0


def test_ops_wrapper_refuses_what_it_cannot_run():
    from autoprog_amd import ops
    from autoprog_amd._lib import AutoProgHipError
    with pytest.raises(AutoProgHipError):
        ops.crop_resize_u8(torch.zeros(2, 3, 8, 8, dtype=torch.uint8), 8, torch.zeros(16, dtype=torch.int32))       # CPU tensors


# ================================================================================================================ 4. the cap of the GPU tests
def test_float32_arithmetic_stays_within_the_cap_of_the_gpu_tests():
    """the GPU tests hold the kernel (float32, every operation rounded) to the float64 restatement: no byte off by more than 1, at most
    0.5 % of the bytes off by 1.  Here the float32 restatement itself against the float64 one, over 800 random boxes at four sizes
    (measured on the CPU: 0.09 % of the bytes, largest difference 1); identity and integer-ratio boxes are equal exactly."""
    g = np.random.RandomState(0)
    py = random.Random(0)
    off = total = worst = 0
    for i in range(800):
        img = g.randint(0, 256, (40, 56, 3)).astype(np.uint8)
        rec = rule(py, 40, 56, (0.08, 1.0), (3 / 4, 4 / 3), 0.5)
        for S in (16, 24, 31, 64):
            a = CR.crop_resize_one(img, S, rec, np.float32).astype(np.int64)
            b = CR.crop_resize_one(img, S, rec, np.float64).astype(np.int64)
            d = np.abs(a - b)
            off, total, worst = off + int((d > 0).sum()), total + d.size, max(worst, int(d.max()))
    print("float32 vs float64 restatement: %d of %d bytes differ (%.3f %%), largest difference %d" % (off, total, 100.0 * off / total, worst))
    assert worst <= 1 and off <= 0.005 * total
    img = g.randint(0, 256, (48, 64, 3)).astype(np.uint8)
    for dt in (np.float32, np.float64):
        assert np.array_equal(CR.crop_resize_one(img, 24, (7, 13, 24, 24, 0), dt), img[7:31, 13:37])
        assert np.array_equal(CR.crop_resize_one(img, 24, (7, 13, 24, 24, 1), dt), img[7:31, 13:37][:, ::-1])
        for rec in ((0, 0, 48, 32, 0), (0, 32, 48, 32, 1), (0, 0, 32, 64, 0), (16, 0, 16, 48, 1)):
            assert np.array_equal(CR.crop_resize_one(img, 16, rec, dt), CR.crop_resize_int(img, 16, rec)), rec
        assert np.array_equal(CR.crop_resize_one(img, 5, (3, 4, 1, 1, 1), dt), np.broadcast_to(img[3, 4], (5, 5, 3)))
