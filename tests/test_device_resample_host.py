"""The antialiased device crop without a GPU: the numpy restatement of Pillow's 8-bit resize (tests/_resample_ref.py) against bytes Pillow
wrote (tests/golden/pil_resample.npz, tools/make_pil_resample_golden.py) and, where Pillow imports, against Pillow itself on fresh cases;
DeviceRandomResizedCrop's draws with an interpolation against an independent restatement of timm's order; the new entry point's presence
in the C ABI and its refusals before any launch."""
import ctypes
import math
import os
import random
import re

import numpy as np
import pytest
import torch

from tests import _resample_ref as RR
from tests.test_device_crop_host import rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "ap_crop_resample_u8"


# ================================================================================================================ 1. the rule is Pillow's
def test_restatement_equals_the_bytes_pillow_wrote():
    z = np.load(os.path.join(ROOT, "tests", "golden", "pil_resample.npz"))
    cases, out = z["cases"], z["out"]
    assert len(cases) >= 60 and str(z["pillow_version"])
    seen, off = set(), 0
    for c in cases:
        canvas, (top, left, h, w, flip, filt, S) = z["canvas_%d" % c[0]], (int(v) for v in c[1:])
        want = out[off:off + S * S * 3].reshape(S, S, 3)
        off += S * S * 3
        got = RR.resample_one(canvas, S, (top, left, h, w, flip, filt))
        assert np.array_equal(got, want), (c.tolist(), int(np.abs(got.astype(np.int64) - want).max()))
        seen.add((filt, flip, S, "up" if max(h, w) < S else "down" if min(h, w) > S else "mixed"))
        if h == w == S:                                            # an identity box is the slice, flipped or not
            sl = canvas[top:top + h, left:left + w]
            assert np.array_equal(want, sl[:, ::-1] if flip else sl)
    assert off == out.size
    # the ground the fixture has to cover: both filters, both flips, every size, up and down, the degenerate boxes
    assert {(f, fl) for f, fl, _, _ in seen} == {(1, 0), (1, 1), (2, 0), (2, 1)}
    assert {S for _, _, S, _ in seen} == {1, 5, 16, 24, 31, 64}
    for filt in (1, 2):
        assert (filt, 0, 31, "up") in seen and (filt, 1, 31, "up") in seen and (filt, 0, 16, "down") in seen
    rows = {tuple(int(v) for v in c[3:5]) for c in cases}
    assert (5, 7) in rows and (64, 64) in rows and (1, 1) in rows and (1, 56) in rows and (40, 1) in rows


def test_restatement_equals_pillow_on_fresh_cases():
    Image = pytest.importorskip("PIL.Image")
    g = np.random.RandomState(7)
    for i in range(60):
        H, W = int(g.randint(1, 71)), int(g.randint(1, 91))
        img = (g.randint(0, 2, (H, W, 3)) * 255 if i % 3 == 0 else g.randint(0, 256, (H, W, 3))).astype(np.uint8)
        h, w = int(g.randint(1, H + 1)), int(g.randint(1, W + 1))
        top, left = int(g.randint(0, H - h + 1)), int(g.randint(0, W - w + 1))
        for filt, pil in ((1, Image.BILINEAR), (2, Image.BICUBIC)):
            S, flip = int(g.choice([1, 5, 16, 24, 31, 64])), int(g.randint(0, 2))
            im = Image.fromarray(img, "RGB").crop((left, top, left + w, top + h)).resize((S, S), pil)
            want = np.asarray(im.transpose(Image.FLIP_LEFT_RIGHT) if flip else im)
            assert np.array_equal(RR.resample_one(img, S, (top, left, h, w, flip, filt)), want), (H, W, top, left, h, w, flip, filt, S)


def test_batched_form_and_flip_order():
    """both layouts give the same pixels; the flip mirrors the RESULT (timm resizes, then flips), which is not the resample of the
    mirrored box when the windows are not symmetric about the box's centre"""
    g = np.random.RandomState(3)
    hwc = g.randint(0, 256, (3, 20, 30, 3)).astype(np.uint8)
    recs = [(0, 0, 20, 30, 0, 1), (2, 3, 17, 11, 1, 2), (5, 0, 9, 30, 1, 1)]
    a = RR.resample(hwc, 7, recs, "nhwc")
    b = RR.resample(np.ascontiguousarray(hwc.transpose(0, 3, 1, 2)), 7, recs, "nchw")
    assert a.shape == (3, 7, 7, 3) and b.shape == (3, 3, 7, 7) and np.array_equal(a, b.transpose(0, 2, 3, 1))
    plain = RR.resample_one(hwc[1], 7, (2, 3, 17, 11, 0, 2))
    assert np.array_equal(a[1], plain[:, ::-1])
    # weights are normalised and the accumulator cannot overflow int32: 255 * sum |K| < 2^31 for every window of strong reductions
    for n, S in ((512, 128), (512, 17), (97, 5), (5, 31)):
        for filt in (1, 2):
            for xmin, K in RR.coefficients(n, S, filt):
                assert abs(int(K.sum()) - (1 << 22)) <= len(K) and 255 * int(np.abs(K).sum()) + (1 << 21) < 2 ** 31 and 0 <= xmin and xmin + len(K) <= n


# ================================================================================================================ 2. draws
def _crop(**kw):
    from autoprog_amd.data import DeviceRandomResizedCrop
    return DeviceRandomResizedCrop(device="cpu", **kw)


def _records(host, B):
    return host.numpy().reshape(-1, 8)[:B]


def box_only(py, eh, ew, scale, ratio):
    """timm 0.4.5 RandomResizedCropAndInterpolation.get_params alone, written here independently of autoprog_amd.data: the caller
    draws random.choice(interpolation) and the flip behind it, in timm's order"""
    for _ in range(10):
        target = py.uniform(scale[0], scale[1]) * (eh * ew)
        aspect = math.exp(py.uniform(math.log(ratio[0]), math.log(ratio[1])))
        w = int(round(math.sqrt(target * aspect)))
        h = int(round(math.sqrt(target / aspect)))
        if 0 < w <= ew and 0 < h <= eh:
            return py.randint(0, eh - h), py.randint(0, ew - w), h, w
    if ew / eh < ratio[0]:
        w, h = ew, int(round(ew / ratio[0]))
    elif ew / eh > ratio[1]:
        h, w = eh, int(round(eh * ratio[1]))
    else:
        h, w = eh, ew
    return (eh - h) // 2, (ew - w) // 2, h, w


@pytest.mark.parametrize("scale", [(0.08, 1.0), (0.35, 1.0)])
@pytest.mark.parametrize("H,W", [(40, 56), (256, 256)])
def test_random_interpolation_draws_box_then_filter_then_flip(H, W, scale):
    B, ratio = 16, (3 / 4, 4 / 3)
    c = _crop(scale=scale, seed=11, interpolation="random")
    assert c.interpolation == "random" and "interpolation" in vars(c)       # a plain attribute
    py = random.Random(11)
    filters = set()
    for step in range(12):                                        # (more steps than ring slots)
        rec = _records(c.draw(B, H, W), B).copy()
        want = []
        for b in range(B):
            box = box_only(py, H, W, scale, ratio)
            filt = py.choice((1, 2))
            want.append(box + (int(py.random() < 0.5), filt))
        assert [tuple(r[:6]) for r in rec.tolist()] == want and c.last == want
        assert not rec[:, 6:].any()
        filters |= {w[5] for w in want}
    assert filters == {1, 2}


@pytest.mark.parametrize("name,code", [(None, 0), ("bilinear", 1), ("bicubic", 2)])
def test_none_and_fixed_filters_consume_the_stream_of_the_plain_object(name, code):
    random.seed(5); np.random.seed(5); torch.manual_seed(5)
    s_py, s_np, s_t = random.getstate(), np.random.get_state(), torch.get_rng_state()
    c = _crop(seed=11, interpolation=name)
    py = random.Random(11)
    for step in range(10):
        rec = _records(c.draw(8, 40, 56), 8).copy()
        want = [rule(py, 40, 56, (0.08, 1.0), (3 / 4, 4 / 3), 0.5) for _ in range(8)]
        assert [tuple(r[:5]) for r in rec.tolist()] == want and (rec[:, 5] == code).all() and not rec[:, 6:].any()
        assert c.last == (want if name is None else [w + (code,) for w in want])
    assert c._py.getstate() == py.getstate()
    assert random.getstate() == s_py and torch.equal(torch.get_rng_state(), s_t)
    now = np.random.get_state()
    assert now[0] == s_np[0] and np.array_equal(now[1], s_np[1]) and now[2:] == s_np[2:]


def test_interpolation_is_an_attribute_and_center_takes_its_own():
    c = _crop(seed=1)
    assert c.interpolation is None
    state = c._py.getstate()
    rec = _records(c.center_records(2, 256, 320, 0.96, interpolation="bicubic"), 2)
    side = int(round(0.96 * 256))
    assert [tuple(r[:6]) for r in rec.tolist()] == [((256 - side) // 2, (320 - side) // 2, side, side, 0, 2)] * 2 == c.last
    rec = _records(c.center_records(2, 256, 320, 0.96), 2)        # the object's setting: None, the record of the two-tap kernel
    assert [tuple(r) for r in rec.tolist()] == [((256 - side) // 2, (320 - side) // 2, side, side, 0, 0, 0, 0)] * 2
    assert c.last == [((256 - side) // 2, (320 - side) // 2, side, side, 0)] * 2
    c.interpolation = "bilinear"
    assert _records(c.center_records(1, 64, 64), 1)[0][5] == 1 and _records(c.draw(1, 64, 64), 1)[0][5] == 1
    assert _records(c.center_records(1, 64, 64, interpolation="bicubic"), 1)[0][5] == 2
    assert c._py.getstate() != state                               # (the draw above)
    state = c._py.getstate()
    c.center_records(1, 64, 64)
    assert c._py.getstate() == state                               # nothing drawn
    for bad in (lambda: _crop(interpolation="lanczos"), lambda: _crop(interpolation=2), lambda: c.center_records(1, 64, 64, interpolation="random"),
                lambda: c.center_records(1, 64, 64, interpolation="box")):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError):
        _crop(interpolation="bicubic").crop(torch.zeros(2, 3, 8, 8, dtype=torch.uint8), 8)     # not on the device


# ================================================================================================================ 3. ABI
def _args(**kw):
    from autoprog_amd._lib import CropResampleArgs
    a = CropResampleArgs()
    a.u8, a.layout, a.B, a.Hi, a.Wi, a.out, a.S, a.records = 4096, 0, 2, 40, 56, 8192, 24, 12288
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_entry_point_is_declared_exported_and_refuses_before_any_launch():
    from autoprog_amd._lib import _SIGNATURES, EXPORTED_SYMBOLS, LIB_PATH, CropResampleArgs, lib
    header = open(os.path.join(ROOT, "include", "autoprog_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(\s*const\s+ap_crop_resample_args\s*\*\s*args\s*,\s*ap_stream_t\s+stream\s*\)" % SYMBOL, header)
    assert SYMBOL in EXPORTED_SYMBOLS and SYMBOL in _SIGNATURES and hasattr(ctypes.CDLL(LIB_PATH), SYMBOL)
    assert _SIGNATURES[SYMBOL] == (ctypes.c_int, [ctypes.POINTER(CropResampleArgs), ctypes.c_void_p])
    assert [n for n, _ in CropResampleArgs._fields_] == ["u8", "layout", "B", "Hi", "Wi", "out", "S", "records", "records_host"]
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
        rec = (ctypes.c_int * 16)(0, 0, 40, 56, 0, 1, 0, 0, *second, 0, 0)
        return f(ctypes.byref(_args(records_host=ctypes.cast(rec, ctypes.c_void_p).value)), None)
    assert host(20, 10, 21, 40, 1, 1) == -1                       # rows 20 .. 40 of 40
    assert host(0, 17, 40, 40, 0, 2) == -1                        # columns 17 .. 56 of 56
    assert host(-1, 0, 8, 8, 0, 1) == -1 and host(0, -1, 8, 8, 0, 1) == -1
    assert host(0, 0, 0, 8, 0, 2) == -1 and host(0, 0, 8, 0, 0, 2) == -1      # h = 0, w = 0
    assert host(0, 0, 8, 8, 2, 1) == -1 and host(0, 0, 8, 8, -1, 1) == -1     # flip outside {0, 1}
    assert host(0, 0, 8, 8, 0, 0) == -1 and host(0, 0, 8, 8, 0, 3) == -1 and host(0, 0, 8, 8, 1, -1) == -1      # filter outside {1, 2}
    rec = (ctypes.c_int * 16)(0, 0, 40, 56, 0, 0, 0, 0, 0, 0, 8, 8, 0, 1, 0, 0)      # the FIRST record's filter is 0
    assert f(ctypes.byref(_args(records_host=ctypes.cast(rec, ctypes.c_void_p).value)), None) == -1
    assert f(ctypes.byref(_args(Hi=1 << 14, Wi=1 << 14, S=8)), None) == -2    # one output row's box rows and tables exceed the LDS budget
    assert f(ctypes.byref(_args(B=0)), None) == 0                  # no launch
    assert f(ctypes.byref(_args(B=0, u8=None, out=None, records=None)), None) == 0


def test_ops_wrapper_refuses_what_it_cannot_run():
    from autoprog_amd import ops
    from autoprog_amd._lib import AutoProgHipError
    assert (ops.RESAMPLE_BILINEAR, ops.RESAMPLE_BICUBIC) == (1, 2)
    with pytest.raises(AutoProgHipError):
        ops.crop_resample_u8(torch.zeros(2, 3, 8, 8, dtype=torch.uint8), 8, torch.zeros(16, dtype=torch.int32))       # CPU tensors
