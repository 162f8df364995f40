"""Device RandAugment without a GPU: the numpy restatement of the pixel rules (tests/_randaug_ref.py) against bytes Pillow wrote
(tests/golden/pil_randaug.npz, tools/make_pil_randaug_golden.py) and, where Pillow imports, against live calls of the API timm uses;
DeviceRandAugment's draws against an independent restatement of timm 0.4.5's order; spec parsing, the record packing, the driver's
argument checks and the new entry point's presence in the C ABI."""
import ctypes
import math
import os
import random
import re

import numpy as np
import pytest
import torch

from tests import _randaug_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "ap_randaug_u8"
FILL = (124, 116, 104)


def _rec(op, filt=0, iarg=0, farg=0.0, m=R.NO_MATRIX):
    return (op, filt, iarg, float(np.float32(farg)), tuple(float(v) for v in m))


# ================================================================================================================ 1. the rules are Pillow's
def test_restatement_equals_the_bytes_pillow_wrote():
    from autoprog_amd.data import DeviceRandAugment
    z = np.load(os.path.join(ROOT, "tests", "golden", "pil_randaug.npz"))
    fill = tuple(int(v) for v in z["fill"])
    assert fill == FILL and len(z["image"]) >= 400 and str(z["pillow_version"])
    seen, chains, off = set(), 0, 0
    for k in range(len(z["image"])):
        img, n = z["image_%d" % z["image"][k]], int(z["n_layers"][k])
        S = img.shape[0]
        recs = DeviceRandAugment.unpack(z["records"][k], 1, 2)[0][:n]
        want = z["out"][off:off + S * S * 3].reshape(S, S, 3)
        off += S * S * 3
        got = img
        for r in recs:
            got = R.apply_record(got, r, fill)
        assert np.array_equal(got, want), (k, S, recs, int(np.abs(got.astype(np.int64) - want).max()))
        chains += n == 2
        for op, filt, iarg, farg, m in recs:
            sign = 0
            if op == R.AFFINE:
                moved = [v for v in (m[1], m[3], m[2], m[5]) if v != 0] if (m[0], m[4]) == (1.0, 1.0) else [m[1]]      # shear / translate, else a rotation
                sign = 1 if moved[0] > 0 else -1
            elif op >= R.BRIGHTNESS:
                sign = 0 if farg == 1.0 else 1 if farg > 1.0 else -1
            seen.add((op, filt, sign, S))
    assert off == z["out"].size and chains >= 4
    # the ground the fixture has to cover: every op, both filters with both signs, factors on both sides of 1, every size
    assert {s[0] for s in seen} == set(range(12))
    assert {(f, sg) for op, f, sg, _ in seen if op == R.AFFINE} == {(1, 1), (1, -1), (2, 1), (2, -1)}
    for op in (R.BRIGHTNESS, R.CONTRAST, R.COLOR, R.SHARPNESS):
        assert {sg for o, _, sg, _ in seen if o == op} == {-1, 0, 1}
    assert {s[3] for s in seen} == {3, 7, 16, 33}


def _images(g, S):
    two = g.randint(0, 2, (S, S, 3)) * 255
    two[..., 2] = np.where(two[..., 2] > 0, 131, 17)
    return [g.randint(0, 256, (S, S, 3)).astype(np.uint8), two.astype(np.uint8), np.full((S, S, 3), (0, 77, 255), dtype=np.uint8)]


def test_restatement_equals_pillow_on_fresh_cases():
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance, ImageOps
    pil = {1: Image.BILINEAR, 2: Image.BICUBIC}
    g = np.random.RandomState(11)
    for S in (1, 2, 3, 5, 12, 24):
        for img in _images(g, S):
            im = Image.fromarray(img, "RGB")
            eq = lambda want, rec: np.array_equal(R.apply_record(img, rec, FILL), np.asarray(want)) or pytest.fail("S %d %s" % (S, rec))
            eq(ImageOps.autocontrast(im), _rec(R.AUTOCONTRAST))
            eq(ImageOps.equalize(im), _rec(R.EQUALIZE))
            eq(ImageOps.invert(im), _rec(R.INVERT))
            for bits in (0, 2, 3, 4):
                eq(ImageOps.posterize(im, bits), _rec(R.POSTERIZE, iarg=bits))
            for t in (0, 1, 128, 200, 256):
                eq(ImageOps.solarize(im, t), _rec(R.SOLARIZE, iarg=t))
                eq(im.point([i if i < t else 255 - i for i in range(256)] * 3), _rec(R.SOLARIZE, iarg=t))
            for a in (0, 33, 110):
                eq(im.point([min(255, i + a) if i < 128 else i for i in range(256)] * 3), _rec(R.SOLARIZE_ADD, iarg=a))
            for f in (0.1, 0.4, 0.7, 1.0, 1.3, 1.6, 1.9):
                f = float(g.uniform(0.1, 1.9)) if f in (0.4, 1.6) else f
                for op, enh in ((R.BRIGHTNESS, ImageEnhance.Brightness), (R.CONTRAST, ImageEnhance.Contrast), (R.COLOR, ImageEnhance.Color),
                                (R.SHARPNESS, ImageEnhance.Sharpness)):
                    eq(enh(im).enhance(f), _rec(op, farg=f))
            for filt in (1, 2):
                for sign in (1, -1):
                    s, p, deg = sign * float(g.uniform(0.01, 0.3)), sign * float(g.uniform(0.01, 0.45)) * S, sign * float(g.uniform(0.1, 30.0))
                    for m in ((1, s, 0, 0, 1, 0), (1, 0, 0, s, 1, 0), (1, 0, p, 0, 1, 0), (1, 0, 0, 0, 1, p), (1, 0, 2.0 * S, 0, 1, 0), R.IDENTITY):
                        eq(im.transform(im.size, Image.AFFINE, m, resample=pil[filt], fillcolor=FILL), _rec(R.AFFINE, filt, m=m))
                    for d in (deg, 30.0 * sign):
                        eq(im.rotate(d, resample=pil[filt], fillcolor=FILL), _rec(R.AFFINE, filt, m=R.rotate_matrix(d, S)))
                assert R.rotate_matrix(360.0, S) is None and np.array_equal(np.asarray(im.rotate(360.0, resample=pil[filt], fillcolor=FILL)), img)


def test_restatement_edge_branches():
    """the branches the GPU tests lean on: identities of AutoContrast / Equalize, step == 0, both clip branches of blend, all-fill affines"""
    g = np.random.RandomState(5)
    const = np.full((9, 9, 3), 37, dtype=np.uint8)
    assert np.array_equal(R.autocontrast(const), const) and np.array_equal(R.equalize(const), const)
    small = g.randint(0, 256, (7, 7, 3)).astype(np.uint8)          # 49 pixels: step = (49 - h) // 255 == 0
    assert np.array_equal(R.equalize(small), small)
    ext = (g.randint(0, 2, (8, 8, 3)) * 255).astype(np.uint8)
    assert R.brightness(ext, 1.9).max() == 255 and R.contrast(ext, 1.9).min() == 0 and R.contrast(ext, 1.9).max() == 255
    assert np.array_equal(R.brightness(ext, 1.0), ext) and np.array_equal(R.sharpness(ext, 1.0), ext) and np.array_equal(R.color(ext, 1.0), ext)
    assert np.array_equal(R.posterize(ext, 0), np.zeros_like(ext)) and np.array_equal(R.solarize(ext, 256), ext)
    fill = np.broadcast_to(np.asarray(FILL, dtype=np.uint8), (8, 8, 3))
    for filt in (1, 2):
        assert np.array_equal(R.affine(ext, R.IDENTITY, filt, FILL), ext)
        for m in ((1, 0, 8.0, 0, 1, 0), (1, 0, 0, 0, 1, -8.5), (float("nan"),) * 6, (1e300, 0, 0, 0, 1e300, 0), (1, 0, float("inf"), 0, 1, 0)):
            assert np.array_equal(R.affine(ext, m, filt, FILL), fill), (filt, m)      # (1e300: already 0.5e300 >= S at pixel 0)
    a = R.apply(np.stack([ext, ext]), [[_rec(R.INVERT), _rec(R.INVERT)], [_rec(R.NONE)]], FILL, "nhwc")
    assert np.array_equal(a[0], ext) and np.array_equal(a[1], ext)
    b = R.apply(np.ascontiguousarray(ext[None].transpose(0, 3, 1, 2)), [[_rec(R.SOLARIZE, iarg=100)]], FILL, "nchw")
    assert np.array_equal(b.transpose(0, 2, 3, 1)[0], R.solarize(ext, 100))


# ================================================================================================================ 2. the draws
def _aug(**kw):
    from autoprog_amd.data import DeviceRandAugment
    kw.setdefault("device", "cpu")
    return DeviceRandAugment(**kw)


def test_draws_follow_timms_order_and_an_independent_restatement():
    aug = _aug(seed=12)
    nprs, py = np.random.RandomState(12), random.Random(12)
    for B, S in ((16, 32), (5, 224), (16, 32)):
        host = aug.draw(B, S)
        want = R.draw(nprs, py, B, S, magnitude=9, mstd=0.5, prob=0.5, n=2, increasing=True)
        assert aug.last == want
        assert host.dtype == torch.int32 and host.numel() == B * 2 * 16
    assert aug._py.getstate() == py.getstate()                     # the same number of draws, gauss's spare value included
    assert aug._np.randint(1 << 30) == nprs.randint(1 << 30)
    assert _aug(seed=12).draw(4, 32).tolist() == _aug(seed=12).draw(4, 32).tolist() != _aug(seed=13).draw(4, 32).tolist()
    assert aug.fill == FILL


def test_consumption_per_op_kind():
    """skip: one random(); otherwise random(), gauss (mstd > 0), the level's random() where the rule negates, choice for the geometric ops"""
    geometric = {"Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel"}
    enhance = {"Color", "Contrast", "Brightness", "Sharpness"}
    for name in R.OP_NAMES:
        for inc in (True, False):
            for mstd in (0.5, 0.0):
                c = R.CountingRandom(random.Random(1))
                rec = R.draw_op(name, c, 32, 9, mstd, 1.0, inc)    # prob 1: never skipped and no draw for it
                want = (["gauss"] if mstd > 0 else []) + (["random"] if name in geometric or (name in enhance and inc) else []) + (["choice"] if name in geometric else [])
                assert c.calls == want, (name, inc, mstd, c.calls)
                assert (rec[0] == R.AFFINE) == (name in geometric) and (rec[1] in (1, 2)) == (name in geometric)
        c = R.CountingRandom(random.Random(1))
        assert R.draw_op(name, c, 32, 9, 0.5, 0.0, True)[0] == R.NONE and c.calls == ["random"]
    # the object consumes what the restatement consumes, op by op
    from autoprog_amd.data import RANDAUG_OPS
    assert RANDAUG_OPS == R.OP_NAMES
    for inc in (1, 0):
        aug, py = _aug(spec="rand-m7-mstd0.5-inc%d" % inc, seed=3), random.Random(3)
        for name in R.OP_NAMES * 3:
            assert aug._draw_op(name, 48) == R.draw_op(name, py, 48, 7, 0.5, 0.5, bool(inc)) and aug._py.getstate() == py.getstate()


def test_prob_and_magnitude_are_read_at_draw_time():
    aug = _aug(seed=4)
    aug.prob = 0.0
    aug.draw(8, 32)
    assert all(r[0] == R.NONE for image in aug.last for r in image)
    aug.prob, aug.magnitude, aug.magnitude_std = 1.0, 0, 0.0       # magnitude 0: every op at its mildest, nothing skipped
    state = aug._py.getstate()
    aug.draw(32, 32)
    flat = [r for image in aug.last for r in image]
    assert all(r[3] == 1.0 for r in flat if r[0] in (R.BRIGHTNESS, R.CONTRAST, R.COLOR, R.SHARPNESS))
    assert all(r[2] == 256 for r in flat if r[0] == R.SOLARIZE) and all(r[2] == 4 for r in flat if r[0] == R.POSTERIZE)
    assert all(r[4] == R.IDENTITY for r in flat if r[0] == R.AFFINE) and aug._py.getstate() != state
    aug.magnitude = 10
    aug.draw(32, 32)
    assert any(r[2] == 0 for image in aug.last for r in image if r[0] == R.SOLARIZE)


def test_levels_at_magnitude_10():
    aug = _aug(spec="rand-m10-inc1", seed=0)
    aug.prob = 1.0
    S, seen = 40, {}
    for name in R.OP_NAMES * 8:
        seen.setdefault(name, set()).add(aug._draw_op(name, S))
    f32 = lambda v: float(np.float32(v))
    for name, op in (("Color", R.COLOR), ("Contrast", R.CONTRAST), ("Brightness", R.BRIGHTNESS), ("Sharpness", R.SHARPNESS)):
        assert {r[3] for r in seen[name]} == {f32(1.9), f32(1.0 - 0.9)} and {r[0] for r in seen[name]} == {op}
    assert seen["Posterize"] == {_rec(R.POSTERIZE, iarg=0)} and seen["Solarize"] == {_rec(R.SOLARIZE, iarg=0)}
    assert seen["SolarizeAdd"] == {_rec(R.SOLARIZE_ADD, iarg=110)}
    assert {r[4] for r in seen["ShearX"]} == {(1.0, 0.3, 0.0, 0.0, 1.0, 0.0), (1.0, -0.3, 0.0, 0.0, 1.0, 0.0)}
    assert {r[4] for r in seen["ShearY"]} == {(1.0, 0.0, 0.0, 0.3, 1.0, 0.0), (1.0, 0.0, 0.0, -0.3, 1.0, 0.0)}
    assert {r[4][2] for r in seen["TranslateXRel"]} == {0.45 * S, -0.45 * S} and {r[4][5] for r in seen["TranslateYRel"]} == {0.45 * S, -0.45 * S}
    assert {r[4] for r in seen["Rotate"]} == {R.rotate_matrix(30.0, S), R.rotate_matrix(-30.0, S)}
    assert {r[1] for r in seen["Rotate"] | seen["ShearX"] | seen["TranslateYRel"]} == {1, 2}
    m = R.rotate_matrix(30.0, S)
    assert m[0] == round(math.cos(-math.radians(30.0)), 15) and abs(m[0] * 20 + m[1] * 20 + m[2] - 20) < 1e-12      # the centre stays
    # the non-increasing rules
    low = _aug(spec="rand-m10-inc0", seed=0)
    low.prob = 1.0
    assert low._draw_op("Posterize", S) == _rec(R.POSTERIZE, iarg=4) and low._draw_op("Solarize", S) == _rec(R.SOLARIZE, iarg=256)
    assert low._draw_op("Color", S) == _rec(R.COLOR, farg=1.9)


# ================================================================================================================ 3. specs, records, arguments
def test_spec_parsing():
    from autoprog_amd.data import parse_randaug_spec
    assert parse_randaug_spec("rand-m9-mstd0.5-inc1") == dict(magnitude=9, n=2, mstd=0.5, inc=True)
    assert parse_randaug_spec("rand-m4-n3-mstd1-inc0") == dict(magnitude=4, n=3, mstd=1.0, inc=False)
    assert parse_randaug_spec("rand-mstd0.5") == dict(magnitude=10, n=2, mstd=0.5, inc=False)       # a missing m: timm's _MAX_LEVEL
    assert parse_randaug_spec("rand") == dict(magnitude=10, n=2, mstd=0.0, inc=False)
    assert parse_randaug_spec("") is None and parse_randaug_spec(None) is None
    for bad in ("rand-m9-w0", "augmix-m3", "original", "rand-m9-foo1", "rand-m", "rand-m9-n0", "rand-m9-n9"):
        with pytest.raises(ValueError):
            parse_randaug_spec(bad)
    off = _aug(spec="")
    x = torch.zeros(2, 3, 4, 4, dtype=torch.uint8)
    assert not off.enabled and off(x) is x and off.last is None
    a = _aug()
    assert (a.magnitude, a.magnitude_std, a.n_layers, a.increasing, a.prob, a.enabled) == (9, 0.5, 2, True, 0.5, True)
    a.set_spec("")
    assert not a.enabled and a.magnitude == 9
    a.set_spec("rand-m3-mstd0.5-inc1")
    assert a.enabled and a.magnitude == 3
    with pytest.raises(ValueError):
        _aug(layout="chw")
    assert _aug(mean=(1.0, 0.5, 0.0)).fill == (255, 128, 0)


def test_records_round_trip_through_the_block():
    from autoprog_amd import ops
    from autoprog_amd.data import DeviceRandAugment
    aug = _aug(spec="rand-m9-n3-mstd0.5-inc1", seed=8)
    host = aug.draw(6, 96)
    assert DeviceRandAugment.unpack(host.numpy(), 6, 3) == aug.last and all(len(image) == 3 for image in aug.last)
    a = host.numpy().reshape(6, 3, ops.RANDAUG_RECORD_WORDS)
    for b, image in enumerate(aug.last):
        for j, (op, filt, iarg, farg, m) in enumerate(image):
            assert (a[b, j, 0], a[b, j, 1], a[b, j, 2]) == (op, filt, iarg)
            assert a[b, j, 3:4].view(np.float32)[0] == np.float32(farg) and float(np.float32(farg)) == farg
            assert a[b, j, 4:].view(np.float64).tolist() == list(m)
    assert (ops.RA_NONE, ops.RA_AUTOCONTRAST, ops.RA_EQUALIZE, ops.RA_INVERT, ops.RA_SOLARIZE, ops.RA_SOLARIZE_ADD, ops.RA_POSTERIZE,
            ops.RA_BRIGHTNESS, ops.RA_CONTRAST, ops.RA_COLOR, ops.RA_SHARPNESS, ops.RA_AFFINE) == tuple(range(12))
    header = open(os.path.join(ROOT, "include", "autoprog_hip.h")).read()
    for name, code in (("AP_RA_NONE", 0), ("AP_RA_EQUALIZE", 2), ("AP_RA_POSTERIZE", 6), ("AP_RA_CONTRAST", 8), ("AP_RA_AFFINE", 11),
                       ("AP_RANDAUG_RECORD_WORDS", 16), ("AP_RANDAUG_MAX_LAYERS", ops.RANDAUG_MAX_LAYERS)):
        assert re.search(r"\b%s = %d\b" % (name, code), header), name


def test_driver_argument_validation():
    from autoprog_amd.data import DeviceBatchPrep
    from autoprog_amd.prog.driver import AutoProgDriver
    prep = DeviceBatchPrep((0.5,) * 3, (0.25,) * 3, device="cpu")
    aug = _aug()
    base = dict(model=None, loss_fn=None, optimizer=None, reducer=None, get_batch=None, r_list=[64, 96], l_list=[3, 3], dp_list=[0.0, 0.0],
                grow_epochs=[0, 1], steps_per_epoch=1)
    for kw in (dict(aa_list=["", "rand-m9"]), dict(aa_list=["", "rand-m9"], batch_prep=prep), dict(augment=aug),
               dict(augment=aug, batch_prep=prep, aa_list=["rand-m9"]), dict(augment=_aug(layout="nhwc"), batch_prep=prep),
               dict(augment=aug, batch_prep=prep, aa_list=["", "rand-m9-w0"])):
        with pytest.raises(ValueError):
            AutoProgDriver(**base, **kw)
    with pytest.raises(TypeError):                                  # keyword only
        AutoProgDriver(*base.values(), 2, True, 4, 4, 0, None, 1, None, "", False, 2, None, "norm", None, prep, None, False, None, None, None, aug)
    drv = AutoProgDriver(**base, batch_prep=prep, augment=aug, aa_list=["", "rand-m9-mstd0.5-inc1"])
    assert drv.augment is aug and drv.aa_list == ["", "rand-m9-mstd0.5-inc1"]
    plain = AutoProgDriver(**base)
    assert plain.augment is None and plain.aa_list is None


def test_entry_point_is_declared_exported_and_refuses_before_any_launch():
    from autoprog_amd._lib import _SIGNATURES, EXPORTED_SYMBOLS, LIB_PATH, RandAugArgs, lib
    header = open(os.path.join(ROOT, "include", "autoprog_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % SYMBOL, header)
    assert SYMBOL in EXPORTED_SYMBOLS and SYMBOL in _SIGNATURES and hasattr(ctypes.CDLL(LIB_PATH), SYMBOL)
    assert lib.ap_abi_version() == 7
    src = open(os.path.join(ROOT, "autoprog_amd", "csrc", "Makefile")).read()
    assert "randaug.hip" in src and re.search(r"randaug\.o: CXXFLAGS \+= -ffp-contract=off", src)
    a = RandAugArgs()
    a.B, a.S, a.n_layers = 0, 8, 2
    assert lib.ap_randaug_u8(ctypes.byref(a), None) == 0           # B = 0: success, nothing is touched
    a.B = 1
    assert lib.ap_randaug_u8(ctypes.byref(a), None) == -4          # null pointers
    for field, bad in (("S", 0), ("S", 16385), ("n_layers", 0), ("n_layers", 9), ("layout", 2), ("B", -1), ("B", 65536)):
        b = RandAugArgs()
        b.B, b.S, b.n_layers = 1, 8, 1
        setattr(b, field, bad)
        assert lib.ap_randaug_u8(ctypes.byref(b), None) == -1, (field, bad)
    assert lib.ap_randaug_u8(None, None) == -4
