"""numpy restatement of ap_randaug_u8's pixel rules (include/autoprog_hip.h) and of timm 0.4.5's RandAugment draw rules
(data.DeviceRandAugment's docstring).  tests/test_device_randaug_host.py holds the pixel rules to Pillow's own bytes (the committed
golden file, and live calls where PIL imports); the GPU tests hold the kernel to these functions with array_equal.

Images are uint8 [S, S, 3]; a record is (op, filter, int argument, float32 factor, (m0 .. m5)).  numpy rounds every float32 / float64
operation on its own, which is what the rules ask for."""
import math

import numpy as np

(NONE, AUTOCONTRAST, EQUALIZE, INVERT, SOLARIZE, SOLARIZE_ADD, POSTERIZE, BRIGHTNESS, CONTRAST, COLOR, SHARPNESS, AFFINE) = range(12)
BILINEAR, BICUBIC = 1, 2
NO_MATRIX = (0.0,) * 6
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
OP_NAMES = ("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast", "Brightness",
            "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")


# ---------------------------------------------------------------------------------------------------------------- pixel rules
def grey(img):
    v = img.astype(np.int64)
    return (19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 0x8000) >> 16


def blend(d, i, f):
    """Image.blend(degenerate, image, f) on integer arrays"""
    f = np.float32(f)
    d, i = np.asarray(d, dtype=np.int64), np.asarray(i, dtype=np.int64)
    t = d.astype(np.float32) + f * (i - d).astype(np.float32)
    assert t.dtype == np.float32
    if 0.0 <= f <= 1.0:
        return t.astype(np.int64)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.int64)


def _point(img, luts):
    """luts: [3, 256]"""
    return np.stack([np.asarray(luts[c], dtype=np.int64)[img[..., c]] for c in range(3)], axis=-1).astype(np.uint8)


def invert(img):
    return _point(img, [255 - np.arange(256)] * 3)


def solarize(img, t):
    i = np.arange(256)
    return _point(img, [np.where(i < t, i, 255 - i)] * 3)


def solarize_add(img, a):
    i = np.arange(256)
    return _point(img, [np.where(i < 128, np.minimum(255, i + a), i)] * 3)


def posterize(img, bits):
    if bits >= 8:
        return img.copy()
    return _point(img, [np.arange(256) & ~(2 ** (8 - bits) - 1)] * 3)


def brightness(img, f):
    return _point(img, [blend(0, np.arange(256), f)] * 3)


def contrast(img, f):
    S = img.shape[0]
    m = int(float(int(grey(img).sum())) / float(S * S) + 0.5)
    return _point(img, [blend(m, np.arange(256), f)] * 3)


def autocontrast(img):
    luts = []
    for c in range(3):
        lo, hi = int(img[..., c].min()), int(img[..., c].max())
        if hi <= lo:
            luts.append(np.arange(256))
            continue
        scale = 255.0 / (hi - lo)
        offset = -lo * scale
        luts.append(np.clip(np.trunc(np.arange(256, dtype=np.float64) * scale + offset), 0, 255).astype(np.int64))
    return _point(img, luts)


def equalize(img):
    S = img.shape[0]
    luts = []
    for c in range(3):
        h = np.bincount(img[..., c].reshape(-1), minlength=256)
        nz = np.nonzero(h)[0]
        step = 0 if len(nz) <= 1 else (S * S - int(h[nz[-1]])) // 255
        if step == 0:
            luts.append(np.arange(256))
            continue
        n, lut = step // 2, []
        for i in range(256):
            lut.append(min(255, n // step))
            n += int(h[i])
        luts.append(np.array(lut))
    return _point(img, luts)


def color(img, f):
    return blend(grey(img)[..., None], img, f).astype(np.uint8)


def smooth(img):
    S = img.shape[0]
    out = img.copy()
    if S < 3:
        return out
    v = img.astype(np.float32)
    k1, k5 = np.float32(1.0) / np.float32(13.0), np.float32(5.0) / np.float32(13.0)
    ss = np.full((S - 2, S - 2, 3), np.float32(0.5), dtype=np.float32)
    for dy in (1, 0, -1):
        row = v[1 + dy:S - 1 + dy]
        kb = k5 if dy == 0 else k1
        ss = ss + ((row[:, 0:S - 2] * k1 + row[:, 1:S - 1] * kb) + row[:, 2:S] * k1)
    assert ss.dtype == np.float32
    out[1:S - 1, 1:S - 1] = np.where(ss <= 0, 0, np.where(ss >= 255, 255, np.trunc(ss))).astype(np.uint8)
    return out


def sharpness(img, f):
    return blend(smooth(img), img, f).astype(np.uint8)


def _cub(v1, v2, v3, v4, d):
    return v2 + d * ((-v1 + v3) + d * ((2 * (v1 - v2) + v3 - v4) + d * (-v1 + v2 - v3 + v4)))


def affine(img, m, filt, fill):
    S = img.shape[0]
    m = [np.float64(v) for v in m]
    xc = (np.arange(S, dtype=np.float64) + 0.5)[None, :]
    yc = (np.arange(S, dtype=np.float64) + 0.5)[:, None]
    with np.errstate(all="ignore"):
        xin = m[0] * xc + m[1] * yc + m[2]
        yin = m[3] * xc + m[4] * yc + m[5]
        inside = (xin >= 0) & (xin < S) & (yin >= 0) & (yin < S)
    xin, yin = np.where(inside, xin, 1.0) - 0.5, np.where(inside, yin, 1.0) - 0.5
    X, Y = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = (xin - X)[..., None], (yin - Y)[..., None]
    src = img.astype(np.float64)
    cl = lambda v: np.clip(v, 0, S - 1)
    if filt == BICUBIC:
        cols = [cl(X - 1 + j) for j in range(4)]
        row = lambda r: _cub(src[r, cols[0]], src[r, cols[1]], src[r, cols[2]], src[r, cols[3]], dx)
        rv = [row(cl(Y - 1))]
        for j in (1, 2, 3):
            yy = Y - 1 + j
            ok = ((yy >= 0) & (yy < S))[..., None]
            rv.append(np.where(ok, row(cl(yy)), rv[-1]))
        v = _cub(rv[0], rv[1], rv[2], rv[3], dy)
        res = np.where(v <= 0, 0, np.where(v >= 255, 255, np.trunc(v)))
    else:
        x0, x1 = cl(X), cl(X + 1)
        lin = lambda r: src[r, x0] + (src[r, x1] - src[r, x0]) * dx
        v1 = lin(cl(Y))
        ok = ((Y + 1 >= 0) & (Y + 1 < S))[..., None]
        v2 = np.where(ok, lin(cl(Y + 1)), v1)
        res = np.trunc(v1 + (v2 - v1) * dy)
    out = np.where(inside[..., None], res, np.asarray(fill, dtype=np.float64)[None, None, :])
    return out.astype(np.uint8)


def apply_record(img, rec, fill):
    op, filt, iarg, farg, m = rec
    if op == AUTOCONTRAST:
        return autocontrast(img)
    if op == EQUALIZE:
        return equalize(img)
    if op == INVERT:
        return invert(img)
    if op == SOLARIZE:
        return solarize(img, iarg)
    if op == SOLARIZE_ADD:
        return solarize_add(img, iarg)
    if op == POSTERIZE:
        return posterize(img, iarg)
    if op == BRIGHTNESS:
        return brightness(img, farg)
    if op == CONTRAST:
        return contrast(img, farg)
    if op == COLOR:
        return color(img, farg)
    if op == SHARPNESS:
        return sharpness(img, farg)
    if op == AFFINE:
        return affine(img, m, BICUBIC if filt == BICUBIC else BILINEAR, fill)
    return img.copy()                                              # none, and every unknown code


def hwc(batch, layout):
    return batch.transpose(0, 2, 3, 1) if layout == "nchw" else batch


def apply(batch, records, fill, layout="nchw"):
    """batch: uint8 [B,3,S,S] / [B,S,S,3]; records: per image a list of records, applied in order -> the same shape"""
    out = []
    for img, recs in zip(hwc(batch, layout), records):
        img = np.ascontiguousarray(img)
        for r in recs:
            img = apply_record(img, r, fill)
        out.append(img)
    out = np.stack(out) if out else np.zeros(hwc(batch, layout).shape, dtype=np.uint8)
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2)) if layout == "nchw" else out


# ---------------------------------------------------------------------------------------------------------------- matrices
def rotate_matrix(deg, S):
    """Image.rotate(deg) on an S x S image; None where Pillow copies"""
    deg = deg % 360.0
    if deg == 0:
        return None
    a = -math.radians(deg)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    c = S / 2.0
    m[2] = m[0] * (-c) + m[1] * (-c) + m[2] + c
    m[5] = m[3] * (-c) + m[4] * (-c) + m[5] + c
    return tuple(m)


# ---------------------------------------------------------------------------------------------------------------- draw rules
class CountingRandom:
    """wraps a random.Random and logs which of its methods are called, in order"""

    def __init__(self, py):
        self.py, self.calls = py, []

    def random(self):
        self.calls.append("random")
        return self.py.random()

    def gauss(self, mu, sigma):
        self.calls.append("gauss")
        return self.py.gauss(mu, sigma)

    def choice(self, seq):
        self.calls.append("choice")
        return self.py.choice(seq)


def draw_op(name, py, S, magnitude, mstd, prob, increasing):
    """timm's AugmentOp.__call__ for one op -> a record; `py` a random.Random (or CountingRandom)"""
    none = (NONE, 0, 0, 0.0, NO_MATRIX)
    if prob < 1.0 and py.random() > prob:
        return none
    mag = magnitude
    if mstd > 0:
        mag = py.gauss(mag, mstd)
    mag = min(10.0, max(0, mag))
    L = mag / 10.0
    neg = lambda v: -v if py.random() > 0.5 else v
    f32 = lambda v: float(np.float32(v))
    if name in ("AutoContrast", "Equalize", "Invert"):
        return ({"AutoContrast": AUTOCONTRAST, "Equalize": EQUALIZE, "Invert": INVERT}[name], 0, 0, 0.0, NO_MATRIX)
    if name in ("Color", "Contrast", "Brightness", "Sharpness"):
        f = 1.0 + neg(L * 0.9) if increasing else L * 1.8 + 0.1
        return ({"Color": COLOR, "Contrast": CONTRAST, "Brightness": BRIGHTNESS, "Sharpness": SHARPNESS}[name], 0, 0, f32(f), NO_MATRIX)
    if name == "Posterize":
        return (POSTERIZE, 0, 4 - int(L * 4) if increasing else int(L * 4), 0.0, NO_MATRIX)
    if name == "Solarize":
        return (SOLARIZE, 0, 256 - int(L * 256) if increasing else int(L * 256), 0.0, NO_MATRIX)
    if name == "SolarizeAdd":
        return (SOLARIZE_ADD, 0, int(L * 110), 0.0, NO_MATRIX)
    if name == "Rotate":
        m = rotate_matrix(neg(L * 30.0), S)
    elif name == "ShearX":
        m = (1.0, neg(L * 0.3), 0.0, 0.0, 1.0, 0.0)
    elif name == "ShearY":
        m = (1.0, 0.0, 0.0, neg(L * 0.3), 1.0, 0.0)
    elif name == "TranslateXRel":
        m = (1.0, 0.0, neg(L * 0.45) * S, 0.0, 1.0, 0.0)
    else:
        assert name == "TranslateYRel", name
        m = (1.0, 0.0, 0.0, 0.0, 1.0, neg(L * 0.45) * S)
    filt = py.choice((BILINEAR, BICUBIC))
    return none if m is None else (AFFINE, filt, 0, 0.0, tuple(float(v) for v in m))


def draw(nprs, py, B, S, magnitude=9, mstd=0.5, prob=0.5, n=2, increasing=True):
    """per image: RandomState.choice(15, n), then the ops' draws in order -> per-image lists of n records"""
    out = []
    for _ in range(B):
        names = [OP_NAMES[k] for k in nprs.choice(15, n)]
        out.append([draw_op(name, py, S, magnitude, mstd, prob, increasing) for name in names])
    return out
