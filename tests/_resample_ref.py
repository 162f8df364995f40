"""numpy restatement of ap_crop_resample_u8's rule (include/autoprog_hip.h), shared by the host and GPU tests of the antialiased device
crop: Pillow's Image.crop(box).resize((S, S), BILINEAR | BICUBIC) on an 8-bit image.  Two separable passes, the horizontal one first and
rounded to uint8, the vertical one on its result.  Coefficients in float64, every operation rounded on its own (numpy scalars and arrays
of float64 never fuse), sums in int64 (Pillow's int32 cannot overflow with normalised weights: 255 * sum |K| < 2^31); the image is
cropped first; the flip acts on the output.

A record is (top, left, h, w, flip, filter) with filter 1 = bilinear, 2 = bicubic."""
import numpy as np

BILINEAR, BICUBIC = 1, 2
PRECISION_BITS = 22


def _bilinear(x):
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    inner = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    outer = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, inner, np.where(x < 2.0, outer, 0.0))


def coefficients(n, S, filt):
    """-> [(xmin, K int64 [taps])] for the S windows of an axis of extent n"""
    f, sup0 = (_bicubic, 2.0) if filt == BICUBIC else (_bilinear, 1.0)
    scale = np.float64(n) / np.float64(S)
    fs = max(scale, np.float64(1.0))
    support = np.float64(sup0) * fs
    ss = np.float64(1.0) / fs
    out = []
    for o in range(S):
        center = (np.float64(o) + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)                 # int(): C truncation
        xmax = min(int(center + support + 0.5), n)
        k = f(((np.arange(xmin, xmax).astype(np.float64) - center) + 0.5) * ss)
        ww = np.float64(0.0)
        for v in k:                                                # in this order
            ww = ww + v
        if ww != 0.0:
            k = k / ww
        K = np.trunc(k * 4194304.0 + np.where(k < 0, -0.5, 0.5)).astype(np.int64)
        out.append((xmin, K))
    return out


def _pass(src, S, filt):
    """src uint8 [n, ...] -> uint8 [S, ...] along axis 0"""
    n = src.shape[0]
    wide = src.astype(np.int64)
    out = np.empty((S,) + src.shape[1:], dtype=np.uint8)
    for o, (xmin, K) in enumerate(coefficients(n, S, filt)):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(K, wide[xmin:xmin + len(K)], axes=(0, 0))
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resample_one(img, S, record):
    """img uint8 [H, W, C]; record (top, left, h, w, flip, filter) -> uint8 [S, S, C]"""
    top, left, h, w, flip, filt = (int(v) for v in record[:6])
    assert filt in (BILINEAR, BICUBIC), filt
    box = img[top:top + h, left:left + w]
    hor = _pass(np.ascontiguousarray(box.transpose(1, 0, 2)), S, filt).transpose(1, 0, 2)      # [h, S, C], uint8
    out = _pass(np.ascontiguousarray(hor), S, filt)
    return np.ascontiguousarray(out[:, ::-1]) if flip else out


def resample(u8, S, records, layout="nchw"):
    """u8 uint8 [B,3,H,W] / [B,H,W,3] (numpy), records [B, >= 6] -> uint8 [B,3,S,S] / [B,S,S,3]"""
    u8, records = np.asarray(u8), np.asarray(records)
    imgs = u8.transpose(0, 2, 3, 1) if layout == "nchw" else u8
    out = np.stack([resample_one(imgs[b], S, records[b]) for b in range(u8.shape[0])])
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2)) if layout == "nchw" else out
