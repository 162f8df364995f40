"""numpy restatement of ap_crop_resize_u8's arithmetic (include/autoprog_hip.h), shared by the host and GPU tests of the device crop.

    f = max((o + 0.5) * (ext / S) - 0.5, 0), i0 = min(floor(f), ext - 1), i1 = min(i0 + 1, ext - 1), l = f - i0     (o = S-1-ox when flipped)
    v = (1-ly)*((1-lx)*p00 + lx*p01) + ly*((1-lx)*p10 + lx*p11);  out = clip(rint(v), 0, 255), half to even

`dtype` is the type every operation is rounded in: float32 is what the kernel computes, float64 the reference the GPU tests measure it
against.  `crop_resize_int` is an integer-only reference for boxes whose sides are integer multiples of S."""
import numpy as np


def _axis(S, ext, flip, dt):
    o = np.arange(S)
    if flip:
        o = S - 1 - o
    scale = dt(ext) / dt(S)
    f = np.maximum((o.astype(dt) + dt(0.5)) * scale - dt(0.5), dt(0))
    i0 = np.minimum(np.floor(f).astype(np.int64), ext - 1)
    i1 = np.minimum(i0 + 1, ext - 1)
    return i0, i1, (f - i0.astype(dt)).astype(dt)


def crop_resize_one(img, S, record, dtype=np.float64):
    """img uint8 [H, W, C]; record (top, left, h, w, flip) -> uint8 [S, S, C]"""
    dt = np.dtype(dtype).type
    top, left, h, w, flip = (int(v) for v in record[:5])
    box = img[top:top + h, left:left + w].astype(dt)
    y0, y1, ly = _axis(S, h, 0, dt)
    x0, x1, lx = _axis(S, w, flip, dt)
    ly, lx = ly[:, None, None], lx[None, :, None]
    one = dt(1)
    p00, p01 = box[y0][:, x0], box[y0][:, x1]
    p10, p11 = box[y1][:, x0], box[y1][:, x1]
    v = (one - ly) * ((one - lx) * p00 + lx * p01) + ly * ((one - lx) * p10 + lx * p11)
    assert v.dtype == np.dtype(dtype)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def crop_resize(u8, S, records, layout="nchw", dtype=np.float64):
    """u8 uint8 [B,3,H,W] / [B,H,W,3] (numpy), records [B, >= 5] -> uint8 [B,3,S,S] / [B,S,S,3]"""
    u8, records = np.asarray(u8), np.asarray(records)
    imgs = u8.transpose(0, 2, 3, 1) if layout == "nchw" else u8
    out = np.stack([crop_resize_one(imgs[b], S, records[b], dtype) for b in range(u8.shape[0])])
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2)) if layout == "nchw" else out


def crop_resize_int(img, S, record):
    """integer-only: img uint8 [H, W, C], a box with h % S == 0 and w % S == 0.  With k = ext / S the source coordinate is o k + (k - 1) / 2:
    an odd k picks pixel o k + (k - 1) / 2, an even k takes the mean of pixels o k + k / 2 - 1 and o k + k / 2; the mean of n = 1, 2 or 4
    bytes is rounded half to even in integers"""
    top, left, h, w, flip = (int(v) for v in record[:5])
    assert h % S == 0 and w % S == 0
    box = img[top:top + h, left:left + w].astype(np.int64)

    def taps(k):
        o = np.arange(S)
        return [o * k + (k - 1) // 2] if k % 2 else [o * k + k // 2 - 1, o * k + k // 2]
    ty, tx = taps(h // S), taps(w // S)
    s = sum(box[y][:, x] for y in ty for x in tx)
    n = len(ty) * len(tx)
    q, rem = s // n, s % n
    q = q + ((2 * rem > n) | ((2 * rem == n) & (q % 2 == 1)))
    out = q.astype(np.uint8)
    return out[:, ::-1] if flip else out
