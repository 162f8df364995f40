#!/usr/bin/env python
"""Writes tests/golden/pil_randaug.npz: small uint8 images, RandAugment records in the word layout of ap_randaug_u8
(include/autoprog_hip.h) and what the installed Pillow makes of them through the calls timm's auto_augment.py uses: ImageOps.autocontrast /
equalize / invert / posterize, Image.point (Solarize, SolarizeAdd), ImageEnhance.Color / Contrast / Brightness / Sharpness,
Image.transform(size, AFFINE, m, resample, fillcolor=...) and Image.rotate(deg, resample, fillcolor=...).
tests/test_device_randaug_host.py holds the numpy restatement of the rules (tests/_randaug_ref.py) to these bytes, and the GPU tests hold
the kernel to the restatement.

    python tools/make_pil_randaug_golden.py             # needs Pillow; rewrites the fixture, deterministic

Layout of the file: image_<i> uint8 [S, S, 3]; image int32 [N] the image of case k; n_layers int32 [N] (1 or 2); records int32 [N, 2, 16];
degrees float64 [N, 2]: the angle handed to Image.rotate where the record came from a rotation (its matrix is then Image.rotate's own),
NaN elsewhere; fill uint8 [3]; out uint8, the N results of S x S x 3 bytes one after the other; pillow_version."""
import math
import os

import numpy as np
import PIL
from PIL import Image, ImageEnhance, ImageOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
(NONE, AUTOCONTRAST, EQUALIZE, INVERT, SOLARIZE, SOLARIZE_ADD, POSTERIZE, BRIGHTNESS, CONTRAST, COLOR, SHARPNESS, AFFINE) = range(12)
PIL_FILTER = {1: Image.BILINEAR, 2: Image.BICUBIC}
ENHANCER = {BRIGHTNESS: ImageEnhance.Brightness, CONTRAST: ImageEnhance.Contrast, COLOR: ImageEnhance.Color, SHARPNESS: ImageEnhance.Sharpness}
FILL = (124, 116, 104)
Z6 = (0.0,) * 6


def pillow(im, rec, deg):
    op, filt, iarg, farg, m = rec
    if op == AUTOCONTRAST:
        return ImageOps.autocontrast(im)
    if op == EQUALIZE:
        return ImageOps.equalize(im)
    if op == INVERT:
        return ImageOps.invert(im)
    if op == SOLARIZE:
        return im.point([i if i < iarg else 255 - i for i in range(256)] * 3)
    if op == SOLARIZE_ADD:
        return im.point([min(255, i + iarg) if i < 128 else i for i in range(256)] * 3)
    if op == POSTERIZE:
        return ImageOps.posterize(im, iarg)
    if op in ENHANCER:
        return ENHANCER[op](im).enhance(farg)
    if op == AFFINE and not math.isnan(deg):
        return im.rotate(deg, resample=PIL_FILTER[filt], fillcolor=FILL)
    if op == AFFINE:
        return im.transform(im.size, Image.AFFINE, m, resample=PIL_FILTER[filt], fillcolor=FILL)
    return im.copy()


def rotate_matrix(deg, S):
    a = -math.radians(deg % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    c = S / 2.0
    m[2] = m[0] * (-c) + m[1] * (-c) + m[2] + c
    m[5] = m[3] * (-c) + m[4] * (-c) + m[5] + c
    return tuple(m)


def op_cases(S, spatial_only):
    """(record, degrees) for every op at its extremes: both filters and both signs of the geometric ops, factors on both sides of 1"""
    f32 = lambda v: float(np.float32(v))
    out = []
    for filt in (1, 2):
        for sign in (1, -1):
            out += [((AFFINE, filt, 0, 0.0, (1.0, 0.3 * sign, 0.0, 0.0, 1.0, 0.0)), math.nan), ((AFFINE, filt, 0, 0.0, (1.0, 0.0, 0.0, 0.3 * sign, 1.0, 0.0)), math.nan),
                    ((AFFINE, filt, 0, 0.0, (1.0, 0.0, 0.45 * sign * S, 0.0, 1.0, 0.0)), math.nan), ((AFFINE, filt, 0, 0.0, (1.0, 0.0, 0.0, 0.0, 1.0, 0.45 * sign * S)), math.nan),
                    ((AFFINE, filt, 0, 0.0, rotate_matrix(30.0 * sign, S)), 30.0 * sign), ((AFFINE, filt, 0, 0.0, rotate_matrix(7.3 * sign, S)), 7.3 * sign)]
    out += [((SHARPNESS, 0, 0, f32(f), Z6), math.nan) for f in (0.1, 0.55, 1.0, 1.9)]
    if spatial_only:
        return out
    out += [((op, 0, 0, 0.0, Z6), math.nan) for op in (AUTOCONTRAST, EQUALIZE, INVERT, NONE)]
    out += [((SOLARIZE, 0, t, 0.0, Z6), math.nan) for t in (0, 77, 256)] + [((SOLARIZE_ADD, 0, a, 0.0, Z6), math.nan) for a in (0, 110)]
    out += [((POSTERIZE, 0, b, 0.0, Z6), math.nan) for b in (0, 1, 4)]
    out += [((op, 0, 0, f32(f), Z6), math.nan) for op in (BRIGHTNESS, CONTRAST, COLOR) for f in (0.1, 0.55, 1.0, 1.9)]
    return out


def pack(recs):
    a = np.zeros((2, 16), dtype=np.int32)
    for j, (op, filt, iarg, farg, m) in enumerate(recs):
        a[j, 0:3] = (op, filt, iarg)
        a[j, 3:4].view(np.float32)[0] = farg
        a[j, 4:16].view(np.float64)[:] = m
    return a


def build():
    g = np.random.RandomState(2025)
    images, cases = [], []                                        # cases: (image, [(record, degrees), ...])
    for S in (3, 7, 16):
        two = g.randint(0, 2, (S, S, 3)) * 255
        two[..., 1] = np.where(two[..., 1] > 0, 200, 40)          # a two-valued channel away from the extremes
        for img in (g.randint(0, 256, (S, S, 3)), two, np.full((S, S, 3), (9, 130, 255))):      # random; 0 / 255 and two-valued; constant
            images.append(img.astype(np.uint8))
            cases += [(len(images) - 1, [c]) for c in op_cases(S, False)]
    images.append(g.randint(0, 256, (33, 33, 3)).astype(np.uint8))
    cases += [(len(images) - 1, [c]) for c in op_cases(33, True)]
    chain_img = 6                                                 # the random 16 x 16 image
    single = op_cases(16, False)
    pick = lambda op, k=0: [c for c in single if c[0][0] == op][k]
    cases += [(chain_img, [pick(AFFINE, 16), pick(EQUALIZE)]), (chain_img, [pick(CONTRAST, 3), pick(AFFINE, 0)]),
              (chain_img, [pick(AUTOCONTRAST), pick(SHARPNESS, 3)]), (chain_img, [pick(SOLARIZE, 1), pick(AFFINE, 15)]),
              (chain_img, [pick(COLOR, 0), pick(POSTERIZE, 1)])]
    out = []
    for i, recs in cases:
        im = Image.fromarray(images[i], "RGB")
        for rec, deg in recs:
            im = pillow(im, rec, deg)
        out.append(np.asarray(im).reshape(-1))
    return (images, np.asarray([i for i, _ in cases], dtype=np.int32), np.asarray([len(r) for _, r in cases], dtype=np.int32),
            np.stack([pack([c[0] for c in r]) for _, r in cases]),
            np.asarray([[c[1] for c in r] + [math.nan] * (2 - len(r)) for _, r in cases], dtype=np.float64), np.concatenate(out))


def main():
    images, image, n_layers, records, degrees, out = build()
    path = os.path.join(ROOT, "tests", "golden", "pil_randaug.npz")
    np.savez_compressed(path, image=image, n_layers=n_layers, records=records, degrees=degrees, fill=np.asarray(FILL, dtype=np.uint8), out=out,
                        pillow_version=np.array(PIL.__version__), **{"image_%d" % i: c for i, c in enumerate(images)})
    print("%s: %d cases, %d result bytes, %d bytes on disk, Pillow %s" % (path, len(image), out.size, os.path.getsize(path), PIL.__version__))


if __name__ == "__main__":
    main()
