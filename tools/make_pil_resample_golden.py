#!/usr/bin/env python
"""Writes tests/golden/pil_resample.npz: small uint8 images, crop records and what the installed Pillow makes of them with
Image.crop(box).resize((S, S), BILINEAR | BICUBIC) and, where the record says so, transpose(FLIP_LEFT_RIGHT) afterwards -- the order of
timm's RandomResizedCropAndInterpolation + RandomHorizontalFlip.  tests/test_device_resample_host.py holds the numpy restatement of the
rule (tests/_resample_ref.py) to these bytes, and the GPU tests hold the kernel to the restatement.

    python tools/make_pil_resample_golden.py            # needs Pillow; rewrites the fixture, deterministic

Layout of the file: canvas_<i> uint8 [H, W, 3]; cases int32 [N, 8] = (canvas, top, left, h, w, flip, filter, S) with filter 1 = bilinear,
2 = bicubic; out uint8, the N results of S x S x 3 bytes one after the other; pillow_version."""
import os

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIL_FILTER = {1: Image.BILINEAR, 2: Image.BICUBIC}


def pillow(canvas, rec, S):
    top, left, h, w, flip, filt = rec
    im = Image.fromarray(canvas, "RGB").crop((left, top, left + w, top + h)).resize((S, S), PIL_FILTER[filt])
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(im)


def build():
    g = np.random.RandomState(2024)
    canvases = [g.randint(0, 256, (40, 56, 3)).astype(np.uint8),                     # 0: random bytes
                (g.randint(0, 2, (40, 56, 3)) * 255).astype(np.uint8),               # 1: 0 / 255 noise (the largest overshoot of bicubic)
                g.randint(0, 256, (5, 7, 3)).astype(np.uint8),                       # 2: the 5 x 7 upscale
                (g.randint(0, 2, (64, 64, 3)) * 255).astype(np.uint8)]               # 3: 0 / 255 noise for the 4x downscale
    cases = []
    for filt in (1, 2):
        for flip in (0, 1):
            cases.append((2, 0, 0, 5, 7, flip, filt, 31))                            # 5 x 7 -> 31
            cases.append((2, 0, 0, 5, 7, flip, filt, 5))
            cases.append((3, 0, 0, 64, 64, flip, filt, 16))                          # 4 x 4 down
            cases.append((1, 10, 20, 20, 20, flip, filt, 5))
            cases.append((3, 1, 3, 62, 51, flip, filt, 24))                          # 2.6 x 2.1 down
            cases.append((0, 0, 0, 40, 56, flip, filt, 16))                          # 2.5 x 3.5 down
        cases.append((0, 0, 0, 40, 56, filt - 1, filt, 64))                          # the whole canvas up
        for S in (1, 5, 16):
            cases.append((0, 3, 4, 1, 1, S & 1, filt, S))                            # 1 x 1
            cases.append((1, 39, 0, 1, 56, 1 - (S & 1), filt, S))                    # 1 x n
            cases.append((0, 0, 55, 40, 1, S & 1, filt, S))                          # n x 1
            cases.append((1, 7, 11, 1, 9, 0, filt, S))
        cases.append((0, 7, 13, 24, 24, 0, filt, 24))                                # identity boxes
        cases.append((1, 7, 13, 24, 24, 1, filt, 24))
        for S in (1, 5, 16, 24, 31):                                                 # general boxes at every size
            for c in (0, 1):
                h, w = int(g.randint(2, 41)), int(g.randint(2, 57))
                cases.append((c, int(g.randint(0, 41 - h)), int(g.randint(0, 57 - w)), h, w, int(g.randint(0, 2)), filt, S))
    cases = np.asarray(cases, dtype=np.int32)
    out = np.concatenate([pillow(canvases[c[0]], tuple(int(v) for v in c[1:7]), int(c[7])).reshape(-1) for c in cases])
    return canvases, cases, out


def main():
    canvases, cases, out = build()
    path = os.path.join(ROOT, "tests", "golden", "pil_resample.npz")
    np.savez_compressed(path, cases=cases, out=out, pillow_version=np.array(PIL.__version__),
                        **{"canvas_%d" % i: c for i, c in enumerate(canvases)})
    print("%s: %d cases, %d result bytes, %d bytes on disk, Pillow %s" % (path, len(cases), out.size, os.path.getsize(path), PIL.__version__))


if __name__ == "__main__":
    main()
