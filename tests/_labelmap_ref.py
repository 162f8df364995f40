"""fp64 numpy restatement of ap_label_map_crop's rule (include/autoprog_hip.h): the forward of roi_align(aligned=False, sampling_ratio=-1)
on the densified top-k label maps, written as the literal sample loop over a dense [C] row per bin.  This is the project's definition,
restated from knowledge of tlt and torchvision, not byte-checked against them (neither is installed)."""
import math

import numpy as np

TOL = 1e-4          # (number of terms + the weight roundings) * 2^-24 with at most 4096 candidates of non-negative terms: under 1e-4
TINY = 1e-37


def _axis(v, n):
    """a sample coordinate -> (low pixel, high pixel, weight of the high pixel)"""
    v = max(v, 0.0)
    lo = int(v)
    if lo >= n - 1:
        lo = hi = n - 1
        v = float(lo)
    else:
        hi = lo + 1
    return lo, hi, v - lo


def dense_bin(scores, classes, C, box, Pn, ph, pw):
    """the dense [C] row of bin (ph, pw) of a Pn x Pn pooling of box = (x1, y1, x2, y2); scores fp64 [Kin, Hm, Wm], classes int64"""
    Kin, Hm, Wm = scores.shape
    x1, y1, x2, y2 = (float(v) for v in box[:4])
    roi_w, roi_h = max(x2 - x1, 1.0), max(y2 - y1, 1.0)
    bin_w, bin_h = roi_w / Pn, roi_h / Pn
    gw, gh = int(math.ceil(roi_w / Pn)), int(math.ceil(roi_h / Pn))
    dense = np.zeros(C, dtype=np.float64)
    for iy in range(gh):
        y = y1 + ph * bin_h + (iy + 0.5) * bin_h / gh
        for ix in range(gw):
            x = x1 + pw * bin_w + (ix + 0.5) * bin_w / gw
            if y < -1.0 or y > Hm or x < -1.0 or x > Wm:
                continue
            yl, yh, ly = _axis(y, Hm)
            xl, xh, lx = _axis(x, Wm)
            hy, hx = 1.0 - ly, 1.0 - lx
            for wgt, cy, cx in ((hy * hx, yl, xl), (hy * lx, yl, xh), (ly * hx, yh, xl), (ly * lx, yh, xh)):
                for k in range(Kin):
                    c = classes[k, cy, cx]
                    if 0 <= c < C:
                        dense[c] += wgt * scores[k, cy, cx]
    return dense * (1.0 / (gh * gw))


def label_map_ref(scores, classes, boxes, P, C):
    """scores [B, Kin, Hm, Wm], classes the same shape (floats are truncated), boxes [B, >= 5] (x1, y1, x2, y2, flip as fp32 values) ->
    per image the list of its 1 + P P rows in SLOT order (slot 1, then the token slots with the flip applied), each row a pair
    (classes ascending, their dense values > 0)"""
    scores = np.asarray(scores, dtype=np.float64)
    classes = np.trunc(np.asarray(classes, dtype=np.float64)).astype(np.int64)
    out = []
    for b in range(scores.shape[0]):
        box = [float(np.float32(v)) for v in boxes[b][:5]]
        flip = int(box[4])
        rows = [dense_bin(scores[b], classes[b], C, box, 1, 0, 0)]
        for ph in range(P):
            for pw in range(P):
                rows.append(dense_bin(scores[b], classes[b], C, box, P, ph, P - 1 - pw if flip else pw))
        sparse = []
        for d in rows:
            nz = np.nonzero(d > 0)[0]
            sparse.append((nz, d[nz]))
        out.append(sparse)
    return out


def topk_row(row, K):
    """the K largest of a row by descending value, equal values by ascending class -> (idx [K] with -1 fillers, val [K], dropped)"""
    cls, val = row
    order = np.lexsort((cls, -val))[:K]
    idx = np.full(K, -1, dtype=np.int64)
    v = np.zeros(K, dtype=np.float64)
    idx[:len(order)], v[:len(order)] = cls[order], val[order]
    rest = np.ones(len(cls), dtype=bool)
    rest[order] = False
    return idx, v, float(val[rest].sum())


def check_row(idx, val, dropped, row, K, what):
    """the comparison rule of the GPU tests on one row; it skips none.  idx [K] int, val [K] fp32, dropped fp32 or None"""
    cls, ref = row
    lookup = dict(zip(cls.tolist(), ref.tolist()))
    idx, val = [int(i) for i in idx], [float(v) for v in val]
    kept = [i for i in idx if i != -1]
    n = len(kept)
    assert idx[n:] == [-1] * (K - n) and all(v == 0.0 for v in val[n:]), "%s: fillers must be (-1, 0.0) behind the pairs: %s %s" % (what, idx, val)
    assert len(set(kept)) == n, "%s: a class twice: %s" % (what, idx)
    for j in range(n):
        assert kept[j] in lookup, "%s: class %d kept, the reference has nothing there" % (what, kept[j])
        r = lookup[kept[j]]
        assert val[j] > 0 and abs(val[j] - r) <= TOL * r + TINY, "%s: pair %d (%d, %.9g), reference %.9g" % (what, j, kept[j], val[j], r)
        if j:
            assert val[j] < val[j - 1] or (val[j] == val[j - 1] and kept[j] > kept[j - 1]), "%s: order broken at pair %d: %s %s" % (what, j, idx, val)
    floor = val[n - 1] if n == K else 0.0
    left = [(c, r) for c, r in lookup.items() if c not in kept]
    for c, r in left:
        assert r <= floor * (1.0 + TOL) + TINY, "%s: class %d with %.9g was left out, the smallest kept value is %.9g" % (what, c, r, floor)
    if dropped is not None:
        want = float(sum(r for _, r in left))
        assert abs(float(dropped) - want) <= TOL * want + TINY, "%s: dropped %.9g, reference %.9g" % (what, float(dropped), want)
