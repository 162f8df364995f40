"""The reference of ops.softmax_topk / SparseTokenLabelTarget.from_logits for the tests: fp64 softmax of inv_temp * x on the bf16 logits
as they are, and the order torch.sort(descending=True, stable=True) gives -- equal logits by ascending class index (-0 equals +0)."""
import torch


def topk_ref(x, k, inv_temp=1.0):
    """x [M, C] (bf16 or any float, on the CPU) -> (idx int64 [M, k], val fp64 [M, k])"""
    xf = x.detach().cpu().double()
    order = torch.sort(xf, dim=1, descending=True, stable=True).indices[:, :k]
    p = torch.softmax(inv_temp * xf, dim=1)
    return order, p.gather(1, order)


def check_pairs(idx, val, ref_idx, ref_val, what=""):
    """the bounds of the issue: idx exact, |val - ref| <= 1e-4 ref + 1e-37 (SURVEY O5's bound for fp32 outputs; the floor is for scores below
    fp32's smallest normal, which the hardware may flush), val non-increasing along k.  -> the largest relative error among normal scores"""
    idx, val = idx.detach().cpu().long(), val.detach().cpu().double()
    bad = (idx != ref_idx).nonzero()
    assert bad.numel() == 0, "%s: %d indices differ, first at row %d k %d: got %d, want %d" % (
        what, bad.shape[0], bad[0, 0], bad[0, 1], idx[bad[0, 0], bad[0, 1]], ref_idx[bad[0, 0], bad[0, 1]])
    err = (val - ref_val).abs()
    over = (err > 1e-4 * ref_val + 1e-37).nonzero()
    normal = ref_val > 1.2e-38
    worst = float((err[normal] / ref_val[normal]).max()) if bool(normal.any()) else 0.0
    print("TOPK %s | worst relative error of a score %.3e (bound 1e-4)" % (what, worst))
    assert over.numel() == 0, "%s: %d scores outside 1e-4 ref + 1e-37, first at row %d k %d: got %.9e, want %.9e" % (
        what, over.shape[0], over[0, 0], over[0, 1], val[over[0, 0], over[0, 1]], ref_val[over[0, 0], over[0, 1]])
    assert bool((val[:, 1:] <= val[:, :-1]).all()), "%s: scores are not non-increasing along k" % what
    return worst
