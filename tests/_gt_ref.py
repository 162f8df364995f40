"""The class rows of TokenLabelGTCrossEntropy on the sparse target [B, 2 + N, K], restated with plain torch on the CPU: the weighted-pair
form of include/autoprog_hip.h (ap_soft_ce_sparse_gt_fwd_bwd), its argmax rule included.  Nothing here imports the GPU side of the package.

  dense_s[c] = (1 - s) * sum_k [idx_k == c] * val_k + s / C              slot 0: ground truth, slot 1: image level
  a_s        = argmax: a class's score is the fp32 sum of its pairs' val in ascending k; the smallest class among those of the largest
               score; class 0 if no score is positive
  ratio_b    = 0.9 - 0.4 * [a_0 == a_1]
  row b      = lam * (ratio_b * dense_1[b] + (1 - ratio_b) * dense_0[b]) + (1 - lam) * (the same of image B-1-b, with ITS ratio)

tests/test_gt_loss_host.py holds this against oracle.ref_cpu.token_label_gt_ce on the densified target."""
import torch

_BIG = 2 ** 31 - 1


def densify(idx, val, C, smoothing, dtype=torch.float32):
    """[B, S, K] pairs -> [B, C, S] as SparseTokenLabelTarget.dense builds it (fp32 by default), with indices outside [0, C) adding nothing"""
    idx, val = idx.cpu().long(), val.cpu().to(dtype)
    B, S, K = idx.shape
    ok = (idx >= 0) & (idx < C)
    t = torch.zeros(B, C, S, dtype=dtype)
    t.scatter_add_(1, torch.where(ok, idx, torch.zeros_like(idx)).permute(0, 2, 1), torch.where(ok, val, torch.zeros_like(val)).permute(0, 2, 1))
    return t * (1.0 - smoothing) + smoothing / C


def slot_scores(idx, val, C):
    """[B, K] -> (fp32 [B, K]: the score of pair k's class, -1 where the index is outside [0, C); bool [B, K])"""
    idx, val = idx.cpu().long(), val.cpu().float()
    ok = (idx >= 0) & (idx < C)
    sc = torch.zeros(idx.shape, dtype=torch.float32)
    for j in range(idx.shape[1]):                      # ascending k, fp32
        sc = sc + torch.where((idx[:, j:j + 1] == idx) & ok[:, j:j + 1], val[:, j:j + 1], torch.zeros(()))
    return torch.where(ok, sc, torch.full_like(sc, -1.0)), ok


def slot_argmax(idx, val, C):
    sc, ok = slot_scores(idx, val, C)
    best = sc.max(-1, keepdim=True)[0]
    cand = torch.where(ok & (sc == best) & (best > 0), idx.cpu().long(), torch.full_like(idx.cpu().long(), _BIG))
    am = cand.min(-1)[0]
    return torch.where(am == _BIG, torch.zeros_like(am), am)


def score_gap(idx, val, C):
    """[B, K] -> fp64 [B]: the largest class score minus the second largest (0 stands for a class without pairs); inf for a slot without a
    positive score (no valid pair, or scores of 0 only), whose argmax is class 0 by the rule and by torch.max on the constant row s / C"""
    sc, ok = slot_scores(idx, val, C)
    out = []
    for b in range(idx.shape[0]):
        per_class = {int(i): float(s) for i, s, o in zip(idx[b].cpu(), sc[b], ok[b]) if o}
        if not per_class or max(per_class.values()) <= 0:
            out.append(float("inf"))
            continue
        top = sorted(per_class.values(), reverse=True) + [0.0]
        out.append(top[0] - top[1])
    return torch.tensor(out, dtype=torch.float64)


def ratios(idx, val, C):
    """[B, 2 + N, K] -> fp64 [B]"""
    same = slot_argmax(idx[:, 0], val[:, 0], C) == slot_argmax(idx[:, 1], val[:, 1], C)
    return 0.9 - 0.4 * same.double()


def class_pairs(idx, val, C, lam=1.0):
    """the weighted pairs of every class row: (int64 [B, 4 K], fp64 [B, 4 K]) in the order own slot 1, own slot 0, partner slot 1, partner
    slot 0 with the weights lam r_b, lam (1 - r_b), (1 - lam) r_p, (1 - lam) (1 - r_p); the label smoothing is not applied here"""
    idx, val = idx.cpu().long(), val.cpu().double()
    r = ratios(idx, val, C)[:, None]
    rp = r.flip(0)
    pi = torch.cat([idx[:, 1], idx[:, 0], idx[:, 1].flip(0), idx[:, 0].flip(0)], dim=1)
    pw = torch.cat([lam * r * val[:, 1], lam * (1 - r) * val[:, 0], (1 - lam) * rp * val[:, 1].flip(0), (1 - lam) * (1 - rp) * val[:, 0].flip(0)], dim=1)
    return pi, pw


def class_target(idx, val, C, smoothing, lam=1.0):
    """fp64 [B, C]: (1 - s) * scatter(weighted pairs) + s / C"""
    pi, pw = class_pairs(idx, val, C, lam)
    ok = (pi >= 0) & (pi < C)
    t = torch.zeros(pi.shape[0], C, dtype=torch.float64)
    t.scatter_add_(1, torch.where(ok, pi, torch.zeros_like(pi)), torch.where(ok, pw, torch.zeros_like(pw)))
    return t * (1.0 - smoothing) + smoothing / C


def soft_ce_rows(logits, t, grad_scale):
    """fp64: row_loss [M] = -sum_c t log_softmax(x), dlogits [M, C] = grad_scale * d(sum of row losses) / dx"""
    x = logits.detach().cpu().double().requires_grad_(True)
    rows = -(t * (x - torch.logsumexp(x, -1, keepdim=True))).sum(-1)
    (rows.sum() * grad_scale).backward()
    return rows.detach(), x.grad


def gt_loss(x_cls, x_aux, idx, val, smoothing, lam, dense_weight, cls_weight):
    """fp64 scalar: the whole TokenLabelGTCrossEntropy from the pairs (class rows from class_target, token rows from their own slots)"""
    B, N, C = x_aux.shape
    t_aux = densify(idx, val, C, smoothing, torch.float64)[:, :, 2:].transpose(1, 2).reshape(B * N, C)
    xc, xa = x_cls.double(), x_aux.double().reshape(B * N, C)
    ce = lambda x, t: (-(t * (x - torch.logsumexp(x, -1, keepdim=True))).sum(-1)).mean()
    return cls_weight * ce(xc, class_target(idx, val, C, smoothing, lam)) + dense_weight * ce(xa, t_aux)


def make_case(B, N, C, K, seed):
    """-> (idx int32 [B, 2 + N, K], val fp32, the ratio every image must get).  Scores descend like a teacher's top-K: (K - k + jitter) / sum.
    image 0: the label is the teacher's top class                         -> 0.5
    image 1: the label is NOT the top pair's class; with K >= 3 pairs 1 and 2 of slot 1 repeat the label's class and their sum beats pair 0
             -> 0.5, and 0.9 for K < 3 (nothing accumulates)
    image 2: slot 0 holds only -1 fillers, the teacher's top class is not 0 -> argmax 0 against it: 0.9
    image 3: slot 0 only fillers and the teacher's top class IS 0           -> 0.5
    later images: the label alternates between the top class and another one"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randperm(C - 1, generator=g)[:K] + 1 for _ in range(B * (2 + N))]).reshape(B, 2 + N, K).int()     # no class 0, no repeats
    raw = torch.arange(K, 0, -1).float() + 0.2 * torch.rand(B, 2 + N, K, generator=g)
    val = raw / raw.sum(-1, keepdim=True)
    want = []
    for b in range(B):
        top = int(idx[b, 1, 0])
        other = 1 + (top % (C - 1))                                  # a class != top, != 0
        idx[b, 0], val[b, 0] = -1, 0.0
        if b == 0 or (b > 3 and b % 2 == 0):
            idx[b, 0, 0], val[b, 0, 0] = top, 1.0
            want.append(0.5)
        elif b == 1:
            idx[b, 0, 0], val[b, 0, 0] = other, 1.0
            if K >= 3:
                idx[b, 1, 1] = idx[b, 1, 2] = other
                want.append(0.5)
            else:
                idx[b, 1, 1:] = torch.tensor([c for c in range(1, C) if c not in (top, other)][:K - 1]).int()
                want.append(0.9)
        elif b == 2:
            want.append(0.9)
        elif b == 3:
            idx[b, 1, 0] = 0
            want.append(0.5)
        else:
            if other in idx[b, 1].tolist():
                idx[b, 1][idx[b, 1] == other] = 0
            idx[b, 0, 0], val[b, 0, 0] = other, 1.0
            want.append(0.9)
    return idx, val, torch.tensor(want, dtype=torch.float64)
