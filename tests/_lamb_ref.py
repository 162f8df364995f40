"""The LAMB rule of ap_lamb_ema_step (include/autoprog_hip.h) in fp64, stated twice: `lamb_flat` in numpy on flat slabs plus tensor offsets,
as the kernel sees them, and `lamb_per_parameter`, a torch loop over tensors as apex's FusedLAMB and timm's Lamb write it.  Restated from
knowledge of that code; neither library is installed, so neither statement is byte-checked against them.

Both take the numbers the kernel takes: fp32-representable betas, eps, rates, decays and scales, and the two bias corrections rounded to
fp32 the way ap_adamw_ema_step forms them (`bias_corrections`)."""
import numpy as np
import torch


def f32(x):
    """the fp32 value nearest to x, as a Python float"""
    return float(np.float32(x))


def bias_corrections(beta1, beta2, t):
    """(1 - beta1^t, sqrt(1 - beta2^t)) as the kernels get them: double arithmetic on the fp32 betas, rounded to fp32 once"""
    b1, b2 = f32(beta1), f32(beta2)
    return f32(1.0 - b1 ** int(t)), f32(np.sqrt(1.0 - b2 ** int(t)))


def clip_coefficient(g, grad_scale, max_norm):
    """clip_grad_norm_'s factor on the MEAN gradient: min(1, max_norm / (grad_scale * ||g|| + 1e-6)); 1 without a bound"""
    if not max_norm:
        return 1.0
    norm = float(grad_scale) * float(np.sqrt((np.asarray(g, dtype=np.float64) ** 2).sum()))
    return min(1.0, float(max_norm) / (norm + 1e-6))


def lamb_flat(p, g, m, v, offsets, group_id, group_tab, t, beta1=0.9, beta2=0.999, eps=1e-6, grad_scale=1.0, max_norm=0.0, clip_value=0.0,
              always_adapt=False, trust_clip=False, ema=(), ema_decay=(), bc=None):
    """one step on flat slabs.  offsets: one entry more than there are tensors, ascending from 0 (elements past offsets[-1] are the
    slab's pad: returned as they came).  group_id: one group number per element; group_tab [G, 2] of {lr_eff, wd}.  bc: the two bias
    corrections when they do not follow from t.  -> dict of fp64 arrays: p, m, v, u, ema (list), wn, un, phi (per tensor), and the
    magnitudes the fp32 roundings of the kernel are counted against (tests/test_gpu_lamb.py): `mag_u` = |r / bc1| + wd * |p| per element,
    with |r| from the NON-CANCELLING moment beta1 |m| + (1 - beta1) |gh|, and `mag` = |p| + lr * phi * mag_u."""
    p, g, m, v = (np.array(a, dtype=np.float64) for a in (p, g, m, v))
    off = np.asarray(offsets, dtype=np.int64)
    n = int(off[-1])
    b1, b2, eps = f32(beta1), f32(beta2), f32(eps)
    bc1, bc2s = bias_corrections(beta1, beta2, t) if bc is None else (float(bc[0]), float(bc[1]))
    tab = np.asarray(group_tab, dtype=np.float32).astype(np.float64)
    gid = np.asarray(group_id[:n], dtype=np.int64)
    lr, wd = tab[gid, 0], tab[gid, 1]
    gh = f32(grad_scale) * g[:n] * clip_coefficient(g[:n], f32(grad_scale), max_norm)
    if clip_value and clip_value > 0:
        gh = np.clip(gh, -f32(clip_value), f32(clip_value))
    m1 = b1 * m[:n] + (1.0 - b1) * gh
    v1 = b2 * v[:n] + (1.0 - b2) * gh * gh
    denom = np.sqrt(v1) / bc2s + eps
    r = m1 / denom
    u = r / bc1 + wd * p[:n]
    r_mag = (b1 * np.abs(m[:n]) + (1.0 - b1) * np.abs(gh)) / denom / bc1
    n_t = off.size - 1
    wn, un, phi = np.zeros(n_t), np.zeros(n_t), np.ones(n_t)
    for i in range(n_t):
        a, b = int(off[i]), int(off[i + 1])
        wn[i] = np.sqrt((p[a:b] ** 2).sum())
        un[i] = np.sqrt((u[a:b] ** 2).sum())
        adapt = always_adapt or (b > a and wd[a] != 0.0)
        if adapt and wn[i] > 0 and un[i] > 0:
            phi[i] = wn[i] / un[i]
        if trust_clip:
            phi[i] = min(phi[i], 1.0)
    phi = phi.astype(np.float32).astype(np.float64)                                  # (formed in fp64, rounded to fp32 once)
    phi_el = np.repeat(phi, np.diff(off))
    out = {"p": p.copy(), "m": m.copy(), "v": v.copy(), "u": u, "wn": wn, "un": un, "phi": phi}
    out["p"][:n] = p[:n] - (lr * phi_el) * u
    out["m"][:n], out["v"][:n] = m1, v1
    out["mag_u"] = r_mag + wd * np.abs(p[:n])
    out["mag"] = np.abs(p[:n]) + lr * phi_el * out["mag_u"]
    out["ema"] = []
    for e, d in zip(ema, ema_decay):
        e = np.array(e, dtype=np.float64)
        d = f32(d)
        e[:n] = d * e[:n] + (1.0 - d) * out["p"][:n]
        out["ema"].append(e)
    return out


def lamb_per_parameter(params, grads, exp_avgs, exp_avg_sqs, lrs, wds, t, beta1=0.9, beta2=0.999, eps=1e-6, grad_scale=1.0, max_norm=0.0,
                       clip_value=0.0, always_adapt=False, trust_clip=False, bc=None):
    """the same step as a loop over parameter tensors, in place on fp64 torch tensors (params, exp_avgs, exp_avg_sqs are updated; grads are
    only read), the way apex and timm write it: global pre-scaling, moments, update = (m / bc1) / denom, `+ wd p` when the group decays,
    the trust ratio from the two tensor norms, p -= lr * trust * update.  lrs / wds: one number per tensor.  -> [(wn, un, phi)] per tensor."""
    b1, b2, eps = f32(beta1), f32(beta2), f32(eps)
    bc1, bc2s = bias_corrections(beta1, beta2, t) if bc is None else (float(bc[0]), float(bc[1]))
    gs = f32(grad_scale)
    if max_norm:
        total = gs * float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))
        gs = gs * min(1.0, float(max_norm) / (total + 1e-6))
    report = []
    for p, g, m, v, lr, wd in zip(params, grads, exp_avgs, exp_avg_sqs, lrs, wds):
        lr, wd = f32(lr), f32(wd)
        gh = g.double() * gs
        if clip_value and clip_value > 0:
            gh = gh.clamp(-f32(clip_value), f32(clip_value))
        m.mul_(b1).add_(gh, alpha=1.0 - b1)
        v.mul_(b2).addcmul_(gh, gh, value=1.0 - b2)
        denom = v.sqrt().div_(bc2s).add_(eps)
        update = (m / bc1).div_(denom)
        if wd != 0.0:
            update.add_(p, alpha=wd)
        wn, un, phi = float(p.norm(2)), float(update.norm(2)), 1.0
        if (wd != 0.0 or always_adapt) and wn > 0 and un > 0:
            phi = wn / un
        if trust_clip:
            phi = min(phi, 1.0)
        phi = f32(phi)
        p.add_(update, alpha=-lr * phi)
        report.append((wn, un, phi))
    return report
