"""The rule of adaptive gradient clipping (AGC) in fp64, stated twice, for tests/test_agc_host.py and tests/test_gpu_agc.py.

It restates timm 0.4.5's `adaptive_clip_grad` and `unitwise_norm` from knowledge of that code.  timm is not a dependency of this project:
the rule is NOT byte-checked against timm.  include/autoprog_hip.h (ap_agc_clip) carries the same text.

  Units.   A tensor with ndim <= 1 is one unit; one with ndim >= 2 has shape[0] units of numel / shape[0] contiguous elements.
  Rule.    pn = ||p||, gn = grad_scale * ||g||, max_norm = max(pn, eps) * clip_factor.  gn < max_norm: untouched.  Otherwise every element
           is multiplied by max_norm / max(gn, 1e-6).  (grad_scale: a pending 1/world; the gradient stays the SUM.)
  Skipped. a unit with its skip byte set is untouched.
  Deviation: a unit whose gn is not finite (an inf or NaN element) is untouched; timm would multiply it by 0 or NaN.

`agc_flat` states it on a flat slab plus unit table with numpy; `agc_per_parameter` as timm writes it, a loop over parameter tensors with
norm(dim=tuple(range(1, ndim)), keepdim=True) in torch.  Both compute in fp64."""
import numpy as np
import torch


def agc_flat(g, p, unit_off, unit_skip, clip_factor, eps=1e-3, grad_scale=1.0):
    """g, p: 1-D arrays; unit_off: n_units + 1 ascending bounds from 0 to len(g), no empty unit; unit_skip: n_units flags.
    -> (clipped gradient fp64 -- elements of untouched units are the inputs' values --, factor per unit fp64 (1 where untouched),
        bool per unit: clipped, bool per unit: non-finite)"""
    g = np.asarray(g, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    off = np.asarray(unit_off, dtype=np.int64)
    skip = np.asarray(unit_skip).astype(bool)
    lens = np.diff(off)
    assert off[0] == 0 and off[-1] == g.size == p.size and (lens > 0).all() and skip.size == lens.size
    bad_el = ~np.isfinite(g)
    nonfinite = np.add.reduceat(bad_el.astype(np.int64), off[:-1]) > 0
    with np.errstate(invalid="ignore", over="ignore"):
        gn = float(grad_scale) * np.sqrt(np.add.reduceat(np.where(bad_el, 0.0, g) ** 2, off[:-1]))
        pn = np.sqrt(np.add.reduceat(p ** 2, off[:-1]))
        max_norm = np.maximum(pn, float(eps)) * float(clip_factor)
        clipped = ~(gn < max_norm) & ~skip & ~nonfinite
        factor = np.where(clipped, max_norm / np.maximum(gn, 1e-6), 1.0)
        el = np.repeat(clipped, lens)
        out = np.where(el, g * np.repeat(factor, lens), g)
    return out, factor, clipped, nonfinite & ~skip


def unitwise_norm(x):
    if x.ndim <= 1:
        return x.norm(2.0)
    return x.norm(2.0, dim=tuple(range(1, x.ndim)), keepdim=True)


def agc_per_parameter(params, grads, clip_factor, eps=1e-3, grad_scale=1.0):
    """the per-parameter loop: params, grads -- lists of tensors of equal shapes.  -> the new gradients, fp64 tensors."""
    out = []
    for p, g in zip(params, grads):
        p64, g64 = p.detach().double(), g.detach().double()
        max_norm = unitwise_norm(p64).clamp(min=eps).mul(clip_factor)
        grad_norm = unitwise_norm(g64) * grad_scale
        clipped = g64 * (max_norm / grad_norm.clamp(min=1e-6))
        keep = (grad_norm < max_norm) | ~torch.isfinite(grad_norm)                # (the stated deviation: a non-finite unit stays)
        out.append(torch.where(keep, g64, clipped))
    return out


def units_of(shapes):
    """the unit table of tensors of these shapes laid back to back: -> n_units + 1 bounds"""
    off = [0]
    for shape in shapes:
        n = int(np.prod(shape)) if len(shape) else 1
        rows = shape[0] if len(shape) >= 2 else 1
        for _ in range(rows):
            off.append(off[-1] + n // rows)
    return off
