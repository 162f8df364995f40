"""Shapes, trip arithmetic and fp64 references of the multi-item cases (tests/test_gpu_multi_item.py, tests/test_multi_item_host.py).

Plain torch on the CPU; nothing here imports the GPU side of the package.

A persistent or grid-capped launch starts `grid` workgroups and workgroup j walks the items j, j + grid, ...: it runs the loop body
ceil((items - j) / grid) times.  A case of tests/test_gpu_multi_item.py must give every workgroup a second item and some a third (the
first, a middle and the last step of a software pipeline all run), with an item count that is no multiple of the grid (the last sweep
is partial).  `trips` is that rule; the GPU cases assert it on the grid the library reports before they launch anything.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

Trips = namedtuple("Trips", "items grid fewest most ok")


def cdiv(a, b):
    return -(-a // b)


def trips(items, grid):
    """-> Trips(items, grid, fewest and most loop trips of a workgroup, the verdict): ok = every workgroup runs the body at least twice,
    some run it a third time, and the items do not divide among the workgroups evenly"""
    if items < 1 or grid < 1:
        raise ValueError("trips: items and grid are positive (got %r, %r)" % (items, grid))
    grid = min(grid, items)
    fewest, most = items // grid, cdiv(items, grid)
    return Trips(items, grid, fewest, most, fewest >= 2 and most >= 3 and items % grid != 0)


def tiles(B, H, W, th, tw):
    return B * cdiv(H, th) * cdiv(W, tw)


def tile_classes(tiles_y, tiles_x):
    """edge-mask class (last tile row: ragged rows masked; last tile column: ragged columns masked) of the tiles of one image in the order the
    convolution kernels decode them: tx = t % tiles_x, ty = (t / tiles_x) % tiles_y (csrc/conv.hip, conv128.hip, conv7.hip: tile_origin)"""
    return [(t // tiles_x == tiles_y - 1, t % tiles_x == tiles_x - 1) for t in range(tiles_y * tiles_x)]


def strip_classes(nstrips, heads):
    """the same for the outlook items of one image: head = it % heads, strip = (it / heads) % nstrips (csrc/outlook.hip, k_outlook_p: decode);
    the last strip is the ragged one"""
    return [it // heads == nstrips - 1 for it in range(nstrips * heads)]


def masks_change(classes, grid):
    """-> (verdict, share): a workgroup's next item is `grid` items on.  Where the items of an image divide the grid, every item of a
    workgroup sits at the SAME place of its image -- same edge masks, only the image changes -- and a previous tile stored under the current
    tile's masks, or a prefetched patch padded by the wrong tile's validity, gives the same bits.  verdict: the grid is no multiple of the
    items per image AND at least half of the places are followed by a place of another mask class"""
    n = len(classes)
    share = sum(classes[i] != classes[(i + grid) % n] for i in range(n)) / float(n)
    return grid % n != 0 and share >= 0.5, share


def full_and_ragged(n, t):
    """a dimension of n pixels holds a full tile of t and a ragged one"""
    return n > t and n % t != 0


# ------------------------------------------------------------------------------------------------------------ LayerNorm backward
def ln_bwd_geometry(C):
    """-> (rows a workgroup holds at once, rows per lane group and trip U) of the pipelined backward kernel: csrc/layernorm.hip,
    pick_group_wide (lane-group width G: 16, doubled up to 64 until it covers C / 8 chunks; V = chunks per lane) and the dispatch in
    ap_layernorm_bwd (k_ln_bwd_pf<1, 2> for V = 1, k_ln_bwd_pf<2, 1> for V = 2)"""
    nch = C // 8
    G = 16
    while G < 64 and G < nch:
        G *= 2
    V = cdiv(nch, G)
    if V > 2:
        raise ValueError("ln_bwd_geometry: C = %d is not on the pipelined kernel" % C)
    return 256 // G, (2 if V == 1 else 1)


def ln_trips(rows, grid, gpb, U):
    """lane group g of grid * gpb handles rows g + u * groups + k * groups * U (u < U) in trip k and runs trip k while its first row
    exists -> Trips in units of lane groups; ok additionally wants the last sweep partial"""
    groups = grid * gpb
    per = [cdiv(max(rows - g, 0), groups * U) for g in (0, groups - 1)]
    most, fewest = per[0], per[1]
    return Trips(rows, groups, fewest, most, fewest >= 2 and most >= 3 and rows % (groups * U) != 0)


def ln_rows(grid, gpb, U):
    """the row count at which EVERY lane group runs three trips and the third is partial (U = 2: its second row is missing for most
    groups); U = 1 cannot have both: two trips for every group and a third for half of them"""
    groups = grid * gpb
    return 2 * groups * U + groups + (groups // 3 | 1) if U > 1 else 2 * groups + groups // 2 + 1


# ------------------------------------------------------------------------------------------------------------------ shapes
# 64-channel 3x3 family and BatchNorm: 32 x 16 tiles -> 2 x 3 = 6 per image, 744; 16 x 16 -> 9 per image, 1116; T = 135036 rows.
# ((240, 33, 17) has 4 tiles of 32 x 16 per image, which divide the grid of 256: every workgroup would meet ONE kind of tile.)
C64_SHAPE = (124, 33, 33)
C128_SHAPE = (110, 33, 17)           # 16 x 16 tiles -> 660
CONV7_SHAPE = (200, 33, 33)          # output map 33 x 33 (a 66 x 66 image): 32 x 16 tiles -> 1200, 16 x 16 -> 1800
OUTLOOK_SHAPE = (700, 7, 7, 3)       # two strips per image and head, the second ragged; 3 heads: 6 items per image (no divisor of a grid
                                     # that is a power of two times 8), 4200 items
LN_TOKENS = (7, 7)                   # LayerNorm rows come as [B, 7, 7] token grids (the pool form needs a grid)
ADAM_SWEEP_F4 = 4096 * 256           # float4s one sweep of k_adamw_ema covers (csrc/optim.hip, adamw_ema_launch: grid <= 256 * 16)
SUMSQ_SWEEP_F4 = 1024 * 256          # ap_sumsq_f32: grid <= 1024
ADAM_N = 4 * (2 * ADAM_SWEEP_F4 + 1001)


def rnd(*shape, scale=1.0, shift=0.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(torch.bfloat16)


def frand(*shape, seed=0, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift


# -------------------------------------------------------------------------------------------------------------- references (fp64)
def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def conv3x3(x, w):
    """x [B,H,W,C] (any float dtype), w [Co,Ci,3,3] -> [B,H,W,Co] in the dtype of the operands"""
    return nhwc(F.conv2d(nchw(x), w, None, 1, 1)).contiguous()


def conv3x3_dgrad(dy, w):
    return nhwc(F.conv_transpose2d(nchw(dy), w, None, 1, 1)).contiguous()


def conv3x3_wgrad(x, dy):
    C = x.shape[-1]
    return torch.nn.grad.conv2d_weight(nchw(x), (dy.shape[-1], C, 3, 3), nchw(dy), stride=1, padding=1)


def s2d_to_image(xs):
    """[B,h,w,16] space-to-depth -> [B,3,2h,2w] (tests/test_gpu_kernels.py::test_conv7_s2d_fwd_wgrad_vs_torch_fp32)"""
    B, h, w, _ = xs.shape
    return xs[..., :12].reshape(B, h, w, 2, 2, 3).permute(0, 5, 1, 3, 2, 4).reshape(B, 3, 2 * h, 2 * w)


def conv7(xs, w):
    return nhwc(F.conv2d(s2d_to_image(xs), w, None, 2, 3)).contiguous()


def conv7_wgrad(xs, dz):
    return torch.nn.grad.conv2d_weight(s2d_to_image(xs), (dz.shape[-1], 3, 7, 7), nchw(dz), stride=2, padding=3)


def bn_relu(x, gamma, beta, eps=1e-5):
    """training-mode BatchNorm + ReLU over the rows of x [T, C] in x's dtype -> (y, mean, rstd, unbiased variance)"""
    mean = x.mean(0)
    var = x.var(0, unbiased=False)
    rstd = (var + eps).rsqrt()
    return torch.relu((x - mean) * rstd * gamma + beta), mean, rstd, var * (x.shape[0] / (x.shape[0] - 1.0))


def bn_beta_between_inputs(x, gamma, beta):
    """x [T, C] bf16, gamma / beta [C] -> (beta' fp32 [C], the smallest |pre-activation| in fp64).  The gradient of BatchNorm + ReLU is
    discontinuous where (x - mean) rstd gamma + beta crosses zero: among 8.6 million elements one lies within fp32 rounding of the
    threshold, fp32 and fp64 put it on different sides and its whole 16 x 8 tile is 'wrong' in a CORRECT kernel (measured on the fp32
    emulation: worst tile 0.32 at a whole rel of 4e-3).  So beta is moved, per channel, until the threshold lies half way between two
    neighbouring bf16 values (of magnitude >= 0.25): no input is closer to it than 2^-10 of its size, a margin a thousand times fp32's
    rounding, and every arithmetic agrees on the mask."""
    xd = x.double()
    mean, rstd = xd.mean(0), (xd.var(0, unbiased=False) + 1e-5).rsqrt()
    sc = rstd * gamma.double()
    t0 = mean - beta.double() / sc
    t0 = torch.where(t0.abs() < 0.25, torch.where(t0 < 0, -0.25, 0.25).double(), t0)
    lo = t0.to(torch.bfloat16)
    hi = (lo.view(torch.int16) + 1).view(torch.bfloat16)
    t = (lo.double() + hi.double()) / 2
    b = (-(t - mean) * sc).float()
    margin = float(((xd - mean) * sc + b.double()).abs().min())
    return b, margin


def pool_grad(dp, H, W):
    """the backward of the 2 x 2 ceil-mode average pool (count_include_pad = False): dp [B,h,w,C] -> [B,H,W,C]"""
    up = dp.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W]
    ones = torch.ones(1, 1, H, W, dtype=dp.dtype)
    cnt = F.avg_pool2d(ones, 2, 2, ceil_mode=True, count_include_pad=False, divisor_override=1)
    cnt = cnt.repeat_interleave(2, 2).repeat_interleave(2, 3)[0, 0, :H, :W]
    return up / cnt[None, :, :, None]


def layernorm_bwd(x, dy, gamma, eps=1e-5):
    """-> (dx, dgamma, dbeta) of y = LayerNorm(x) gamma + beta for the output gradient dy, in the operands' dtype"""
    mu = x.mean(-1, keepdim=True)
    rstd = (x.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
    xh = (x - mu) * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return dx, (dy * xh).sum(0), dy.sum(0)


def adamw_ema(p, g, m, v, wd_mask, emas, decays, lr, b1, b2, eps, wd, step, gscale, clip_value):
    """one fp64 elementwise AdamW step (torch.optim.AdamW's order: decoupled decay first) with value clipping, then the EMA lerps
    -> (p, m, v, [ema])"""
    g = (g * gscale).clamp(-clip_value, clip_value) if clip_value > 0 else g * gscale
    p = torch.where(wd_mask.bool(), p * (1.0 - lr * wd), p)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * (m / (v.sqrt() / bc2 ** 0.5 + eps))
    return p, m, v, [d * e + (1.0 - d) * p for d, e in zip(decays, emas)]
