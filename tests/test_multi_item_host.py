"""The multi-item cases' own arithmetic and references (CPU only).

 (a) tests/_multi_item.py::trips / ln_trips -- the rule every case of tests/test_gpu_multi_item.py asserts on the library's grid before it
     launches -- against a direct count of what each workgroup walks, and on the shapes the cases use with the caps the launch code holds;
 (b) the fp64 references of the convolution, BatchNorm and LayerNorm-backward cases against their fp32 emulation rounded to bf16 at the
     cases' shapes: the worst 16 x 8 tile stays below the WHOLE-tensor tolerance, half the per-tile bound -- the condition
     tests/test_tilecheck_host.py sets for TILE_FACTOR, here for tensors of a thousand and more tiles per workgroup sweep.  Batches are
     cut to a part of the GPU cases' (the images are independent and identically drawn; the per-tile statistics do not change with B).
"""
import pytest
import torch

from tests import _multi_item as MI
from tests import _tilecheck as T

TOL_BF16 = 1e-2
TOL_CONV = 5e-3          # tests/test_gpu_kernels.py: the convolutions' outputs and input gradients


def b16(t):
    return t.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------------ (a) trips
@pytest.mark.parametrize("items,grid", [(1, 1), (5, 8), (8, 8), (9, 8), (16, 8), (17, 8), (23, 8), (24, 8), (25, 8), (960, 256), (4400, 2048)])
def test_trips_against_a_direct_walk(items, grid):
    per = [len(range(j, items, grid)) for j in range(min(grid, items))]
    t = MI.trips(items, grid)
    assert (t.fewest, t.most) == (min(per), max(per)) and sum(per) == items
    assert t.ok == (min(per) >= 2 and max(per) >= 3 and items % grid != 0)


def test_trips_verdicts():
    assert MI.trips(17, 8).ok and MI.trips(23, 8).ok and MI.trips(25, 8).ok
    assert not MI.trips(16, 8).ok            # two sweeps exactly: no third item, no partial sweep
    assert not MI.trips(24, 8).ok            # three full sweeps: the last sweep is not partial
    assert not MI.trips(15, 8).ok            # some workgroups stop after their first item
    assert not MI.trips(9, 8).ok and not MI.trips(5, 8).ok
    assert MI.trips(5, 8).grid == 5          # a launch never starts more workgroups than items
    with pytest.raises(ValueError):
        MI.trips(0, 8)


def test_the_cases_shapes_meet_the_conditions_at_the_caps_in_the_launch_code():
    """what the GPU cases assert on the library's answer, here on the caps written in csrc (conv.hip: cv_grid 256, the prefetching
    weight-gradient kernel 256, cw_grid 512; conv128.hip: one workgroup per CU, 256; conv7.hip: 512 / 512; outlook.hip olk_launch:
    ncu * per_cu, per_cu <= 2048 / T with T = 256 or 512; bnrelu.hip bn_grid: 2048 blocks x 32 rows at C = 64)"""
    B, H, W = MI.C64_SHAPE
    for th, tw, cap in ((32, 16, 256), (16, 16, 256), (16, 16, 512)):
        assert MI.trips(MI.tiles(B, H, W, th, tw), cap).ok and MI.full_and_ragged(H, th) and MI.full_and_ragged(W, tw)
        assert MI.masks_change(MI.tile_classes(MI.cdiv(H, th), MI.cdiv(W, tw)), cap)[0]
    assert MI.trips(MI.cdiv(B * H * W, 32), 2048).ok and B * H * W > 2 * 65536
    B, H, W = MI.C128_SHAPE
    assert MI.trips(MI.tiles(B, H, W, 16, 16), 256).ok and MI.masks_change(MI.tile_classes(MI.cdiv(H, 16), MI.cdiv(W, 16)), 256)[0]
    B, H, W = MI.CONV7_SHAPE
    assert MI.trips(MI.tiles(B, H, W, 32, 16), 512).ok and MI.trips(MI.tiles(B, H, W, 16, 16), 512).ok
    assert MI.full_and_ragged(H, 32) and MI.full_and_ragged(W, 16)
    assert MI.masks_change(MI.tile_classes(2, 3), 512)[0] and MI.masks_change(MI.tile_classes(3, 3), 512)[0]
    B, H, W, heads = MI.OUTLOOK_SHAPE
    strips = MI.cdiv((H + 1) // 2, 3)
    assert strips == 2 and ((H + 1) // 2) % 3 != 0
    for cap in (256 * 8, 256 * 4):           # 2048 / T workgroups per CU, T = 256 or 512 threads (the LDS image of a 7 x 7 item allows more)
        assert MI.trips(B * strips * heads, cap).ok and MI.masks_change(MI.strip_classes(strips, heads), cap)[0]
    assert MI.trips(MI.ADAM_N // 4, MI.ADAM_SWEEP_F4).ok and MI.trips((MI.ADAM_N - 1) // 4, MI.SUMSQ_SWEEP_F4).ok and (MI.ADAM_N // 4) % 2 == 1


def test_masks_change_refuses_items_per_image_that_divide_the_grid():
    """(240, 33, 17) on 32 x 16 tiles: 4 tiles per image on 256 workgroups -- workgroup j walks j, j + 256, ... all at one (ty, tx); likewise
    2 strips x 2 heads on a grid that is a multiple of 8"""
    ok, share = MI.masks_change(MI.tile_classes(2, 2), 256)
    assert not ok and share == 0.0
    assert MI.masks_change(MI.strip_classes(2, 2), 1024) == (False, 0.0)
    ok, share = MI.masks_change(MI.tile_classes(2, 3), 256)          # 6 per image: the next item is 256 % 6 = 4 places on
    assert ok and share == 1.0
    cls = MI.tile_classes(2, 3)
    assert cls == [(False, False), (False, False), (False, True), (True, False), (True, False), (True, True)]
    assert MI.masks_change(MI.tile_classes(3, 3), 256) == (True, 8 / 9.0)
    assert MI.masks_change(MI.strip_classes(2, 3), 1024)[0] and MI.masks_change(MI.strip_classes(2, 3), 2048)[0]
    assert not MI.masks_change(MI.strip_classes(2, 3), 768)[0]       # a multiple of 6


@pytest.mark.parametrize("C,grid", [(384, 768), (768, 512), (192, 768)])
def test_layernorm_backward_rows_and_trips(C, grid):
    gpb, U = MI.ln_bwd_geometry(C)
    assert (gpb, U) == {384: (4, 2), 768: (4, 1), 192: (8, 2)}[C]
    rows = MI.cdiv(MI.ln_rows(grid, gpb, U), 49) * 49
    groups = grid * gpb
    per = [len(range(g, rows, groups * U)) for g in range(groups)]          # trips of lane group g: while its first row exists
    t = MI.ln_trips(rows, grid, gpb, U)
    assert (t.fewest, t.most) == (min(per), max(per)) and t.ok
    assert t.most == 3 and t.fewest == (3 if U == 2 else 2)
    if U == 2:                               # the third trip's second row is missing for some lane groups
        assert any(g + 2 * groups * U + groups >= rows for g in range(groups))
    assert not MI.ln_trips(2 * groups * U, grid, gpb, U).ok


# ------------------------------------------------------------------------------- (b) the references inside their own bounds
@pytest.mark.parametrize("shape,C", [(MI.C64_SHAPE, 64), (MI.C128_SHAPE, 128)], ids=["c64", "c128"])
def test_convolution_emulation_stays_under_half_the_tile_bound(shape, C):
    B, H, W = shape
    B = min(B, 48)
    x, dy = MI.rnd(B, H, W, C, seed=1), MI.rnd(B, H, W, C, seed=2)
    w = b16(MI.frand(C, C, 3, 3, seed=3, scale=0.05 * (64.0 / C) ** 0.5))
    for what, got, ref in (("forward", MI.conv3x3(x.float(), w.float()), MI.conv3x3(x.double(), w.double())),
                           ("input gradient", MI.conv3x3_dgrad(dy.float(), w.float()), MI.conv3x3_dgrad(dy.double(), w.double()))):
        rep = T.assert_tiled(b16(got).reshape(-1, C), ref.reshape(-1, C), TOL_CONV, what)
        print("conv3x3 C = %d %s: whole %.2e worst tile %.2e" % (C, what, rep.whole, rep.worst))
        assert rep.worst <= TOL_CONV
    c0 = MI.frand(C, C, 3, 3, seed=4)
    e = T.rel(c0 + MI.conv3x3_wgrad(x.float(), dy.float()), c0.double() + MI.conv3x3_wgrad(x.double(), dy.double()))
    print("conv3x3 C = %d weight gradient: fp32 against fp64 %.2e" % (C, e))
    assert e < 1e-5


def test_conv7_emulation_stays_under_half_the_tile_bound():
    B, H, W = MI.CONV7_SHAPE
    B = 24
    xs = torch.cat([MI.rnd(B, H, W, 12, seed=1), torch.zeros(B, H, W, 4, dtype=torch.bfloat16)], -1)
    w = b16(MI.frand(64, 3, 7, 7, seed=2, scale=0.1))
    rep = T.assert_tiled(b16(MI.conv7(xs.float(), w.float())).reshape(-1, 64), MI.conv7(xs.double(), w.double()).reshape(-1, 64), TOL_CONV, "conv7")
    assert rep.worst <= TOL_CONV
    dz = MI.rnd(B, H, W, 64, seed=3)
    assert T.rel(MI.conv7_wgrad(xs.float(), dz.float()), MI.conv7_wgrad(xs.double(), dz.double())) < 1e-5


def test_batchnorm_emulation_stays_under_half_the_tile_bound():
    B, H, W = MI.C64_SHAPE
    x, dy = MI.rnd(B * H * W, 64, scale=1.5, shift=0.3, seed=1), MI.rnd(B * H * W, 64, seed=2)
    g = MI.frand(64, seed=3, scale=0.3, shift=1.0)
    b, margin = MI.bn_beta_between_inputs(x, g, MI.frand(64, seed=4, scale=0.3))
    assert margin > 1e-5                     # (fp32 rounding of the pre-activation: ~2e-7)
    xr = x.double().requires_grad_(True)
    yr, mr, rr, _ = MI.bn_relu(xr, g.double(), b.double())
    yr.backward(dy.double())
    xf = x.float().requires_grad_(True)
    yf, mf, rf, _ = MI.bn_relu(xf, g, b)
    yf.backward(dy.float())
    assert T.assert_tiled(b16(yf.detach()), yr.detach(), TOL_BF16, "bn + relu").worst <= TOL_BF16
    assert T.assert_tiled(b16(xf.grad), xr.grad, 1.5e-2, "bn + relu backward").worst <= 1.5e-2
    assert T.rel(mf, mr) < 1e-4 and T.rel(rf, rr) < 1e-4


@pytest.mark.parametrize("C", [384, 768])
def test_layernorm_backward_emulation_stays_under_half_the_tile_bound(C):
    grid = 768 if C == 384 else 512
    gpb, U = MI.ln_bwd_geometry(C)
    B = MI.cdiv(MI.ln_rows(grid, gpb, U), 49)
    H, W = MI.LN_TOKENS
    x, dy, dres = MI.rnd(B, H, W, C, scale=2.0, shift=0.5, seed=1), MI.rnd(B, H, W, C, seed=2), MI.rnd(B, H, W, C, seed=3)
    dp = MI.rnd(B, (H + 1) // 2, (W + 1) // 2, C, seed=4)
    gamma = MI.frand(C, seed=5, scale=0.3, shift=1.0)
    for pool in (False, True):
        d64 = dy.double() + (MI.pool_grad(dp.double(), H, W) if pool else 0)
        d32 = dy.float() + (MI.pool_grad(dp.float(), H, W) if pool else 0)
        ref = MI.layernorm_bwd(x.double().reshape(-1, C), d64.reshape(-1, C), gamma.double())
        got = MI.layernorm_bwd(x.float().reshape(-1, C), d32.reshape(-1, C), gamma)
        rep = T.assert_tiled(b16(got[0] + dres.float().reshape(-1, C)), ref[0] + dres.double().reshape(-1, C), TOL_BF16, "layernorm backward")
        assert rep.worst <= TOL_BF16
        assert T.rel(got[1], ref[1]) < 3e-3 and T.rel(got[2], ref[2]) < 3e-3


def test_pool_gradient_reference_is_autograds():
    H, W = 7, 5
    dp = MI.frand(2, 4, 3, 8, seed=1).double()
    y = torch.zeros(2, H, W, 8, dtype=torch.float64, requires_grad=True)
    pooled = torch.nn.functional.avg_pool2d(y.permute(0, 3, 1, 2), 2, 2, ceil_mode=True, count_include_pad=False).permute(0, 2, 3, 1)
    (pooled * dp).sum().backward()
    assert torch.allclose(MI.pool_grad(dp, H, W), y.grad, atol=1e-14)


def test_adamw_reference_is_torchs():
    n = 1001
    p0, g = MI.frand(n, seed=1).double(), MI.frand(n, seed=2).double()
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([q], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    m, v, p = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), p0
    ones = torch.ones(n, dtype=torch.uint8)
    for step in (1, 2, 3):
        q.grad = g.clone()
        opt.step()
        p, m, v, _ = MI.adamw_ema(p, g, m, v, ones, [], [], 1e-3, 0.9, 0.999, 1e-8, 0.05, step, 1.0, 0.0)
    assert torch.allclose(p, q.detach(), rtol=1e-12, atol=1e-14)
