"""Host side of the device batch preparation (autoprog_amd/data.py): the per-step draws follow timm 0.4.5's Mixup / RandomErasing rules as
data.DeviceBatchPrep's docstring restates them, from the object's own generators; the normalisation table is torch's expression."""
import math
import random

import numpy as np
import pytest
import torch

from autoprog_amd import ops
from autoprog_amd.data import DeviceBatchPrep, MixedLabelTarget, normalisation_table, MIX_CUTMIX, MIX_MIXUP, MIX_NONE

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
P, W8 = ops.PREP_PARAM_WORDS, ops.PREP_BOX_WORDS


def make(**kw):
    return DeviceBatchPrep(MEAN, STD, device="cpu", **kw)


def records(host, B, count):
    return host[P:].reshape(B, count, W8).numpy()


def test_table_is_the_torch_expression_bit_for_bit():
    u8 = torch.arange(256, dtype=torch.uint8).view(1, 1, 1, 256).expand(1, 3, 1, 256)
    mean = torch.tensor([m * 255 for m in MEAN]).view(1, 3, 1, 1)
    std = torch.tensor([s * 255 for s in STD]).view(1, 3, 1, 1)
    want = (u8.float().sub_(mean).div_(std)).reshape(3, 256)            # timm's PrefetchLoader
    t = normalisation_table(MEAN, STD)
    assert t.dtype == torch.float32 and torch.equal(t, want)
    assert torch.equal(make().table_cpu, want)


def test_draw_is_reproducible_and_independent_of_the_global_streams():
    kw = dict(mixup_alpha=0.8, cutmix_alpha=1.0, re_prob=0.5, re_mode="rand", re_count=2, seed=11)
    a, b, c = make(**kw), make(**kw), make(**dict(kw, seed=12))
    random.seed(1); np.random.seed(1); torch.manual_seed(1)
    state = (random.getstate(), np.random.get_state()[1].copy(), torch.get_rng_state().clone())
    seq_a = [a.draw(8, 64, 96).clone() for _ in range(20)]
    assert random.getstate() == state[0] and np.array_equal(np.random.get_state()[1], state[1]) and torch.equal(torch.get_rng_state(), state[2])
    random.seed(99); np.random.seed(99)
    for _ in range(5):
        random.random(); np.random.rand()
    seq_b = [b.draw(8, 64, 96).clone() for _ in range(20)]
    seq_c = [c.draw(8, 64, 96).clone() for _ in range(20)]
    assert all(torch.equal(x, y) for x, y in zip(seq_a, seq_b))
    assert not all(torch.equal(x, y) for x, y in zip(seq_a, seq_c))
    assert [int(x[7]) for x in seq_a] == list(range(20))                # the noise key advances with the step


@pytest.mark.parametrize("H,W,count", [(224, 224, 1), (64, 96, 2), (448, 448, 3), (32, 32, 1)])
def test_erase_boxes_follow_the_rule(H, W, count):
    B, draws, re_prob = 4, 500, 0.37                                       # 2000 images
    prep = make(re_prob=re_prob, re_count=count, seed=H + count)
    s = (H + W) / 2 + 1
    erased = 0
    for _ in range(draws):
        rec = records(prep.draw(B, H, W), B, count)
        for b in range(B):
            n = 0
            for top, left, h, w in rec[b, :, :4]:
                if h == 0:
                    assert w == 0
                    continue
                n += 1
                assert h >= 1 and w >= 1 and top >= 0 and left >= 0 and top + h <= H and left + w <= W and h < H and w < W
                # each of h, w is within 0.5 of its real root and the roots are below H, W: h w is within (H + W) / 2 + 0.25 of the target area
                assert 0.02 * H * W / count - s <= h * w <= H * W / (3 * count) + s
                # the aspect of the unrounded roots lies between these two quotients
                assert (h + 0.5) / (w - 0.5) >= 0.3 and (h - 0.5) / (w + 0.5) <= 1 / 0.3
            assert n in (0, count)                                         # no image whose ten attempts all failed, at these sizes
            erased += n > 0
    n_img = B * draws
    sigma = math.sqrt(re_prob * (1 - re_prob) / n_img)
    assert abs(erased / n_img - re_prob) <= 4 * sigma, (erased / n_img, re_prob)


def test_re_prob_is_a_plain_attribute():
    prep = make(re_prob=0.0, seed=5)
    assert all(not prep.draw(16, 64, 64)[P:].any() for _ in range(20))
    prep.re_prob = 1.0
    rec = records(prep.draw(16, 64, 64), 16, 1)
    assert (rec[:, 0, 2] > 0).all()


def test_mix_draws():
    H, W = 96, 64
    prep = make(mixup_alpha=0.8, cutmix_alpha=1.0, seed=2)
    seen = set()
    for _ in range(2000):
        h = prep.draw(4, H, W)
        mode, lam = int(h[0]), float(h[:16].view(torch.float32)[1])
        yl, yh, xl, xh = (int(v) for v in h[2:6])
        seen.add(mode)
        assert prep.last["lam"] == pytest.approx(lam, rel=1e-6) and float(h[:16].view(torch.float32)[8]) == np.float32(1.0 - prep.last["lam"])
        if mode == MIX_CUTMIX:
            assert 0 <= yl <= yh <= H and 0 <= xl <= xh <= W
            assert prep.last["lam"] == 1.0 - (yh - yl) * (xh - xl) / float(H * W)          # correct_lam, exactly
        elif mode == MIX_MIXUP:
            assert 0.0 <= lam < 1.0 and (yl, yh, xl, xh) == (0, 0, 0, 0)
        else:
            assert lam == 1.0
    assert {MIX_MIXUP, MIX_CUTMIX} <= seen
    only_cut = make(cutmix_alpha=1.0, seed=3)
    assert all(int(only_cut.draw(4, H, W)[0]) in (MIX_CUTMIX, MIX_NONE) for _ in range(200))
    only_mix = make(mixup_alpha=0.4, seed=3)
    assert all(int(only_mix.draw(4, H, W)[0]) in (MIX_MIXUP, MIX_NONE) for _ in range(200))
    never = make(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.0, seed=4)
    for _ in range(500):
        h = never.draw(4, H, W)
        assert int(h[0]) == MIX_NONE and float(h[:16].view(torch.float32)[1]) == 1.0
    off = make(seed=4)
    assert not off.mix_enabled and int(off.draw(4, H, W)[0]) == MIX_NONE


def test_unsupported_modes_raise():
    for mode in ("pair", "elem"):
        with pytest.raises(NotImplementedError):
            make(mixup_alpha=0.8, mode=mode)
    with pytest.raises(ValueError):
        make(re_count=9)
    with pytest.raises(ValueError):
        make(re_mode="noise")


@pytest.mark.parametrize("lam", [1.0, 0.37, 0.0])
def test_mixed_label_target_dense(lam):
    labels = torch.tensor([3, 7, 7, 0, 999])
    t = MixedLabelTarget(labels, lam, smoothing=0.1, num_classes=1000).dense()
    assert t.shape == (5, 1000) and float((t.sum(1) - 1).abs().max()) < 1e-6
    off, on = 0.1 / 1000, 1 - 0.1 + 0.1 / 1000
    one = torch.full((5, 1000), off).scatter_(1, labels.view(-1, 1), on)
    assert torch.allclose(t, lam * one + (1 - lam) * one.flip(0), atol=1e-7)       # timm's mixup_target
    assert float(t[1, 7]) == pytest.approx(lam * on + (1 - lam) * off, abs=1e-6) and float(t[2, 7]) == pytest.approx(on, abs=1e-6)
