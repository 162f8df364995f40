"""A/B of the device batch preparation: (a) the composition a user has to write in torch without ops.input_prep --
`u8.float().sub_(mean).div_(std)`, the erase fill, the flip + blend, then ops.resize_bilinear_s2d16 -- against (b) ops.input_prep, one
launch.  B = 128, 224 -> {224, 192, 160, 128} and B = 64, 448 -> 448, for {plain, erase 0.25 pixel, mixup, cutmix}.

Timing: HIP events around ITERS back-to-back calls after WARM warm-up calls of the same shape; three interleaved repeats of the pair
(a, b, a, b, a, b) per row; the spread column is (max - min) / min over the three.  Bytes are what the ALGORITHM needs, from the shapes:
uint8 in (twice when the partner image is read) + bf16 space-to-depth out; the rate is those bytes over the time of (b), printed as a
fraction of the copy rate ap_calib_copy reaches on the same device in the same process (read + write of a 256 MiB buffer).

    python tools/bench_input_prep.py > profiles/input_prep_ab.txt"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autoprog_amd import ops                                        # noqa: E402
from autoprog_amd.data import DeviceBatchPrep, MIX_CUTMIX, MIX_MIXUP  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
WARM, ITERS, REPEATS = 5, 40, 3


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS * 1e3                          # microseconds per call


def copy_rate():
    n = 256 << 20
    src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    us = min(timed(lambda: ops.calib_copy(src, dst)) for _ in range(3))
    return 2 * n / (us * 1e-6)


def draw_until(prep, B, H, want_mode=None, want_boxes=False):
    """a draw of the wanted kind (the row's label says what it times), from the object's own seeded streams"""
    for _ in range(1000):
        host = prep.draw(B, H, H).clone()
        if (want_mode is None or prep.last["mode"] == want_mode) and (not want_boxes or prep.last["boxes"]):
            return host, dict(prep.last)
    raise RuntimeError("no draw of the wanted kind in 1000")


def composition(u8, mean, std, d, noise, size):
    """what the parent commit leaves to the caller: timm's PrefetchLoader arithmetic, RandomErasing's fill (per-pixel normal noise from
    a buffer drawn up front: the draw itself is not charged), Mixup's flip + blend, then the project's resize kernel"""
    x = u8.float().sub_(mean).div_(std)
    if d["mode"] == MIX_MIXUP:
        flipped = x.flip(0).mul_(1.0 - d["lam"])                          # timm Mixup._mix_batch
        x.mul_(d["lam"]).add_(flipped)
    elif d["mode"] == MIX_CUTMIX:
        yl, yh, xl, xh = d["box"]
        x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
    for b, top, left, h, w in d["boxes"]:
        x[b, :, top:top + h, left:left + w] = noise[:, :h, :w]
    return ops.resize_bilinear_s2d16(x, size)


def main():
    assert torch.cuda.is_available(), "this benchmark measures an MI355X; there is nothing to report without one"
    rate = copy_rate()
    print("device: %s   ap_calib_copy: %.0f GB/s (read + write)" % (torch.cuda.get_device_name(0), rate / 1e9))
    print("times in microseconds per call, HIP events, %d calls after %d warm-up calls, %d interleaved repeats (min; spread = (max-min)/min)" % (ITERS, WARM, REPEATS))
    print("%-4s %-9s %-14s %10s %8s %10s %8s %8s %9s %9s" % ("B", "size", "case", "torch (a)", "spread", "prep (b)", "spread", "a / b", "MB moved", "of copy"))
    mean = torch.tensor([m * 255 for m in MEAN], device="cuda").view(1, 3, 1, 1)
    std = torch.tensor([s * 255 for s in STD], device="cuda").view(1, 3, 1, 1)
    losers = []
    for B, hi, outs in ((128, 224, (224, 192, 160, 128)), (64, 448, (448,))):
        u8 = torch.randint(0, 256, (B, 3, hi, hi), dtype=torch.uint8, device="cuda")
        noise = torch.randn(3, hi, hi, device="cuda")
        for ho in outs:
            for case in ("plain", "erase 0.25", "mixup", "cutmix"):
                kw = dict(re_prob=0.25, re_mode="pixel") if case.startswith("erase") else {}
                if case == "mixup":
                    kw = dict(mixup_alpha=0.8)
                if case == "cutmix":
                    kw = dict(cutmix_alpha=1.0)
                prep = DeviceBatchPrep(MEAN, STD, seed=7, **kw)
                host, d = draw_until(prep, B, hi, {"mixup": MIX_MIXUP, "cutmix": MIX_CUTMIX}.get(case), case.startswith("erase"))
                block = host.cuda()
                table = prep.table()

                def a():
                    return composition(u8, mean, std, d, noise, ho)

                def b():
                    return ops.input_prep(u8, ho, out="s2d16", table=table, params=block, mix=prep.mix_enabled, n_boxes=prep.re_count,
                                          erase_mode=prep.re_mode)
                ta, tb = [], []
                for _ in range(REPEATS):
                    ta.append(timed(a))
                    tb.append(timed(b))
                bytes_ = u8.numel() * (2 if d["mode"] else 1) + B * ho * ho * 4 * 2         # 16 bf16 per 2 x 2 block = 8 bytes per pixel
                frac = bytes_ / (min(tb) * 1e-6) / rate
                print("%-4d %-9s %-14s %10.1f %7.1f%% %10.1f %7.1f%% %8.2f %9.1f %8.1f%%" % (
                    B, "%d->%d" % (hi, ho), case, min(ta), 100 * (max(ta) - min(ta)) / min(ta), min(tb), 100 * (max(tb) - min(tb)) / min(tb),
                    min(ta) / min(tb), bytes_ / 1e6, 100 * frac))
                if not min(ta) > max(tb):
                    losers.append((B, hi, ho, case))
    print("rows where ops.input_prep is not faster than the composition by more than the spread: %s" % (losers or "none"))


if __name__ == "__main__":
    main()
