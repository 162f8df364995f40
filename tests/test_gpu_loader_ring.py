"""ring.PinnedRing under the four loader stages of data.py, as tests/test_gpu_graph.py holds it under StepScalars: a stage is called more
often than the ring has slots, every call behind a few milliseconds of device-side sleep and with no synchronisation in between, so the
host has drawn call t + k's records long before the copy of call t's runs.  Every call must still have been launched on its own records:
its output equals a fresh, synchronous launch of the stage's ops.* entry point on the records the stage drew for that call."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, H, W, S = 4, 16, 16, 8
HM = WM = 6
KIN, R, K, C = 2, 32, 2, 50
SLEEP = 6_000_000                        # a few milliseconds of GPU time in front of every call


def _crop_stage(interpolation):
    from autoprog_amd import ops
    from autoprog_amd.data import DeviceRandomResizedCrop
    stage = DeviceRandomResizedCrop(seed=3, interpolation=interpolation)
    u8 = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    entry = ops.crop_resample_u8 if interpolation else ops.crop_resize_u8

    def fresh(last):
        rec = np.zeros((B, ops.CROP_RECORD_WORDS), dtype=np.int32)
        rec[:, :len(last[0])] = last
        rec = torch.from_numpy(rec)
        return (entry(u8, S, rec.cuda(), host_records=rec),)

    return lambda: (stage.crop(u8, S),), lambda: list(stage.last), fresh


def _randaug_stage():
    from autoprog_amd import ops
    from autoprog_amd.data import DeviceRandAugment
    stage = DeviceRandAugment(seed=5)
    u8 = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)).cuda()
    stage(u8)                                                          # (its per-shape buffers; the call below clones the one it returns)

    def fresh(last):
        block = np.zeros(B * stage.n_layers * ops.RANDAUG_RECORD_WORDS, dtype=np.int32)
        DeviceRandAugment.pack(last, block)
        rec = torch.from_numpy(block)
        return (ops.randaug_u8(u8, rec.cuda(), stage.n_layers, stage.fill, host_records=rec),)

    return lambda: (stage(u8).clone(),), lambda: [list(image) for image in stage.last], fresh


def _label_map_stage():
    from autoprog_amd import ops
    from autoprog_amd.data import DeviceLabelMapCrop, DeviceRandomResizedCrop, StoredLabelMaps
    crop, stage = DeviceRandomResizedCrop(seed=7, device="cpu"), DeviceLabelMapCrop(k=K, num_classes=C)
    g = torch.Generator().manual_seed(3)
    scores = torch.rand(B, KIN, HM, WM, generator=g).cuda()
    classes = torch.randint(0, C, (B, KIN, HM, WM), dtype=torch.int32, generator=g).cuda()
    stored = StoredLabelMaps(torch.arange(B), (scores, classes))

    def call():
        crop.draw(B, H, W)                                             # the boxes alone: nothing of the crop runs on the device
        t = stage.target(stored, crop, R)
        return t.idx.clone(), t.val.clone()                            # the stage refills one target in place

    def fresh(last):
        rec = np.zeros((B, ops.LABEL_MAP_BOX_WORDS), dtype=np.float32)
        rec[:, :5] = last
        rec = torch.from_numpy(rec).reshape(-1)
        return ops.label_map_crop(scores, classes, stored.labels, rec.cuda(), R // 16, K, C, host_records=rec)

    return call, lambda: list(stage.last), fresh


STAGES = {"crop": lambda: _crop_stage(None), "antialiased-crop": lambda: _crop_stage("random"), "randaug": _randaug_stage,
          "label-map-crop": _label_map_stage}


@pytest.mark.parametrize("name", list(STAGES))
def test_calls_enqueued_far_ahead_of_the_gpu_keep_their_own_records(name):
    from autoprog_amd.ring import PinnedRing
    call, last, fresh = STAGES[name]()
    torch.cuda.synchronize()
    outs, records = [], []
    for _ in range(2 * PinnedRing.SLOTS + 4):
        torch.cuda._sleep(SLEEP)
        outs.append(call())
        records.append(last())
    torch.cuda.synchronize()
    assert len(set(map(repr, records))) > PinnedRing.SLOTS             # (the calls drew different records: a stale block would show)
    for i, (got, rec) in enumerate(zip(outs, records)):
        want = fresh(rec)
        torch.cuda.synchronize()
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want)), (name, i, rec)
