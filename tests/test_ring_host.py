"""ring.PinnedRing without a GPU: the slots come in rotation, a block has the length and dtype asked for, another size makes a new ring,
and DeviceLabelMapCrop.records() keeps to one ring however often it is called at one B (it once pinned, or not, by its first caller)."""
import numpy as np
import pytest
import torch

from autoprog_amd.ring import PinnedRing


def _base(t):
    return t.untyped_storage().data_ptr()


def test_slots_rotate_and_a_block_is_what_was_asked_for():
    ring = PinnedRing("cpu")
    assert ring.pinned is False and PinnedRing("cuda").pinned == torch.cuda.is_available()
    blocks, slots = [], []
    for i in range(2 * ring.SLOTS + 3):
        h = ring.next(24)
        assert h.dtype == torch.int32 and tuple(h.shape) == (24,) and h.is_contiguous() and not h.is_cuda
        assert int(h.numpy().sum()) == (0 if i < ring.SLOTS else 24 * (i - ring.SLOTS))      # a block comes back as it was left
        h.numpy()[:] = i
        blocks.append(h.data_ptr())
        slots.append(ring.slot)
    assert slots == [(i + 1) % ring.SLOTS for i in range(len(slots))]
    assert len(set(blocks[:ring.SLOTS])) == ring.SLOTS                                         # SLOTS different blocks ...
    assert all(blocks[i] == blocks[i - ring.SLOTS] for i in range(ring.SLOTS, len(blocks)))    # ... then the same ones again
    assert all(0 <= p - min(blocks) <= (ring.SLOTS - 1) * 24 * 4 for p in blocks)              # rows of one allocation


def test_another_size_or_dtype_makes_a_new_ring():
    ring = PinnedRing("cpu")
    a = ring.next(16)
    a.numpy()[:] = 7
    b = ring.next(40)
    assert tuple(b.shape) == (40,) and b.dtype == torch.int32 and _base(b) != _base(a) and not b.numpy().any()
    assert int(a[0]) == 7                                            # a block handed out earlier stays its holder's
    c = ring.next(40, torch.float32)
    assert tuple(c.shape) == (40,) and c.dtype == torch.float32 and _base(c) != _base(b)
    assert _base(ring.next(40, torch.float32)) == _base(c)            # the same request again: the same ring


def test_send_without_a_gpu_is_a_plain_copy_into_the_slot_s_own_tensor():
    ring = PinnedRing("cpu")
    with pytest.raises(RuntimeError):                                # nothing drawn yet
        ring.send("cpu")
    ring.record()                                                    # (no copy to mark without a GPU: nothing happens)
    seen = []
    for i in range(ring.SLOTS + 2):
        h = ring.next(8)
        h.numpy()[:] = i
        d = ring.send("cpu")
        assert d.dtype == torch.int32 and d.data_ptr() != h.data_ptr() and d.tolist() == [i] * 8
        seen.append(d.data_ptr())
    assert len(set(seen)) == ring.SLOTS and seen[ring.SLOTS:] == seen[:2]


def test_label_map_records_stay_on_one_ring():
    from autoprog_amd.data import DeviceLabelMapCrop, DeviceRandomResizedCrop
    crop, lm = DeviceRandomResizedCrop(seed=3, device="cpu"), DeviceLabelMapCrop(k=5)
    B, bases, ptrs = 4, set(), []
    for _ in range(2 * lm.SLOTS + 1):
        crop.draw(B, 32, 48)
        h = lm.records(crop, B, 6, 6)
        assert h.dtype == torch.float32 and tuple(h.shape) == (B * 8,)
        assert np.array_equal(h.numpy().reshape(B, 8)[:, :5], np.asarray(lm.last, dtype=np.float32))
        bases.add(_base(h))
        ptrs.append(h.data_ptr())
    assert len(bases) == 1 and len(set(ptrs)) == lm.SLOTS and ptrs[lm.SLOTS:] == ptrs[:lm.SLOTS + 1]
    assert lm._ring.pinned == torch.cuda.is_available()              # decided by the machine, not by which method was called first
