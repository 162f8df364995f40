"""The ring of pinned host blocks behind every per-step host-to-device record copy (data.py's four stages, graph.StepScalars).

A copy from pinned memory reads its source when it EXECUTES on the GPU, not when it is enqueued, and the host runs many steps ahead of
the GPU: with one block, step t + k's records would overwrite step t's before the copy of step t has run.  So the host writes into
the next of SLOTS blocks, and a block is taken again only after the event recorded behind its last copy: the host runs at most
SLOTS - 1 steps ahead of the copies.  The ring knows nothing of what its users write: a block comes back as it was left."""
import torch


class PinnedRing:
    SLOTS = 8

    def __init__(self, device):
        """device: where the blocks are headed.  They are pinned iff that is a GPU and there is one (the one rule for every user)"""
        self.pinned = torch.device(device).type == "cuda" and torch.cuda.is_available()
        self.slot = 0
        self._n = self._dtype = self._host = None
        self._dev = [None] * self.SLOTS
        self._events = [None] * self.SLOTS

    def next(self, n, dtype=torch.int32):
        """-> the next slot's host block of n words of dtype (a CPU tensor), once the copy that last read that slot has executed.  Another
        n or dtype than the last call's makes a new ring, whose slots go on in rotation from the current one (any slot of a new ring is free)"""
        if n != self._n or dtype is not self._dtype:
            host = torch.zeros(self.SLOTS, n, dtype=dtype)
            self._host = host.pin_memory() if self.pinned else host
            self._dev = [None] * self.SLOTS
            self._events = [None] * self.SLOTS
            self._n, self._dtype = n, dtype
        self.slot = (self.slot + 1) % self.SLOTS
        ev = self._events[self.slot]
        if ev is not None:
            ev.synchronize()
        return self._host[self.slot]

    def record(self):
        """marks the copy just enqueued on the current stream as the reader of the current slot"""
        if self.pinned:
            ev = self._events[self.slot]
            if ev is None:
                ev = self._events[self.slot] = torch.cuda.Event()
            ev.record()

    def send(self, device):
        """enqueues the one copy of the current slot's block (the one next() returned last) to the slot's own tensor on `device` -> that
        tensor"""
        if self._host is None:
            raise RuntimeError("PinnedRing.send() before the first next(): there is no block to send")
        host = self._host[self.slot]
        dev = self._dev[self.slot]
        if dev is None:
            dev = self._dev[self.slot] = torch.empty(self._n, dtype=self._dtype, device=device)
        dev.copy_(host, non_blocking=True)
        self.record()
        return dev
