"""What the device paths of the shard writer and reader share and nothing compares: pinned host memory, the 16-byte
alignment of device rows, and device-event timing."""
from __future__ import annotations

from typing import List


def align16(n: int) -> int:
    """n rounded up to a multiple of 16: the CRC kernel loads aligned rows as 16-byte words, so every payload and every
    unpacked row starts at such an offset of its device buffer."""
    return (n + 15) & ~15


class _HostArena:
    """Host memory for the encoded frames of the device path: pinned blocks (a device-to-host copy into pinned memory
    is asynchronous and runs at the link's rate), carved front to back -- torch's pinned allocator rounds every request
    up to a power of two, so the blocks are asked for in such sizes and shared.  Falls back to pageable memory (the
    copies then block) if the host refuses to pin."""

    def __init__(self, block_bytes: int, pin: bool = True):
        self.block_bytes, self.pin = int(block_bytes), bool(pin)
        self._block, self._used = None, 0

    def _empty(self, n: int):
        import torch
        if self.pin:
            try:
                return torch.empty(n, dtype=torch.uint8, pin_memory=True)
            except RuntimeError:
                self.pin = False
        return torch.empty(n, dtype=torch.uint8)

    def take(self, n: int):
        """A uint8 host tensor of n bytes."""
        if n > self.block_bytes:
            return self._empty(n)
        if self._block is None or self._used + n > self.block_bytes:
            self._block, self._used = self._empty(self.block_bytes), 0
        t = self._block[self._used:self._used + n]
        self._used += (n + 63) & ~63
        return t

    def reset(self) -> None:
        """Everything taken so far is free again (the caller knows that no copy still uses it)."""
        self._used = 0


class DeviceTimer:
    """Device events in the order they were stamped, read as (start, end) pairs."""

    def __init__(self):
        self.events: list = []

    def stamp(self) -> None:
        import torch
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.events.append(e)

    def spans_ms(self, stride: int = 2) -> List[float]:
        """The stamps come in groups of `stride`, each group a run of pairs: the total time [ms] of the first pair of
        every group, of the second, ... (stride 2: one total, over every pair).  Synchronises the device."""
        import torch
        torch.cuda.synchronize()
        ev = self.events
        return [float(sum(a.elapsed_time(b) for a, b in zip(ev[j::stride], ev[j + 1::stride]))) for j in range(0, stride, 2)]


class ReadTimer(DeviceTimer):
    """Device events around the reader's unpack and CRC launches (read_episodes_device(timer=...)); tools/bench_shards.py."""

    def __init__(self):
        super().__init__()
        self.packed_bytes = self.unpacked_bytes = self.crc_bytes = 0

    def kernel_ms(self):
        """(unpack ms, CRC ms): the stamps come in fours per shard -- around the unpack call, around the CRC calls."""
        unpack, crc = self.spans_ms(4)
        return unpack, crc
