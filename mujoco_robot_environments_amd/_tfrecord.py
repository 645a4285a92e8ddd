"""CRC-32C (Castagnoli) and TFRecord framing: length, masked CRC of the length, payload, masked CRC of the payload.
``read_records`` reads and checks whole payloads and is the reference for ``scan_records``, which finds them from the
framing alone; neither is built on the other."""
from __future__ import annotations

import os
import struct
from typing import Iterator

import numpy as np

_CRC_TABLE = None
_NATIVE = False
_HEAD, _TAIL = 12, 4     # bytes of framing in front of a payload (length + its CRC) and behind it (the payload's CRC)


def _crc_table():
    global _CRC_TABLE
    if _CRC_TABLE is None:
        t = np.zeros(256, np.uint32)
        for i in range(256):
            c = i
            for _ in range(8):
                c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
            t[i] = c
        _CRC_TABLE = t
    return _CRC_TABLE


def _native_crc():
    """mre_crc32c of the C-ABI library (hardware CRC32 instruction), if the library is built."""
    global _NATIVE
    if _NATIVE is False:
        _NATIVE = None
        try:
            if os.path.exists(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libmre.so")):
                from . import lib as _lib
                fn = _lib.lib().mre_crc32c
                _NATIVE = lambda d: int(fn(bytes(d), len(d)))  # noqa: E731
        except Exception:
            _NATIVE = None
    return _NATIVE


def crc32c(data: bytes) -> int:
    """CRC-32C: the library's routine when it is built (images are megabytes), a byte-wise table otherwise."""
    fast = _native_crc()
    if fast is not None:
        return fast(data)
    t, crc = _crc_table(), 0xFFFFFFFF
    for b in memoryview(data).tobytes():
        crc = int(t[(crc ^ b) & 0xFF]) ^ (crc >> 8)
    return crc ^ 0xFFFFFFFF


def crc32c_combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """CRC-32C of A || B from crc32c(A), crc32c(B) and len(B) (mre_crc32c_combine of the C-ABI library: the record
    CRC of an episode whose image pieces were checksummed elsewhere)."""
    from . import lib as _lib
    return int(_lib.lib().mre_crc32c_combine(int(crc_a) & 0xFFFFFFFF, int(crc_b) & 0xFFFFFFFF, int(len_b)))


def _mask(c: int) -> int:
    return ((((c >> 15) | (c << 17)) & 0xFFFFFFFF) + 0xA282EAD8) & 0xFFFFFFFF


def _masked_crc(data: bytes) -> int:
    return _mask(crc32c(data))


def record_bytes(payload_bytes: int) -> int:
    """What a record of that many payload bytes takes in a TFRecord file."""
    return _HEAD + payload_bytes + _TAIL


def write_record(f, payload: bytes) -> None:
    head = struct.pack("<Q", len(payload))
    f.write(head)
    f.write(struct.pack("<I", _masked_crc(head)))
    f.write(payload)
    f.write(struct.pack("<I", _masked_crc(payload)))


def write_framed(f, pieces, payload_bytes: int, payload_crc: int) -> None:
    """A record from checksummed pieces: `pieces` (buffers) are written one after another as its payload, of
    `payload_bytes` in all and of that CRC-32C (unmasked); no payload byte is read to frame it.  ``write_record`` is
    the reference for it and shares nothing with it."""
    head = struct.pack("<Q", payload_bytes)
    f.write(head)
    f.write(struct.pack("<I", _masked_crc(head)))
    for p in pieces:
        f.write(p)
    f.write(struct.pack("<I", _mask(payload_crc)))


def read_records(path: str) -> Iterator[bytes]:
    with open(path, "rb") as f:
        while True:
            head = f.read(8)
            if len(head) < 8:
                return
            (n,) = struct.unpack("<Q", head)
            (c1,) = struct.unpack("<I", f.read(4))
            if c1 != _masked_crc(head):
                raise ValueError("TFRecord: bad length CRC")
            payload = f.read(n)
            (c2,) = struct.unpack("<I", f.read(4))
            if c2 != _masked_crc(payload):
                raise ValueError("TFRecord: bad payload CRC")
            yield payload


def scan_records(path: str) -> Iterator[tuple]:
    """(payload offset, payload length, stored masked CRC-32C of the payload) of every record of a TFRecord file, from
    its framing alone: the length header is checked against its CRC on the spot, the payload is skipped, not read.
    A file that ends inside a record, or a header that fails its CRC, raises ValueError."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        pos = 0
        while pos < size:
            head = f.read(_HEAD)
            if len(head) < _HEAD:
                raise ValueError(f"{path}: cut short inside the length header of the record at byte {pos}")
            (n,) = struct.unpack("<Q", head[:8])
            (c1,) = struct.unpack("<I", head[8:])
            if c1 != _masked_crc(head[:8]):
                raise ValueError(f"{path}: bad length CRC in the record at byte {pos}")
            if pos + record_bytes(n) > size:
                raise ValueError(f"{path}: cut short inside the record at byte {pos} ({n} payload bytes announced)")
            f.seek(pos + _HEAD + n)
            (c2,) = struct.unpack("<I", f.read(_TAIL))
            yield pos + _HEAD, n, c2
            pos += record_bytes(n)
