"""The protobuf wire format of ``tf.train.Example``, as far as TFDS's example serializer uses it: the encoder, and two
walks over a serialised Example.  ``decode_example`` (on ``_fields``) decodes every value and is the reference for
``locate_example`` (on ``_headers``), which only finds where the values lie; ``_pack_varints`` / ``_unpack_varints`` are
the references for the HIP kernels of records.py.  The two walks share nothing but ``_read_varint``."""
from __future__ import annotations

from typing import Dict

import numpy as np

from ._tfrecord import crc32c


def _varint(n: int) -> bytes:
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _ld_head(field: int, n: int) -> bytes:
    """What a length-delimited field puts in front of a payload of n bytes: its key and the length."""
    return _varint((field << 3) | 2) + _varint(n)


def _ld(field: int, payload: bytes) -> bytes:   # length-delimited field
    return _ld_head(field, len(payload)) + payload


def _pack_varints(a: np.ndarray) -> bytes:
    """Packed varints of non-negative integers < 2^14 (pixel bytes, flags, pixel coordinates): vectorised."""
    a = a.reshape(-1).astype(np.uint16)
    two = a >= 128
    out = np.empty(a.size + int(two.sum()), np.uint8)
    pos = np.arange(a.size) + np.concatenate([[0], np.cumsum(two)[:-1]]) if a.size else np.zeros(0, np.int64)
    out[pos] = np.where(two, (a & 0x7F) | 0x80, a).astype(np.uint8)
    out[pos[two] + 1] = (a[two] >> 7).astype(np.uint8)
    return out.tobytes()


class EncodedLeaf:
    """One step's share of a big feature, already in wire form: ``data`` (any buffer: bytes, numpy uint8 array) are the
    bytes that go INSIDE the feature's packed list -- packed varints for an int64_list, little-endian float32 for a
    float_list -- and ``crc`` is the CRC-32C of exactly those bytes."""
    __slots__ = ("data", "crc", "nbytes")

    def __init__(self, data, crc: int):
        self.data, self.crc = data, int(crc) & 0xFFFFFFFF
        self.nbytes = memoryview(data).nbytes

    @classmethod
    def from_host(cls, array: np.ndarray) -> "EncodedLeaf":
        """The host encoding of one frame (what the device path must reproduce)."""
        a = np.asarray(array)
        data = a.astype("<f4").tobytes() if a.dtype.kind == "f" else _pack_varints(a)
        return cls(data, crc32c(data))


def _feature(value) -> bytes:
    """One tf.train.Feature: bytes_list for a list of bytes, float_list for floating arrays, int64_list otherwise."""
    if isinstance(value, (list, tuple)) and value and isinstance(value[0], (bytes, bytearray)):
        body = b"".join(_ld(1, bytes(v)) for v in value)
        return _ld(1, body)                                   # bytes_list
    a = np.asarray(value)
    if a.dtype.kind == "f":
        return _ld(2, _ld(1, a.astype("<f4").tobytes()))      # float_list, packed
    # fast path (at most two varint bytes per value): uint8 / bool arrays by type, anything else by its value range
    if a.size and (a.dtype in (np.uint8, np.bool_) or (a.min() >= 0 and a.max() < (1 << 14))):
        return _ld(3, _ld(1, _pack_varints(a)))               # int64_list, packed
    packed = b"".join(_varint(int(v) & 0xFFFFFFFFFFFFFFFF) for v in a.reshape(-1))
    return _ld(3, _ld(1, packed))                             # int64_list, packed


def encode_example(features: Dict[str, object]) -> bytes:
    entries = b""
    for k in sorted(features):
        entry = _ld(1, k.encode()) + _ld(2, _feature(features[k]))
        entries += _ld(1, entry)                              # map<string, Feature> entry
    return _ld(1, entries)                                    # Example.features


def _read_varint(b: bytes, i: int):
    n, s = 0, 0
    while True:
        c = b[i]
        i += 1
        n |= (c & 0x7F) << s
        if not c & 0x80:
            return n, i
        s += 7


def _fields(b: bytes):
    i = 0
    while i < len(b):
        key, i = _read_varint(b, i)
        f, wt = key >> 3, key & 7
        if wt == 2:
            n, i = _read_varint(b, i)
            yield f, b[i:i + n]
            i += n
        elif wt == 0:
            v, i = _read_varint(b, i)
            yield f, v
        elif wt == 5:
            yield f, b[i:i + 4]
            i += 4
        else:
            raise ValueError("unsupported wire type")


def _unpack_varints(v: bytes) -> np.ndarray:
    b = np.frombuffer(v, np.uint8)
    if b.size == 0:
        return np.zeros(0, np.int64)
    last = (b & 0x80) == 0                       # final byte of every varint
    if last.all():
        return b.astype(np.int64)
    start = np.concatenate([[0], np.nonzero(last)[0][:-1] + 1])
    length = np.nonzero(last)[0] + 1 - start
    if length.max() <= 2:                        # (values < 2^14: pixel bytes and coordinates)
        lo = (b[start] & 0x7F).astype(np.int64)
        hi = np.where(length == 2, b[np.minimum(start + 1, b.size - 1)].astype(np.int64) << 7, 0)
        return lo + hi
    vals, i = [], 0
    while i < len(v):
        n, i = _read_varint(v, i)
        vals.append(n - (1 << 64) if n >= (1 << 63) else n)
    return np.asarray(vals, np.int64)


def decode_example(payload: bytes) -> Dict[str, object]:
    out = {}
    for f, feats in _fields(payload):
        if f != 1:
            continue
        for f2, entry in _fields(feats):
            key, val = None, None
            for f3, x in _fields(entry):
                if f3 == 1:
                    key = x.decode()
                elif f3 == 2:
                    for f4, lst in _fields(x):
                        if f4 == 1:
                            val = [bytes(v) for _, v in _fields(lst)]
                        elif f4 == 2:
                            val = np.concatenate([np.frombuffer(v, "<f4") for _, v in _fields(lst)] or [np.zeros(0, "<f4")])
                        elif f4 == 3:
                            val = np.concatenate([_unpack_varints(v) for _, v in _fields(lst)] or [np.zeros(0, np.int64)])
            out[key] = val
    return out


_LIST_KINDS = {1: "bytes", 2: "float", 3: "int64"}


def _headers(b, lo: int, hi: int):
    """(field, wire type, start, end) of every field of the message b[lo:hi], from its headers alone: a length-delimited
    field's body is b[start:end]; a varint or fixed32 field is stepped over.  Lengths are held inside [lo, hi)."""
    i = lo
    try:
        while i < hi:
            key, i = _read_varint(b, i)
            f, wt = key >> 3, key & 7
            if wt == 2:
                n, i = _read_varint(b, i)
                if i + n > hi:
                    raise ValueError(f"field {f} at byte {i}: {n} bytes announced, {hi - i} left")
                yield f, wt, i, i + n
                i += n
            elif wt == 0:
                start = i
                _, i = _read_varint(b, i)
                yield f, wt, start, i
            elif wt == 5:
                yield f, wt, i, i + 4
                i += 4
            else:
                raise ValueError("unsupported wire type")
            if i > hi:
                raise ValueError(f"field {f} runs past the end of its message")
    except IndexError:
        raise ValueError("a varint runs past the end of the payload") from None


def locate_example(payload) -> Dict[str, tuple]:
    """Where every feature's data lies in a serialised tf.train.Example: {key: (kind, offset, length)} with kind
    "bytes" / "float" / "int64", and payload[offset : offset + length] the packed data of the list (float: little-endian
    float32; int64: packed varints; bytes: the list's whole body, elements not located).  Framing only: it walks the map
    entries as ``decode_example`` does, on a memoryview and by offsets, and looks at no byte beyond the headers.  It
    accepts less than ``decode_example``: a list given as unpacked elements, or as more than one packed chunk, raises
    ValueError, as does a length that runs past the end or an unsupported wire type."""
    b = memoryview(payload).cast("B")
    out: Dict[str, tuple] = {}
    for f, wt, lo, hi in _headers(b, 0, len(b)):
        if f != 1 or wt != 2:
            continue
        for _, wt2, lo2, hi2 in _headers(b, lo, hi):             # map<string, Feature> entries
            if wt2 != 2:
                raise ValueError("Features: a map entry that is not length-delimited")
            key, where = None, None
            for f3, wt3, lo3, hi3 in _headers(b, lo2, hi2):
                if f3 == 1 and wt3 == 2:
                    key = bytes(b[lo3:hi3]).decode()
                elif f3 == 2 and wt3 == 2:
                    for f4, wt4, lo4, hi4 in _headers(b, lo3, hi3):    # Feature: one of the three lists
                        if wt4 != 2 or f4 not in _LIST_KINDS:
                            raise ValueError(f"Feature: field {f4} with wire type {wt4}")
                        kind = _LIST_KINDS[f4]
                        if kind == "bytes":
                            where = (kind, lo4, hi4 - lo4)
                            continue
                        chunks = list(_headers(b, lo4, hi4))
                        if any(f5 != 1 or wt5 != 2 for f5, wt5, _, _ in chunks):
                            raise ValueError(f"'{key}': {kind}_list with unpacked elements")
                        if len(chunks) > 1:
                            raise ValueError(f"'{key}': {kind}_list in {len(chunks)} packed chunks")
                        where = (kind, chunks[0][2], chunks[0][3] - chunks[0][2]) if chunks else (kind, lo4, 0)
            if key is None or where is None:
                raise ValueError("Features: a map entry without key or value")
            out[key] = where
    return out
