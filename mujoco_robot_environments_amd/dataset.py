"""RLDS episode shards in TFDS's on-disk format from batched rollouts -- the on-disk side of the reference's data
generation (transporter_network_data_generation.py:56-111: ``tfds.rlds.rlds_base.DatasetConfig`` +
``envlogger.EnvLogger`` with a ``TFDSBackendWriter``), without envlogger / TensorFlow.

What ``TFDSBackendWriter(data_directory, split_name, max_episodes_per_file, ds_config)`` leaves in ``data_directory``,
and what is written here (all restated from the public TFDS / RLDS / TFRecord / protobuf formats; TensorFlow is
absent from this image, so ``tests/test_dataset_tfds.py`` -- ``tfds.builder_from_directory`` on a written
directory -- skips here and runs wherever tensorflow_datasets is importable):

* ``<name>-<split>.tfrecord-XXXXX-of-NNNNN``: TFRecord files (length, masked CRC-32C of the length, payload, masked
  CRC-32C of the payload), ``max_episodes_per_file`` episodes each (config/dataset/default.yaml:3), one
  ``tf.train.Example`` per EPISODE.  Feature keys are the ``/``-joined paths of ``rlds_base.build_info``'s feature
  tree -- ``steps`` is a ``tfds.features.Dataset`` of the step fields, the ``episode_metadata_info`` entries sit at
  the TOP level beside it -- and every leaf is serialised the way TFDS's example serializer does it: a step field
  is ONE flat list over all steps (leading step axis, then the tensor's own shape), integers AND uint8 AND bool go to
  ``int64_list`` (the default ``Encoding.NONE`` of ``tfds.features.Tensor``: one varint per pixel byte), float32 AND
  float64 go to ``float_list`` (the Example proto has no double list):

      steps/observation/overhead_camera/rgb     int64_list   T * H * W * 3
      steps/observation/overhead_camera/depth   float_list   T * H * W
      steps/action/pose                         float_list   T * 7
      steps/action/pixel_coords                 int64_list   T * 2
      steps/action/gripper_rot, steps/reward, steps/discount          float_list   T
      steps/is_first, steps/is_last, steps/is_terminal                int64_list   T
      intrinsics/{fx,fy,cx,cy}, extrinsics/{x,y,z,qx,qy,qz,qw}        float_list   1   (calibration_metadata, :88-95)

* ``features.json``: the feature tree as TFDS serialises it (proto3 JSON of ``feature.proto``: ``pythonClassName`` +
  one of ``featuresDict`` / ``sequence`` / ``tensor``; int64 fields as strings).
* ``dataset_info.json``: proto3 JSON of ``DatasetInfo`` (name, version 0.0.1 -- TFDSBackendWriter's default --,
  ``fileFormat``, one split with ``shardLengths`` / ``numBytes`` as strings and the standard ``filepathTemplate``).

Where the per-byte work runs: ``BatchedEpisodeLogger`` looks at the observations it is handed.  CUDA tensors (env
``render=True``) are encoded on the device -- the varints of the rgb frames and the CRC-32C of both images come from
``records.py`` / csrc/mre_records.hip, and ``EpisodeWriter.write_encoded_episode`` frames the finished pieces without
reading them again (the record's CRC is combined from the pieces' CRCs).  numpy observations take the host path below
(``write_episode``), which is also what the device path is tested against, byte for byte.

``read_episodes`` parses a directory back BY ITS features.json (it is a generic reader of this format, not a mirror
of the writer), and tests/test_dataset.py round-trips through it.  ``read_episodes_device`` is the same reader with
the image leaves decoded on the device (``scan_records`` + ``locate_example`` find the bytes on the host from the
framing alone; ``records.varint_unpack_rows`` / ``crc32c_rows`` do the per-byte work), held to ``read_episodes`` leaf
for leaf in tests/test_gpu_record_reader.py.
"""
from __future__ import annotations

import json
import os
import struct
from typing import Dict, Iterator, List, Optional

import numpy as np

# ------------------------------------------------------------------ CRC-32C (Castagnoli), TFRecord mask
_CRC_TABLE = None


def _crc_table():
    global _CRC_TABLE
    if _CRC_TABLE is None:
        t = np.zeros((8, 256), np.uint32)
        for i in range(256):
            c = i
            for _ in range(8):
                c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
            t[0, i] = c
        for k in range(1, 8):
            t[k] = (t[k - 1] >> np.uint32(8)) ^ t[0, t[k - 1] & np.uint32(0xFF)]
        _CRC_TABLE = t
    return _CRC_TABLE


def crc32c(data: bytes) -> int:
    """CRC-32C, slicing-by-8 over numpy words for the bulk (images are megabytes)."""
    t = _crc_table()
    crc = 0xFFFFFFFF
    n = len(data)
    mv = memoryview(data)
    # bulk: process 8 bytes per step in Python is still slow for MBs; use a vectorised fold over
    # independent 4 KiB blocks is not possible for a CRC without combine -- so fall back to the C
    # helper of libmre.so when it is there
    fast = _native_crc()
    if fast is not None:
        return fast(data)
    t0 = t[0]
    for b in mv.tobytes():
        crc = int(t0[(crc ^ b) & 0xFF]) ^ (crc >> 8)
    return crc ^ 0xFFFFFFFF


_NATIVE = False


def _native_crc():
    """mre_crc32c of the C-ABI library (hardware CRC32 instruction), if the library is built."""
    global _NATIVE
    if _NATIVE is False:
        _NATIVE = None
        try:
            import ctypes as C
            so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libmre.so")
            if os.path.exists(so):
                from . import lib as _lib
                L = _lib.lib()
                L.mre_crc32c.restype = C.c_uint32
                L.mre_crc32c.argtypes = [C.c_char_p, C.c_size_t]
                _NATIVE = lambda d: int(L.mre_crc32c(bytes(d), len(d)))  # noqa: E731
        except Exception:
            _NATIVE = None
    return _NATIVE


def _mask(c: int) -> int:
    return ((((c >> 15) | (c << 17)) & 0xFFFFFFFF) + 0xA282EAD8) & 0xFFFFFFFF


def _masked_crc(data: bytes) -> int:
    return _mask(crc32c(data))


def write_record(f, payload: bytes) -> None:
    head = struct.pack("<Q", len(payload))
    f.write(head)
    f.write(struct.pack("<I", _masked_crc(head)))
    f.write(payload)
    f.write(struct.pack("<I", _masked_crc(payload)))


def crc32c_combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """CRC-32C of A || B from crc32c(A), crc32c(B) and len(B) (mre_crc32c_combine of the C-ABI library: the record
    CRC of an episode whose image pieces were checksummed elsewhere)."""
    from . import lib as _lib
    return int(_lib.lib().mre_crc32c_combine(int(crc_a) & 0xFFFFFFFF, int(crc_b) & 0xFFFFFFFF, int(len_b)))


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
            head = f.read(12)
            if len(head) < 12:
                raise ValueError(f"{path}: cut short inside the length header of the record at byte {pos}")
            (n,) = struct.unpack("<Q", head[:8])
            (c1,) = struct.unpack("<I", head[8:])
            if c1 != _masked_crc(head[:8]):
                raise ValueError(f"{path}: bad length CRC in the record at byte {pos}")
            if pos + 12 + n + 4 > size:
                raise ValueError(f"{path}: cut short inside the record at byte {pos} ({n} payload bytes announced)")
            f.seek(pos + 12 + n)
            (c2,) = struct.unpack("<I", f.read(4))
            yield pos + 12, n, c2
            pos += 12 + n + 4


# ------------------------------------------------------------------ tf.train.Example wire format
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


def _ld(field: int, payload: bytes) -> bytes:   # length-delimited field
    return _varint((field << 3) | 2) + _varint(len(payload)) + payload


def _pack_varints(a: np.ndarray) -> bytes:
    """Packed varints of non-negative integers < 2^14 (pixel bytes, flags, pixel coordinates): vectorised."""
    a = a.reshape(-1).astype(np.uint16)
    two = a >= 128
    out = np.empty(a.size + int(two.sum()), np.uint8)
    pos = np.arange(a.size) + np.concatenate([[0], np.cumsum(two)[:-1]]) if a.size else np.zeros(0, np.int64)
    out[pos] = np.where(two, (a & 0x7F) | 0x80, a).astype(np.uint8)
    out[pos[two] + 1] = (a[two] >> 7).astype(np.uint8)
    return out.tobytes()


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


# ------------------------------------------------------------------ TFDS metadata
_FEATURES_PKG = "tensorflow_datasets.core.features."


def _tensor_feature(shape, dtype: str) -> dict:
    """features.json node of tfds.features.Tensor(shape, dtype) / tfds.features.Scalar(dtype) (shape ())."""
    cls = "scalar.Scalar" if len(shape) == 0 else "tensor_feature.Tensor"
    sh = {"dimensions": [str(int(d)) for d in shape]} if len(shape) else {}
    return {"pythonClassName": _FEATURES_PKG + cls, "tensor": {"shape": sh, "dtype": dtype, "encoding": "none"}}


def _dict_feature(children: dict) -> dict:
    return {"pythonClassName": _FEATURES_PKG + "features_dict.FeaturesDict", "featuresDict": {"features": children}}


def rlds_features(height: int, width: int) -> dict:
    """features.json of ``rlds_base.build_info(ds_config)`` for the reference's ds_config
    (transporter_network_data_generation.py:56-86): FeaturesDict{steps: Dataset(FeaturesDict{observation, action,
    reward, discount, is_first, is_last, is_terminal}), **episode_metadata_info}."""
    h, w = int(height), int(width)
    step = _dict_feature({
        "observation": _dict_feature({"overhead_camera/rgb": _tensor_feature((h, w, 3), "uint8"),
                                      "overhead_camera/depth": _tensor_feature((h, w), "float32")}),
        "action": _dict_feature({"pose": _tensor_feature((7,), "float64"),
                                 "pixel_coords": _tensor_feature((2,), "int32"),
                                 "gripper_rot": _tensor_feature((), "float64")}),
        "reward": _tensor_feature((), "float64"), "discount": _tensor_feature((), "float64"),
        "is_first": _tensor_feature((), "bool"), "is_last": _tensor_feature((), "bool"),
        "is_terminal": _tensor_feature((), "bool")})
    return _dict_feature({
        "steps": {"pythonClassName": _FEATURES_PKG + "dataset_feature.Dataset",
                  "sequence": {"feature": step, "length": "-1"}},
        "intrinsics": _dict_feature({k: _tensor_feature((), "float64") for k in ("fx", "fy", "cx", "cy")}),
        "extrinsics": _dict_feature({k: _tensor_feature((), "float64") for k in ("x", "y", "z", "qx", "qy", "qz", "qw")})})


def feature_leaves(node: dict, prefix: str = "", in_sequence: bool = False):
    """(example key, shape tuple, dtype, inside a Dataset / Sequence) of every tensor leaf of a features.json tree."""
    if "featuresDict" in node:
        for k, v in node["featuresDict"]["features"].items():
            yield from feature_leaves(v, f"{prefix}/{k}" if prefix else k, in_sequence)
    elif "sequence" in node:
        yield from feature_leaves(node["sequence"]["feature"], prefix, True)
    elif "tensor" in node:
        dims = node["tensor"].get("shape", {}).get("dimensions", [])
        yield prefix, tuple(int(d) for d in dims), node["tensor"]["dtype"], in_sequence
    else:
        raise ValueError(f"features.json: unsupported feature at '{prefix}': {sorted(node)}")


# ------------------------------------------------------------------ the writer
class EpisodeWriter:
    """Shard writer mirroring ``TFDSBackendWriter(data_directory, split_name, max_episodes_per_file,
    ds_config)`` (transporter_network_data_generation.py:103-111)."""

    VERSION = "0.0.1"   # TFDSBackendWriter's default `version`

    def __init__(self, data_directory: str, name: str, height: int, width: int, split_name: str = "train",
                 max_episodes_per_file: int = 10):
        self.dir, self.name, self.split = data_directory, name, split_name
        self.h, self.w = int(height), int(width)
        self.max_per_file = int(max_episodes_per_file)
        os.makedirs(self.dir, exist_ok=True)
        self._shards: List[int] = []
        self._file = None
        self._in_file = 0
        self._episodes = 0
        self._bytes = 0

    def features(self) -> dict:
        return rlds_features(self.h, self.w)

    def _tmp_path(self, k: int) -> str:
        return os.path.join(self.dir, f"{self.name}-{self.split}.tfrecord-{k:05d}.tmp")

    def _roll(self):
        if self._file is not None:
            self._file.close()
            self._shards.append(self._in_file)
        self._file = open(self._tmp_path(len(self._shards)), "wb")
        self._in_file = 0

    RGB_KEY = "steps/observation/overhead_camera/rgb"
    DEPTH_KEY = "steps/observation/overhead_camera/depth"

    @staticmethod
    def _small_features(steps: List[dict], metadata: dict) -> dict:
        """Every feature of an episode but the two images."""
        T = len(steps)
        zero_act = {"pose": np.zeros(7), "pixel_coords": np.zeros(2, np.int64), "gripper_rot": 0.0}
        acts = [s.get("action") or zero_act for s in steps]
        feats = {
            "steps/action/pose": np.concatenate([np.asarray(a["pose"], np.float64).reshape(7) for a in acts]),
            "steps/action/pixel_coords": np.concatenate([np.asarray(a["pixel_coords"], np.int64).reshape(2) for a in acts]),
            "steps/action/gripper_rot": np.asarray([float(a["gripper_rot"]) for a in acts]),
            "steps/reward": np.asarray([float(s.get("reward", 0.0)) for s in steps]),
            "steps/discount": np.asarray([float(s.get("discount", 0.0)) for s in steps]),
            "steps/is_first": np.asarray([int(bool(s.get("is_first", k == 0))) for k, s in enumerate(steps)], np.int64),
            "steps/is_last": np.asarray([int(bool(s.get("is_last", k == T - 1))) for k, s in enumerate(steps)], np.int64),
            "steps/is_terminal": np.asarray([int(bool(s.get("is_terminal", False))) for s in steps], np.int64),
        }
        for grp in ("intrinsics", "extrinsics"):       # episode_metadata_info entries: top-level features
            for k, v in metadata[grp].items():
                feats[f"{grp}/{k}"] = np.asarray([float(v)])
        return feats

    def write_episode(self, steps: List[dict], metadata: dict) -> None:
        """steps: RLDS steps, each {"observation": {...}, "action": {...} or None (last step), "reward",
        "discount", "is_first", "is_last", "is_terminal"}."""
        if self._file is None or self._in_file >= self.max_per_file:
            self._roll()
        rgb, depth = [], []
        for s in steps:
            o = s["observation"]
            r = np.asarray(o["overhead_camera/rgb"], np.uint8)
            d = np.asarray(o["overhead_camera/depth"], np.float32)
            assert r.shape == (self.h, self.w, 3) and d.shape == (self.h, self.w), (r.shape, d.shape)
            rgb.append(r.reshape(-1))
            depth.append(d.reshape(-1))
        feats = self._small_features(steps, metadata)
        feats[self.RGB_KEY] = np.concatenate(rgb) if rgb else np.zeros(0, np.uint8)
        feats[self.DEPTH_KEY] = np.concatenate(depth) if depth else np.zeros(0, np.float32)
        payload = encode_example(feats)
        write_record(self._file, payload)
        self._bytes += len(payload)
        self._in_file += 1
        self._episodes += 1

    def write_encoded_episode(self, steps: List[dict], metadata: dict) -> None:
        """``write_episode`` for steps whose two images are ``EncodedLeaf`` pieces (observation: {"overhead_camera/rgb":
        packed varints of the frame, "overhead_camera/depth": its float32 bytes}), and the same bytes in the file.  The
        small features are encoded here as usual; the Example's framing around the images is built from the pieces'
        LENGTHS, the record's CRC from their CRCs (``crc32c_combine``), and the pieces go to the file one after
        another -- no megabyte is read or copied on the way."""
        if self._file is None or self._in_file >= self.max_per_file:
            self._roll()
        small = self._small_features(steps, metadata)
        big = {self.RGB_KEY: (3, [s["observation"]["overhead_camera/rgb"] for s in steps]),      # int64_list
               self.DEPTH_KEY: (2, [s["observation"]["overhead_camera/depth"] for s in steps])}  # float_list
        assert all(p.nbytes == 4 * self.h * self.w for p in big[self.DEPTH_KEY][1]), "depth piece: H * W float32"

        def head(field: int, n: int) -> bytes:    # what _ld(field, payload of n bytes) puts in front of the payload
            return _varint((field << 3) | 2) + _varint(n)

        # the map entries in key order, as encode_example lays them out; parts = [bytes | EncodedLeaf]
        parts: list = []
        for k in sorted(list(small) + list(big)):
            key = _ld(1, k.encode())
            if k in small:
                parts.append(_ld(1, key + _ld(2, _feature(small[k]))))
                continue
            kind, pieces = big[k]
            n = sum(p.nbytes for p in pieces)
            h_list = head(1, n)                          # <kind>_list.value, packed
            h_kind = head(kind, len(h_list) + n)         # Feature.<kind>_list
            h_feat = head(2, len(h_kind) + len(h_list) + n)      # map entry: value
            n_entry = len(key) + len(h_feat) + len(h_kind) + len(h_list) + n
            parts.append(head(1, n_entry) + key + h_feat + h_kind + h_list)
            parts.extend(pieces)
        total = sum(len(p) if isinstance(p, bytes) else p.nbytes for p in parts)
        parts.insert(0, head(1, total))                  # Example.features
        merged: list = []                                # neighbouring small parts as one
        for p in parts:
            if isinstance(p, bytes) and merged and isinstance(merged[-1], bytes):
                merged[-1] += p
            else:
                merged.append(p)
        n_payload, crc = 0, 0
        for p in merged:
            c, n = (crc32c(p), len(p)) if isinstance(p, bytes) else (p.crc, p.nbytes)
            crc = crc32c_combine(crc, c, n)
            n_payload += n
        f = self._file
        lead = struct.pack("<Q", n_payload)
        f.write(lead)
        f.write(struct.pack("<I", _masked_crc(lead)))
        for p in merged:
            f.write(p if isinstance(p, bytes) else p.data)
        f.write(struct.pack("<I", _mask(crc)))
        self._bytes += n_payload
        self._in_file += 1
        self._episodes += 1

    def dataset_info(self) -> dict:
        """dataset_info.json: proto3 JSON of tfds' DatasetInfo message (int64 fields are strings)."""
        return {"name": self.name, "version": self.VERSION, "fileFormat": "tfrecord", "moduleName": "",
                "description": "RLDS episodes of RearrangementEnv (overhead camera, scripted pick / place actions)",
                "splits": [{"name": self.split, "shardLengths": [str(n) for n in self._shards],
                            "numBytes": str(self._bytes),
                            "filepathTemplate": "{DATASET}-{SPLIT}.{FILEFORMAT}-{SHARD_X_OF_Y}"}]}

    def close(self) -> dict:
        if self._file is not None:
            self._file.close()
            self._shards.append(self._in_file)
            self._file = None
        n = len(self._shards)
        for k in range(n):
            os.replace(self._tmp_path(k), os.path.join(self.dir, f"{self.name}-{self.split}.tfrecord-{k:05d}-of-{n:05d}"))
        info = self.dataset_info()
        with open(os.path.join(self.dir, "dataset_info.json"), "w") as f:
            json.dump(info, f, indent=2)
        with open(os.path.join(self.dir, "features.json"), "w") as f:
            json.dump(self.features(), f, indent=4)
        return info


_NP_DTYPE = {"uint8": np.uint8, "int32": np.int32, "int64": np.int64, "bool": np.bool_, "float32": np.float32,
             "float64": np.float64}


def _nest(tree: dict, key: str, leaf_names, value):
    """Put `value` at the path of `key` in a nested dict; `leaf_names` are the feature names on the way (a name may
    contain '/' itself, e.g. overhead_camera/rgb)."""
    node = tree
    for name in leaf_names[:-1]:
        node = node.setdefault(name, {})
    node[leaf_names[-1]] = value


def _leaf_paths(node: dict, path=()):
    if "featuresDict" in node:
        for k, v in node["featuresDict"]["features"].items():
            yield from _leaf_paths(v, path + (k,))
    elif "sequence" in node:
        yield from _leaf_paths(node["sequence"]["feature"], path)
    else:
        yield path


def read_episodes(data_directory: str, name: Optional[str] = None, split_name: str = "train") -> Iterator[dict]:
    """Generic reader of a TFDS directory of this kind: dataset_info.json names the dataset, its split and shard
    count, features.json says how every Example key is typed and shaped.  Yields nested dicts shaped like the
    feature tree ({"steps": {...arrays with a leading step axis...}, "intrinsics": {...}, "extrinsics": {...}})."""
    with open(os.path.join(data_directory, "features.json")) as f:
        feat = json.load(f)
    with open(os.path.join(data_directory, "dataset_info.json")) as f:
        info = json.load(f)
    name = name or info["name"]
    split = next(sp for sp in info["splits"] if sp["name"] == split_name)
    n = len(split["shardLengths"])
    leaves = list(feature_leaves(feat))
    paths = list(_leaf_paths(feat))
    for k in range(n):
        p = os.path.join(data_directory, f"{name}-{split_name}.{info['fileFormat']}-{k:05d}-of-{n:05d}")
        count = 0
        for rec in read_records(p):
            e = decode_example(rec)
            out: dict = {}
            for (key, shape, dtype, seq), path in zip(leaves, paths):
                v = np.asarray(e[key])
                v = v.reshape((-1,) + shape) if seq else v.reshape(shape)
                _nest(out, key, path, v.astype(_NP_DTYPE[dtype]))
            count += 1
            yield out
        if count != int(split["shardLengths"][k]):
            raise ValueError(f"{p}: {count} records, dataset_info.json says {split['shardLengths'][k]}")


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


def _is_image_leaf(shape, dtype: str, seq: bool) -> bool:
    return seq and len(shape) >= 2 and dtype in ("uint8", "float32")


class ReadTimer:
    """Device events around the reader's unpack and CRC launches (read_episodes_device(timer=...)); tools/bench_shards.py."""

    def __init__(self):
        self.events: list = []
        self.packed_bytes = self.unpacked_bytes = self.crc_bytes = 0

    def stamp(self) -> None:
        import torch
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.events.append(e)

    def kernel_ms(self):
        """(unpack ms, CRC ms): the stamps come in fours per shard -- around the unpack call, around the CRC calls."""
        import torch
        torch.cuda.synchronize()
        ev = self.events
        return (float(sum(a.elapsed_time(b) for a, b in zip(ev[0::4], ev[1::4]))),
                float(sum(a.elapsed_time(b) for a, b in zip(ev[2::4], ev[3::4]))))


def read_episodes_device(data_directory: str, name: Optional[str] = None, split_name: str = "train", device=None,
                         verify: bool = True, timer: Optional[ReadTimer] = None) -> Iterator[dict]:
    """``read_episodes`` with the image leaves decoded on the device: the same tree, dtypes and shapes, where a tensor
    leaf of rank >= 2 inside the step sequence with dtype uint8 or float32 is a CUDA tensor (uint8 [T, H, W, 3],
    float32 [T, H, W]) and everything else is numpy, decoded on the host from its located bytes.  Driven by
    features.json like ``read_episodes``; the HIP path has no host fallback (no GPU, no reader).

    Per shard: ``scan_records`` finds the records from the framing; the file goes to the device once through pinned
    memory, each payload to a 16-byte aligned offset (the CRC kernel loads aligned rows as 16-byte words);
    ``locate_example`` finds every feature's bytes; ALL uint8 image lists of the shard are unpacked by one
    ``records.varint_unpack_rows`` call; a float32 image is the payload's bytes as they are (a byte-slice copy, then a
    view: its offset in the payload is not a multiple of 4).  verify=True: the CRC-32C of every payload is computed on
    the device (``records.crc32c_rows``) and compared with the stored one.  One synchronise per shard, for the statuses
    and the CRCs.  A CRC mismatch, a non-zero unpack status or a record count other than dataset_info.json's raises
    ValueError naming the file, the record and the key; the shard's records before the bad one are yielded, none after.
    ``timer`` (a ReadTimer) puts device events around the unpack and the CRC launches and counts their bytes."""
    import torch
    from . import records as R
    with open(os.path.join(data_directory, "features.json")) as f:
        feat = json.load(f)
    with open(os.path.join(data_directory, "dataset_info.json")) as f:
        info = json.load(f)
    name = name or info["name"]
    split = next(sp for sp in info["splits"] if sp["name"] == split_name)
    n = len(split["shardLengths"])
    leaves = list(feature_leaves(feat))
    paths = list(_leaf_paths(feat))
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    arena = None
    for k in range(n):
        p = os.path.join(data_directory, f"{name}-{split_name}.{info['fileFormat']}-{k:05d}-of-{n:05d}")
        recs = list(scan_records(p))
        if len(recs) != int(split["shardLengths"][k]):
            raise ValueError(f"{p}: {len(recs)} records, dataset_info.json says {split['shardLengths'][k]}")
        if not recs:
            continue
        size = os.path.getsize(p)
        if arena is None or arena.block_bytes < size:
            arena = _HostArena(1 << max(size - 1, 1).bit_length())
        arena.reset()                                      # the previous shard's copies ended with its synchronise
        h_file = arena.take(size)
        with open(p, "rb") as f:
            if f.readinto(h_file.numpy()) != size:
                raise ValueError(f"{p}: changed while it was read")
        host = memoryview(h_file.numpy())
        base, total = [], 0                                # payload r lies at d_file[base[r] : base[r] + length]
        for _, length, _ in recs:
            base.append(total)
            total += (length + 15) & ~15
        with torch.cuda.device(dev):
            d_file = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
            for (off, length, _), b in zip(recs, base):
                if length:
                    d_file[b:b + length].copy_(h_file[off:off + length], non_blocking=True)
            # the host's share: framing, the small leaves, the rows of the one unpack call
            episodes, rows, row_of = [], [], []            # rows: (src_off, src_len, nvalues, out_off)
            n_out = 0
            for r, ((off, length, _), b) in enumerate(zip(recs, base)):
                pay = host[off:off + length]
                try:
                    where = locate_example(pay)
                    small, T = {}, None
                    for key, shape, dtype, seq in leaves:
                        kind, o, ln = where[key]
                        per = int(np.prod(shape, dtype=np.int64))
                        if _is_image_leaf(shape, dtype, seq) and kind == ("int64" if dtype == "uint8" else "float"):
                            if dtype == "float32":
                                if ln % (4 * per):
                                    raise ValueError(f"'{key}': {ln} bytes are no whole number of float32 {shape} frames")
                                T = ln // (4 * per) if T is None else T
                            continue
                        v = (_unpack_varints(pay[o:o + ln]) if kind == "int64" else
                             np.frombuffer(pay[o:o + ln], "<f4") if kind == "float" else None)
                        if v is None:
                            raise ValueError(f"'{key}': a bytes list where features.json has a {dtype} tensor")
                        small[key] = v
                        if seq and T is None:
                            T = v.size // per
                    if T is None:      # uint8 image leaves only: a value ends at every byte with the high bit clear
                        key, shape = next((ky, sh) for ky, sh, dt, sq in leaves if sq)
                        _, o, ln = where[key]
                        T = int(np.count_nonzero(np.frombuffer(pay[o:o + ln], np.uint8) < 0x80)) // int(np.prod(shape))
                except (ValueError, KeyError) as e:
                    raise ValueError(f"{p}: record {r}: {e}") from None
                image = {}
                for key, shape, dtype, seq in leaves:
                    if key in small:
                        continue
                    _, o, ln = where[key]
                    if dtype == "uint8":
                        nv = T * int(np.prod(shape, dtype=np.int64))
                        rows.append((b + o, ln, nv, n_out))
                        row_of.append((r, key))
                        image[key] = (n_out, nv)
                        n_out += (nv + 15) & ~15
                    else:
                        if ln != 4 * T * int(np.prod(shape, dtype=np.int64)):
                            raise ValueError(f"{p}: record {r}: '{key}': {ln} bytes for {T} steps of float32 {shape}")
                        image[key] = d_file[b + o:b + o + ln].clone().view(torch.float32)
                episodes.append((small, image, T))
            status = None
            if timer is not None:
                timer.stamp()
            if rows:
                desc = np.asarray(rows, np.int64).T
                d_out = torch.empty(max(n_out, 1), dtype=torch.uint8, device=dev)
                _, status = R.varint_unpack_rows(d_file, desc[0], desc[1], desc[2], desc[3], out=d_out)
            if timer is not None:
                timer.stamp()
                timer.stamp()
                timer.packed_bytes += int(sum(x[1] for x in rows))
                timer.unpacked_bytes += int(sum(x[2] for x in rows))
            crcs = None
            if verify:
                crcs = torch.cat([R.crc32c_rows(d_file[b:b + length].view(1, -1)) if length else
                                  torch.zeros(1, dtype=torch.int32, device=dev) for (_, length, _), b in zip(recs, base)])
                if timer is not None:
                    timer.crc_bytes += int(sum(length for _, length, _ in recs))
            if timer is not None:
                timer.stamp()
            parts = [t for t in (status, crcs) if t is not None]
            back = torch.cat(parts).cpu().numpy() if parts else np.zeros(0, np.int32)   # the shard's one synchronise
        status_h = back[:len(rows)] if status is not None else np.zeros(0, np.int32)
        crc_h = back[len(status_h):].view(np.uint32)
        bad = {}                                           # record -> message, the first per record
        for (r, key), st in zip(row_of, status_h):
            if st and r not in bad:
                bad[r] = f"'{key}': malformed packed varints (unpack status {int(st):#x})"
        if verify:
            for r, (_, _, stored) in enumerate(recs):
                if _mask(int(crc_h[r])) != stored:
                    bad[r] = "bad payload CRC (computed on the device; it covers every key of the record)"
        for r, (small, image, T) in enumerate(episodes):
            if r in bad:
                raise ValueError(f"{p}: record {r}: {bad[r]}")
            out: dict = {}
            for (key, shape, dtype, seq), path in zip(leaves, paths):
                if key in small:
                    v = small[key]
                    v = v.reshape((-1,) + shape) if seq else v.reshape(shape)
                    v = v.astype(_NP_DTYPE[dtype])
                elif dtype == "uint8":
                    o, nv = image[key]
                    v = d_out[o:o + nv].view((T,) + shape)
                else:
                    v = image[key].view((T,) + shape)
                _nest(out, key, path, v)
            yield out


class BatchedEpisodeLogger:
    """The EnvLogger of the batched env: collects (observation, action) of every env step by step and
    writes one episode per env -- ``with BatchedEpisodeLogger(env, writer) as log: log.reset(ts);
    log.step(action, ts)``.  Observations may be CUDA tensors (env render=True) or numpy arrays, and that decides
    where the frames are encoded; the files are the same.

    CUDA observations: the logged, active rows are encoded on the device (records.py: varints + CRC-32C of the rgb
    frames, CRC-32C of the depth frames) in chunks of envs that keep the device staging at ``staging_bytes`` whatever
    N x T is, and come back as a few large asynchronous copies -- one synchronise per logged step (for the packed
    lengths; it also retires the previous step's copies), none per env.  ``frames_encoded_on_device`` counts them.
    numpy observations: copied as they are and encoded by ``EpisodeWriter.write_episode`` on the host.

    Either way the HOST holds every logged frame until ``flush()`` -- packed on the device path (1 .. 2 bytes per rgb
    byte + 4 per depth pixel), raw on the host path -- because episodes are written in env order, which keeps the shards
    comparable byte for byte.  Writing finished episodes early would bound that memory, and reorder the records."""

    def __init__(self, env, writer: EpisodeWriter, env_mask: Optional[np.ndarray] = None,
                 staging_bytes: int = 1 << 30, pin_host: bool = True, time_kernels: bool = False):
        self.env, self.writer = env, writer
        self.mask = np.ones(env.num_envs, bool) if env_mask is None else np.asarray(env_mask, bool)
        self._steps: List[List[dict]] = [[] for _ in range(env.num_envs)]
        self._meta = None
        self.frames_encoded_on_device = 0
        self.staging_bytes = int(staging_bytes)
        self._arena = _HostArena(self.staging_bytes, pin_host)
        self._staging = None      # device uint8 [staging_bytes], reused by every chunk of every step
        self._in_flight: list = []   # device tensors that enqueued work still reads; dropped at the next synchronise
        self._lazy: list = []     # (EncodedLeaf list, host int32 tensor of their CRCs): filled in once the copy landed
        self._events = [] if time_kernels else None   # device events, in (start, end) pairs around the encode kernels

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.flush()

    @staticmethod
    def _np(x):
        return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)

    def _obs(self, ts, i):
        o = ts.observation
        return {"overhead_camera/rgb": self._np(o["overhead_camera/rgb"][i]),
                "overhead_camera/depth": self._np(o["overhead_camera/depth"][i])}

    # ---------------------------------------------------------------- device path
    @staticmethod
    def _on_device(ts) -> bool:
        return bool(getattr(ts.observation["overhead_camera/rgb"], "is_cuda", False))

    def _settle(self) -> None:
        """After a synchronise: everything enqueued before it has landed."""
        for leaves, crcs in self._lazy:
            for leaf, c in zip(leaves, crcs.numpy().view(np.uint32)):
                leaf.crc = int(c)
        self._lazy, self._in_flight = [], []

    def _encode_on_device(self, ts, rows: np.ndarray) -> List[dict]:
        """Observations (EncodedLeaf pairs) of env rows[k] for every k.  The leaves' bytes and CRCs are valid after the
        next synchronise of the stream (the next logged step's, or flush's)."""
        import torch
        from . import records as R
        rgb, depth = ts.observation["overhead_camera/rgb"], ts.observation["overhead_camera/depth"]
        n_src = int(rgb.shape[0])
        rgb, depth = rgb.reshape(n_src, -1), depth.reshape(n_src, -1)
        assert rgb.dtype == torch.uint8 and depth.dtype == torch.float32, (rgb.dtype, depth.dtype)
        rb, db = int(rgb.shape[1]), 4 * int(depth.shape[1])
        dev = rgb.device
        with torch.cuda.device(dev):
            idx = R.row_index(rows, n_src, dev)
            self._stamp()
            _, sizes = R.varint_size_rows(rgb, idx)
            self._stamp()
            sizes_h = sizes.cpu().numpy().astype(np.int64)    # the step's one synchronise
            self._settle()
            whole = rows.size == n_src                         # every env, in order: depth rows leave from where they are
            if self._staging is None:
                self._staging = torch.empty(self.staging_bytes, dtype=torch.uint8, device=dev)
            per_row = 2 * rb + (0 if whole else db)
            chunk = max(1, (self.staging_bytes - 16) // per_row)
            if per_row + 16 > self._staging.numel():           # a single frame above the budget: its own buffer
                self._staging = torch.empty(per_row + 16, dtype=torch.uint8, device=dev)
            obs: List[dict] = []
            for a in range(0, rows.size, chunk):
                b = min(rows.size, a + chunk)
                n = b - a
                out = self._staging[:2 * n * rb]
                self._stamp()
                _, _, _, crc = R.varint_pack_rows(rgb, idx[a:b], out)
                dcrc = R.crc32c_rows(depth, idx[a:b])
                self._stamp()
                if whole:
                    dsrc = depth[a:b]
                else:
                    d0 = (2 * n * rb + 15) & ~15
                    dsrc = self._staging[d0:d0 + n * db].view(torch.float32).view(n, -1)
                    torch.index_select(depth, 0, idx[a:b], out=dsrc)
                total = int(sizes_h[a:b].sum())
                h_rgb, h_depth = self._arena.take(total), self._arena.take(n * db)
                h_crc = self._arena.take(8 * n).view(torch.int32)
                h_rgb.copy_(out[:total], non_blocking=True)
                h_depth.view(torch.float32).view(n, -1).copy_(dsrc, non_blocking=True)
                h_crc.copy_(torch.cat([crc, dcrc]), non_blocking=True)
                np_rgb, np_depth = h_rgb.numpy(), h_depth.numpy()
                ends = np.cumsum(sizes_h[a:b])
                l_rgb = [EncodedLeaf(np_rgb[e - m:e], 0) for e, m in zip(ends, sizes_h[a:b])]
                l_depth = [EncodedLeaf(np_depth[k * db:(k + 1) * db], 0) for k in range(n)]
                self._lazy.append((l_rgb + l_depth, h_crc))
                self._in_flight += [crc, dcrc, idx]
                obs += [{"overhead_camera/rgb": r, "overhead_camera/depth": d} for r, d in zip(l_rgb, l_depth)]
            self._in_flight += [rgb, depth]
        self.frames_encoded_on_device += int(rows.size)
        return obs

    def _stamp(self) -> None:
        if self._events is not None:
            import torch
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self._events.append(e)

    def kernel_ms(self) -> float:
        """Device time [ms] of the encode kernels so far (time_kernels=True): device events around the sizing pass of
        every logged step and around the pack + CRC launches of every chunk; gathers and copies are outside."""
        import torch
        torch.cuda.synchronize()
        ev = self._events or []
        return float(sum(a.elapsed_time(b) for a, b in zip(ev[0::2], ev[1::2])))

    def _observations(self, ts, rows: np.ndarray) -> List[dict]:
        if rows.size and self._on_device(ts):
            return self._encode_on_device(ts, rows)
        return [self._obs(ts, i) for i in rows]

    def reset(self, ts) -> None:
        self._meta = self.env.get_camera_metadata()   # calibration_metadata on the FIRST step (:88-95)
        # an env whose reset() failed (PropPlacer found no pose: the reference's reset() raises and the loop drops the
        # episode, transporter_network_data_generation.py:137-139) logs nothing
        failed = getattr(self.env, "placement_failed", None)
        if failed is not None:
            self.mask = self.mask & ~np.asarray(failed, bool)
        rows = np.nonzero(self.mask)[0]
        for i, o in zip(rows, self._observations(ts, rows)):
            self._steps[i] = [{"observation": o, "action": None, "reward": 0.0, "discount": 0.0,
                               "is_first": True, "is_last": False, "is_terminal": False}]

    def step(self, action: dict, ts, active: Optional[np.ndarray] = None) -> None:
        """RLDS convention: the action is stored with the step it was taken FROM; the new timestep opens
        the next step."""
        act = self.mask if active is None else (self.mask & np.asarray(active, bool))
        pose, pix = np.asarray(action["pose"]), np.asarray(action["pixel_coords"])
        rows = np.nonzero(act)[0]
        for i, o in zip(rows, self._observations(ts, rows)):
            self._steps[i][-1]["action"] = {"pose": pose[i], "pixel_coords": pix[i],
                                            "gripper_rot": float(np.broadcast_to(action["gripper_rot"], (self.env.num_envs,))[i])}
            self._steps[i].append({"observation": o, "action": None, "reward": float(np.broadcast_to(ts.reward, (self.env.num_envs,))[i]),
                                   "discount": float(np.broadcast_to(ts.discount, (self.env.num_envs,))[i]),
                                   "is_first": False, "is_last": False, "is_terminal": False})

    def flush(self) -> None:
        if self._lazy or self._in_flight:
            import torch
            torch.cuda.synchronize()
            self._settle()
        for i in np.nonzero(self.mask)[0]:
            if self._steps[i]:
                self._steps[i][-1]["is_last"] = True
                obs = [s["observation"] for s in self._steps[i]]
                if any(isinstance(v, EncodedLeaf) for o in obs for v in o.values()):
                    for o in obs:     # an episode with both kinds of steps: the host ones are encoded here
                        for name, v in o.items():
                            if not isinstance(v, EncodedLeaf):
                                o[name] = EncodedLeaf.from_host(v)
                    self.writer.write_encoded_episode(self._steps[i], self._meta)
                else:
                    self.writer.write_episode(self._steps[i], self._meta)
                self._steps[i] = []
        self._arena = _HostArena(self._arena.block_bytes, self._arena.pin)
