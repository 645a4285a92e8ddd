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

The layers live in modules of their own and this one is their face (every name is importable from here): ``_tfrecord``
(CRC-32C, record framing), ``_example`` (the Example wire format), ``_tfds`` (features.json, dataset_info.json, shard
names, the nested tree) and ``_shard_io`` (pinned host memory, alignment, device-event timing).  Here are the writer,
the two readers and the logger.
"""
from __future__ import annotations

import json
import os
from typing import Iterator, List, NamedTuple, Optional

import numpy as np

from ._example import (EncodedLeaf, _LIST_KINDS, _feature, _fields, _headers, _ld, _ld_head, _pack_varints,  # noqa: F401
                       _read_varint, _unpack_varints, _varint, decode_example, encode_example, locate_example)
from ._shard_io import DeviceTimer, ReadTimer, _HostArena, align16  # noqa: F401
from ._tfds import (_FEATURES_PKG, _NP_DTYPE, Leaf, _dict_feature, _is_image_leaf, _nest, _tensor_feature,  # noqa: F401
                    check_record_count, feature_leaves, nest_leaves, open_split, rlds_features, shard_path)
from ._tfrecord import (_crc_table, _mask, _masked_crc, _native_crc, crc32c, crc32c_combine, read_records,  # noqa: F401
                        record_bytes, scan_records, write_framed, write_record)


# ------------------------------------------------------------------ the writer
class EpisodeWriter:
    """Shard writer mirroring ``TFDSBackendWriter(data_directory, split_name, max_episodes_per_file,
    ds_config)`` (transporter_network_data_generation.py:103-111)."""

    VERSION = "0.0.1"   # TFDSBackendWriter's default `version`
    RGB_KEY = "steps/observation/overhead_camera/rgb"
    DEPTH_KEY = "steps/observation/overhead_camera/depth"

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
        return shard_path(self.dir, self.name, self.split, k)

    def _roll(self):
        if self._file is not None:
            self._file.close()
            self._shards.append(self._in_file)
        self._file = open(self._tmp_path(len(self._shards)), "wb")
        self._in_file = 0

    def _begin_record(self):
        """The file the next record goes to: a new shard once this one holds max_episodes_per_file."""
        if self._file is None or self._in_file >= self.max_per_file:
            self._roll()
        return self._file

    def _end_record(self, payload_bytes: int) -> None:
        self._bytes += payload_bytes
        self._in_file += 1
        self._episodes += 1

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
        f = self._begin_record()
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
        write_record(f, payload)
        self._end_record(len(payload))

    def _encoded_parts(self, steps: List[dict], metadata: dict) -> list:
        """The Example of ``write_encoded_episode`` as [bytes | EncodedLeaf]: the map entries in key order, as
        ``encode_example`` lays them out, the framing around the images built from the pieces' LENGTHS alone."""
        small = self._small_features(steps, metadata)
        big = {self.RGB_KEY: (3, [s["observation"]["overhead_camera/rgb"] for s in steps]),      # int64_list
               self.DEPTH_KEY: (2, [s["observation"]["overhead_camera/depth"] for s in steps])}  # float_list
        assert all(p.nbytes == 4 * self.h * self.w for p in big[self.DEPTH_KEY][1]), "depth piece: H * W float32"
        parts: list = []
        for k in sorted(list(small) + list(big)):
            key = _ld(1, k.encode())
            if k in small:
                parts.append(_ld(1, key + _ld(2, _feature(small[k]))))
                continue
            kind, pieces = big[k]
            n = sum(p.nbytes for p in pieces)
            h_list = _ld_head(1, n)                          # <kind>_list.value, packed
            h_kind = _ld_head(kind, len(h_list) + n)         # Feature.<kind>_list
            h_feat = _ld_head(2, len(h_kind) + len(h_list) + n)      # map entry: value
            n_entry = len(key) + len(h_feat) + len(h_kind) + len(h_list) + n
            parts.append(_ld_head(1, n_entry) + key + h_feat + h_kind + h_list)
            parts.extend(pieces)
        total = sum(len(p) if isinstance(p, bytes) else p.nbytes for p in parts)
        parts.insert(0, _ld_head(1, total))              # Example.features
        merged: list = []                                # neighbouring small parts as one
        for p in parts:
            if isinstance(p, bytes) and merged and isinstance(merged[-1], bytes):
                merged[-1] += p
            else:
                merged.append(p)
        return merged

    def write_encoded_episode(self, steps: List[dict], metadata: dict) -> None:
        """``write_episode`` for steps whose two images are ``EncodedLeaf`` pieces (observation: {"overhead_camera/rgb":
        packed varints of the frame, "overhead_camera/depth": its float32 bytes}), and the same bytes in the file.  The
        small features are encoded here as usual; the Example's framing around the images is built from the pieces'
        LENGTHS, the record's CRC from their CRCs (``crc32c_combine``), and the pieces go to the file one after
        another -- no megabyte is read or copied on the way."""
        f = self._begin_record()
        parts = self._encoded_parts(steps, metadata)
        n_payload, crc = 0, 0
        for p in parts:
            c, n = (crc32c(p), len(p)) if isinstance(p, bytes) else (p.crc, p.nbytes)
            crc = crc32c_combine(crc, c, n)
            n_payload += n
        write_framed(f, (p if isinstance(p, bytes) else p.data for p in parts), n_payload, crc)
        self._end_record(n_payload)

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
            os.replace(self._tmp_path(k), shard_path(self.dir, self.name, self.split, k, n))
        info = self.dataset_info()
        with open(os.path.join(self.dir, "dataset_info.json"), "w") as f:
            json.dump(info, f, indent=2)
        with open(os.path.join(self.dir, "features.json"), "w") as f:
            json.dump(self.features(), f, indent=4)
        return info


# ------------------------------------------------------------------ the host reader
def read_episodes(data_directory: str, name: Optional[str] = None, split_name: str = "train") -> Iterator[dict]:
    """Generic reader of a TFDS directory of this kind: dataset_info.json names the dataset, its split and shard
    count, features.json says how every Example key is typed and shaped.  Yields nested dicts shaped like the
    feature tree ({"steps": {...arrays with a leading step axis...}, "intrinsics": {...}, "extrinsics": {...}})."""
    split = open_split(data_directory, name, split_name)
    for path, stated in split.shards:
        count = 0
        for rec in read_records(path):
            e = decode_example(rec)
            out = nest_leaves(split.leaves, lambda leaf: e[leaf.key])
            count += 1
            yield out
        check_record_count(path, count, stated)


# ------------------------------------------------------------------ the device reader, stage by stage
class _Shard(NamedTuple):
    """One shard on both sides: its records as ``scan_records`` gives them, the file's bytes on the host, and the
    payloads on the device, record r at d_file[base[r] : base[r] + length]."""
    path: str
    recs: list
    host: memoryview
    base: list
    d_file: object


class _Plan(NamedTuple):
    """One record as the host planned it: the leaves it decoded itself, the step count, and where the images that the
    device decodes lie in the payload."""
    small: dict        # key -> flat numpy values
    T: int
    rows: list         # uint8 images: (key, offset, packed bytes, values)
    floats: list       # float32 images: (key, offset, bytes)


class _Launched(NamedTuple):
    """What was enqueued for a shard: every record's image leaves as flat device tensors, and what must come back."""
    images: list       # per record: key -> device tensor
    row_of: list       # (record, key) of every row of the unpack call
    status: object     # int32 per row, on the device; None without rows
    crcs: object       # the payloads' CRC-32C, int32 per record, on the device; None without verify


def _record_error(path: str, r: int, what) -> ValueError:
    return ValueError(f"{path}: record {r}: {what}")


def _upload_shard(path: str, recs: list, arena: _HostArena, dev) -> _Shard:
    """The file goes to the device once through pinned memory, each payload to a 16-byte aligned base."""
    import torch
    size = os.path.getsize(path)
    arena.reset()                                      # the previous shard's copies ended with its synchronise
    h_file = arena.take(size)
    with open(path, "rb") as f:
        if f.readinto(h_file.numpy()) != size:
            raise ValueError(f"{path}: changed while it was read")
    base, total = [], 0
    for _, length, _ in recs:
        base.append(total)
        total += align16(length)
    d_file = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    for (off, length, _), b in zip(recs, base):
        if length:
            d_file[b:b + length].copy_(h_file[off:off + length], non_blocking=True)
    return _Shard(path, recs, memoryview(h_file.numpy()), base, d_file)


def _step_count(leaves: List[Leaf], where: dict, small: dict, pay) -> int:
    """T of one record.  The first leaf of the step sequence, in features.json's order, whose length tells decides:
    (1) a leaf the host decoded, by its values, or (2) a float32 image, by its bytes.  With uint8 images only,
    (3) the first one's values are counted: a value ends at every byte with the high bit clear."""
    for leaf in leaves:
        if leaf.seq and leaf.key in small:
            return small[leaf.key].size // leaf.per
        if leaf.seq and leaf.dtype == "float32":
            return where[leaf.key][2] // (4 * leaf.per)
    leaf = next(x for x in leaves if x.seq)
    _, o, ln = where[leaf.key]
    return int(np.count_nonzero(np.frombuffer(pay[o:o + ln], np.uint8) < 0x80)) // leaf.per


def _plan_record(pay, leaves: List[Leaf]) -> _Plan:
    """The host's share of one record, from its bytes alone: the framing, the small leaves, T, the image rows of the
    unpack call and the float images' slices.  Raises ValueError / KeyError without naming the record."""
    where = locate_example(pay)
    small, images = {}, []
    for leaf in leaves:
        kind, o, ln = where[leaf.key]
        if _is_image_leaf(leaf.shape, leaf.dtype, leaf.seq) and kind == ("int64" if leaf.dtype == "uint8" else "float"):
            if leaf.dtype == "float32" and ln % (4 * leaf.per):
                raise ValueError(f"'{leaf.key}': {ln} bytes are no whole number of float32 {leaf.shape} frames")
            images.append(leaf)
        elif kind == "bytes":
            raise ValueError(f"'{leaf.key}': a bytes list where features.json has a {leaf.dtype} tensor")
        else:
            small[leaf.key] = _unpack_varints(pay[o:o + ln]) if kind == "int64" else np.frombuffer(pay[o:o + ln], "<f4")
    T = _step_count(leaves, where, small, pay)
    rows, floats = [], []
    for leaf in images:
        _, o, ln = where[leaf.key]
        if leaf.dtype == "uint8":
            rows.append((leaf.key, o, ln, T * leaf.per))
        elif ln != 4 * T * leaf.per:
            raise ValueError(f"'{leaf.key}': {ln} bytes for {T} steps of float32 {leaf.shape}")
        else:
            floats.append((leaf.key, o, ln))
    return _Plan(small, T, rows, floats)


def _launch(shard: _Shard, plans: List[_Plan], verify: bool, timer: Optional[ReadTimer]) -> _Launched:
    """ALL uint8 image lists of the shard in one unpack call, rows of 16-byte aligned starts in one buffer; a float32
    image is the payload's bytes as they are (a byte-slice copy, then a view: its offset in the payload is not a
    multiple of 4); with verify, the CRC-32C of every payload."""
    import torch
    from . import records as R
    d_file, dev = shard.d_file, shard.d_file.device
    images = [{key: d_file[b + o:b + o + ln].clone().view(torch.float32) for key, o, ln in plan.floats}
              for plan, b in zip(plans, shard.base)]
    rows, row_of, n_out = [], [], 0                    # rows: (src_off, src_len, nvalues, out_off)
    for r, (plan, b) in enumerate(zip(plans, shard.base)):
        for key, o, ln, nv in plan.rows:
            rows.append((b + o, ln, nv, n_out))
            row_of.append((r, key))
            n_out += align16(nv)
    status = None
    if timer is not None:
        timer.stamp()
    if rows:
        desc = np.asarray(rows, np.int64).T
        d_out = torch.empty(max(n_out, 1), dtype=torch.uint8, device=dev)
        _, status = R.varint_unpack_rows(d_file, desc[0], desc[1], desc[2], desc[3], out=d_out)
        for (r, key), (_, _, nv, o) in zip(row_of, rows):
            images[r][key] = d_out[o:o + nv]
    if timer is not None:
        timer.stamp()
        timer.stamp()
        timer.packed_bytes += int(sum(x[1] for x in rows))
        timer.unpacked_bytes += int(sum(x[2] for x in rows))
    crcs = None
    if verify:
        crcs = torch.cat([R.crc32c_rows(d_file[b:b + length].view(1, -1)) if length else
                          torch.zeros(1, dtype=torch.int32, device=dev) for (_, length, _), b in zip(shard.recs, shard.base)])
        if timer is not None:
            timer.crc_bytes += int(sum(length for _, length, _ in shard.recs))
    if timer is not None:
        timer.stamp()
    return _Launched(images, row_of, status, crcs)


def _first_errors(shard: _Shard, launched: _Launched) -> dict:
    """{record: message}, the first per record, from the unpack statuses and the CRCs: read back together, which is the
    shard's one synchronise."""
    import torch
    parts = [t for t in (launched.status, launched.crcs) if t is not None]
    back = torch.cat(parts).cpu().numpy() if parts else np.zeros(0, np.int32)
    n_rows = len(launched.row_of) if launched.status is not None else 0
    bad: dict = {}
    for (r, key), st in zip(launched.row_of, back[:n_rows]):
        if st and r not in bad:
            bad[r] = f"'{key}': malformed packed varints (unpack status {int(st):#x})"
    if launched.crcs is not None:
        for r, ((_, _, stored), crc) in enumerate(zip(shard.recs, back[n_rows:].view(np.uint32))):
            if _mask(int(crc)) != stored:
                bad[r] = "bad payload CRC (computed on the device; it covers every key of the record)"
    return bad


def read_episodes_device(data_directory: str, name: Optional[str] = None, split_name: str = "train", device=None,
                         verify: bool = True, timer: Optional[ReadTimer] = None) -> Iterator[dict]:
    """``read_episodes`` with the image leaves decoded on the device: the same tree, dtypes and shapes, where a tensor
    leaf of rank >= 2 inside the step sequence with dtype uint8 or float32 is a CUDA tensor (uint8 [T, H, W, 3],
    float32 [T, H, W]) and everything else is numpy, decoded on the host from its located bytes.  Driven by
    features.json like ``read_episodes``; the HIP path has no host fallback (no GPU, no reader).

    Per shard: ``scan_records`` finds the records from the framing; ``_upload_shard`` sends the file to the device;
    ``_plan_record`` finds every feature's bytes with ``locate_example`` and decodes the small leaves on the host;
    ``_launch`` enqueues the unpack (``records.varint_unpack_rows``) and, with verify=True, the CRC-32C of every payload
    (``records.crc32c_rows``), compared with the stored one; ``_first_errors`` is the one synchronise per shard, for the
    statuses and the CRCs.  A CRC mismatch, a non-zero unpack status or a record count other than dataset_info.json's
    raises ValueError naming the file, the record and the key; the shard's records before the bad one are yielded, none
    after.  ``timer`` (a ReadTimer) puts device events around the unpack and the CRC launches and counts their bytes."""
    import torch
    split = open_split(data_directory, name, split_name)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    arena = None
    for path, stated in split.shards:
        recs = list(scan_records(path))
        check_record_count(path, len(recs), stated)
        if not recs:
            continue
        size = os.path.getsize(path)
        if arena is None or arena.block_bytes < size:
            arena = _HostArena(1 << max(size - 1, 1).bit_length())
        with torch.cuda.device(dev):
            shard = _upload_shard(path, recs, arena, dev)
            plans = []
            for r, (off, length, _) in enumerate(recs):
                try:
                    plans.append(_plan_record(shard.host[off:off + length], split.leaves))
                except (ValueError, KeyError) as e:
                    raise _record_error(path, r, e) from None
            launched = _launch(shard, plans, verify, timer)
            bad = _first_errors(shard, launched)
        for r, (plan, images) in enumerate(zip(plans, launched.images)):
            if r in bad:
                raise _record_error(path, r, bad[r])
            yield nest_leaves(split.leaves, lambda leaf: plan.small[leaf.key] if leaf.key in plan.small else
                              images[leaf.key].view((plan.T,) + leaf.shape))


# ------------------------------------------------------------------ the logger
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
        self._timer = DeviceTimer() if time_kernels else None   # (start, end) pairs around the encode kernels

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

    def _stamp(self) -> None:
        if self._timer is not None:
            self._timer.stamp()

    def kernel_ms(self) -> float:
        """Device time [ms] of the encode kernels so far (time_kernels=True): device events around the sizing pass of
        every logged step and around the pack + CRC launches of every chunk; gathers and copies are outside."""
        if self._timer is None:
            import torch
            torch.cuda.synchronize()
            return 0.0
        return self._timer.spans_ms(2)[0]

    def _packed_sizes(self, rgb, idx) -> np.ndarray:
        """The packed length of every logged rgb row, on the host: the sizing pass and the step's one synchronise."""
        from . import records as R
        self._stamp()
        _, sizes = R.varint_size_rows(rgb, idx)
        self._stamp()
        sizes_h = sizes.cpu().numpy().astype(np.int64)
        self._settle()
        return sizes_h

    def _encode_chunk(self, rgb, depth, idx, sizes_h: np.ndarray, depth_rows) -> List[dict]:
        """One chunk of envs (device rows `idx`, packed rgb lengths `sizes_h`): pack and checksum into the staging, the
        three copies to the host, and the leaves whose CRCs land with them.  `depth_rows` are the chunk's depth rows
        where they lie already, or None: then they are gathered into the staging behind the rgb bytes."""
        import torch
        from . import records as R
        n, rb, db = int(idx.numel()), int(rgb.shape[1]), 4 * int(depth.shape[1])
        out = self._staging[:2 * n * rb]
        self._stamp()
        _, _, _, crc = R.varint_pack_rows(rgb, idx, out)
        dcrc = R.crc32c_rows(depth, idx)
        self._stamp()
        if depth_rows is None:
            d0 = align16(2 * n * rb)
            depth_rows = self._staging[d0:d0 + n * db].view(torch.float32).view(n, -1)
            torch.index_select(depth, 0, idx, out=depth_rows)
        total = int(sizes_h.sum())
        h_rgb, h_depth = self._arena.take(total), self._arena.take(n * db)
        h_crc = self._arena.take(8 * n).view(torch.int32)
        h_rgb.copy_(out[:total], non_blocking=True)
        h_depth.view(torch.float32).view(n, -1).copy_(depth_rows, non_blocking=True)
        h_crc.copy_(torch.cat([crc, dcrc]), non_blocking=True)
        np_rgb, np_depth = h_rgb.numpy(), h_depth.numpy()
        l_rgb = [EncodedLeaf(np_rgb[e - m:e], 0) for e, m in zip(np.cumsum(sizes_h), sizes_h)]
        l_depth = [EncodedLeaf(np_depth[k * db:(k + 1) * db], 0) for k in range(n)]
        self._lazy.append((l_rgb + l_depth, h_crc))
        self._in_flight += [crc, dcrc, idx]
        return [{"overhead_camera/rgb": r, "overhead_camera/depth": d} for r, d in zip(l_rgb, l_depth)]

    def _encode_on_device(self, ts, rows: np.ndarray) -> List[dict]:
        """Observations (EncodedLeaf pairs) of env rows[k] for every k.  The leaves' bytes and CRCs are valid after the
        next synchronise of the stream (the next logged step's, or flush's)."""
        import torch
        from . import records as R
        rgb, depth = ts.observation["overhead_camera/rgb"], ts.observation["overhead_camera/depth"]
        n_src = int(rgb.shape[0])
        rgb, depth = rgb.reshape(n_src, -1), depth.reshape(n_src, -1)
        assert rgb.dtype == torch.uint8 and depth.dtype == torch.float32, (rgb.dtype, depth.dtype)
        dev = rgb.device
        obs: List[dict] = []
        with torch.cuda.device(dev):
            idx = R.row_index(rows, n_src, dev)
            sizes_h = self._packed_sizes(rgb, idx)
            whole = rows.size == n_src                         # every env, in order: depth rows leave from where they are
            if self._staging is None:
                self._staging = torch.empty(self.staging_bytes, dtype=torch.uint8, device=dev)
            per_row = 2 * int(rgb.shape[1]) + (0 if whole else 4 * int(depth.shape[1]))
            chunk = max(1, (self.staging_bytes - 16) // per_row)
            if per_row + 16 > self._staging.numel():           # a single frame above the budget: its own buffer
                self._staging = torch.empty(per_row + 16, dtype=torch.uint8, device=dev)
            for a in range(0, rows.size, chunk):
                b = min(rows.size, a + chunk)
                obs += self._encode_chunk(rgb, depth, idx[a:b], sizes_h[a:b], depth[a:b] if whole else None)
            self._in_flight += [rgb, depth]
        self.frames_encoded_on_device += int(rows.size)
        return obs

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
        if not rows.size:
            return
        n = (self.env.num_envs,)
        rot, reward, discount = (np.broadcast_to(x, n) for x in (action["gripper_rot"], ts.reward, ts.discount))
        for i, o in zip(rows, self._observations(ts, rows)):
            self._steps[i][-1]["action"] = {"pose": pose[i], "pixel_coords": pix[i], "gripper_rot": float(rot[i])}
            self._steps[i].append({"observation": o, "action": None, "reward": float(reward[i]),
                                   "discount": float(discount[i]),
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
