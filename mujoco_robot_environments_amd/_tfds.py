"""The TFDS side of a shard directory: features.json (the feature tree as TFDS serialises it), dataset_info.json, the
shard files' names, and the way from an Example's flat keys back to the nested tree.  Nothing here is one side of a
compared pair: the writer and both readers share it."""
from __future__ import annotations

import json
import os
from typing import List, NamedTuple, Optional

import numpy as np

_FEATURES_PKG = "tensorflow_datasets.core.features."
_NP_DTYPE = {"uint8": np.uint8, "int32": np.int32, "int64": np.int64, "bool": np.bool_, "float32": np.float32,
             "float64": np.float64}


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


class Leaf(NamedTuple):
    """A tensor leaf of a features.json tree: its Example key, shape, dtype name, whether it lies inside a Dataset /
    Sequence, and the feature names on the way to it (a name may contain '/' itself, e.g. overhead_camera/rgb)."""
    key: str
    shape: tuple
    dtype: str
    seq: bool
    path: tuple

    @property
    def per(self) -> int:
        """Values of one step (of the whole leaf outside a sequence)."""
        return int(np.prod(self.shape, dtype=np.int64))


def _walk(node: dict, prefix: str = "", in_sequence: bool = False, path: tuple = ()):
    if "featuresDict" in node:
        for k, v in node["featuresDict"]["features"].items():
            yield from _walk(v, f"{prefix}/{k}" if prefix else k, in_sequence, path + (k,))
    elif "sequence" in node:
        yield from _walk(node["sequence"]["feature"], prefix, True, path)
    elif "tensor" in node:
        dims = node["tensor"].get("shape", {}).get("dimensions", [])
        yield Leaf(prefix, tuple(int(d) for d in dims), node["tensor"]["dtype"], in_sequence, path)
    else:
        raise ValueError(f"features.json: unsupported feature at '{prefix}': {sorted(node)}")


def feature_leaves(node: dict, prefix: str = "", in_sequence: bool = False):
    """(example key, shape tuple, dtype, inside a Dataset / Sequence) of every tensor leaf of a features.json tree."""
    for leaf in _walk(node, prefix, in_sequence):
        yield leaf[:4]


def _is_image_leaf(shape, dtype: str, seq: bool) -> bool:
    return seq and len(shape) >= 2 and dtype in ("uint8", "float32")


def shard_path(directory: str, name: str, split: str, k: int, of: Optional[int] = None, file_format: str = "tfrecord") -> str:
    """Shard k of `of`; with of=None the temporary name the writer uses until close() knows how many there are."""
    stem = os.path.join(directory, f"{name}-{split}.{file_format}-{k:05d}")
    return f"{stem}.tmp" if of is None else f"{stem}-of-{of:05d}"


class Split(NamedTuple):
    leaves: List[Leaf]
    shards: list          # (path, the record count dataset_info.json states, as it stands there)


def open_split(directory: str, name: Optional[str] = None, split_name: str = "train") -> Split:
    """What a reader needs of a directory: dataset_info.json names the dataset, its split and shard count,
    features.json says how every Example key is typed and shaped."""
    with open(os.path.join(directory, "features.json")) as f:
        feat = json.load(f)
    with open(os.path.join(directory, "dataset_info.json")) as f:
        info = json.load(f)
    lengths = next(sp for sp in info["splits"] if sp["name"] == split_name)["shardLengths"]
    paths = [shard_path(directory, name or info["name"], split_name, k, len(lengths), info["fileFormat"])
             for k in range(len(lengths))]
    return Split(list(_walk(feat)), list(zip(paths, lengths)))


def check_record_count(path: str, found: int, stated) -> None:
    if found != int(stated):
        raise ValueError(f"{path}: {found} records, dataset_info.json says {stated}")


def _nest(tree: dict, key: str, leaf_names, value):
    """Put `value` at the path of `key` in a nested dict; `leaf_names` are the feature names on the way (a name may
    contain '/' itself, e.g. overhead_camera/rgb)."""
    node = tree
    for name in leaf_names[:-1]:
        node = node.setdefault(name, {})
    node[leaf_names[-1]] = value


def nest_leaves(leaves, value_of) -> dict:
    """The nested dict shaped like the feature tree.  value_of(leaf) is the leaf's flat host values, which get their
    shape (a leading step axis inside a sequence) and dtype here, or a device tensor, which is placed as it is."""
    out: dict = {}
    for leaf in leaves:
        v = value_of(leaf)
        if not getattr(v, "is_cuda", False):
            v = np.asarray(v)
            v = (v.reshape((-1,) + leaf.shape) if leaf.seq else v.reshape(leaf.shape)).astype(_NP_DTYPE[leaf.dtype])
        _nest(out, leaf.key, leaf.path, v)
    return out
