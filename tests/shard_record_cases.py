"""One fixed script over the episode-shard path (mujoco_robot_environments_amd/dataset.py and the modules behind it) and
``digests(group)``, which runs one group of it and returns {case name: sha256 or message}.  The record
tests/golden/shard_record.json is made by tests/golden/make_shard_record.py with the package of the commit BEFORE a
regrouping of that path: such a change touches no kernel and no byte of the format, so it keeps every digest and every
message.  numpy only (the logger's device cases hand ``to_obs`` a function that moves the same arrays to the device).

Host groups (tests/test_shard_record.py): the sha256 of every file of the directories that ``write_episode``,
``write_encoded_episode`` and the logger on a stub env leave behind -- frames of 5 x 7 and 6 x 8, episodes of 1, 2 and 5
steps, pixels all below 128 / all at or above 128 / random, two episodes per shard so that shards roll, an ``env_mask``, a
failed placement, ``active`` subsets -- and the type and text of the error for every malformed input of ``errors``.
Device group (tests/test_gpu_shard_cases.py): the directories R1 .. R4 and E1 .. E6 below, which that test reads with
``read_episodes_device`` against ``read_episodes``; the record holds the ReadTimer's byte counts on R1 and the messages of
E1 .. E6.  A message names its directory as <DIR>.
"""
import collections
import hashlib
import json
import os
import tempfile

import numpy as np

META = {"intrinsics": {"fx": -579.4, "fy": 579.4, "cx": 319.5, "cy": 239.5},
        "extrinsics": {"x": 0.45, "y": 0.0, "z": 1.3, "qx": 0.0, "qy": 0.7071, "qz": 0.7071, "qw": 0.0}}
SIZES = [(5, 7), (6, 8)]
KINDS = {"low": (0, 128), "high": (128, 256), "random": (0, 256)}
TimeStep = collections.namedtuple("TimeStep", ["step_type", "reward", "discount", "observation"])
RGB, DEPTH = "overhead_camera/rgb", "overhead_camera/depth"


def _D():
    from mujoco_robot_environments_amd import dataset
    return dataset


def dir_digests(directory: str) -> dict:
    out = {}
    for n in sorted(os.listdir(directory)):
        with open(os.path.join(directory, n), "rb") as f:
            out[n] = hashlib.sha256(f.read()).hexdigest()
    return out


def message(directory: str, fn) -> str:
    """"<exception type>: <text>" of what fn() raises, the directory's name replaced by <DIR>."""
    try:
        fn()
    except Exception as e:  # noqa: BLE001 (the type is part of the record)
        text = f"{type(e).__name__}: {e}"
        return text.replace(str(directory), "<DIR>") if directory else text
    return "no exception"


# ------------------------------------------------------------------ the two write paths
def frames(kind: str, T: int, H: int, W: int, seed: int):
    rs = np.random.RandomState(seed)
    lo, hi = KINDS[kind]
    return [(rs.randint(lo, hi, (H, W, 3)).astype(np.uint8), (rs.rand(H, W) * 3).astype(np.float32)) for _ in range(T)]


def rlds_steps(frame_list, encoded: bool, seed: int):
    D = _D()
    rs = np.random.RandomState(seed)
    T = len(frame_list)
    steps = []
    for k, (rgb, depth) in enumerate(frame_list):
        obs = {RGB: D.EncodedLeaf.from_host(rgb), DEPTH: D.EncodedLeaf.from_host(depth)} if encoded else {RGB: rgb, DEPTH: depth}
        act = None if k == T - 1 else {"pose": rs.rand(7), "pixel_coords": rs.randint(0, 640, 2), "gripper_rot": 0.25 * k}
        steps.append({"observation": obs, "action": act, "reward": float(k), "discount": 1.0 if k else 0.0,
                      "is_first": k == 0, "is_last": k == T - 1, "is_terminal": False})
    return steps


def write_directory(directory: str, encoded: bool, H: int, W: int, kind: str, lengths=(1, 2, 5), name="shards"):
    """Episodes of `lengths` steps, two per shard, through one of the two write paths; returns close()'s dataset_info."""
    w = _D().EpisodeWriter(directory, name, H, W, max_episodes_per_file=2)
    for e, T in enumerate(lengths):
        steps = rlds_steps(frames(kind, T, H, W, seed=10 * T + e), encoded, seed=100 + e)
        (w.write_encoded_episode if encoded else w.write_episode)(steps, META)
    return w.close()


def _written(encoded: bool) -> dict:
    out = {}
    for H, W in SIZES:
        for kind in KINDS:
            with tempfile.TemporaryDirectory() as d:
                info = write_directory(d, encoded, H, W, kind)
                assert info["splits"][0]["shardLengths"] == ["2", "1"], info
                for n, h in dir_digests(d).items():
                    out[f"{H}x{W} {kind} {n}"] = h
    return out


# ------------------------------------------------------------------ the logger on a stub env
N_ENVS = 5
LOGGER_VARIANTS = ("subsets", "all")


class StubEnv:
    num_envs = N_ENVS

    def __init__(self, failed=None):
        if failed is not None:
            self.placement_failed = failed

    def get_camera_metadata(self):
        return META


def logger_directory(directory: str, H: int, W: int, variant: str, to_obs=None, **logger_kwargs):
    """A run of BatchedEpisodeLogger on StubEnv: "subsets" has an env_mask (env 3 off), a failed placement (env 1) and
    three steps with `active` subsets, the last of which holds one env; "all" logs every env in two steps.  Env 0 has
    pixels below 128, env 2 at or above 128, the others random.  `to_obs` maps each observation array (numpy) to what the
    logger is handed.  Returns the logger."""
    D = _D()
    to_obs = to_obs or (lambda a: a)
    rs = np.random.RandomState(H * W + len(variant))
    if variant == "subsets":
        env = StubEnv(np.array([0, 1, 0, 0, 0], bool))
        mask = np.array([1, 1, 1, 0, 1], bool)
        actives = [np.array(a, bool) for a in ([1, 1, 1, 1, 0], [1, 0, 0, 1, 1], [0, 0, 1, 0, 0])]
    else:
        env, mask, actives = StubEnv(), None, [None, None]

    def timestep(k):
        rgb = rs.randint(0, 256, (N_ENVS, H, W, 3)).astype(np.uint8)
        rgb[0] //= 2
        rgb[2] = 128 + rgb[2] // 2
        depth = (rs.rand(N_ENVS, H, W) * 3).astype(np.float32)
        return TimeStep(None, rs.rand(N_ENVS), 1.0 if k else np.zeros(N_ENVS), {RGB: to_obs(rgb), DEPTH: to_obs(depth)})

    writer = D.EpisodeWriter(directory, "logged", H, W, max_episodes_per_file=2)
    log = D.BatchedEpisodeLogger(env, writer, env_mask=mask, **logger_kwargs)
    log.reset(timestep(0))
    for k, active in enumerate(actives):
        action = {"pose": rs.rand(N_ENVS, 7), "pixel_coords": rs.randint(0, 640, (N_ENVS, 2)),
                  "gripper_rot": 0.5 if k == 0 else rs.rand(N_ENVS)}
        log.step(action, timestep(k + 1), active)
    log.flush()
    writer.close()
    return log


def logger_cases(H: int, W: int, variant: str, directory: str) -> dict:
    return {f"{H}x{W} {variant} {n}": h for n, h in dir_digests(directory).items()}


def _logged() -> dict:
    out = {}
    for H, W in SIZES:
        for variant in LOGGER_VARIANTS:
            with tempfile.TemporaryDirectory() as d:
                logger_directory(d, H, W, variant)
                out.update(logger_cases(H, W, variant, d))
    return out


# ------------------------------------------------------------------ malformed inputs of the host functions
def _errors() -> dict:
    D = _D()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        write_directory(d, False, 6, 8, "random", lengths=(2, 2), name="bad")
        path = os.path.join(d, "bad-train.tfrecord-00000-of-00001")
        with open(path, "rb") as f:
            blob = f.read()
        (off0, n0, _), (off1, n1, _) = list(D.scan_records(path))
        cut = os.path.join(d, "cut")

        def with_bytes(data, reader):
            with open(cut, "wb") as f:
                f.write(bytes(data))
            return message(d, lambda: list(reader(cut)))

        flipped = bytearray(blob)
        flipped[off1 - 12 + 1] ^= 0x04                       # one bit of the second record's length
        out["read_records: bad length CRC"] = with_bytes(flipped, D.read_records)
        out["scan_records: bad length CRC"] = with_bytes(flipped, D.scan_records)
        flipped = bytearray(blob)
        flipped[off1 + n1 // 2] ^= 0x01                      # one bit of the second record's payload
        out["read_records: bad payload CRC"] = with_bytes(flipped, D.read_records)
        out["scan_records: cut inside the header"] = with_bytes(blob[:off1 - 5], D.scan_records)
        out["scan_records: cut inside the record"] = with_bytes(blob[:off1 + n1 // 2], D.scan_records)
        out["scan_records: cut inside the payload CRC"] = with_bytes(blob[:off1 + n1 + 2], D.scan_records)
        info_path = os.path.join(d, "dataset_info.json")
        with open(info_path) as f:
            info = json.load(f)
        info["splits"][0]["shardLengths"][0] = "3"
        with open(info_path, "w") as f:
            json.dump(info, f)
        out["read_episodes: a record count other than dataset_info.json's"] = message(d, lambda: list(D.read_episodes(d)))

    ld, varint = D._ld, D._varint
    good = D.encode_example({"a": np.arange(5), "b": np.arange(3.0)})
    inner = ld(1, ld(1, b"k") + ld(2, ld(3, ld(1, b"\x01\x02\x03"))))
    unpacked = b"".join(varint((1 << 3) | 0) + varint(v) for v in (3, 200, 5))
    located = {
        "a length past the end": good[:-3],
        "Features announces more than the payload holds": varint((1 << 3) | 2) + varint(len(inner) + 9) + inner,
        "a varint that never ends": b"\x0a\xff\xff",
        "fixed64 in front of the features": varint((2 << 3) | 1) + b"\0" * 8 + good,
        "group start inside a Feature": ld(1, ld(1, ld(1, b"k") + ld(2, varint((3 << 3) | 3)))),
        "unpacked elements": ld(1, ld(1, ld(1, b"k") + ld(2, ld(3, unpacked)))),
        "two packed chunks": ld(1, ld(1, ld(1, b"k") + ld(2, ld(3, ld(1, b"\x01") + ld(1, b"\x02"))))),
        "an entry without a value": ld(1, ld(1, ld(1, b"k"))),
        "an entry that is not length-delimited": ld(1, varint((1 << 3) | 0) + varint(7)),
    }
    for name, payload in located.items():
        out[f"locate_example: {name}"] = message("", lambda p=payload: D.locate_example(p))
    out["decode_example: fixed64 in front of the features"] = message(
        "", lambda: D.decode_example(located["fixed64 in front of the features"]))
    out["feature_leaves: an unsupported feature"] = message(
        "", lambda: list(D.feature_leaves(_features_dict({"x": {"pythonClassName": "text", "text": {}}}))))
    return out


# ------------------------------------------------------------------ hand-made directories for the device reader
_PKG = "tensorflow_datasets.core.features."


def _tensor(shape, dtype):
    return {"pythonClassName": _PKG + "tensor_feature.Tensor",
            "tensor": {"shape": {"dimensions": [str(d) for d in shape]}, "dtype": dtype, "encoding": "none"}}


def _features_dict(children):
    return {"pythonClassName": _PKG + "features_dict.FeaturesDict", "featuresDict": {"features": children}}


def _step_tree(step_leaves: dict):
    return _features_dict({"steps": {"pythonClassName": _PKG + "dataset_feature.Dataset",
                                     "sequence": {"feature": _features_dict(step_leaves), "length": "-1"}}})


def hand_made(directory: str, name: str, features: dict, shards) -> None:
    """A TFDS directory from Example payloads: `shards` is a list of lists of payload bytes."""
    D = _D()
    os.makedirs(directory, exist_ok=True)
    for k, payloads in enumerate(shards):
        with open(os.path.join(directory, f"{name}-train.tfrecord-{k:05d}-of-{len(shards):05d}"), "wb") as f:
            for p in payloads:
                D.write_record(f, p)
    with open(os.path.join(directory, "features.json"), "w") as f:
        json.dump(features, f)
    with open(os.path.join(directory, "dataset_info.json"), "w") as f:
        json.dump({"name": name, "fileFormat": "tfrecord",
                   "splits": [{"name": "train", "shardLengths": [str(len(p)) for p in shards]}]}, f)


R1_LENGTHS = (1, 2, 5, 3, 1)


def make_r1(directory: str) -> None:
    """6 x 8 frames, five episodes of 1, 2, 5, 3, 1 steps over three shards."""
    info = write_directory(directory, False, 6, 8, "random", lengths=R1_LENGTHS, name="r1")
    assert info["splits"][0]["shardLengths"] == ["2", "2", "1"]


def odd_floats(shape, seed: int) -> np.ndarray:
    """float32 with NaNs of several payloads, both infinities, -0.0 and denormals among ordinary values."""
    rs = np.random.RandomState(seed)
    bits = rs.rand(*shape).astype(np.float32).view(np.uint32).reshape(-1).copy()
    special = np.array([0x7FC00000, 0x7F800001, 0xFFC12345, 0x7FFFFFFF, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001], np.uint32)
    bits[rs.permutation(bits.size)[:special.size]] = special
    return bits.view(np.float32).reshape(shape)


def make_r2(directory: str) -> None:
    """5 x 7 frames whose float32 images carry NaN payloads and -0.0, three episodes of 2, 1, 3 steps."""
    w = _D().EpisodeWriter(directory, "r2", 5, 7, max_episodes_per_file=2)
    for e, T in enumerate((2, 1, 3)):
        fr = [(rgb, odd_floats((5, 7), 50 + 7 * e + k)) for k, (rgb, _) in enumerate(frames("random", T, 5, 7, seed=e))]
        w.write_episode(rlds_steps(fr, False, seed=e), META)
    w.close()


R3_KEY = "steps/image"
R3_LENGTHS = (1, 3, 2)


def r3_images():
    rs = np.random.RandomState(33)
    return [rs.randint(0, 256, (T, 5, 7, 3)).astype(np.uint8) for T in R3_LENGTHS]


def make_r3(directory: str) -> None:
    """The step sequence holds one uint8 (5, 7, 3) leaf and nothing else; shards of 2, 0 and 1 records."""
    a, b, c = [_D().encode_example({R3_KEY: im}) for im in r3_images()]
    hand_made(directory, "r3", _step_tree({"image": _tensor((5, 7, 3), "uint8")}), [[a, b], [], [c]])


def make_r4(directory: str) -> None:
    """A uint8 image leaf stored as a float_list, a float32 image leaf not named depth, and one scalar leaf."""
    rs = np.random.RandomState(44)
    payloads = []
    for T in (2, 3):
        payloads.append(_D().encode_example({"steps/mask": rs.randint(0, 256, (T, 5, 7)).astype(np.float32),
                                             "steps/height": odd_floats((T, 5, 7), T),
                                             "steps/count": rs.randint(0, 1000, T)}))
    tree = _step_tree({"mask": _tensor((5, 7), "uint8"), "height": _tensor((5, 7), "float32"), "count": _tensor((), "int32")})
    hand_made(directory, "r4", tree, [payloads])


def _flipped_r1(directory: str, source: str, varint_byte: bool) -> None:
    """A copy of R1 with one byte of record 1's rgb list changed: one bit of a byte in its middle, or the second byte of
    the first two-byte value behind the middle set to 0x81 (a varint of three bytes)."""
    D = _D()
    os.makedirs(directory)
    shard = "r1-train.tfrecord-00000-of-00003"
    for n in os.listdir(source):
        with open(os.path.join(source, n), "rb") as f:
            blob = bytearray(f.read())
        if n == shard:
            off, length, _ = list(D.scan_records(os.path.join(source, n)))[1]
            _, o, ln = D.locate_example(memoryview(blob)[off:off + length])["steps/observation/" + RGB]
            if varint_byte:
                rgb = np.frombuffer(bytes(blob[off + o:off + o + ln]), np.uint8)
                i = int(np.nonzero(rgb[ln // 2:] >= 128)[0][0]) + ln // 2
                assert rgb[i + 1] == 1
                blob[off + o + i + 1] = 0x81
            else:
                blob[off + o + ln // 2] ^= 0x01
        with open(os.path.join(directory, n), "wb") as f:
            f.write(bytes(blob))


def make_error_directory(case: str, directory: str, r1: str) -> dict:
    """The directory of E1 .. E6 (r1: a directory made by make_r1); returns read_episodes_device's keyword arguments."""
    enc = _D().encode_example
    image = _tensor((5, 7), "float32")
    if case == "E1 a float image of no whole number of frames":
        hand_made(directory, "e1", _step_tree({"height": image}), [[enc({"steps/height": np.arange(36.0)})]])
    elif case == "E2 a float image of the wrong length for T":
        hand_made(directory, "e2", _step_tree({"count": _tensor((), "int32"), "height": image}),
                  [[enc({"steps/count": np.arange(2), "steps/height": np.arange(105.0)})]])
    elif case == "E3 a bytes list where a tensor is declared":
        hand_made(directory, "e3", _step_tree({"count": _tensor((), "int32")}), [[enc({"steps/count": [b"ab", b"c"]})]])
    elif case == "E4 a key missing from the Example":
        hand_made(directory, "e4", _step_tree({"count": _tensor((), "int32"), "height": image}),
                  [[enc({"steps/count": np.arange(2), "steps/height": np.arange(70.0)}), enc({"steps/count": np.arange(2)})]])
    elif case == "E5 a flipped byte, verify on":
        _flipped_r1(directory, r1, varint_byte=False)
    elif case == "E6 a malformed varint, verify off":
        _flipped_r1(directory, r1, varint_byte=True)
        return {"verify": False}
    else:
        raise KeyError(case)
    return {}


ERROR_CASES = ("E1 a float image of no whole number of frames", "E2 a float image of the wrong length for T",
               "E3 a bytes list where a tensor is declared", "E4 a key missing from the Example",
               "E5 a flipped byte, verify on", "E6 a malformed varint, verify off")


def device_error(case: str, directory: str, r1: str):
    """(episodes yielded before the error, its message) of read_episodes_device on the case's directory."""
    D = _D()
    kwargs = make_error_directory(case, directory, r1)
    got = []

    def read():
        for ep in D.read_episodes_device(directory, **kwargs):
            got.append(ep)
    return got, message(directory, read)


def r1_timer_counts(r1: str) -> dict:
    D = _D()
    timer = D.ReadTimer()
    episodes = list(D.read_episodes_device(r1, timer=timer))
    unpack_ms, crc_ms = timer.kernel_ms()
    assert len(episodes) == len(R1_LENGTHS) and len(timer.events) == 12 and unpack_ms > 0 and crc_ms > 0
    return {f"R1 timer {k}": str(getattr(timer, k)) for k in ("packed_bytes", "unpacked_bytes", "crc_bytes")}


def _device_reader() -> dict:
    out = {}
    with tempfile.TemporaryDirectory() as d:
        r1 = os.path.join(d, "r1")
        make_r1(r1)
        out.update(r1_timer_counts(r1))
        for case in ERROR_CASES:
            got, msg = device_error(case, os.path.join(d, case[:2]), r1)
            out[case] = f"after {len(got)} episodes: {msg}"
    return out


GROUPS = {"write_episode": lambda: _written(False), "write_encoded_episode": lambda: _written(True),
          "logger": _logged, "errors": _errors}
GPU_GROUPS = {"device_reader": _device_reader}


def digests(group: str) -> dict:
    return {**GROUPS, **GPU_GROUPS}[group]()

