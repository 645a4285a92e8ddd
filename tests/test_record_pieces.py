"""Episode records from encoded pieces, host side: the CRC combine of the C-ABI library and
``EpisodeWriter.write_encoded_episode``, which frames frames that were packed and checksummed elsewhere.  Here the
pieces come from the host encoders (``_pack_varints`` + ``crc32c``), and the files must equal ``write_episode``'s
byte for byte.  CPU only; the device encoders are held to the same host functions in tests/test_gpu_records.py."""
import filecmp
import os

import numpy as np
import pytest

from mujoco_robot_environments_amd import dataset as D
from mujoco_robot_environments_amd import lib

META = {"intrinsics": {"fx": -579.4, "fy": 579.4, "cx": 319.5, "cy": 239.5},
        "extrinsics": {"x": 0.45, "y": 0.0, "z": 1.3, "qx": 0.0, "qy": 0.7071, "qz": 0.7071, "qw": 0.0}}


@pytest.fixture(scope="module", autouse=True)
def _built():
    lib.build()


@pytest.mark.parametrize("len_a", [0, 1, 7, 4096, 123457])
@pytest.mark.parametrize("len_b", [0, 1, 7, 4096, 123457])
def test_crc32c_combine_equals_crc_of_concatenation(len_a, len_b):
    rs = np.random.RandomState(len_a * 31 + len_b)
    a, b = rs.bytes(len_a), rs.bytes(len_b)
    got = lib.lib().mre_crc32c_combine(D.crc32c(a), D.crc32c(b), len_b)
    assert got == D.crc32c(a + b)
    assert D.crc32c_combine(D.crc32c(a), D.crc32c(b), len_b) == got


def test_crc32c_combine_chain_of_pieces():
    """A record is many pieces: folding left to right gives the CRC of the whole."""
    rs = np.random.RandomState(3)
    pieces = [rs.bytes(n) for n in (5, 0, 921600, 13, 1, 70000)]
    crc = 0
    for p in pieces:
        crc = D.crc32c_combine(crc, D.crc32c(p), len(p))
    assert crc == D.crc32c(b"".join(pieces))


def _frames(kind: str, T: int, H: int, W: int, seed: int):
    rs = np.random.RandomState(seed)
    lo, hi = {"low": (0, 128), "high": (128, 256), "random": (0, 256)}[kind]
    return [(rs.randint(lo, hi, (H, W, 3)).astype(np.uint8), (rs.rand(H, W) * 3).astype(np.float32)) for _ in range(T)]


def _steps(frames, encoded: bool, seed: int):
    rs = np.random.RandomState(seed)
    T = len(frames)
    steps = []
    for k, (rgb, depth) in enumerate(frames):
        if encoded:
            obs = {"overhead_camera/rgb": D.EncodedLeaf.from_host(rgb), "overhead_camera/depth": D.EncodedLeaf.from_host(depth)}
        else:
            obs = {"overhead_camera/rgb": rgb, "overhead_camera/depth": depth}
        act = None if k == T - 1 else {"pose": rs.rand(7), "pixel_coords": rs.randint(0, 640, 2), "gripper_rot": 0.0}
        steps.append({"observation": obs, "action": act, "reward": float(k), "discount": 1.0 if k else 0.0,
                      "is_first": k == 0, "is_last": k == T - 1, "is_terminal": False})
    return steps


def _write(directory, frames_per_episode, encoded: bool, H: int, W: int):
    w = D.EpisodeWriter(str(directory), "pieces", H, W, max_episodes_per_file=2)
    for e, frames in enumerate(frames_per_episode):
        steps = _steps(frames, encoded, seed=100 + e)
        (w.write_encoded_episode if encoded else w.write_episode)(steps, META)
    return w.close()


def _same_directories(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and any("tfrecord" in n for n in names)
    for n in names:
        assert filecmp.cmp(os.path.join(a, n), os.path.join(b, n), shallow=False), n


@pytest.mark.parametrize("kind", ["low", "high", "random"])
@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("H,W", [(6, 8), (480, 640)])
def test_write_encoded_episode_matches_write_episode(tmp_path, kind, T, H, W):
    episodes = [_frames(kind, T, H, W, seed) for seed in range(3 if H < 100 else 1)]
    info_a = _write(tmp_path / "plain", episodes, False, H, W)
    info_b = _write(tmp_path / "pieces", episodes, True, H, W)
    assert info_a == info_b
    _same_directories(tmp_path / "plain", tmp_path / "pieces")


def test_encoded_episodes_round_trip(tmp_path):
    H, W = 10, 12
    episodes = [_frames("random", T, H, W, seed=T) for T in (1, 3, 4)]
    _write(tmp_path, episodes, True, H, W)
    eps = list(D.read_episodes(str(tmp_path)))
    assert len(eps) == 3
    for frames, e in zip(episodes, eps):
        s = e["steps"]
        T = len(frames)
        assert s["observation"]["overhead_camera/rgb"].shape == (T, H, W, 3)
        for k, (rgb, depth) in enumerate(frames):
            assert np.array_equal(s["observation"]["overhead_camera/rgb"][k], rgb)
            assert np.array_equal(s["observation"]["overhead_camera/depth"][k], depth)
        assert s["is_first"].tolist() == [True] + [False] * (T - 1) and s["is_last"].tolist() == [False] * (T - 1) + [True]
        assert s["reward"].tolist() == [float(k) for k in range(T)]
        assert e["intrinsics"]["fx"] == np.float64(np.float32(META["intrinsics"]["fx"]))


def test_logger_mixes_host_and_encoded_steps(tmp_path):
    """A logger whose episode holds both kinds of observation encodes the host ones at flush: same file either way."""
    H, W = 6, 8
    frames = _frames("random", 3, H, W, seed=9)

    class Env:
        num_envs = 1

        def get_camera_metadata(self):
            return META

    out = []
    for mixed in (False, True):
        d = tmp_path / ("mixed" if mixed else "plain")
        w = D.EpisodeWriter(str(d), "pieces", H, W)
        log = D.BatchedEpisodeLogger(Env(), w)
        log._meta = META
        log._steps[0] = _steps(frames, False, seed=1)
        if mixed:
            o = log._steps[0][1]["observation"]
            o["overhead_camera/rgb"] = D.EncodedLeaf.from_host(o["overhead_camera/rgb"])
        log.flush()
        w.close()
        out.append(d)
    _same_directories(*out)
