"""The host side of the device reader: ``dataset.locate_example`` -- where every feature's bytes
lie in a serialised Example, from the framing alone -- against ``decode_example``, which stays the reference, and
``dataset.scan_records`` against ``read_records``.  CPU only; the unpack kernel and ``read_episodes_device`` are held to
the same host functions in tests/test_gpu_record_reader.py."""
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


def _steps(T: int, H: int, W: int, encoded: bool, seed: int):
    rs = np.random.RandomState(seed)
    steps = []
    for k in range(T):
        rgb, depth = rs.randint(0, 256, (H, W, 3)).astype(np.uint8), (rs.rand(H, W) * 3).astype(np.float32)
        if encoded:
            obs = {"overhead_camera/rgb": D.EncodedLeaf.from_host(rgb), "overhead_camera/depth": D.EncodedLeaf.from_host(depth)}
        else:
            obs = {"overhead_camera/rgb": rgb, "overhead_camera/depth": depth}
        act = None if k == T - 1 else {"pose": rs.rand(7), "pixel_coords": rs.randint(0, 640, 2), "gripper_rot": 0.0}
        steps.append({"observation": obs, "action": act, "reward": float(k), "discount": 1.0 if k else 0.0,
                      "is_first": k == 0, "is_last": k == T - 1, "is_terminal": False})
    return steps


def _shard(directory, T, H, W, encoded, episodes=1):
    w = D.EpisodeWriter(str(directory), "reader", H, W, max_episodes_per_file=4)
    for e in range(episodes):
        (w.write_encoded_episode if encoded else w.write_episode)(_steps(T, H, W, encoded, seed=7 * T + e), META)
    w.close()
    return os.path.join(str(directory), "reader-train.tfrecord-00000-of-00001")


@pytest.mark.parametrize("encoded", [False, True], ids=["write_episode", "write_encoded_episode"])
@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("H,W", [(6, 8), (480, 640)])
def test_located_slices_decode_to_the_reference(tmp_path, H, W, T, encoded):
    (payload,) = list(D.read_records(_shard(tmp_path, T, H, W, encoded)))
    ref = D.decode_example(payload)
    where = D.locate_example(payload)
    assert set(where) == set(ref) and len(ref) == 21
    spans = []
    for key, (kind, off, n) in where.items():
        assert 0 <= off and off + n <= len(payload), key
        spans.append((off, off + n))
        piece = payload[off:off + n]
        if kind == "int64":
            got = D._unpack_varints(piece)
        else:
            assert kind == "float"
            got = np.frombuffer(piece, "<f4")
        assert got.dtype == ref[key].dtype and np.array_equal(got, ref[key]), key
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "located slices overlap"
    off = where[D.EpisodeWriter.DEPTH_KEY][1]
    print(f"T {T} {H}x{W}: depth payload at byte {off} (mod 4: {off % 4})")
    assert where[D.EpisodeWriter.RGB_KEY][0] == "int64" and where[D.EpisodeWriter.DEPTH_KEY][2] == 4 * T * H * W


def test_locate_example_takes_a_memoryview_and_a_bytes_list():
    payload = D.encode_example({"names": [b"ab", b"", b"cde"], "x": np.arange(3.0), "empty": np.zeros(0, np.int64)})
    where = D.locate_example(memoryview(bytearray(payload)))
    kind, off, n = where["names"]
    assert kind == "bytes" and payload[off:off + n] == b"".join(D._ld(1, v) for v in (b"ab", b"", b"cde"))
    assert where["x"][0] == "float" and where["x"][2] == 12
    assert where["empty"][0] == "int64" and where["empty"][2] == 0


def test_scan_records_agrees_with_read_records(tmp_path):
    path = _shard(tmp_path, 2, 6, 8, False, episodes=3)
    payloads = list(D.read_records(path))
    scanned = list(D.scan_records(path))
    assert len(scanned) == len(payloads) == 3
    blob = open(path, "rb").read()
    for (off, n, crc), pay in zip(scanned, payloads):
        assert n == len(pay) and blob[off:off + n] == pay
        assert crc == D._masked_crc(pay)
    assert scanned[-1][0] + scanned[-1][1] + 4 == len(blob)


def test_scan_records_rejects_a_cut_shard_and_a_bad_length(tmp_path):
    path = _shard(tmp_path, 2, 6, 8, False, episodes=2)
    blob = open(path, "rb").read()
    (off0, n0, _), (off1, n1, _) = list(D.scan_records(path))
    cut = os.path.join(str(tmp_path), "cut")
    for end in (off1 + n1 // 2, off1 + n1 + 2, off1 - 5):      # inside the payload, its CRC, the length header
        open(cut, "wb").write(blob[:end])
        with pytest.raises(ValueError, match="cut short"):
            list(D.scan_records(cut))
    flipped = bytearray(blob)
    flipped[off1 - 12 + 1] ^= 0x04                             # one bit of the second record's length
    open(cut, "wb").write(bytes(flipped))
    it = D.scan_records(cut)
    assert next(it) == (off0, n0, D._masked_crc(blob[off0:off0 + n0]))
    with pytest.raises(ValueError, match="length CRC"):
        next(it)


def test_locate_example_errors():
    good = D.encode_example({"a": np.arange(5), "b": np.arange(3.0)})
    assert set(D.locate_example(good)) == {"a", "b"}
    with pytest.raises(ValueError):                            # a length that runs past the end
        D.locate_example(good[:-3])
    inner = D._ld(1, D._ld(1, b"k") + D._ld(2, D._ld(3, D._ld(1, b"\x01\x02\x03"))))
    with pytest.raises(ValueError):                            # Features announces more than the payload holds
        D.locate_example(D._varint((1 << 3) | 2) + D._varint(len(inner) + 9) + inner)
    with pytest.raises(ValueError):                            # a varint that never ends
        D.locate_example(b"\x0a\xff\xff")
    with pytest.raises(ValueError, match="wire type"):         # fixed64 (wire type 1) in front of the features
        D.locate_example(D._varint((2 << 3) | 1) + b"\0" * 8 + good)
    with pytest.raises(ValueError, match="wire type"):         # group start (wire type 3) inside a Feature
        D.locate_example(D._ld(1, D._ld(1, D._ld(1, b"k") + D._ld(2, D._varint((3 << 3) | 3)))))
    unpacked = b"".join(D._varint((1 << 3) | 0) + D._varint(v) for v in (3, 200, 5))   # value: 3, value: 200, value: 5
    example = D._ld(1, D._ld(1, D._ld(1, b"k") + D._ld(2, D._ld(3, unpacked))))
    with pytest.raises(ValueError, match="unpacked"):
        D.locate_example(example)
    two_chunks = D._ld(1, D._ld(1, D._ld(1, b"k") + D._ld(2, D._ld(3, D._ld(1, b"\x01") + D._ld(1, b"\x02")))))
    assert np.array_equal(D.decode_example(two_chunks)["k"], [1, 2])
    with pytest.raises(ValueError, match="chunks"):
        D.locate_example(two_chunks)
