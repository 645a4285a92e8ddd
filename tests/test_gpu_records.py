"""Episode-record encoding on the device (csrc/mre_records.hip): the varint pack and CRC-32C
kernels against the host encoders of dataset.py -- exact equality, there is no tolerance in a file format -- and the
logger's device path against its host path, file for file."""
import collections
import filecmp
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MRE_ERR_ARG = -1
FRAME = 480 * 640 * 3


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from mujoco_robot_environments_amd import lib
    lib.lib()
    assert torch.cuda.is_available()
    return torch


def _content(kind: str, rows: int, row_bytes: int, seed: int) -> np.ndarray:
    rs = np.random.RandomState(seed)
    if kind == "low":
        return rs.randint(0, 128, (rows, row_bytes)).astype(np.uint8)
    if kind == "high":
        return rs.randint(128, 256, (rows, row_bytes)).astype(np.uint8)
    if kind == "random":
        return rs.randint(0, 256, (rows, row_bytes)).astype(np.uint8)
    a = rs.randint(0, 128, (rows, row_bytes)).astype(np.uint8)   # "last": the only value >= 128 of a row is its last
    a[:, -1] = 128 + rs.randint(0, 128, rows)
    return a


def _host(rows_np):
    """What the host writer makes of each row: packed bytes, their CRC."""
    from mujoco_robot_environments_amd import dataset as D
    packed = [D._pack_varints(r) for r in rows_np]
    return packed, [D.crc32c(p) for p in packed]


def _check_pack(torch, out, off, ln, crc, rows_np):
    packed, crcs = _host(rows_np)
    off_h, len_h = off.cpu().numpy(), ln.cpu().numpy().view(np.uint32)
    crc_h = crc.cpu().numpy().view(np.uint32)
    lens = np.array([len(p) for p in packed], np.int64)
    print(f"rows {len(packed)}: packed {int(lens.sum())} bytes; len equal {np.array_equal(len_h, lens)}, "
          f"crc equal {crc_h.tolist() == crcs}")
    assert np.array_equal(len_h.astype(np.int64), lens)
    assert np.array_equal(off_h, np.concatenate([[0], np.cumsum(lens)[:-1]]))
    assert crc_h.tolist() == crcs
    total = int(lens.sum())
    assert out[:total].cpu().numpy().tobytes() == b"".join(packed)


@pytest.mark.parametrize("kind", ["low", "high", "random", "last"])
@pytest.mark.parametrize("rows", [1, 5, 64])
@pytest.mark.parametrize("row_bytes", [1, 3, 127, 4097, FRAME])
def test_varint_pack_matches_host(torch_cuda, row_bytes, rows, kind):
    torch = torch_cuda
    from mujoco_robot_environments_amd import records as R
    a = _content(kind, rows, row_bytes, seed=row_bytes % 1000 + rows)
    out, off, ln, crc = R.varint_pack_rows(torch.from_numpy(a).cuda())
    _check_pack(torch, out, off, ln, crc, a)
    off2, ln2 = R.varint_size_rows(torch.from_numpy(a).cuda())     # the sizing pass alone says the same
    assert torch.equal(off2, off) and torch.equal(ln2, ln)


@pytest.mark.parametrize("row_bytes", [1, 3, 127, 4097, FRAME])
def test_varint_pack_index_list_and_stride(torch_cuda, row_bytes):
    """Rows picked through an index list with gaps, out of order and twice, from a buffer whose row stride is not the
    row length (and leaves the rows unaligned)."""
    torch = torch_cuda
    from mujoco_robot_environments_amd import records as R
    src_rows, stride = 9, row_bytes + 5
    a = _content("random", src_rows, stride, seed=row_bytes % 997)
    idx = np.array([8, 0, 3, 3, 6], np.int32)
    src = torch.from_numpy(a).cuda()[:, :row_bytes]
    assert src.stride(0) == stride
    out, off, ln, crc = R.varint_pack_rows(src, R.row_index(idx, src_rows, src.device))
    _check_pack(torch, out, off, ln, crc, a[idx, :row_bytes])
    c = R.crc32c_rows(src, R.row_index(idx, src_rows, src.device))
    from mujoco_robot_environments_amd import dataset as D
    assert c.cpu().numpy().view(np.uint32).tolist() == [D.crc32c(a[i, :row_bytes].tobytes()) for i in idx]


def test_row_index_is_checked_on_the_host(torch_cuda):
    from mujoco_robot_environments_amd import records as R
    for bad in ([0, 4], [-1], []):
        with pytest.raises(ValueError):
            R.row_index(np.array(bad, np.int64), 4, "cuda:0")


@pytest.mark.parametrize("row_bytes", [1, 5, 8192, 8193, 40000, 65536 + 16])
def test_crc32c_rows_matches_host(torch_cuda, row_bytes):
    torch = torch_cuda
    from mujoco_robot_environments_amd import dataset as D, records as R
    a = _content("random", 7, row_bytes, seed=row_bytes % 991)
    c = R.crc32c_rows(torch.from_numpy(a).cuda())
    assert c.cpu().numpy().view(np.uint32).tolist() == [D.crc32c(r.tobytes()) for r in a]


def test_crc32c_rows_of_rendered_depth(torch_cuda):
    from mujoco_robot_environments_amd import dataset as D, records as R
    from mujoco_robot_environments_amd.tasks.rearrangement import BatchedRearrangementEnv, colour_separator_task_config
    env = BatchedRearrangementEnv(cfg=colour_separator_task_config(), num_envs=8, seed=5, solver="Newton", render=True)
    ts = env.reset()
    depth = ts.observation["overhead_camera/depth"]
    assert depth.is_cuda and tuple(depth.shape) == (8, 480, 640)
    c = R.crc32c_rows(depth).cpu().numpy().view(np.uint32).tolist()
    host = depth.cpu().numpy()
    assert c == [D.crc32c(host[i].astype("<f4").tobytes()) for i in range(8)]
    idx = R.row_index([6, 1], 8, depth.device)
    assert R.crc32c_rows(depth, idx).cpu().numpy().view(np.uint32).tolist() == [c[6], c[1]]
    rgb = ts.observation["overhead_camera/rgb"]
    out, off, ln, crc = R.varint_pack_rows(rgb, idx)
    _check_pack(torch_cuda, out, off, ln, crc, rgb.cpu().numpy().reshape(8, -1)[[6, 1]])
    env.close()


def test_small_capacity_is_refused_and_nothing_is_written(torch_cuda):
    torch = torch_cuda
    from mujoco_robot_environments_amd import lib, records as R
    rows, row_bytes, guard = 5, 4097, 4096
    worst = 2 * rows * row_bytes
    src = torch.from_numpy(_content("high", rows, row_bytes, seed=1)).cuda()
    buf = torch.full((worst + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    for cap in (worst - 1, row_bytes, 1):
        with pytest.raises(lib.MreError, match=rf"\({MRE_ERR_ARG}\).*out_capacity"):
            R.varint_pack_rows(src, out=buf[:cap])
        torch.cuda.synchronize()
        assert bool((buf == 0xA5).all()), "a refused call wrote to the buffer"
    # the exact worst case is accepted, filled to the last byte (every value >= 128), and the guard behind it stays
    out, off, ln, crc = R.varint_pack_rows(src, out=buf[:worst])
    _check_pack(torch, out, off, ln, crc, src.cpu().numpy())
    assert int(ln.sum()) == worst
    assert bool((buf[worst:] == 0xA5).all()), "written beyond out_capacity"


TimeStep = collections.namedtuple("TimeStep", ["step_type", "reward", "discount", "observation"])


def _host_copy(ts):
    return TimeStep(ts.step_type, ts.reward, ts.discount, {k: v.cpu().numpy() for k, v in ts.observation.items()
                                                            if k.startswith("overhead_camera/")})


def test_logger_device_path_writes_the_same_shards(torch_cuda, tmp_path):
    """64 envs, camera on, one scripted pick / place pair, seeded: the run's timesteps go to three loggers -- numpy
    copies of the observations (host path), the CUDA tensors (device path), and the CUDA tensors again with a staging
    budget of a few frames (many chunks per step).  Same files, byte for byte."""
    from mujoco_robot_environments_amd import dataset as D
    from mujoco_robot_environments_amd.tasks.rearrangement import BatchedRearrangementEnv, colour_separator_task_config
    N = 64
    cfg = colour_separator_task_config()
    env = BatchedRearrangementEnv(cfg=cfg, num_envs=N, seed=11, solver="Newton", render=True)
    cam = "overhead_camera/overhead_camera"
    H, W = env.overhead_camera_height, env.overhead_camera_width
    dirs = [tmp_path / n for n in ("host", "device", "device_chunked")]
    writers = [D.EpisodeWriter(str(d), "colour_splitter", H, W, max_episodes_per_file=cfg.dataset.max_episodes_per_file)
               for d in dirs]
    logs = [D.BatchedEpisodeLogger(env, writers[0]), D.BatchedEpisodeLogger(env, writers[1]),
            D.BatchedEpisodeLogger(env, writers[2], staging_bytes=16 << 20)]
    ts = env.reset()
    assert ts.observation["overhead_camera/rgb"].is_cuda
    logs[0].reset(_host_copy(ts))
    logs[1].reset(ts)
    logs[2].reset(ts)
    in_progress, pick, place = env.sort_colours()
    assert in_progress.any()
    for pose in (pick, place):
        a = {"pose": pose.copy(), "pixel_coords": env.world_2_pixel(cam, pose[:, :3]), "gripper_rot": 0.0}
        ts = env.step(a)
        logs[0].step(a, _host_copy(ts), in_progress)
        logs[1].step(a, ts, in_progress)
        logs[2].step(a, ts, in_progress)
    for log in logs:
        log.flush()
    infos = [w.close() for w in writers]
    frames = N + 2 * int(in_progress.sum())
    print(f"frames logged {frames}; on the device: {[log.frames_encoded_on_device for log in logs]}")
    assert logs[0].frames_encoded_on_device == 0
    assert logs[1].frames_encoded_on_device == frames and logs[2].frames_encoded_on_device == frames
    assert infos[0] == infos[1] == infos[2]
    names = sorted(os.listdir(dirs[0]))
    assert {"features.json", "dataset_info.json"} < set(names) and sum("tfrecord" in n for n in names) == 7
    for d in dirs[1:]:
        assert sorted(os.listdir(d)) == names
        for n in names:
            assert filecmp.cmp(os.path.join(dirs[0], n), os.path.join(d, n), shallow=False), (d.name, n)
    env.close()


def test_one_call_across_4_gib(torch_cuda):
    """2400 frames of 480 x 640 x 3 bytes of value 200 -> 2400 x 1 843 200 packed bytes in ONE call: the last rows lie
    behind 2^32, which is what the 64-bit offsets are for.  (Last in the file: it holds 6.6 GB of device memory.)"""
    torch = torch_cuda
    from mujoco_robot_environments_amd import dataset as D, records as R
    free, _ = torch.cuda.mem_get_info()
    if free < 16e9:
        pytest.skip(f"{free / 1e9:.1f} GB of device memory free, 16 GB wanted")
    rows = 2400
    src = torch.full((rows, FRAME), 200, dtype=torch.uint8, device="cuda")
    out, off, ln, crc = R.varint_pack_rows(src)
    torch.cuda.synchronize()
    assert out.numel() == 2 * rows * FRAME and out.numel() > 1 << 32
    assert bool((ln == 2 * FRAME).all())
    assert int(off[-1]) == (rows - 1) * 2 * FRAME and int(off[-1]) > 1 << 32
    want = D._pack_varints(np.full(FRAME, 200, np.uint8))
    assert out[int(off[-1]):].cpu().numpy().tobytes() == want
    mid = 1 + (1 << 32) // (2 * FRAME)      # the row that straddles 2^32
    assert out[int(off[mid - 1]):int(off[mid])].cpu().numpy().tobytes() == want
    crcs = crc.cpu().numpy().view(np.uint32)
    assert int(crcs[-1]) == D.crc32c(want) and bool((crcs == crcs[0]).all())
