"""The branches of ``read_episodes_device`` and of the logger's device path on directories of a few kilobytes
(tests/shard_record_cases.py): the reader against ``read_episodes`` on the same directory, leaf for leaf and bit for bit; its
errors, the ReadTimer's byte counts and the logger's files against the record tests/golden/shard_record.json, which was made
with the package of the commit before dataset.py was split by layer.  No case holds an episode of zero steps."""
import json
import os

import numpy as np
import pytest

from tests import shard_record_cases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shard_record.json")
MAKERS = {"r1": C.make_r1, "r2": C.make_r2, "r3": C.make_r3, "r4": C.make_r4}
# what read_episodes_device hands back as CUDA tensors: leaves stored as their own list kind
DEVICE_LEAVES = {"r1": {"steps/observation/overhead_camera/rgb", "steps/observation/overhead_camera/depth"},
                 "r2": {"steps/observation/overhead_camera/rgb", "steps/observation/overhead_camera/depth"},
                 "r3": {"steps/image"}, "r4": {"steps/height"}}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from mujoco_robot_environments_amd import lib
    lib.lib()
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def record():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def directories(tmp_path_factory):
    """{case: (directory, what read_episodes gives for it)}: made and read on the host once."""
    from mujoco_robot_environments_amd import dataset as D
    out = {}
    for case, make in MAKERS.items():
        d = str(tmp_path_factory.mktemp(case))
        make(d)
        out[case] = (d, list(D.read_episodes(d)))
    return out


def _leaves(tree, prefix=""):
    for k, v in tree.items():
        if isinstance(v, dict):
            yield from _leaves(v, f"{prefix}{k}/")
        else:
            yield prefix + k, v


def _same(torch, case, host, dev):
    assert len(dev) == len(host) > 0
    for e, (a, b) in enumerate(zip(host, dev)):
        la, lb = dict(_leaves(a)), dict(_leaves(b))
        assert list(la) == list(lb)
        for key, va in la.items():
            vb = lb[key]
            assert isinstance(vb, torch.Tensor) == (key in DEVICE_LEAVES[case]), key
            if isinstance(vb, torch.Tensor):
                assert vb.is_cuda and vb.is_contiguous()
                vb = vb.cpu().numpy()
            assert vb.dtype == va.dtype and vb.shape == va.shape, (e, key, vb.dtype, va.dtype, vb.shape, va.shape)
            assert vb.tobytes() == va.tobytes(), (e, key)


@pytest.mark.parametrize("kwargs", [{}, {"verify": False}, {"device": "cuda:0"}], ids=["verify", "no-verify", "device"])
@pytest.mark.parametrize("case", list(MAKERS))
def test_device_reader_equals_the_host_reader(torch_cuda, directories, case, kwargs):
    from mujoco_robot_environments_amd import dataset as D
    d, host = directories[case]
    _same(torch_cuda, case, host, list(D.read_episodes_device(d, **kwargs)))


def test_r1_layout_and_timer(torch_cuda, directories, record):
    """Several payloads at 16-byte aligned bases of one device buffer, rows of different lengths under one unpack call;
    the timer's events come in fours per shard and its byte counts are the record's."""
    from mujoco_robot_environments_amd import dataset as D
    d, host = directories["r1"]
    assert [e["steps"]["reward"].shape[0] for e in host] == list(C.R1_LENGTHS)
    shards = sorted(n for n in os.listdir(d) if "tfrecord" in n)
    assert [len(list(D.scan_records(os.path.join(d, n)))) for n in shards] == [2, 2, 1]
    timer = D.ReadTimer()
    _same(torch_cuda, "r1", host, list(D.read_episodes_device(d, timer=timer)))
    unpack_ms, crc_ms = timer.kernel_ms()
    assert len(timer.events) == 4 * len(shards) and unpack_ms > 0 and crc_ms > 0
    got = {f"R1 timer {k}": str(getattr(timer, k)) for k in ("packed_bytes", "unpacked_bytes", "crc_bytes")}
    print(got)
    assert got == {k: record["device_reader"][k] for k in got}
    assert timer.unpacked_bytes == sum(C.R1_LENGTHS) * 6 * 8 * 3


def test_r2_float_offsets_are_not_multiples_of_four(directories):
    from mujoco_robot_environments_amd import dataset as D
    d, host = directories["r2"]
    offsets = []
    for n in sorted(n for n in os.listdir(d) if "tfrecord" in n):
        for payload in D.read_records(os.path.join(d, n)):
            offsets.append(D.locate_example(payload)[D.EpisodeWriter.DEPTH_KEY][1])
    assert len(offsets) == 3 and all(o % 4 for o in offsets), offsets
    depth = np.concatenate([e["steps"]["observation"]["overhead_camera/depth"].reshape(-1) for e in host])
    bits = depth.view(np.uint32)
    assert np.isnan(depth).sum() >= 12 and (bits == 0x80000000).sum() >= 3 and (bits == 0xFFC12345).sum() >= 3


def test_r3_is_what_was_written(directories):
    """T found by counting values, the middle shard empty: the host reader gives the three episodes as they were written."""
    d, host = directories["r3"]
    assert os.path.getsize(os.path.join(d, "r3-train.tfrecord-00001-of-00003")) == 0
    images = C.r3_images()
    assert [e["steps"]["image"].shape[0] for e in host] == list(C.R3_LENGTHS)
    assert all(e["steps"]["image"].tobytes() == im.tobytes() and list(e["steps"]) == ["image"] for e, im in zip(host, images))


def test_r4_host_reader_types(directories):
    _, host = directories["r4"]
    assert [e["steps"]["mask"].shape for e in host] == [(2, 5, 7), (3, 5, 7)] and host[0]["steps"]["mask"].dtype == np.uint8


@pytest.mark.parametrize("case", C.ERROR_CASES)
def test_device_reader_errors(torch_cuda, directories, record, tmp_path, case):
    got, msg = C.device_error(case, str(tmp_path / "bad"), directories["r1"][0])
    print(msg)
    assert f"after {len(got)} episodes: {msg}" == record["device_reader"][case]
    if case[:2] in ("E5", "E6"):                # record 0 is still yielded, and equals the host reader's
        assert len(got) == 1
        _same(torch_cuda, "r1", directories["r1"][1][:1], got)


@pytest.mark.parametrize("variant,kwargs", [("subsets", {}), ("all", {}), ("subsets", {"staging_bytes": 300}),
                                            ("all", {"staging_bytes": 300}), ("subsets", {"pin_host": False})])
def test_logger_device_path_writes_the_recorded_files(torch_cuda, record, tmp_path, variant, kwargs):
    """L1: the stub env's observations as CUDA tensors of 6 x 8, N = 5.  "subsets" takes the index_select branch, "all"
    leaves the depth rows where they are; 300 bytes of staging are less than one frame needs, so every chunk is one env
    and the frame gets a buffer of its own.  The files are those of the same observations given as numpy."""
    torch = torch_cuda
    H, W = 6, 8
    log = C.logger_directory(str(tmp_path), H, W, variant, to_obs=lambda a: torch.from_numpy(a).cuda(), **kwargs)
    frames = {"subsets": 3 + 2 + 2 + 1, "all": 3 * C.N_ENVS}[variant]
    assert log.frames_encoded_on_device == frames and log.staging_bytes == kwargs.get("staging_bytes", 1 << 30)
    assert log._arena.pin == kwargs.get("pin_host", True)
    got = C.logger_cases(H, W, variant, str(tmp_path))
    want = {k: v for k, v in record["logger"].items() if k.startswith(f"{H}x{W} {variant} ")}
    assert want and got == want
