"""CPU tests of the orthographic heightmap (mujoco_robot_environments_amd/perception.py, csrc/mre_heightmap_point.h)
against the numpy statement of tests/heightmap_cases.py, bit for bit:

  * hm_point, the very text the kernel runs per pixel, compiled by g++ (-O2 -ffp-contract=off: no fused multiply-add,
    as the statement says) into tests/heightmap_host: cell, height bits and validity of every pixel of every case;
  * heightmap_reference, the torch fallback, on CPU tensors: every output of every case;
  * world_2_cell on the world points of the pixels: the cell the statement puts them in;
  * the argument rules of mre_heightmap that need no device to refuse a call.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import heightmap_cases as HC

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "heightmap_host", "heightmap_host.cpp")
IDS = ["x".join(map(str, s)) + "-" + "x".join(map(str, o)) for s, o in HC.SHAPES]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the host harness"
    exe = str(tmp_path_factory.mktemp("heightmap_host") / "heightmap_host")
    subprocess.check_call([gxx, "-O2", "-ffp-contract=off", "-std=c++17", SRC, "-o", exe])
    return exe


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("shape,out", HC.SHAPES, ids=IDS)
def test_the_kernels_per_pixel_code_on_the_host_equals_the_numpy_statement(harness, tmp_path, shape, out):
    for c in HC.cases(shape, out):
        lo, hi, inv_cell = HC.grid32(c["bounds"], c["cell"])
        fi, fo = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(fi, "wb") as f:
            f.write(np.asarray(shape, np.int32).tobytes())
            f.write(np.concatenate([c["cam"], lo, hi, [inv_cell, c["max_depth"], out[1], out[0]]]).astype(np.float32).tobytes())
            f.write(c["depth"].tobytes())
        subprocess.check_call([harness, fi, fo])
        got = np.fromfile(fo, np.uint32).reshape(shape + (4,))
        cx, cy, hz, valid = HC.numpy_points(c["depth"], c["cam"], lo, hi, inv_cell, c["max_depth"], out)
        assert np.array_equal(got[..., 3] != 0, valid), c["name"]
        for k, want in enumerate((cx, cy, hz)):   # a NaN is a NaN (its payload is not part of the statement)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got[..., k].view(np.float32)), nan), (c["name"], k)
            assert np.array_equal(got[..., k][~nan], _bits(want)[~nan]), (c["name"], k)


def _same(r, want, rgb, seg, what):
    hmap, cmap, smap, src = want
    assert r.height.dtype == torch.float32 and r.src.dtype == torch.int32
    assert np.array_equal(_bits(r.height.cpu().numpy()), _bits(hmap)), what
    assert np.array_equal(r.src.cpu().numpy(), src), what
    if rgb:
        assert r.colour.dtype == torch.uint8 and np.array_equal(r.colour.cpu().numpy(), cmap), what
    else:
        assert r.colour is None
    if seg:
        assert r.seg.dtype == torch.uint8 and np.array_equal(r.seg.cpu().numpy(), smap), what
    else:
        assert r.seg is None


@pytest.mark.parametrize("shape,out", HC.SHAPES, ids=IDS)
def test_heightmap_on_cpu_tensors_equals_the_numpy_statement(shape, out):
    from mujoco_robot_environments_amd import perception as P
    filled = 0
    for i, c in enumerate(HC.cases(shape, out)):
        assert P.heightmap_shape(c["bounds"], c["cell"]) == out
        kw = dict(cam=c["cam"], bounds=c["bounds"], cell=c["cell"], max_depth=c["max_depth"])
        d, rgb, seg = (torch.from_numpy(c[k].copy()) for k in ("depth", "rgb", "seg"))
        want = HC.statement(c)
        _same(P.heightmap(d, rgb, seg, **kw), want, True, True, c["name"])
        with_rgb, with_seg = [(False, False), (True, False), (False, True)][i % 3]
        _same(P.heightmap(d, rgb if with_rgb else None, seg if with_seg else None, **kw), want, with_rgb, with_seg, c["name"])
        filled += int((want[3] >= 0).sum())
        if c["name"].startswith("sees nothing"):
            assert (want[3] == -1).all() and (want[0] == 0).all() and (want[1] == 0).all() and (want[2] == 255).all()
        if c["name"] == "straight down: constant depth":   # equal heights: the first pixel of a cell wins it
            cx, cy, hz, valid = HC.numpy_points(c["depth"], c["cam"], *HC.grid32(c["bounds"], c["cell"]), c["max_depth"], out)
            assert valid.any() and len(np.unique(hz[valid])) == 1
            first = {}
            for e, v, u in zip(*np.nonzero(valid)):
                first.setdefault((e, int(cy[e, v, u]), int(cx[e, v, u])), v * shape[2] + u)
            assert all(want[3][k] == i0 for k, i0 in first.items()) and len(first) == int((want[3] >= 0).sum())
    assert filled > 0


def test_the_cases_exercise_what_they_are_meant_to():
    """Ties, cells with many pixels, empty cells and the bounds' own heights all occur in the cases."""
    shape, out = HC.SHAPES[4]   # 2 x 48 x 64 -> 4 x 3
    for c in HC.cases(shape, out):
        if c["name"] == "overhead: scene":
            valid = HC.numpy_points(c["depth"], c["cam"], *HC.grid32(c["bounds"], c["cell"]), c["max_depth"], out)[3]
            assert valid.sum() > 100 * out[0] * out[1]
    shape, out = HC.SHAPES[3]   # 2 x 48 x 64 -> 160 x 120
    assert all((HC.statement(c)[3] >= 0).mean() < 0.2 for c in HC.cases(shape, out))
    shape, out = HC.SHAPES[0]   # 1 x 1 x 4 -> 1 x 1: all four pixels compete
    for c in HC.cases(shape, out):
        if c["name"] in ("straight down: scene", "straight down: constant depth"):
            assert HC.numpy_points(c["depth"], c["cam"], *HC.grid32(c["bounds"], c["cell"]), c["max_depth"], out)[3].sum() == 4
    shape, out = HC.SHAPES[2]
    c = [c for c in HC.cases(shape, out) if c["name"] == "straight down: on the bounds"][0]
    lo, hi, inv_cell = HC.grid32(c["bounds"], c["cell"])
    hz = HC.statement(c)[0]
    assert (hz == hi[2] - lo[2]).any() and ((hz == 0) & (HC.statement(c)[3] >= 0)).any()   # both ends are inside


@pytest.mark.parametrize("shape,out", HC.SHAPES[1:4], ids=IDS[1:4])
def test_world_2_cell_agrees_with_the_statement(shape, out):
    from mujoco_robot_environments_amd import perception as P
    for c in HC.cases(shape, out):
        lo, hi, inv_cell = HC.grid32(c["bounds"], c["cell"])
        cx, cy, hz, valid = HC.numpy_points(c["depth"], c["cam"], lo, hi, inv_cell, c["max_depth"], out)
        pts = np.stack(HC.numpy_world(c["depth"], c["cam"]), axis=-1)[valid]
        got = P.world_2_cell(pts, c["bounds"], c["cell"])
        assert isinstance(got, np.ndarray) and got.dtype == np.int64
        assert np.array_equal(got, np.stack([cx[valid], cy[valid]], axis=-1).astype(np.int64)), c["name"]
        t = P.world_2_cell(torch.from_numpy(pts[:, :2]), c["bounds"], c["cell"])
        assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), got)
    assert P.world_2_cell([0.2 - 1e-3, -0.4 + 1e-3, 0.5], ((0.2, -0.4, 0.39), (0.8, 0.4, 0.69)), 0.0025).tolist() == [-1, 0]


def test_heightmap_camera_is_pixel_2_world():
    """pos + d A (u, v, 1) is the reference's pixel_2_world (tasks/rearrangement.py:505-531): K^-1, the depth along -z,
    the inverse extrinsics."""
    from mujoco_robot_environments_amd import perception as P
    pos, mat, fovy = HC.CAMERAS["oblique rolled"]
    h, w = 48, 64
    cam = P.heightmap_camera(pos, mat, fovy, h, w)
    assert cam.dtype == np.float32 and cam.shape == (12,) and np.array_equal(cam, HC.camera12(pos, mat, fovy, h, w))
    f = (1.0 / np.tan(np.deg2rad(fovy) / 2)) * h / 2.0
    K = np.array([[-f, 0, (w - 1) / 2], [0, f, (h - 1) / 2], [0, 0, 1]])
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = mat.T, -mat.T @ np.asarray(pos)
    for u, v, d in [(0, 0, 0.7), (63, 47, 1.9), (20.5, 11.25, 1.0)]:
        ray = np.linalg.inv(K) @ np.array([u, v, 1.0])
        want = (np.linalg.inv(E) @ np.concatenate([ray * -d, [1.0]]))[:3]
        got = cam[9:].astype(np.float64) + d * (cam[:9].astype(np.float64).reshape(3, 3) @ np.array([u, v, 1.0]))
        assert np.allclose(got, want, atol=1e-5)


def test_heightmap_rejects_bad_shapes_and_grids():
    from mujoco_robot_environments_amd import perception as P
    c = HC.cases(*HC.SHAPES[1])[0]
    d = torch.from_numpy(c["depth"].copy())
    kw = dict(cam=c["cam"], bounds=c["bounds"], cell=c["cell"])
    for bad in (dict(cell=0.0), dict(cell=float("nan")), dict(bounds=((0, 0, 1), (1, 1, 0))), dict(max_depth=0.0),
                dict(bounds=((0, 0, 0), (1, 1, float("inf")))), dict(cell=1e-5)):
        with pytest.raises(ValueError):
            P.heightmap(d, **{**kw, **bad})
    with pytest.raises(ValueError):
        P.heightmap(d[0], **kw)
    with pytest.raises(ValueError):
        P.heightmap(d, torch.zeros((2, 3, 8), dtype=torch.uint8), **kw)
    with pytest.raises(ValueError):
        P.heightmap(d, None, torch.zeros((2, 3, 9), dtype=torch.uint8), **kw)


def test_bad_arguments_are_refused_without_a_gpu():
    """The rules of mre_heightmap that are checked before any device call: MRE_ERR_ARG and a message that names it."""
    from mujoco_robot_environments_amd import lib as L
    L.build()
    lib = L.lib()
    cam = np.arange(12, dtype=np.float32)
    b = np.array([0, 0, 0, 1, 1, 1], np.float32)
    p = 4096   # never dereferenced: every call below is refused on its scalars or on the pointers' own values
    good = dict(depth=p, rgb=None, seg=None, n=1, h=4, w=4, cam=cam.ctypes.data, bounds=b.ctypes.data, inv_cell=4.0,
                max_depth=99.0, out_h=4, out_w=4, hmap=p, cmap=None, smap=None, src=None)
    nan_b, swapped = b.copy(), b.copy()
    nan_b[4], swapped[[2, 5]] = np.nan, (1, 0)
    bad = [dict(n=-1), dict(h=0), dict(w=0), dict(h=65536, w=32768), dict(out_h=0), dict(out_w=0), dict(out_h=4097),
           dict(out_w=4097), dict(inv_cell=0.0), dict(inv_cell=-1.0), dict(inv_cell=float("inf")), dict(inv_cell=float("nan")),
           dict(max_depth=0.0), dict(max_depth=float("inf")), dict(max_depth=float("nan")), dict(bounds=nan_b.ctypes.data),
           dict(bounds=swapped.ctypes.data), dict(bounds=None), dict(cam=None), dict(depth=None), dict(hmap=None),
           dict(depth=p + 1), dict(hmap=p + 2), dict(src=p + 2), dict(rgb=p), dict(cmap=p), dict(seg=p), dict(smap=p)]
    for kw in bad:
        a = {**good, **kw}
        rc = lib.mre_heightmap(None, *[a[k] for k in good])
        assert rc == -1, (kw, rc)   # MRE_ERR_ARG
        assert lib.mre_last_error().startswith(b"mre_heightmap"), kw
    assert lib.mre_heightmap(None, *[{**good, "n": 0}[k] for k in good]) == 0   # n = 0: MRE_OK, nothing launched
