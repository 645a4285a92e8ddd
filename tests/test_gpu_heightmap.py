"""GPU tests of mre_heightmap (csrc/mre_heightmap.hip) against the numpy statement of tests/heightmap_cases.py, EXACTLY:
every bit of every output, no tolerance and no cell left out.  The shapes are the smallest at which each mechanism of the
kernel can break:

    1x1x4 -> 1x1            every pixel competes for one cell: the max and the tie rule
    2x3x8 -> 5x7            a map smaller than a tile, envs kept apart
    3x24x32 -> 33x47        several tiles of 32 cells each way, partial last tiles, pixels on tile borders
    3x48x64 -> 70x130       the same for the tile of 64 cells the kernel is built with
    2x48x64 -> 160x120      cells finer than the pixel pitch: mostly empty cells
    2x48x64 -> 4x3          hundreds of pixels per cell: LDS contention, many ties
    1x480x640 -> 320x240    the camera's frame at the default cell

each under the cameras and depth contents of heightmap_cases.cases: the configured overhead pose, obliques, a low close
camera with tile corners behind it (the whole-image path), one that sees nothing of the bounds, ray-cast scenes, one
constant depth straight down (the index decides), depths salted with 0, negatives, NaN, +-inf, 100 and the neighbours
of max_depth, and heights exactly on lo_z and hi_z.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import heightmap_cases as HC

pytestmark = pytest.mark.gpu

DEV = "cuda"
IDS = ["x".join(map(str, s)) + "-" + "x".join(map(str, o)) for s, o in HC.SHAPES]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _raw(a):
    """mre_heightmap on torch's current stream with the arguments of dict a (pointers as ints or None); the status."""
    from mujoco_robot_environments_amd import lib as L
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.lib().mre_heightmap(stream, a["depth"], a["rgb"], a["seg"], a["n"], a["h"], a["w"], a["cam"], a["bounds"],
                               a["inv_cell"], a["max_depth"], a["out_h"], a["out_w"], a["hmap"], a["cmap"], a["smap"],
                               a["src"])
    torch.cuda.synchronize()
    return rc


def _host(case):
    """cam, bounds as contiguous float32 arrays (kept alive by the caller) and inv_cell of a case."""
    lo, hi, inv_cell = HC.grid32(case["bounds"], case["cell"])
    return np.ascontiguousarray(case["cam"]), np.ascontiguousarray(np.concatenate([lo, hi])), float(inv_cell)


def _same(r, want, rgb, seg, what):
    hmap, cmap, smap, src = want
    assert np.array_equal(_bits(r.height.cpu().numpy()), _bits(hmap)), what
    assert np.array_equal(r.src.cpu().numpy(), src), what
    if rgb:
        assert np.array_equal(r.colour.cpu().numpy(), cmap), what
    else:
        assert r.colour is None
    if seg:
        assert np.array_equal(r.seg.cpu().numpy(), smap), what
    else:
        assert r.seg is None


@pytest.mark.parametrize("shape,out", HC.SHAPES, ids=IDS)
def test_kernel_matches_the_numpy_statement_exactly(shape, out):
    from mujoco_robot_environments_amd import perception as P
    n, h, w = shape
    for i, c in enumerate(HC.cases(shape, out)):
        kw = dict(cam=c["cam"], bounds=c["bounds"], cell=c["cell"], max_depth=c["max_depth"])
        d, rgb, seg = (torch.from_numpy(c[k].copy()).to(DEV) for k in ("depth", "rgb", "seg"))
        want = HC.statement(c)
        a = P.heightmap(d, rgb, seg, **kw)
        assert a.height.is_cuda and a.height.shape == (n,) + out
        _same(a, want, True, True, c["name"])
        # every case also with one of the other output combinations in turn
        with_rgb, with_seg = [(False, False), (True, False), (False, True)][i % 3]
        _same(P.heightmap(d, rgb if with_rgb else None, seg if with_seg else None, **kw), want, with_rgb, with_seg, c["name"])
        if c["name"].endswith("scene"):   # a second call on the same input: the same bytes
            b = P.heightmap(d, rgb, seg, **kw)
            assert torch.equal(a.height.view(torch.int32), b.height.view(torch.int32)) and torch.equal(a.src, b.src)
            assert torch.equal(a.colour, b.colour) and torch.equal(a.seg, b.seg)
        if i % 4 == 0:                    # without src, through the C ABI: the other outputs are the same
            cam, bounds, inv_cell = _host(c)
            hmap = torch.full((n,) + out, -77.0, dtype=torch.float32, device=DEV)
            smap = torch.full((n,) + out, 77, dtype=torch.uint8, device=DEV)
            rc = _raw(dict(depth=d.data_ptr(), rgb=None, seg=seg.data_ptr(), n=n, h=h, w=w, cam=cam.ctypes.data,
                           bounds=bounds.ctypes.data, inv_cell=inv_cell, max_depth=c["max_depth"], out_h=out[0],
                           out_w=out[1], hmap=hmap.data_ptr(), cmap=None, smap=smap.data_ptr(), src=None))
            assert rc == 0
            assert np.array_equal(_bits(hmap.cpu().numpy()), _bits(want[0])) and np.array_equal(smap.cpu().numpy(), want[2])


def test_images_and_outputs_between_guards():
    """The images sit one element into their allocations between guard regions whose depth, read as a pixel, is the
    highest point the bounds admit (it would win its cell and show its guard colour and label); the outputs sit inside
    sentinel-filled buffers at odd offsets.  No guard may show in a result and no sentinel outside the outputs may
    change."""
    shape, out = HC.SHAPES[2]
    n, h, w = shape
    hw, cells = h * w, out[0] * out[1]
    c = [c for c in HC.cases(shape, out) if c["name"] == "straight down: scene"][0]
    lo, hi, inv_cell = HC.grid32(c["bounds"], c["cell"])
    d_hi = np.float32(np.float32(1.25) - hi[2])   # straight down from z = 1.25: this depth is a point exactly on hi_z
    one = HC.numpy_points(np.full((1, h, w), d_hi, np.float32), c["cam"], lo, hi, inv_cell, 99.0, out)
    assert one[3].any() and (one[2][one[3]] == hi[2] - lo[2]).all()
    assert (HC.statement(c)[0] < hi[2] - lo[2]).all()              # ... above everything in the scene

    def guarded(src, fill, dtype, per):
        buf = torch.full(((n + 2) * hw * per + 2,), fill, dtype=dtype, device=DEV)
        view = buf[per * hw + 1: per * hw + 1 + n * hw * per]
        view.copy_(torch.from_numpy(src.copy()).to(DEV).reshape(-1))
        return buf, view

    dbuf, dview = guarded(c["depth"], float(d_hi), torch.float32, 1)
    rbuf, rview = guarded(np.minimum(c["rgb"], 250), 255, torch.uint8, 3)
    sbuf, sview = guarded(np.minimum(c["seg"], 250), 254, torch.uint8, 1)
    want = HC.numpy_heightmap(c["depth"], np.minimum(c["rgb"], 250), np.minimum(c["seg"], 250), c["cam"], c["bounds"],
                              c["cell"], c["max_depth"], out)
    assert (want[3] >= 0).sum() > 500
    outs = {"hmap": torch.full((n * cells + 2,), -77.0, dtype=torch.float32, device=DEV),
            "cmap": torch.full((3 * n * cells + 2,), 253, dtype=torch.uint8, device=DEV),
            "smap": torch.full((n * cells + 2,), 253, dtype=torch.uint8, device=DEV),
            "src": torch.full((n * cells + 2,), -77, dtype=torch.int32, device=DEV)}
    cam, bounds, inv_cell = _host(c)
    rc = _raw(dict(depth=dview.data_ptr(), rgb=rview.data_ptr(), seg=sview.data_ptr(), n=n, h=h, w=w, cam=cam.ctypes.data,
                   bounds=bounds.ctypes.data, inv_cell=inv_cell, max_depth=c["max_depth"], out_h=out[0], out_w=out[1],
                   **{k: v[1:].data_ptr() for k, v in outs.items()}))
    assert rc == 0
    for k, wanted in zip(("hmap", "cmap", "smap", "src"), want):
        got = outs[k].cpu().numpy()
        assert np.array_equal(got[1:-1].view(np.uint32 if k == "hmap" else got.dtype),
                              wanted.reshape(-1).view(np.uint32 if k == "hmap" else wanted.dtype)), k
        assert got[0] == got[-1] and got[0] in (-77, 253), k
    assert not (want[1] == 255).any() and not (want[2] == 254).any()   # so a guard's colour or label would have shown
    assert (dbuf[:hw + 1] == float(d_hi)).all() and (dbuf[hw + 1 + n * hw:] == float(d_hi)).all()


def test_bad_arguments_return_err_arg_and_write_nothing():
    from mujoco_robot_environments_amd import lib as L
    shape, out = HC.SHAPES[1]
    n, h, w = shape
    c = HC.cases(shape, out)[0]
    want = HC.statement(c)
    d = torch.from_numpy(np.concatenate([c["depth"].reshape(-1), [1.0]]).astype(np.float32)).to(DEV)
    rgb, seg = (torch.from_numpy(c[k].copy()).to(DEV) for k in ("rgb", "seg"))
    cells = out[0] * out[1]
    outs = {"hmap": torch.full((n * cells + 1,), -77.0, dtype=torch.float32, device=DEV),
            "cmap": torch.full((3 * n * cells,), 253, dtype=torch.uint8, device=DEV),
            "smap": torch.full((n * cells,), 253, dtype=torch.uint8, device=DEV),
            "src": torch.full((n * cells + 1,), -77, dtype=torch.int32, device=DEV)}
    cam, bounds, inv_cell = _host(c)
    host_depth = np.ones(n * h * w, np.float32)
    good = dict(depth=d.data_ptr(), rgb=rgb.data_ptr(), seg=seg.data_ptr(), n=n, h=h, w=w, cam=cam.ctypes.data,
                bounds=bounds.ctypes.data, inv_cell=inv_cell, max_depth=c["max_depth"], out_h=out[0], out_w=out[1],
                **{k: v.data_ptr() for k, v in outs.items()})
    variants = []
    for k, val in ((2, np.nan), (4, np.inf), (0, bounds[3] + 1), (1, bounds[4] + 1), (2, bounds[5] + 1)):
        b = bounds.copy()
        b[k] = val
        variants.append(b)
    inf, nan = float("inf"), float("nan")
    bad = [dict(n=-1), dict(h=0), dict(w=0), dict(h=65536, w=32768), dict(out_h=0), dict(out_w=0), dict(out_h=4097),
           dict(out_w=4097), dict(inv_cell=0.0), dict(inv_cell=-1.0), dict(inv_cell=inf), dict(inv_cell=nan),
           dict(max_depth=0.0), dict(max_depth=-1.0), dict(max_depth=inf), dict(max_depth=nan),
           *[dict(bounds=b.ctypes.data) for b in variants], dict(bounds=None), dict(cam=None),
           dict(depth=None), dict(hmap=None), dict(depth=good["depth"] + 1), dict(depth=good["depth"] + 2),
           dict(hmap=good["hmap"] + 2), dict(src=good["src"] + 2), dict(depth=host_depth.ctypes.data),
           dict(rgb=None), dict(cmap=None), dict(seg=None), dict(smap=None)]

    def untouched(kw):
        assert (outs["hmap"] == -77.0).all() and (outs["src"] == -77).all(), kw
        assert (outs["cmap"] == 253).all() and (outs["smap"] == 253).all(), kw

    for kw in bad:
        rc = _raw({**good, **kw})
        assert rc == -1, (kw, rc)   # MRE_ERR_ARG
        assert L.lib().mre_last_error().startswith(b"mre_heightmap"), kw
        untouched(kw)
    assert _raw({**good, "n": 0}) == 0   # n = 0: MRE_OK, nothing launched
    untouched("n = 0")
    assert _raw(good) == 0               # and the good call writes every element it owns, and no other
    assert np.array_equal(_bits(outs["hmap"][:-1].cpu().numpy()), _bits(want[0].reshape(-1)))
    assert np.array_equal(outs["cmap"].cpu().numpy(), want[1].reshape(-1))
    assert np.array_equal(outs["smap"].cpu().numpy(), want[2].reshape(-1))
    assert np.array_equal(outs["src"][:-1].cpu().numpy(), want[3].reshape(-1))
    assert float(outs["hmap"][-1]) == -77.0 and int(outs["src"][-1]) == -77


def test_a_strided_view_and_a_cpu_tensor_go_through_the_wrapper_like_the_fallback():
    from mujoco_robot_environments_amd import perception as P
    shape, out = HC.SHAPES[3]
    c = HC.cases(shape, out)[0]
    h, w = shape[1] // 2, shape[2]
    pos, mat, fovy = HC.CAMERAS["overhead"]
    kw = dict(cam=HC.camera12(pos, mat, fovy, h, w), bounds=c["bounds"], cell=c["cell"])
    d, rgb, seg = (torch.from_numpy(c[k].copy()) for k in ("depth", "rgb", "seg"))
    ref = P.heightmap_reference(d[:, ::2], rgb[:, ::2], seg[:, ::2], **kw)
    assert (ref.src >= 0).sum() > 100
    view = d.to(DEV)[:, ::2]
    assert not view.is_contiguous()
    got = P.heightmap(view, rgb.to(DEV)[:, ::2], seg.to(DEV)[:, ::2], **kw)
    cpu = P.heightmap(d[:, ::2], rgb[:, ::2], seg[:, ::2], **kw)   # CPU tensors: the fallback
    for a in (got, cpu):
        assert torch.equal(a.height.cpu().view(torch.int32), ref.height.view(torch.int32))
        assert torch.equal(a.colour.cpu(), ref.colour) and torch.equal(a.seg.cpu(), ref.seg) and torch.equal(a.src.cpu(), ref.src)
    assert got.height.is_cuda and not cpu.height.is_cuda
    # the torch statement on the device is the statement too (what tools/bench_heightmap.py times the kernel against)
    dev_ref = P.heightmap_reference(d.to(DEV), rgb.to(DEV), seg.to(DEV), cam=c["cam"], bounds=c["bounds"], cell=c["cell"])
    want = HC.statement(c)
    assert np.array_equal(_bits(dev_ref.height.cpu().numpy()), _bits(want[0])) and np.array_equal(dev_ref.src.cpu().numpy(), want[3])


def test_env_heightmap_of_16_envs_after_reset():
    """env.heightmap() is the statement applied to the env's own render() output, exactly; every cube that the camera
    sees (>= 50 pixels) has cells of its own in the label map, and the highest of them is within one cell size -- the
    map's own resolution -- of the cube's highest corner."""
    from mujoco_robot_environments_amd import perception as P
    from mujoco_robot_environments_amd.model import compile as MC
    from mujoco_robot_environments_amd.tasks.rearrangement import (BatchedRearrangementEnv, HEIGHTMAP_BOUNDS, OVERHEAD,
                                                                   colour_separator_task_config)
    N, cell = 16, 0.0025
    env = BatchedRearrangementEnv(cfg=colour_separator_task_config(), num_envs=N, render=True)
    try:
        env.reset()
        rgb, depth, seg = env.render()
        hm = env.heightmap()
        assert hm.height.shape == (N, 320, 240) and hm.colour.shape == (N, 320, 240, 3) and hm.height.is_cuda
        cam = env._cameras[OVERHEAD]
        cam12 = HC.camera12(cam["pos"], cam["mat"], cam["fovy"], 480, 640)
        want = HC.numpy_heightmap(depth.cpu().numpy(), rgb.cpu().numpy(), seg.cpu().numpy(), cam12, HEIGHTMAP_BOUNDS, cell,
                                  99.0, (320, 240))
        _same(hm, want, True, True, "env.heightmap()")
        given = env.heightmap(depth, rgb, seg)
        assert torch.equal(given.height.view(torch.int32), hm.height.view(torch.int32)) and torch.equal(given.src, hm.src)
        assert (want[3] >= 0).mean() > 0.5
        visible = env.prop_labels(seg)["visible_pixels"]
        pose = env.physics.sites()[2].astype(np.float64)
        unit = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
        height, smap = want[0], want[2]
        checked = 0
        for i in range(N):
            for p in range(int(env.nprops[i])):
                if visible[i, p] < 50:
                    continue
                q = pose[i, p, 3:7]
                top = (pose[i, p, :3] + (unit * env.prop_half_size[i, p]) @ MC.q2m(q / np.linalg.norm(q)).T)[:, 2].max()
                own = smap[i] == 12 + p
                assert own.any(), (i, p)
                assert abs(float(height[i][own].max()) - (top - HEIGHTMAP_BOUNDS[0][2])) <= cell, (i, p, top)
                col, row = P.world_2_cell(pose[i, p, :3], HEIGHTMAP_BOUNDS, cell)
                assert 0 <= col < 240 and 0 <= row < 320
                checked += 1
        assert checked >= N
    finally:
        env.close()
