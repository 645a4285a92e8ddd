"""GPU tests of mre_heightmap_views (csrc/mre_heightmap_views.hip) against the fused numpy statement of
tests/heightmap_views_cases.py, EXACTLY: every bit of every output, no tolerance and no cell left out.  The shapes are
those of tests/test_gpu_heightmap.py with three views each -- one cell for every pixel of every view, a map smaller than a
tile, partial tiles, views of different size, mostly empty cells, hundreds of pixels per cell, and the sizes of the
reference's three cameras -- on ray-cast scenes and on salted depths; then the same view twice, a view that sees nothing,
one constant depth in two sizes, one view and eight; guards around every image, sentinels around every output, the
refusals, and a 16-env BatchedRearrangementEnv with the reference's two oblique cameras added.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import heightmap_cases as HC
from tests import heightmap_views_cases as VC

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _torch_views(case, device=DEV, rgb=True, seg=True):
    t = lambda a: torch.from_numpy(a.copy()).to(device)
    return [(t(v["depth"]), t(v["rgb"]) if rgb else None, t(v["seg"]) if seg else None, v["cam"]) for v in case["views"]]


def _kw(case):
    return dict(bounds=case["bounds"], cell=case["cell"], max_depth=case["max_depth"])


def _raw(a):
    """mre_heightmap_views on torch's current stream with the arguments of dict a: depth / rgb / seg lists of pointers (or
    None), height / width lists, cam float32 [views, 12], the rest as the entry takes them; the status."""
    from mujoco_robot_environments_amd import lib as L
    nv = a["views"]
    arr = lambda v: None if v is None else (C.c_void_p * len(v))(*v)
    depth, rgb, seg = arr(a["depth"]), arr(a["rgb"]), arr(a["seg"])
    height, width = np.asarray(a["height"], np.int32), np.asarray(a["width"], np.int32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.lib().mre_heightmap_views(stream, nv, depth, rgb, seg, a["n"], height.ctypes.data, width.ctypes.data, a["cam"],
                                     a["bounds"], a["inv_cell"], a["max_depth"], a["out_h"], a["out_w"], a["hmap"],
                                     a["cmap"], a["smap"], a["src"], a["view"])
    torch.cuda.synchronize()
    return rc


def _host(case):
    """cams, bounds as contiguous float32 arrays (kept alive by the caller) and inv_cell of a case."""
    lo, hi, inv_cell = HC.grid32(case["bounds"], case["cell"])
    cams = np.ascontiguousarray(np.stack([v["cam"] for v in case["views"]]), np.float32)
    return cams, np.ascontiguousarray(np.concatenate([lo, hi])), float(inv_cell)


def _raw_args(case, views, outs, cams, bounds, inv_cell):
    """The arguments of _raw for torch views [(depth, rgb, seg, cam)] and a dict of output pointers."""
    some = lambda k: None if views[0][k] is None else [v[k].data_ptr() for v in views]
    return dict(views=len(views), depth=some(0), rgb=some(1), seg=some(2), n=case["n"],
                height=[v[0].shape[1] for v in views], width=[v[0].shape[2] for v in views], cam=cams.ctypes.data,
                bounds=bounds.ctypes.data, inv_cell=inv_cell, max_depth=case["max_depth"], out_h=case["out"][0],
                out_w=case["out"][1], **outs)


def _same(r, want, rgb, seg, what):
    hmap, cmap, smap, src, view = want[:5]
    assert np.array_equal(_bits(r.height.cpu().numpy()), _bits(hmap)), what
    assert np.array_equal(r.src.cpu().numpy(), src), what
    assert np.array_equal(r.view.cpu().numpy(), view), what
    if rgb:
        assert np.array_equal(r.colour.cpu().numpy(), cmap), what
    else:
        assert r.colour is None
    if seg:
        assert np.array_equal(r.seg.cpu().numpy(), smap), what
    else:
        assert r.seg is None


@pytest.mark.parametrize("n,sizes,out", VC.SHAPES, ids=VC.IDS)
def test_kernel_matches_the_numpy_statement_exactly(n, sizes, out):
    from mujoco_robot_environments_amd import perception as P
    for i, c in enumerate(VC.cases(n, sizes, out)):
        want = VC.statement(c)
        views = _torch_views(c)
        a = P.heightmap_views(views, **_kw(c))
        assert a.height.is_cuda and a.height.shape == (n,) + out and a.view.dtype == torch.uint8
        _same(a, want, True, True, c["name"])
        # every case also with one of the other output combinations in turn
        with_rgb, with_seg = [(False, False), (True, False), (False, True)][(i + n) % 3]
        bare = [(d, rgb if with_rgb else None, seg if with_seg else None, cam) for d, rgb, seg, cam in views]
        _same(P.heightmap_views(bare, **_kw(c)), want, with_rgb, with_seg, c["name"])
        b = P.heightmap_views(views, **_kw(c))   # a second call on the same input: the same bytes
        assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))
        # without src, without view, without both, through the C ABI: the other outputs are the same
        cams, bounds, inv_cell = _host(c)
        for with_src, with_view in ((False, True), (True, False), (False, False)):
            hmap = torch.full((n,) + out, -77.0, dtype=torch.float32, device=DEV)
            smap = torch.full((n,) + out, 77, dtype=torch.uint8, device=DEV)
            src = torch.full((n,) + out, -77, dtype=torch.int32, device=DEV)
            view = torch.full((n,) + out, 77, dtype=torch.uint8, device=DEV)
            outs = dict(hmap=hmap.data_ptr(), cmap=None, smap=smap.data_ptr(), src=src.data_ptr() if with_src else None,
                        view=view.data_ptr() if with_view else None)
            assert _raw(_raw_args(c, [(d, None, seg, cam) for d, _, seg, cam in views], outs, cams, bounds, inv_cell)) == 0
            assert np.array_equal(_bits(hmap.cpu().numpy()), _bits(want[0])) and np.array_equal(smap.cpu().numpy(), want[2])
            assert np.array_equal(src.cpu().numpy(), want[3]) if with_src else bool((src == -77).all())
            assert np.array_equal(view.cpu().numpy(), want[4]) if with_view else bool((view == 77).all())


def test_the_further_cases():
    from mujoco_robot_environments_amd import perception as P
    for c in VC.further().values():
        _same(P.heightmap_views(_torch_views(c), **_kw(c)), VC.statement(c), True, True, c["name"])
    assert len(VC.further()["eight views"]["views"]) == 8 and len(VC.further()["one view"]["views"]) == 1


def test_one_view_equals_mre_heightmap_bit_for_bit():
    from mujoco_robot_environments_amd import perception as P
    for shape, out in (HC.SHAPES[2], HC.SHAPES[6], HC.SHAPES[4]):
        for c in HC.cases(shape, out):
            d, rgb, seg = (torch.from_numpy(c[k].copy()).to(DEV) for k in ("depth", "rgb", "seg"))
            kw = dict(bounds=c["bounds"], cell=c["cell"], max_depth=c["max_depth"])
            single = P.heightmap(d, rgb, seg, cam=c["cam"], **kw)
            fused = P.heightmap_views([(d, rgb, seg, c["cam"])], **kw)
            assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(single, fused[:4])), c["name"]
            assert torch.equal(fused.view, torch.where(single.src >= 0, 0, 255).to(torch.uint8)), c["name"]


def _guard_case():
    """Two straight-down views of different size and the overhead view on the 33 x 47 map, with for each the depth that,
    read as a pixel of that view, is a point higher than everything in the scene and inside the bounds."""
    n, sizes, out = VC.MID
    (h, w), big = sizes[0], (2 * sizes[0][0], 2 * sizes[0][1])
    down = [VC._single("straight down: scene", n, hh, ww, out) for hh, ww in ((h, w), big)]
    views = [VC._view_of(down[0]), VC._view_of(down[1]), VC.scene_view("overhead", n, h, w)]
    c = VC._case("guards", n, views, out)
    lo, hi, inv_cell = HC.grid32(c["bounds"], c["cell"])
    guards = [np.float32(np.float32(1.25) - hi[2]), np.float32(np.float32(1.25) - hi[2]), np.float32(1.3 - 0.68)]
    return c, guards


def test_images_between_guards_and_outputs_between_sentinels():
    """Every view's images sit one element into their allocations between guard regions whose depth would win its cells
    and show the guard's colour and label; the outputs sit inside sentinel-filled buffers at odd offsets, view at byte
    offsets 0, 1 and 3.  No guard may show in a result and no sentinel outside the outputs may change."""
    c, guards = _guard_case()
    n, out = c["n"], c["out"]
    cells = out[0] * out[1]
    lo, hi, inv_cell = HC.grid32(c["bounds"], c["cell"])
    capped = [dict(v, rgb=np.minimum(v["rgb"], 250), seg=np.minimum(v["seg"], 250)) for v in c["views"]]
    c = dict(c, views=capped)
    want = VC.merge([VC.single_statement(c, i) for i in range(3)])
    assert (want[3] >= 0).sum() > 500 and all((want[4] == i).any() for i in range(3))
    for v, g in zip(capped, guards):   # the guard depth is a valid point of its view, above everything in the fused map
        one = HC.numpy_points(np.full_like(v["depth"][:1], g), v["cam"], lo, hi, inv_cell, 99.0, out)
        assert one[3].any() and one[2][one[3]].min() > want[0].max()

    def guarded(src, fill, dtype, per):
        hw = src.shape[1] * src.shape[2]
        buf = torch.full(((n + 2) * hw * per + 2,), fill, dtype=dtype, device=DEV)
        view = buf[per * hw + 1: per * hw + 1 + n * hw * per]
        view.copy_(torch.from_numpy(src.copy()).to(DEV).reshape(-1))
        return buf, view

    bufs = [(guarded(v["depth"], float(g), torch.float32, 1), guarded(v["rgb"], 255, torch.uint8, 3),
             guarded(v["seg"], 254, torch.uint8, 1)) for v, g in zip(capped, guards)]
    cams, bounds, inv_cell = _host(c)
    for view_offset in (0, 1, 3):
        outs = {"hmap": torch.full((n * cells + 2,), -77.0, dtype=torch.float32, device=DEV),
                "cmap": torch.full((3 * n * cells + 2,), 253, dtype=torch.uint8, device=DEV),
                "smap": torch.full((n * cells + 2,), 253, dtype=torch.uint8, device=DEV),
                "src": torch.full((n * cells + 2,), -77, dtype=torch.int32, device=DEV),
                "view": torch.full((n * cells + 4,), 253, dtype=torch.uint8, device=DEV)}
        first = {"hmap": 1, "cmap": 1, "smap": 1, "src": 1, "view": view_offset}
        args = dict(views=3, depth=[b[0][1].data_ptr() for b in bufs], rgb=[b[1][1].data_ptr() for b in bufs],
                    seg=[b[2][1].data_ptr() for b in bufs], n=n, height=[v["depth"].shape[1] for v in capped],
                    width=[v["depth"].shape[2] for v in capped], cam=cams.ctypes.data, bounds=bounds.ctypes.data,
                    inv_cell=inv_cell, max_depth=c["max_depth"], out_h=out[0], out_w=out[1],
                    **{k: v[first[k]:].data_ptr() for k, v in outs.items()})
        assert _raw(args) == 0
        for k, wanted in zip(("hmap", "cmap", "smap", "src", "view"), want):
            got = outs[k].cpu().numpy()
            body = got[first[k]: first[k] + wanted.size]
            as_bits = lambda x: x.view(np.uint32) if k == "hmap" else x
            assert np.array_equal(as_bits(body), as_bits(np.ascontiguousarray(wanted).reshape(-1))), (k, view_offset)
            rest = np.concatenate([got[:first[k]], got[first[k] + wanted.size:]])
            assert len(rest) >= 2 and (rest == (-77 if k in ("hmap", "src") else 253)).all(), (k, view_offset)
    assert not (want[1] == 255).any() and not (want[2] == 254).any()   # so a guard's colour or label would have shown
    for (dbuf, dview), _, _ in bufs:
        edge = (len(dbuf) - len(dview) - 2) // 2 + 1
        assert (dbuf[:edge] == dbuf[0]).all() and (dbuf[edge + len(dview):] == dbuf[0]).all()


def test_bad_arguments_return_err_arg_and_write_nothing():
    from mujoco_robot_environments_amd import lib as L
    n, sizes, out = VC.SHAPES[3]   # views of different size
    c = VC.cases(n, sizes, out)[0]
    want = VC.statement(c)
    views = _torch_views(c)
    d0 = torch.cat([views[0][0].reshape(-1), torch.ones(1, device=DEV)])   # one float of room for the misaligned variants
    views[0] = (d0[:-1].view(views[0][0].shape),) + views[0][1:]
    cells = out[0] * out[1]
    outs = {"hmap": torch.full((n * cells + 1,), -77.0, dtype=torch.float32, device=DEV),
            "cmap": torch.full((3 * n * cells,), 253, dtype=torch.uint8, device=DEV),
            "smap": torch.full((n * cells,), 253, dtype=torch.uint8, device=DEV),
            "src": torch.full((n * cells + 1,), -77, dtype=torch.int32, device=DEV),
            "view": torch.full((n * cells,), 253, dtype=torch.uint8, device=DEV)}
    cams, bounds, inv_cell = _host(c)
    good = _raw_args(c, views, {k: v.data_ptr() for k, v in outs.items()}, cams, bounds, inv_cell)
    host = np.ones(n * 48 * 64 * 3, np.float32)
    variants = []
    for k, val in ((2, np.nan), (4, np.inf), (0, bounds[3] + 1), (1, bounds[4] + 1), (2, bounds[5] + 1)):
        b = bounds.copy()
        b[k] = val
        variants.append(b)
    inf, nan = float("inf"), float("nan")
    swap = lambda key, i, val: {key: [val if j == i else p for j, p in enumerate(good[key])]}
    bad = [dict(views=0), dict(views=9), dict(n=-1), swap("height", 1, 0), swap("width", 2, 0),
           {**swap("height", 1, 16384), **swap("width", 1, 16384)}, dict(out_h=0), dict(out_w=0), dict(out_h=4097),
           dict(out_w=4097), dict(inv_cell=0.0), dict(inv_cell=-1.0), dict(inv_cell=inf), dict(inv_cell=nan),
           dict(max_depth=0.0), dict(max_depth=-1.0), dict(max_depth=inf), dict(max_depth=nan),
           *[dict(bounds=b.ctypes.data) for b in variants], dict(bounds=None), dict(cam=None), dict(depth=None),
           swap("depth", 1, None), dict(hmap=None), swap("depth", 0, good["depth"][0] + 1), swap("depth", 0, good["depth"][0] + 2),
           dict(hmap=good["hmap"] + 2), dict(src=good["src"] + 2), swap("depth", 2, host.ctypes.data),
           swap("rgb", 1, host.ctypes.data), swap("seg", 0, host.ctypes.data), dict(view=host.ctypes.data),
           dict(hmap=host.ctypes.data), dict(rgb=None), dict(cmap=None), dict(seg=None), dict(smap=None),
           swap("rgb", 2, None), swap("seg", 1, None)]

    def untouched(kw):
        assert (outs["hmap"] == -77.0).all() and (outs["src"] == -77).all(), kw
        assert (outs["cmap"] == 253).all() and (outs["smap"] == 253).all() and (outs["view"] == 253).all(), kw

    for kw in bad:
        rc = _raw({**good, **kw})
        assert rc == -1, (kw, rc)   # MRE_ERR_ARG
        assert L.lib().mre_last_error().startswith(b"mre_heightmap_views"), kw
        untouched(kw)
    assert _raw({**good, "n": 0}) == 0   # n = 0: MRE_OK, nothing launched
    untouched("n = 0")
    assert _raw(good) == 0               # and the good call writes every element it owns, and no other
    assert np.array_equal(_bits(outs["hmap"][:-1].cpu().numpy()), _bits(want[0].reshape(-1)))
    assert np.array_equal(outs["cmap"].cpu().numpy(), want[1].reshape(-1))
    assert np.array_equal(outs["smap"].cpu().numpy(), want[2].reshape(-1))
    assert np.array_equal(outs["src"][:-1].cpu().numpy(), want[3].reshape(-1))
    assert np.array_equal(outs["view"].cpu().numpy(), want[4].reshape(-1))
    assert float(outs["hmap"][-1]) == -77.0 and int(outs["src"][-1]) == -77


def test_a_strided_view_and_mixed_devices_give_what_the_reference_gives(monkeypatch):
    from mujoco_robot_environments_amd import perception as P
    n, sizes, out = VC.SHAPES[4]
    c = VC.cases(n, sizes, out)[0]
    h, w = sizes[0][0] // 2, sizes[0][1]
    cpu = _torch_views(c, device="cpu")
    cams = [HC.camera12(*HC.CAMERAS[name][:2], HC.fovy_for(HC.CAMERAS[name][2], h, w), h, w) for name in VC.NAMES]
    halves = lambda vs: [(d[:, ::2], rgb[:, ::2], seg[:, ::2], cam) for (d, rgb, seg, _), cam in zip(vs, cams)]
    ref = P.heightmap_views_reference(halves(cpu), **_kw(c))
    assert (ref.src >= 0).sum() > 100 and len(torch.unique(ref.view)) == 4
    called = []
    inner = P.heightmap_views_reference
    monkeypatch.setattr(P, "heightmap_views_reference", lambda *a, **k: called.append(1) or inner(*a, **k))
    on = halves(_torch_views(c))
    assert not on[0][0].is_contiguous()
    got = P.heightmap_views(on, **_kw(c))                 # strided views on the device: made contiguous, one launch
    assert got.height.is_cuda and not called
    mixed = P.heightmap_views([on[0], halves(cpu)[1], on[2]], **_kw(c))   # mixed devices: the reference, on view 0's device
    assert mixed.height.is_cuda and called == [1]
    on_cpu = P.heightmap_views(halves(cpu), **_kw(c))     # CPU tensors: the reference
    assert not on_cpu.height.is_cuda and called == [1, 1]
    for a in (got, mixed, on_cpu):
        assert all(torch.equal(x.cpu().view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, ref))
    # the composition on the device is the statement too (what tools/bench_heightmap_views.py times the kernel against)
    _same(inner(_torch_views(c), **_kw(c)), VC.statement(c), True, True, "composition on the device")


@pytest.fixture(scope="module")
def env():
    from mujoco_robot_environments_amd import config
    from mujoco_robot_environments_amd.tasks.rearrangement import BatchedRearrangementEnv, OVERHEAD, colour_separator_task_config
    e = BatchedRearrangementEnv(cfg=colour_separator_task_config(), num_envs=16, render=True)
    try:
        e.reset()
        obliques = config.compose(overrides=["arena/cameras=rearrangement", "arena/props=colour_splitter"]).arena.cameras
        e.cameras = [OVERHEAD] + [e.add_camera(c.name, c.pos, c.quat, c.fovy, c.height, c.width) for c in obliques]
        yield e
    finally:
        e.close()


def test_env_views_of_16_envs_after_reset(env):
    """render_views gives every camera at its configured size, heightmap_views is the statement on those renders, and the
    fused maps hold everything the overhead-only maps hold, at least as high."""
    from mujoco_robot_environments_amd import perception as P
    from mujoco_robot_environments_amd.tasks.rearrangement import HEIGHTMAP_BOUNDS
    N, cell, out = 16, 0.0025, (320, 240)
    assert env.cameras == ["overhead_camera/overhead_camera", "front_camera/front_camera", "left_camera/left_camera"]
    with pytest.raises(ValueError):
        env.add_camera("front_camera", [0, 0, 1], [1, 0, 0, 0], 60.0, 4, 4)
    frames = env.render_views(env.cameras)
    sizes = [(480, 640), (640, 640), (640, 640)]
    for (rgb, depth, seg), (h, w) in zip(frames, sizes):
        assert rgb.shape == (N, h, w, 3) and depth.shape == (N, h, w) and seg.shape == (N, h, w) and depth.is_cuda
    plain = env.render()
    assert all(torch.equal(a, b) for a, b in zip(plain, frames[0]))          # the overhead view is render()'s
    assert env.render(camera=env.cameras[1])[1].shape == (N, 480, 640)      # render() keeps the overhead size
    fused = env.heightmap_views(env.cameras, frames)
    assert isinstance(fused, P.FusedHeightMap) and fused.height.shape == (N,) + out and fused.height.is_cuda
    singles = []
    for name, (rgb, depth, seg), (h, w) in zip(env.cameras, frames, sizes):
        cam = env._cameras[name]
        assert (cam["height"], cam["width"]) == (h, w)
        singles.append(HC.numpy_heightmap(depth.cpu().numpy(), rgb.cpu().numpy(), seg.cpu().numpy(),
                                          HC.camera12(cam["pos"], cam["mat"], cam["fovy"], h, w), HEIGHTMAP_BOUNDS, cell, 99.0, out))
    want = VC.merge(singles)
    _same(fused, want, True, True, "env.heightmap_views()")
    own = env.heightmap_views(env.cameras)   # renders for itself: the same state, the same maps
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(own, fused))
    over = env.heightmap()
    had = (over.src >= 0)
    assert bool((fused.src >= 0)[had].all()) and bool((fused.height[had] >= over.height[had]).all())
    assert int((fused.src >= 0).sum()) >= int(had.sum()) and all(bool((fused.view == k).any()) for k in range(3))


def test_transporter_batch_and_act_on_fused_maps(env):
    from mujoco_robot_environments_amd import perception as P
    from mujoco_robot_environments_amd.tasks.rearrangement import HEIGHTMAP_BOUNDS
    cell = 0.0025
    fused = env.heightmap_views(env.cameras)
    _, pick, place = env.sort_colours(peek=True)
    cells = [P.world_2_cell(p[:, :3], HEIGHTMAP_BOUNDS, cell) for p in (pick, place)]
    kw = dict(seed=5, env_ids=env.env_ids, draw=2, n_rotations=4, crop=16, channels=P.CHANNELS_RGBH, dtype=torch.bfloat16)

    def same_batch(a, b):
        for x, y in zip(a, b):
            if isinstance(x, torch.Tensor):
                assert torch.equal(x.view(torch.int16) if x.dtype == torch.bfloat16 else x, y.view(torch.int16) if y.dtype == torch.bfloat16 else y)
            else:
                assert np.array_equal(np.asarray(x), np.asarray(y))

    same_batch(env.transporter_batch(5, draw=2, n_rotations=4, crop=16, maps=fused), P.transporter_batch(fused, *cells, **kw))
    same_batch(env.transporter_batch(5, draw=2, n_rotations=4, crop=16), P.transporter_batch(env.heightmap(), *cells, **kw))
    sample = env.transporter_sample(5, draw=2, n_rotations=4, crop=16, maps=fused)
    want = P.transporter_sample(fused, *cells, seed=5, env_ids=env.env_ids, draw=2, n_rotations=4, crop=16)
    assert torch.equal(sample.maps.height.view(torch.int32), want.maps.height.view(torch.int32))
    assert torch.equal(sample.crops.height.view(torch.int32), want.crops.height.view(torch.int32))
    # acting on the fused maps: a one-hot attention at the demonstrator's pick cell, identity key and query
    rows, cols = fused.height.shape[1:]
    seen = {}

    def attention(scene):
        seen["scene"] = scene
        x = torch.zeros((len(cells[0]), 1, rows, cols), dtype=torch.bfloat16, device=DEV)
        x[torch.arange(len(cells[0])), 0, torch.as_tensor(cells[0][:, 1]), torch.as_tensor(cells[0][:, 0])] = 1.0
        return x

    take_height = lambda x: x[:, 3:4].contiguous()
    pick_pose, place_pose, picked, placed = env.transporter_act(attention, take_height, take_height, channels=P.CHANNELS_RGBH,
                                                                dtype=torch.bfloat16, n_rotations=4, crop=16, maps=fused)
    identity = torch.tensor([1, 0, 0, 0, 1, 0], dtype=torch.float32, device=DEV).repeat(env.num_envs, 1)
    assert torch.equal(seen["scene"].view(torch.int16), P.warp_inputs(fused.height, fused.colour, mats=identity, channels=P.CHANNELS_RGBH,
                                                                      dtype=torch.bfloat16).view(torch.int16))
    assert np.array_equal(picked.cells.cpu().numpy(), cells[0])
    assert pick_pose.shape == place_pose.shape == (env.num_envs, 7) and np.isfinite(pick_pose).all() and np.isfinite(place_pose).all()
    assert np.allclose(np.linalg.norm(place_pose[:, 3:], axis=1), 1.0)
    env.step({"pose": pick_pose})
    env.step({"pose": place_pose})
    assert env.mode == "pick"


def test_the_heightmaps_example_runs_with_views_at_16_envs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "transporter_heightmaps.py"), "--num-envs", "16", "--views"],
                         cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "3 views fused" in out.stdout and out.stdout.count("cells alone") == 3, out.stdout
