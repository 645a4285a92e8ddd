"""GPU tests of the frame labels on rendered frames and of the batched perception calls of BatchedRearrangementEnv
(prop_bboxes / prop_labels / props_info / pixel_2_world_batch) against their per-env forms."""
import numpy as np
import pytest

from tests import labels_cases as LC

pytestmark = pytest.mark.gpu

H, W = 480, 640


def parent_prop_bboxes(seg):
    """prop_bboxes as it was before the labels kernel: ~40 torch launches over [N, H, W] masks."""
    import torch
    n, h, w = seg.shape
    out = torch.full((n, 4, 4), -1, dtype=torch.int64, device=seg.device)
    for p in range(4):
        m = seg == (12 + p)
        cols, rows = m.any(dim=1), m.any(dim=2)
        vis = cols.any(dim=1)
        box = torch.stack([cols.int().argmax(dim=1), rows.int().argmax(dim=1),
                           w - 1 - cols.flip(1).int().argmax(dim=1), h - 1 - rows.flip(1).int().argmax(dim=1)], dim=1)
        out[:, p] = torch.where(vis[:, None], box, out[:, p])
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def frames():
    """8 bench scenes, the arm of env 1 moved over the table; one render, one numpy statement."""
    import bench
    from mujoco_robot_environments_amd.tasks.rearrangement import BatchedRearrangementEnv, colour_separator_task_config
    N = 8
    env = BatchedRearrangementEnv(cfg=colour_separator_task_config(), num_envs=N, render=True)
    nprops, sizes = bench.setup_envs(env.physics, 0, np.arange(N))
    env.nprops = np.asarray(nprops, np.int32)
    qp = env.physics.qpos().copy()
    qp[1, :7] = [0.3, 0.4, 0.0, -1.6, 0.0, 2.0, 0.8]
    env.physics.set_state(qp, env.physics.qvel())
    _, depth, seg = env.render(rgb=False)
    seg_np, depth_np = seg.cpu().numpy(), depth.cpu().numpy()
    assert seg_np.shape == (N, H, W)
    yield env, seg, depth, seg_np, depth_np, LC.numpy_labels(seg_np, depth_np, 12, 4)
    env.close()


def test_labels_of_rendered_frames_match_the_numpy_statement_exactly(frames):
    from mujoco_robot_environments_amd import perception as P
    env, seg, depth, seg_np, depth_np, (stats, zmin) = frames
    lab = P.seg_labels(seg, depth)
    assert np.array_equal(lab.box.cpu().numpy(), stats[..., :4])
    assert np.array_equal(lab.count.cpu().numpy(), stats[..., 4])
    assert np.array_equal(lab.sum_xy.cpu().numpy(), stats[..., 5:7])
    assert np.array_equal(lab.zmin.cpu().numpy().view(np.uint32), zmin.view(np.uint32))
    assert np.isfinite(depth_np).all() and (depth_np >= 0).all()   # what the kernel's zmin relies on
    assert ((seg_np[1] >= 2) & (seg_np[1] <= 11)).sum() > 500       # robot hulls are in view in env 1


def test_prop_bboxes_equal_the_parent_formula_and_labels_say_what_is_visible(frames):
    env, seg, depth, seg_np, depth_np, (stats, zmin) = frames
    want = parent_prop_bboxes(seg)
    for boxes in (env.prop_bboxes(), env.prop_bboxes(seg)):
        assert boxes.dtype == np.int64 and boxes.shape == (8, 4, 4) and np.array_equal(boxes, want)
    out = env.prop_labels()
    assert np.array_equal(out["bbox"], want) and np.array_equal(out["visible_pixels"], stats[..., 4])
    assert np.array_equal(out["nearest_depth"].view(np.uint32), zmin.view(np.uint32))
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(out["centroid"], stats[..., 5:7] / stats[..., 4:5].astype(np.float64), equal_nan=True)
    in_use = np.arange(4)[None, :] < env.nprops[:, None]
    assert in_use.sum() >= 16 and (~in_use).any()
    home = np.arange(8) != 1
    assert (out["visible_pixels"][home][in_use[home]] > 0).all()
    assert (out["visible_pixels"][~in_use] == 0).all() and (out["bbox"][~in_use] == -1).all()
    assert np.isinf(out["nearest_depth"][~in_use]).all() and np.isnan(out["centroid"][~in_use]).all()
    # the nearest depth of a visible cube is its top face: above the table, below the camera
    vis = out["visible_pixels"] > 0
    assert (out["nearest_depth"][vis] > 0.3).all() and (out["nearest_depth"][vis] < 1.3 - 0.4).all()


@pytest.fixture(scope="module")
def env4():
    from mujoco_robot_environments_amd.tasks.rearrangement import BatchedRearrangementEnv, colour_separator_task_config
    env = BatchedRearrangementEnv(cfg=colour_separator_task_config(), num_envs=4, render=True)
    env.reset()
    yield env
    env.close()


def test_props_info_agrees_with_props_info_env(env4):
    env = env4
    qp = env.physics.qpos().copy()
    saved = qp.copy()
    qp[0, 15:18] = [3.0, 3.0, 0.45]   # cube 0 of env 0 out of the camera's view: the scalar call's bbox is empty
    env.physics.set_state(qp, env.physics.qvel())
    try:
        for render in (True, False):
            env.render_observations = render
            info = env.props_info()
            assert info["position"].shape == (4, 4, 3) and info["orientation"].shape == (4, 4, 4)
            assert info["rgba"].shape == (4, 4, 4) and info["bbox"].shape == (4, 4, 4) and info["in_use"].shape == (4, 4)
            assert info["bbox"].dtype == np.int64 and info["visible_pixels"].shape == (4, 4)
            assert np.array_equal(info["in_use"], np.arange(4)[None, :] < env.nprops[:, None])
            empties = 0
            for i in range(4):
                one = env.props_info_env(i)
                assert sorted(one) == [12 + p for p in range(int(env.nprops[i]))]
                for p in range(int(env.nprops[i])):
                    a = one[12 + p]
                    assert np.abs(info["position"][i, p] - a["position"]).max() <= 1e-12
                    assert np.abs(info["orientation"][i, p] - a["orientation"]).max() <= 1e-12
                    assert np.array_equal(info["rgba"][i, p], a["rgba"])
                    if len(a["bbox"]) == 0:
                        empties += 1
                        assert (info["bbox"][i, p] == -1).all() and info["visible_pixels"][i, p] == 0
                    else:
                        assert np.array_equal(info["bbox"][i, p], a["bbox"])
                        assert not render or info["visible_pixels"][i, p] > 0
            assert empties == (1 if render else 0)
            assert (info["bbox"][~info["in_use"]] == -1).all()
            assert np.isnan(info["position"][~info["in_use"]]).all()
    finally:
        env.render_observations = True
        env.physics.set_state(saved, env.physics.qvel())


def test_pixel_2_world_batch_rows_equal_the_scalar_call(env4):
    from mujoco_robot_environments_amd.tasks.rearrangement import OVERHEAD
    env = env4
    _, depth, seg = env.render(rgb=False)
    lab = env.prop_labels(seg, depth)
    assert (lab["visible_pixels"][:, 0] > 0).all()
    seg_np = seg.cpu().numpy()
    table = np.array([np.argwhere(seg_np[i] == 1)[1000 + 37 * i][::-1] for i in range(4)], np.float64)   # (x, y)
    cases = [lab["centroid"][:, 0], table, np.tile([W - 1.0, H - 1.0], (4, 1))]
    try:
        for render in (True, False):
            env.render_observations = render
            for coords in cases:
                got = env.pixel_2_world_batch(OVERHEAD, coords)
                assert got.shape == (4, 3) and got.dtype == np.float64
                for i in range(4):
                    assert np.abs(got[i] - env.pixel_2_world(OVERHEAD, coords[i], env=i)).max() <= 1e-12
                if render:   # the caller's depth image instead of a render
                    assert np.array_equal(env.pixel_2_world_batch(OVERHEAD, coords, depth=depth), got)
            bad = cases[1].copy()
            bad[2, 0] = W
            with pytest.raises(ValueError):
                env.pixel_2_world_batch(OVERHEAD, bad)
        # a cube's centroid pixel goes back to the cube: it lies inside the silhouette, so the point is on the cube's
        # surface -- within its half diagonal (0.016 * sqrt(3) < 0.03) of the centre
        env.render_observations = True
        centre = env.physics.sites()[2][:, 0, :3].astype(np.float64)
        back = env.pixel_2_world_batch(OVERHEAD, cases[0], depth=depth)
        assert np.abs(back - centre).max() < 0.03, (back, centre)
    finally:
        env.render_observations = True
