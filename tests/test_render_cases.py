"""The camera cases (tests/render_cases.py) judged on the CPU, from the oracle's output alone: every case stays within the
caps of fragile pixels, every probe pixel shows the geom it was aimed at and is not fragile, and every family has the
property it was built for."""
import numpy as np
import pytest

from tests import render_cases as RC


def _has(seg, ids):
    return np.isin(seg, list(ids)).any()


@pytest.mark.parametrize("name", RC.NAMES)
def test_fragile_shares_are_within_the_caps_and_probes_hold(name):
    c = RC.case(name)
    seg_share, rgb_share = RC.fragile_shares(name)
    print(f"{name}: {c.N} x {c.height}x{c.width}, seg-fragile {100 * seg_share:.2f} %, rgb-fragile off the ground {100 * rgb_share:.2f} %")
    assert seg_share <= RC.SEG_CAP and rgb_share <= RC.RGB_CAP
    assert 1 <= c.N <= 4 and c.width % 4 == 0
    if c.family == "A":
        assert c.probes
    im = RC.oracle_images(name)
    for env, v, u, g in c.probes:
        rgb, depth, seg, sf, rf = im[env]
        assert seg[v, u] == g, (env, v, u, g, seg[v, u])
        assert not rf[v, u], (env, v, u)
    level = np.array_equal(c.cam_mat[2], [0.0, 1.0, 0.0])      # optical axis exactly horizontal, no roll: d2 = y, no cancellation
    for i in range(c.N):
        rgb, depth, seg, sf, rf = im[i]
        assert RC.depth_ties(c, i) == 0, (i, RC.depth_ties(c, i))      # no two faces in one plane on a judged pixel
        if (seg == 0).any() and not level:     # the ground's depth bar needs d2 = h / depth >= GROUND_D2_MIN (render_cases.py)
            assert c.cam_pos[2] / depth[seg == 0].max() >= RC.GROUND_D2_MIN, c.cam_pos[2] / depth[seg == 0].max()
        # cube slots that are not in use never show
        assert not _has(seg, range(RC.PROP_GEOM0 + int(c.nprops[i]), RC.PROP_GEOM0 + 4))


def test_every_shape_has_its_cases_and_probes():
    assert len(RC.NAMES) == len(set(RC.NAMES)) and set(RC.NAMES) == set(RC._all())
    for W, H in RC.SHAPES:
        probes = RC.shape_probes(H, W)
        assert probes[0] == (0, 0) and all(0 <= u < W and 0 <= v < H for u, v in probes)
        assert (W <= 768) or any(u >= 768 for u, v in probes)
        if (W, H) == (800, 600):
            assert [p[2] for p in RC.case("A-800x600-natural").probes] == [785]
            continue
        marked = {(v, u) for _, v, u, _ in RC.case(f"A-{W}x{H}-cubes").probes}
        assert marked == {(v, u) for u, v in probes}
        hull = RC.case(f"A-{W}x{H}-hull").probes[0]
        assert hull[3] in RC.LINK_HULLS and (hull[2], hull[1]) == probes[-1]


def test_aim_camera_inverts_the_pinhole_model():
    r = np.random.default_rng(0)
    for _ in range(20):
        H, W = int(r.integers(1, 200)), 4 * int(r.integers(1, 300))
        fovy, Rc = r.uniform(5, 120), RC.overhead_mat(r.uniform(0, 360))
        X, pix, depth = r.uniform(-1, 1, 3), (r.uniform(0, W - 1), r.uniform(0, H - 1)), r.uniform(0.2, 2)
        cam = RC.aim_camera(X, pix, depth, Rc, fovy, H, W)
        u, v, d = RC.world_to_pixel(X, cam, Rc, fovy, H, W)
        assert abs(u - pix[0]) < 1e-3 and abs(v - pix[1]) < 1e-3 and abs(d - depth) < 1e-6


@pytest.mark.parametrize("size", RC.CAMERA_SIZES)
def test_camera_family_properties(size):
    H, W = size
    t = f"{H}x{W}"
    # side: ground, table, hulls, cubes and sky
    seg = RC.oracle_images(f"B-side-{t}")[0][2]
    assert _has(seg, [0]) and _has(seg, [1]) and _has(seg, RC.HULLS_LOW + RC.LINK_HULLS) and _has(seg, range(12, 16)) and _has(seg, [255])
    print(f"B-side-{t}: ground {100 * (seg == 0).mean():.1f} %, sky {100 * (seg == 255).mean():.1f} %")
    # level: the optical axis is exactly horizontal, only side faces of the cubes are entered, both signs of both axes
    c = RC.case(f"B-level-{t}")
    assert np.array_equal(c.cam_mat[2], [0.0, 1.0, 0.0])
    faces = set()
    for g in range(12, 16):
        pos, mat, size_, typ = RC.geoms_of(c, 0)
        assert abs(((c.cam_pos - pos[g]) @ mat[g])[2]) <= size_[g][2]
        faces |= RC.entry_faces(c, 0, g)
    assert faces == {(0, 1), (0, -1), (1, 1), (1, -1)}, faces
    # rolled: 37 degrees about the optical axis of the reference camera
    c = RC.case(f"B-rolled37-{t}")
    R0 = RC.overhead_mat()
    assert np.allclose(c.cam_mat[:, 2], R0[:, 2]) and abs(np.rad2deg(np.arccos(c.cam_mat[:, 0] @ R0[:, 0])) - 37) < 1e-4
    # fovy
    assert RC.case(f"B-fovy10-{t}").fovy == 10.0 and RC.case(f"B-fovy120-{t}").fovy == 120.0
    assert _has(RC.oracle_images(f"B-fovy10-{t}")[0][2], [12]) and _has(RC.oracle_images(f"B-fovy120-{t}")[0][2], [0])
    # near: a corner of a hull that is in the image lies behind the near plane (the whole-screen rectangle branch)
    c = RC.case(f"B-near-{t}")
    seg = RC.oracle_images(c.name)[0][2]
    pos, mat, size_, typ = RC.geoms_of(c, 0)
    sg = np.array([[a, b, d] for a in (-1, 1) for b in (-1, 1) for d in (-1, 1)], float)
    behind = [g for g in RC.HULLS_LOW + RC.LINK_HULLS
              if (((pos[g] + (sg * size_[g]) @ mat[g].T - c.cam_pos) @ c.cam_mat)[:, 2] > -RC.NEAR).any() and (seg == g).any()]
    print(f"B-near-{t}: visible hulls with a corner behind the near plane: {behind}")
    assert behind
    # slab: inside exactly one slab of the cube, and the cube is seen
    c = RC.case(f"B-slab-{t}")
    pos, mat, size_, typ = RC.geoms_of(c, 0)
    g = c.meta["slab_geom"]
    inside = np.abs((c.cam_pos - pos[g]) @ mat[g]) <= size_[g]
    assert inside.sum() == 1 and (RC.oracle_images(c.name)[0][2] == g).any()
    # inside: within all three slabs of the hull, which then is not in the image while other geoms are
    c = RC.case(f"B-inside-{t}")
    pos, mat, size_, typ = RC.geoms_of(c, 0)
    g = c.meta["inside_geom"]
    seg = RC.oracle_images(c.name)[0][2]
    assert (np.abs((c.cam_pos - pos[g]) @ mat[g]) < size_[g] - RC.NEAR).all() and not (seg == g).any() and _has(seg, range(2, 16))


def _count(name, env, g):
    return int((RC.oracle_images(name)[env][2] == g).sum())


def test_scene_family_properties():
    from oracle import render_oracle as RO
    A = RC.model()
    # tumbling: no cube axis within 5 degrees of vertical, every cube seen from above
    c = RC.case("C-tumbling-top")
    for i in range(c.N):
        pos, mat, size, typ = RC.geoms_of(c, i)
        for g in range(12, 16):
            assert np.abs(mat[g][2]).max() < np.cos(np.deg2rad(5)) and _count(c.name, i, g) > 0
    # occluded: cube 0 shows fewer pixels than with cube 1 parked, cube 1 shows
    for view in ("top", "side"):
        c = RC.case(f"C-occluded-{view}")
        for env, v in c.meta["occluded"]:
            if v != view:
                continue
            alone = RO.render(A, c.qpos[env].astype(np.float64), 1, c.sizes[env], c.prop_rgb[env], c.geom_rgb.astype(np.float64),
                              c.cam_pos, c.cam_mat, c.fovy, c.height, c.width)[2]
            n0, n1, na = _count(c.name, env, 12), _count(c.name, env, 13), int((alone == 12).sum())
            print(f"{c.name} env {env}: cube 0 shows {n0} of {na} pixels, cube 1 {n1}")
            assert 0 < n0 < na and n1 > 0
    # under the hull: from above cube 0 shows, but fewer pixels than with the arm at home
    c = RC.case("C-under-hull-top")
    q = c.qpos[0].astype(np.float64)
    q[:7] = A["home_qpos"]
    free = RO.render(A, q, 4, c.sizes[0], c.prop_rgb[0], c.geom_rgb.astype(np.float64), c.cam_pos, c.cam_mat, c.fovy, c.height, c.width)[2]
    n0, nf = _count(c.name, 0, 12), int((free == 12).sum())
    print(f"C-under-hull-top: cube 0 shows {n0} of {nf} pixels")
    assert 0 < n0 < nf
    # nprops: the unused cubes lie in view (they show once they are in use) and are not drawn
    for view in ("top", "side"):
        c = RC.case(f"C-nprops-{view}")
        assert c.nprops.tolist() == [2, 3]
        for env, ids in c.meta["unused"].items():
            full = RO.render(A, c.qpos[env].astype(np.float64), 4, c.sizes[env], c.prop_rgb[env], c.geom_rgb.astype(np.float64),
                             c.cam_pos, c.cam_mat, c.fovy, c.height, c.width)[2]
            for g in ids:
                assert (full == g).any() and _count(c.name, env, g) == 0
    # sizes: no two axes alike; colours: differ between envs
    s = RC.case("C-sizes-top").sizes
    assert (np.abs(s[..., 0] - s[..., 1]) > 1e-4).all() and (np.abs(s[..., 1] - s[..., 2]) > 1e-4).all() and s.min() >= 0.008
    p = RC.case("C-colours-top").prop_rgb
    assert not np.array_equal(p[0], p[1]) and not np.array_equal(p[1], p[2])
    a, b = RC.oracle_images("C-colours-top")[0], RC.oracle_images("C-colours-top")[1]
    assert np.array_equal(a[2], b[2]) and not np.array_equal(a[0], b[0])
