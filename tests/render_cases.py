"""Cases for the batched camera (csrc/mre_render.hip, mre_render) and the rule a device image is compared with the
oracle's by.  A plain module: everything here runs on the CPU and uses the oracle only
(tests/test_render_cases.py judges the cases, tests/test_gpu_render_cases.py runs them on the device).

A case is a zero-step render: 1..4 envs whose state is written with set_state (qpos rows in float32, nothing is
ever stepped), one camera, one image shape.  The oracle is given the same float32 values widened to double.

Fragile pixels are judged by the oracle alone: the case is rendered again with every ray moved by (+-0.02, +-0.02)
pixel (four renders).  0.02 px is about 5e-5 rad: far above the float32 error of a ray (1e-7), far below a pixel,
so it marks silhouettes and checker edges and nothing else.
  seg-fragile   one of the four changes the pixel's geom id
  rgb-fragile   seg-fragile, or one of the four moves a colour channel by more than 1
Caps (conditions on the cases, not measurements): seg-fragile <= 2 % of a case's pixels, rgb-fragile pixels that are
not ground <= 2 %, no probe pixel fragile.  Ground is exempt from the second cap: the checker near the horizon
is fragile by nature.

Comparison (the bars of tests/test_gpu_render.py, on every pixel that is not fragile):
  seg    equal on every pixel that is not seg-fragile
  depth  |d - d_oracle| <= 2e-5 * max(1, d_oracle) wherever seg agrees; sky holds exactly 100 and id 255
  rgb    |delta| <= 3 on every pixel that is not rgb-fragile (pooled over all cases: <= 1 on 99.99 %); sky pixels
         equal the oracle's tint bytes

A pitched camera computes the ground's ray component d2 = G6 x + G7 y - G8 from terms of magnitude ~0.5, so its float32
error is ABSOLUTE, about 1e-7, and the ground depth h / d2 carries 1e-7 / d2 of relative error: every case keeps
d2 >= 0.02 on its ground pixels (GROUND_D2_MIN, checked by the CPU test), five times inside the bar.  The one exception is
the camera whose optical axis is exactly horizontal: G6 = G8 = 0, G7 = 1, no cancellation, the error stays relative.
Two faces in one plane are the other thing no float32 kernel can be held to: see depth_ties.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

OFFSETS = ((0.02, 0.02), (0.02, -0.02), (-0.02, 0.02), (-0.02, -0.02))
SEG_CAP = RGB_CAP = 0.02
DEPTH_TOL = 2e-5
RGB_MAX, RGB_POOLED_SHARE = 3, 0.9999
GROUND_D2_MIN = 0.02
NEAR = 0.01                   # the near plane of kernel and oracle

CAM_POS = np.array([0.7, 0.0, 1.3])          # the reference's data-collection camera
CAM_QUAT = np.array([0.707, 0.0, 0.0, -0.707])
FOVY = 61.0
TABLE_TOP = 0.4
HALF = 0.0155
ARM_OVER_TABLE = (0.3, 0.4, 0.25, -1.6, 0.2, 2.0, 0.8)     # (joints 3 and 5 off 0: at 0 the hulls of links 2 | 3 have faces in one plane)
PROP_GEOM0, HULLS_LOW, LINK_HULLS = 12, tuple(range(2, 12)), (16, 17, 18, 19)

# family A: W x H; the first fourteen are the shapes the lane arithmetic of k_render singles out, the last three the
# controls it calls safe
SHAPES = ((4, 5), (4, 320), (32, 9), (32, 41), (64, 1), (64, 21), (264, 5), (640, 3), (772, 4), (776, 4), (800, 8),
          (800, 600), (1028, 2), (1280, 2), (64, 16), (128, 8), (640, 4))
CAMERA_SIZES = ((48, 64), (120, 160))        # family B: H x W


# ------------------------------------------------------------------ small helpers
def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def qaxis(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def q2m(q):
    from mujoco_robot_environments_amd.model import compile as MC
    return MC.q2m(np.asarray(q, np.float64) / np.linalg.norm(q))


@functools.lru_cache(maxsize=None)
def model():
    from mujoco_robot_environments_amd.model import compile as MC
    return MC.compile_scene()


def overhead_mat(roll_deg=0.0):
    """The reference camera's orientation (looking straight down), rolled about its optical axis."""
    R = q2m(CAM_QUAT)
    a = np.deg2rad(roll_deg)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    return f32(R @ Rz)


def look_at(pos, target, roll_deg=0.0):
    """cam_mat (camera -> world, MuJoCo convention: looks along -z, y up) of a camera at pos facing target."""
    z = np.asarray(pos, np.float64) - np.asarray(target, np.float64)
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    a = np.deg2rad(roll_deg)
    x, y = np.cos(a) * x + np.sin(a) * y, -np.sin(a) * x + np.cos(a) * y
    return f32(np.stack([x, y, z], axis=1))


def focal(fovy, height):
    return 0.5 * height / np.tan(np.deg2rad(fovy) / 2)


def pixel_ray(u, v, fovy, height, width):
    """Camera-frame ray through pixel (u, v), z component -1 (so its parameter is the depth along the axis)."""
    f = focal(fovy, height)
    return np.array([(u - 0.5 * (width - 1)) / f, -(v - 0.5 * (height - 1)) / f, -1.0])


def world_to_pixel(X, cam_pos, Rc, fovy, height, width):
    """The pinhole model of tasks/rearrangement.py world_2_pixel: -> (u, v, depth along the axis)."""
    f = focal(fovy, height)
    c = Rc.T @ (np.asarray(X, np.float64) - cam_pos)
    return 0.5 * (width - 1) + f * c[0] / -c[2], 0.5 * (height - 1) - f * c[1] / -c[2], -c[2]


def aim_camera(point, pixel, depth, Rc, fovy, height, width):
    """The cam_pos (float32 values) that puts the world point -- a cube's top-face centre, a hull's centre -- on the
    pixel (u, v), `depth` metres along the optical axis: the inverse of world_to_pixel."""
    return f32(np.asarray(point, np.float64) - Rc @ (pixel_ray(pixel[0], pixel[1], fovy, height, width) * depth))


def on_pixel(cam_pos, pixel, depth, Rc, fovy, height, width):
    """The world point that a fixed camera sees on the pixel at that depth."""
    return cam_pos + Rc @ (pixel_ray(pixel[0], pixel[1], fovy, height, width) * depth)


@dataclass
class Case:
    name: str
    family: str                   # "A" shapes | "B" cameras | "C" scenes | "D" steps of the background-cache sequence
    height: int
    width: int
    fovy: float
    cam_pos: np.ndarray           # [3] float32 values
    cam_mat: np.ndarray           # [3, 3] float32 values
    nprops: np.ndarray            # [N] int32
    sizes: np.ndarray             # [N, 4, 3] float32 values
    qpos: np.ndarray              # [N, 43] float32
    prop_rgb: np.ndarray          # [N, 4, 3] uint8
    geom_rgb: np.ndarray          # [20, 3] float32
    probes: list = field(default_factory=list)     # (env, v, u, geom id the pixel must show)
    meta: dict = field(default_factory=dict)

    @property
    def N(self):
        return len(self.qpos)


GEOM_RGB = np.linspace(0.2, 0.9, 60).reshape(20, 3).astype(np.float32)


def _colours(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 4, 3)).astype(np.uint8)


def _blank(n, arm=ARM_OVER_TABLE):
    """qpos rows: the arm at `arm`, fingers at 0, every cube parked inside the table (in use or not, it is out of sight)."""
    A = model()
    q = np.zeros((n, 43))
    q[:, :7] = A["home_qpos"] if arm is None else arm
    for p in range(4):
        q[:, 15 + 7 * p: 22 + 7 * p] = [0.4 + 0.1 * p, 0.6, 0.2, 1.0, 0, 0, 0]
    return q


def _put(q, i, p, pos, quat=(1.0, 0, 0, 0)):
    q[i, 15 + 7 * p: 18 + 7 * p] = pos
    q[i, 18 + 7 * p: 22 + 7 * p] = quat


def _case(name, family, H, W, fovy, cam_pos, cam_mat, q, nprops=4, sizes=None, prop_rgb=None, probes=(), geom_rgb=None, **meta):
    n = len(q)
    sizes = np.full((n, 4, 3), HALF) if sizes is None else np.asarray(sizes, np.float64)
    return Case(name, family, int(H), int(W), float(np.float32(fovy)), f32(cam_pos), f32(cam_mat).reshape(3, 3),
                np.broadcast_to(np.asarray(nprops, np.int32), (n,)).copy(), f32(sizes), np.asarray(q, np.float32),
                _colours(n, len(name) + 7 * W + H) if prop_rgb is None else np.asarray(prop_rgb, np.uint8),
                GEOM_RGB if geom_rgb is None else np.asarray(geom_rgb, np.float32), list(probes), meta)


def ordinary_scene(n=1, seed=5, half=HALF):
    """The arm over the table and four cubes on it, two of them tumbled (turned about a random axis, lifted clear)."""
    r = np.random.default_rng(seed)
    q = _blank(n)
    spots = [(0.6, 0.1), (0.8, -0.2), (0.55, -0.3), (0.9, 0.25)]
    for i in range(n):
        for p, (x, y) in enumerate(spots):
            x, y = x + r.uniform(-0.03, 0.03), y + r.uniform(-0.03, 0.03)
            if p < 2:
                _put(q, i, p, [x, y, TABLE_TOP + half], qaxis([0, 0, 1], r.uniform(-np.pi, np.pi)))
            else:
                _put(q, i, p, [x, y, TABLE_TOP + 2 * half], qaxis(r.standard_normal(3), r.uniform(0.3, 2.8)))
    return q


# ------------------------------------------------------------------ the oracle
@functools.lru_cache(maxsize=None)
def oracle_images(name: str):
    """[env] -> (rgb [H, W, 3] u8, depth [H, W], seg [H, W], seg_fragile [H, W] bool, rgb_fragile [H, W] bool)."""
    return images_of(case(name))


def images_of(c: "Case"):
    from oracle import render_oracle as RO
    out = []
    for i in range(c.N):
        def ren(off):
            return RO.render(model(), c.qpos[i].astype(np.float64), int(c.nprops[i]), c.sizes[i], c.prop_rgb[i],
                             c.geom_rgb.astype(np.float64), c.cam_pos, c.cam_mat, c.fovy, c.height, c.width, pixel_offset=off)
        rgb, depth, seg = ren((0.0, 0.0))
        sf = np.zeros(seg.shape, bool)
        rf = np.zeros(seg.shape, bool)
        for off in OFFSETS:
            r2, _, s2 = ren(off)
            sf |= s2 != seg
            rf |= (np.abs(r2.astype(int) - rgb.astype(int)) > 1).any(-1)
        out.append((rgb, depth, seg, sf, rf | sf))
    return out


def geoms_of(c: Case, i: int):
    """(pos, mat, size, type) of env i's geoms, from the oracle's kinematics."""
    from oracle import render_oracle as RO
    return RO.geom_poses(model(), c.qpos[i].astype(np.float64), int(c.nprops[i]), c.sizes[i])


TIE_REL = 1e-6


def depth_ties(c: "Case", i: int, im=None):
    """Pixels of env i, not seg-fragile, on which a second geom lies within TIE_REL (relative) of the nearest one: two
    faces in one plane (the hulls of arm links 2 and 3 are flush while joint 3 is at 0).  Which of them shows is decided
    by rounding, in the oracle as in the kernel, and no sub-pixel offset tells: the cases must have none."""
    rgb, depth, seg, sf, rf = (oracle_images(c.name) if im is None else im)[i]
    pos, mat, size, typ = geoms_of(c, i)
    u, v = np.meshgrid(np.arange(c.width), np.arange(c.height))
    f = focal(c.fovy, c.height)
    dc = np.stack([(u - 0.5 * (c.width - 1)) / f, -(v - 0.5 * (c.height - 1)) / f, -np.ones(u.shape)], axis=-1)
    dw = dc @ c.cam_mat.T
    near = np.zeros(seg.shape, int)
    for g in range(len(typ)):
        if typ[g] <= 0:
            continue
        o, d = (c.cam_pos - pos[g]) @ mat[g], dw @ mat[g]
        with np.errstate(divide="ignore", invalid="ignore"):
            t1, t2 = (-size[g] - o) / d, (size[g] - o) / d
            tn, tf = np.minimum(t1, t2).max(-1), np.maximum(t1, t2).min(-1)
        near += (tn <= tf) & (tn >= NEAR) & (np.abs(tn - depth) <= TIE_REL * depth)
    return int(((near >= 2) & ~sf).sum())


def fragile_shares(name: str, im=None):
    """Per case: (seg-fragile share, share of rgb-fragile pixels that are not ground), over all its envs."""
    im = oracle_images(name) if im is None else im
    tot = sum(o[2].size for o in im)
    return sum(o[3].sum() for o in im) / tot, sum((o[4] & (o[2] != 0)).sum() for o in im) / tot


def entry_faces(c: Case, i: int, g: int):
    """{(axis, sign)} of the faces of box g that the oracle's rays of env i enter through."""
    rgb, depth, seg, sf, rf = oracle_images(c.name)[i]
    pos, mat, size, typ = geoms_of(c, i)
    vv, uu = np.nonzero((seg == g) & ~sf)
    out = set()
    for v, u in zip(vv, uu):
        p = c.cam_pos + c.cam_mat @ (pixel_ray(u, v, c.fovy, c.height, c.width) * depth[v, u])
        loc = (p - pos[g]) @ mat[g]
        k = int(np.argmax(np.abs(loc) / size[g]))
        out.add((k, int(np.sign(loc[k]))))
    return out


# ------------------------------------------------------------------ comparison
def compare(name: str, i: int, rgb, depth, seg):
    """Device images of env i against the oracle.  -> (problems [str], stats {depth, rgb, n, above1}): the worst
    relative depth error (in units of max(1, d)), the worst rgb error, the pixels counted and those above 1."""
    o_rgb, o_depth, o_seg, sf, rf = oracle_images(name)[i]
    seg = np.asarray(seg).astype(int)
    depth = np.asarray(depth, np.float64)
    problems = []
    bad = (seg != o_seg) & ~sf
    if bad.any():
        v, u = np.argwhere(bad)[0]
        ids = sorted(set(o_seg[bad].tolist()))
        problems.append(f"seg differs on {int(bad.sum())} pixels that are not fragile (oracle ids {ids}; first at row {v}, "
                        f"column {u}: device {seg[v, u]}, oracle {o_seg[v, u]})")
    same = seg == o_seg
    derr = np.abs(depth - o_depth) / np.maximum(1.0, o_depth)
    worst_d = float(derr[same].max()) if same.any() else 0.0
    if worst_d > DEPTH_TOL:
        v, u = np.argwhere(same & (derr > DEPTH_TOL))[0]
        problems.append(f"depth off by {worst_d:.3g} x max(1, d) (first at row {v}, column {u}: {depth[v, u]!r} vs {o_depth[v, u]!r})")
    sky = same & (o_seg == 255)
    if sky.any() and not ((depth[sky] == 100.0).all() and np.array_equal(np.asarray(rgb)[sky], o_rgb[sky])):
        problems.append("sky pixels must hold depth 100 and the oracle's tint bytes")
    ok = same & ~rf
    drgb = np.abs(np.asarray(rgb)[ok].astype(int) - o_rgb[ok].astype(int))
    worst_c = int(drgb.max()) if drgb.size else 0
    if worst_c > RGB_MAX:
        problems.append(f"rgb off by {worst_c} on a pixel that is not fragile")
    return problems, dict(depth=worst_d, rgb=worst_c, n=int(drgb.size), above1=int((drgb > 1).sum()))


# ------------------------------------------------------------------ family A: image shapes
def shape_fovy(H, W):
    """fovy 61 unless the image is so wide that its columns would reach past 35 degrees off the axis."""
    f = max(focal(FOVY, H), 0.5 * W / 0.7)
    return float(np.float32(np.rad2deg(2 * np.arctan(0.5 * H / f))))


def shape_probes(H, W):
    """(u, v): first pixel, last column of the first row, a pixel of the last row's first and last 4-pixel group, and one
    in columns >= 768 where the image has them -- a later probe in the row and 4-pixel group of an earlier one is left out."""
    cand = [(0, 0), (W - 1, 0), (1, H - 1), (W - 2, H - 1)]
    if W > 768:
        cand.append(((768 + W) // 2, H // 2))
    out, seen = [], set()
    for u, v in cand:
        if (u >> 2, v) not in seen:
            seen.add((u >> 2, v))
            out.append((u, v))
    return out


A_DEPTH = 0.5     # cube tops hang this far below the camera, above the arm: nothing but air in between


def a_cubes(W, H):
    """Two envs, cubes in mid-air 0.5 m under an overhead camera that aim_camera points so that env 0's cube 0 shows on
    the first probe; the other cubes sit where the camera sees the other probes (env 1: in the opposite order, so
    every probe is tried with two cube ids).  The cubes are 15.5 mm, or smaller where probes are close: 0.3 of the
    distance between the nearest two, so no cube covers another's probe and +-0.02 px stays on the top face."""
    fovy, Rc, probes = shape_fovy(H, W), overhead_mat(), shape_probes(H, W)
    n = min(4, len(probes))
    sep = min([max(abs(a[0] - b[0]), abs(a[1] - b[1])) for a in probes for b in probes if a != b] or [1])
    half = float(np.float32(min(HALF, 0.3 * sep * A_DEPTH / focal(fovy, H))))     # cubes of neighbouring probes stay apart
    nominal = np.array([0.4, 0.0, 1.7])
    top0 = f32(on_pixel(nominal, probes[0], A_DEPTH, Rc, fovy, H, W))
    cam = aim_camera(top0, probes[0], A_DEPTH, Rc, fovy, H, W)
    q = _blank(2, arm=None)
    marks = []
    for i in range(2):
        for p in range(n):
            k = p if i == 0 else len(probes) - 1 - p
            top = top0 if (i, p) == (0, 0) else on_pixel(cam, probes[k], A_DEPTH, Rc, fovy, H, W)
            _put(q, i, p, top - [0, 0, half])
            marks.append((i, probes[k][1], probes[k][0], PROP_GEOM0 + p))
    return _case(f"A-{W}x{H}-cubes", "A", H, W, fovy, cam, Rc, q, nprops=n, sizes=np.full((2, 4, 3), half), probes=marks)


def a_hull(W, H, which):
    """The arm over the table, cubes on it, and the overhead camera aimed at the centre of a link hull (geoms 16..19) so
    that it shows on the last probe (which = -1) or the first (0); the hull is the first, counted from one that
    depends on the shape, that the oracle sees there with the case inside the caps (a 20-pixel image has to be free
    of fragile pixels), from 0.9 m, else 0.7 or 1.1."""
    from oracle import render_oracle as RO
    fovy, Rc, probes = shape_fovy(H, W), overhead_mat(), shape_probes(H, W)
    u, v = probes[which]
    q = ordinary_scene(1, seed=W + H)
    pos, mat, size, typ = RO.geom_poses(model(), f32(q[0]), 4, np.full((4, 3), HALF))
    start = (W // 4 + H) % 4
    for depth in (0.9, 0.7, 1.1):
        for k in range(4):
            g = LINK_HULLS[(start + k) % 4]
            cam = aim_camera(pos[g], (u, v), depth, Rc, fovy, H, W)
            c = _case(f"A-{W}x{H}-hull{'-first' if which == 0 else ''}", "A", H, W, fovy, cam, Rc, q, probes=[(0, v, u, g)])
            im = images_of(c)
            if im[0][2][v, u] == g and not im[0][4][v, u] and max(fragile_shares(c.name, im)) <= SEG_CAP and depth_ties(c, 0, im) == 0:
                return c
    raise AssertionError(f"no link hull shows on pixel {(u, v)} of {W}x{H}")


def a_natural():
    """800 x 600, fovy 61, the ordinary scene under the reference camera's height and orientation, aimed so that cube 1
    shows in column 785: the one full-size image of the suite."""
    H, W = 600, 800
    q = ordinary_scene(1, seed=1)
    top = f32(q[0, 22:25]) + [0, 0, HALF]
    Rc = overhead_mat()
    cam = aim_camera(top, (785, 300), CAM_POS[2] - top[2], Rc, FOVY, H, W)
    return _case("A-800x600-natural", "A", H, W, FOVY, cam, Rc, q, probes=[(0, 300, 785, PROP_GEOM0 + 1)])


# ------------------------------------------------------------------ family B: cameras
def _b(name, H, W, fovy, cam_pos, cam_mat, q=None, **meta):
    return _case(f"B-{name}-{H}x{W}", "B", H, W, fovy, cam_pos, cam_mat, ordinary_scene(1, seed=5) if q is None else q, **meta)


def b_side(H, W):
    """From the side, 2.1 m up, pitched 18 degrees down: ground to the far plane, table, hulls, cubes and sky.  The far
    plane at 100 m cuts the ground where d2 = 2.1 / 100, so GROUND_D2_MIN holds on every ground pixel.  The cubes are
    80 mm ones: from 3 m a 31 mm cube is half a pixel of the 48-row image."""
    pos = np.array([2.6, -1.1, 2.1])
    return _b("side", H, W, FOVY, pos, look_at(pos, [0.5, 0.0, 1.35]), ordinary_scene(1, seed=5, half=0.04),
              sizes=np.full((1, 4, 3), 0.04), horizon=True)


def b_level(H, W):
    """At the height of the cubes' centres on the table, beside it, looking exactly along -x: the camera is inside the z
    slab of every upright cube, so only their side faces can be entered.  Four upright cubes turned by 20, 110, 200 and
    290 degrees show both signs of both axes."""
    q = _blank(1)
    for p, (x, y) in enumerate([(0.9, -0.3), (0.8, -0.1), (0.9, 0.1), (0.8, 0.3)]):
        _put(q, 0, p, [x, y, TABLE_TOP + HALF], qaxis([0, 0, 1], np.deg2rad(20 + 90 * p)))
    pos = np.array([1.6, 0.0, TABLE_TOP + HALF])
    Rc = np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]])      # x_cam = +y, y_cam = +z, z_cam = +x (looks along -x)
    return _b("level", H, W, FOVY, pos, Rc, q)


def b_rolled(H, W):
    return _b("rolled37", H, W, FOVY, CAM_POS, overhead_mat(37.0))


def b_fovy(H, W, fovy):
    """fovy 10 looks at cube 0 alone; fovy 120 sees the whole table and the ground around it."""
    q = ordinary_scene(1, seed=5)
    pos = CAM_POS.copy()
    if fovy < 30:
        pos[:2] = f32(q[0, 15:17]) + [0.01, -0.005]
    return _b(f"fovy{int(fovy)}", H, W, fovy, pos, overhead_mat(), q)


def b_near(H, W):
    """3 cm outside the +x face of the link-7 hull, looking down along the gripper: corners of that hull (and of others)
    lie behind the near plane, so their screen rectangle is the whole image."""
    pos, mat, size, typ = geoms_of_state(ordinary_scene(1, seed=5)[0])
    p = pos[4] + [size[4][0] + 0.03, 0.0, -0.01]
    return _b("near", H, W, 90.0, p, look_at(p, pos[5] + [0.0, 0.0, -0.1]))


def b_slab(H, W):
    """Inside the x slab of upright, unturned cube 0 (5 mm off its centre plane), outside its y and z slabs."""
    q = ordinary_scene(1, seed=5)
    _put(q, 0, 0, [0.6, 0.1, TABLE_TOP + HALF])
    pos = np.array([0.605, -0.35, 0.75])
    return _b("slab", H, W, FOVY, pos, look_at(pos, [0.6, 0.1, TABLE_TOP + HALF]), q, slab_geom=PROP_GEOM0)


def b_inside(H, W):
    """Inside the hull of link 4, looking down at the table: that hull is invisible to kernel and oracle alike."""
    pos, mat, size, typ = geoms_of_state(ordinary_scene(1, seed=5)[0])
    return _b("inside", H, W, FOVY, pos[19] + [0.01, 0.0, 0.0], overhead_mat(), inside_geom=19)


def geoms_of_state(qrow):
    from oracle import render_oracle as RO
    return RO.geom_poses(model(), f32(qrow), 4, np.full((4, 3), HALF))


# ------------------------------------------------------------------ family C: scenes
C_SIDE_POS = np.array([1.9, -0.9, 1.0])


def _c(name, q, **kw):
    """A scene under the overhead camera and under a side camera that looks down at the table (no horizon), 48 x 64."""
    return [_case(f"C-{name}-top", "C", 48, 64, FOVY, CAM_POS, overhead_mat(), q, **kw),
            _case(f"C-{name}-side", "C", 48, 64, FOVY, C_SIDE_POS, look_at(C_SIDE_POS, [0.65, 0.0, 0.45]), q, **kw)]


def c_tumbling():
    r = np.random.default_rng(18)
    q = _blank(4)
    for i in range(4):
        for p in range(4):
            qq = r.standard_normal(4)
            while np.abs(q2m(qq)[2]).max() > np.cos(np.deg2rad(10)):      # no face near level
                qq = r.standard_normal(4)
            _put(q, i, p, [r.uniform(0.45, 0.95), r.uniform(-0.35, 0.35), r.uniform(0.5, 0.8)], qq / np.linalg.norm(qq))
    return _c("tumbling", q)


def c_occluded():
    """Cube 1 hangs on the line from each camera to cube 0 (env 0: the overhead one, env 1: the side one), half a cube off
    it, so part of cube 0 is hidden.  80 mm cubes: several pixels wide in both views."""
    h = 0.04
    q = _blank(2)
    for i, cam in enumerate((CAM_POS, C_SIDE_POS)):
        c0 = np.array([0.7, 0.1, TABLE_TOP + h])
        d = (cam - c0) / np.linalg.norm(cam - c0)
        _put(q, i, 0, c0)
        _put(q, i, 1, c0 + 0.25 * d + [h, 0.5 * h, 0.0], qaxis([0, 0, 1], 0.4))
    return _c("occluded", q, nprops=2, sizes=np.full((2, 4, 3), h), occluded=((0, "top"), (1, "side")))


def c_under_hull():
    """Cube 0 (an 80 mm one) on the table where the overhead camera's ray past the middle of the link-7 hull's +x face
    comes down: seen from above, the hull covers about half of it."""
    h = 0.04
    q = ordinary_scene(1, seed=5)
    pos, mat, size, typ = geoms_of_state(q[0])
    edge = pos[4] + mat[4] @ [size[4][0], 0.0, 0.0]
    top = CAM_POS + (edge - CAM_POS) * (CAM_POS[2] - (TABLE_TOP + 2 * h)) / (CAM_POS[2] - edge[2])
    _put(q, 0, 0, top - [0, 0, h])
    sizes = np.full((1, 4, 3), HALF)
    sizes[0, 0] = h
    return _c("under-hull", q, sizes=sizes)


def c_nprops():
    """Envs with 2 and 3 cubes in use; the unused ones lie on the table in plain view and must not be drawn."""
    q = ordinary_scene(2, seed=8)
    return _c("nprops", q, nprops=[2, 3], unused={0: (14, 15), 1: (15,)})


def c_sizes():
    """Half sizes from 8 to 40 mm, different along every axis, per env and cube."""
    r = np.random.default_rng(23)
    q = ordinary_scene(3, seed=9)
    sizes = f32(r.uniform(0.008, 0.04, (3, 4, 3)))
    for i in range(3):
        for p in range(4):
            q[i, 17 + 7 * p] = TABLE_TOP + 0.08
    return _c("sizes", q, sizes=sizes)


def c_colours():
    """The same state in three envs, cube colours per env: primaries, their complements, greys."""
    q = np.repeat(ordinary_scene(1, seed=5), 3, axis=0)
    rgb = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0]],
                    [[0, 255, 255], [255, 0, 255], [255, 255, 0], [0, 0, 255]],
                    [[10, 10, 10], [90, 90, 90], [170, 170, 170], [250, 250, 250]]], np.uint8)
    return _c("colours", q, prop_rgb=rgb)


# ------------------------------------------------------------------ family D: what one live handle is asked for in turn
D_STEPS = ("top", "side", "top", "fovy45", "30x40", "recoloured")     # the order tests/test_gpu_render_cases.py renders them in


def d_cache():
    """Two envs of the ordinary scene under: the overhead camera, the side camera, the overhead one with fovy 45, with a
    30 x 40 image, and with other colours for the static geoms and hulls (set_render_colours(geom_rgb=...))."""
    q = ordinary_scene(2, seed=12)
    side = look_at(C_SIDE_POS, [0.65, 0.0, 0.45])
    mk = lambda name, H, W, fovy, pos, mat, **kw: _case(f"D-cache-{name}", "D", H, W, fovy, pos, mat, q, prop_rgb=_colours(2, 99), **kw)
    return [mk("top", 48, 64, FOVY, CAM_POS, overhead_mat()), mk("side", 48, 64, FOVY, C_SIDE_POS, side),
            mk("fovy45", 48, 64, 45.0, CAM_POS, overhead_mat()), mk("30x40", 30, 40, FOVY, CAM_POS, overhead_mat()),
            mk("recoloured", 48, 64, FOVY, CAM_POS, overhead_mat(), geom_rgb=GEOM_RGB[::-1].copy())]


# ------------------------------------------------------------------ the list
def _build_all():
    cases = []
    for W, H in SHAPES:
        if (W, H) == (800, 600):
            cases.append(a_natural())
            continue
        cases.append(a_cubes(W, H))
        cases.append(a_hull(W, H, -1))
        if len(shape_probes(H, W)) > 1:
            cases.append(a_hull(W, H, 0))
    for H, W in CAMERA_SIZES:
        cases += [b_side(H, W), b_level(H, W), b_rolled(H, W), b_fovy(H, W, 10.0), b_fovy(H, W, 120.0), b_near(H, W),
                  b_slab(H, W), b_inside(H, W)]
    for fn in (c_tumbling, c_occluded, c_under_hull, c_nprops, c_sizes, c_colours):
        cases += fn()
    cases += d_cache()
    return {c.name: c for c in cases}


@functools.lru_cache(maxsize=None)
def _all():
    return _build_all()


def case(name: str) -> Case:
    return _all()[name]


def _names():
    """Case names without building the cases (pytest collects them; a_hull consults the oracle)."""
    out = []
    for W, H in SHAPES:
        if (W, H) == (800, 600):
            out.append("A-800x600-natural")
            continue
        out += [f"A-{W}x{H}-cubes", f"A-{W}x{H}-hull"]
        if len(shape_probes(H, W)) > 1:
            out.append(f"A-{W}x{H}-hull-first")
    for H, W in CAMERA_SIZES:
        out += [f"B-{k}-{H}x{W}" for k in ("side", "level", "rolled37", "fovy10", "fovy120", "near", "slab", "inside")]
    for k in ("tumbling", "occluded", "under-hull", "nprops", "sizes", "colours"):
        out += [f"C-{k}-top", f"C-{k}-side"]
    out += [f"D-cache-{k}" for k in ("top", "side", "fovy45", "30x40", "recoloured")]
    return tuple(out)


NAMES = _names()
