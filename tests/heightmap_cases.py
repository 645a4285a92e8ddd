"""The numpy statement of the orthographic heightmap (perception.heightmap, mre_heightmap; include/mre.h) and the
cameras, scenes and depth images the CPU and GPU tests run it on.  The statement is float32, every operation rounded on
its own (numpy float32 arrays do exactly that); images come from a small float64 ray caster: the table plane plus
axis-aligned boxes, depth measured along the camera's axis like the batched camera's.

A case is a dict: cam float32 [12], bounds (lo, hi), cell, max_depth, out (rows, columns), depth float32 [n, h, w],
rgb uint8 [n, h, w, 3], seg uint8 [n, h, w].  ``cases(shape, out)`` builds them once per shape (cached, read-only) and
``statement(case)`` evaluates the numpy statement once per case (cached)."""
import functools

import numpy as np

F = np.float32
# source n x h x w -> map rows x columns: what each can break is said in tests/test_gpu_heightmap.py
SHAPES = [((1, 1, 4), (1, 1)), ((2, 3, 8), (5, 7)), ((3, 24, 32), (33, 47)), ((2, 48, 64), (160, 120)),
          ((2, 48, 64), (4, 3)), ((1, 480, 640), (320, 240)), ((3, 48, 64), (70, 130))]
LO = (0.2, -0.4, 0.39)       # the env's default box: 0.6 m of x from LO in every case, cell = 0.6 / columns
HI_Z = 0.69
TABLE_Z = 0.4
NOTHING = 100.0              # the camera's depth where no geom is hit


# ------------------------------------------------------------------------------------------------------------ cameras
def q2m(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def look_at(pos, target, roll_deg=0.0):
    """Camera-to-world rotation of a camera at pos looking along its -z at target, rolled about that axis."""
    z = np.asarray(pos, np.float64) - np.asarray(target, np.float64)
    z /= np.linalg.norm(z)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.99 else np.array([0.0, 1.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c, s = np.cos(np.deg2rad(roll_deg)), np.sin(np.deg2rad(roll_deg))
    return np.stack([x, y, z], axis=1) @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


# name -> (position, rotation, fovy): the configured overhead pose, tilted and rolled obliques, a low close camera that
# stands INSIDE the box of the map (tile corners beside and behind it: the whole-image path), one that looks away from
# the table (nothing inside the bounds), and one straight down with an exact matrix (equal heights at equal depths)
CAMERAS = {
    "overhead": ((0.7, 0.0, 1.3), q2m([0.707, 0.0, 0.0, -0.707]), 61.0),
    "oblique": ((1.3, -0.7, 1.2), look_at((1.3, -0.7, 1.2), (0.5, 0.0, 0.45), 20.0), 50.0),
    "oblique rolled": ((0.1, 0.6, 1.0), look_at((0.1, 0.6, 1.0), (0.5, 0.0, 0.4), -35.0), 70.0),
    "low close": ((0.45, -0.15, 0.55), look_at((0.45, -0.15, 0.55), (0.8, 0.3, 0.4), 10.0), 80.0),
    "sees nothing": ((0.5, 0.0, 1.0), look_at((0.5, 0.0, 1.0), (0.6, 0.1, 2.0)), 61.0),
    "straight down": ((0.5, 0.0, 1.25), np.eye(3), 45.0),
}


def fovy_for(fovy, h, w):
    """The vertical field of view at which an h x w image spans what a 3 : 4 image spans across at ``fovy``; a source
    narrower than 16 pixels looks through a narrow lens (half-width 0.25 at unit depth) so that its few pixels land
    inside the map."""
    across = 0.25 if w < 16 else np.tan(np.deg2rad(fovy) / 2) / 0.75
    return float(np.rad2deg(2 * np.arctan(across * h / w)))


def camera12(pos, mat, fovy, h, w):
    """A = -R K^-1 row-major (float64, rounded once), then pos: perception.heightmap_camera, stated again."""
    f = (1.0 / np.tan(np.deg2rad(fovy) / 2)) * h / 2.0
    K = np.array([[-f, 0, (w - 1) / 2], [0, f, (h - 1) / 2], [0, 0, 1]])
    return np.concatenate([(-np.asarray(mat, np.float64) @ np.linalg.inv(K)).reshape(9), np.asarray(pos, np.float64)]).astype(F)


# ---------------------------------------------------------------------------------------------------------- ray caster
def boxes(env):
    """[(centre, half size, seg byte, rgb)] of env's scene: cubes on the table, a tall one, one across the map's edge."""
    s = 0.01 * env
    return [((0.40 + s, -0.10, 0.43), (0.03, 0.03, 0.03), 12, (200, 40, 40)),
            ((0.60, 0.15 - s, 0.44), (0.04, 0.05, 0.04), 13, (40, 200, 40)),
            ((0.50, 0.05 + s, 0.50), (0.025, 0.025, 0.10), 14, (40, 40, 200)),
            ((0.80, -0.38, 0.45), (0.06, 0.06, 0.05), 15, (200, 200, 40))]


def ray_cast(cam, n, h, w):
    """(depth float32, rgb uint8, seg uint8) of n envs seen through cam: depth is the ray parameter of pos + d A (u, v, 1),
    which is the distance along the camera's axis."""
    A, pos = cam[:9].astype(np.float64).reshape(3, 3), cam[9:].astype(np.float64)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    d = np.stack([u, v, np.ones_like(u)], axis=-1) @ A.T        # [h, w, 3]
    depth = np.full((n, h, w), NOTHING)
    seg = np.full((n, h, w), 255, np.uint8)
    rgb = np.zeros((n, h, w, 3), np.uint8)
    shade = ((7 * u + 13 * v) % 32).astype(np.uint8)           # neighbouring pixels of one object differ
    with np.errstate(divide="ignore", invalid="ignore"):
        for e in range(n):
            t = (TABLE_Z - pos[2]) / d[..., 2]
            hit = np.isfinite(t) & (t > 1e-6)
            depth[e][hit], seg[e][hit] = t[hit], 1
            rgb[e][hit] = np.array([120, 120, 120], np.uint8) + shade[hit][:, None]
            for c, half, sid, col in boxes(e):
                t0 = (np.asarray(c) - np.asarray(half) - pos) / d
                t1 = (np.asarray(c) + np.asarray(half) - pos) / d
                near, far = np.minimum(t0, t1).max(axis=-1), np.maximum(t0, t1).min(axis=-1)
                hit = np.isfinite(near) & (near <= far) & (near > 1e-6) & (near < depth[e])
                depth[e][hit], seg[e][hit] = near[hit], sid
                rgb[e][hit] = np.array(col, np.uint8) + shade[hit][:, None]
    return depth.astype(F), rgb, seg


# --------------------------------------------------------------------------------------------------------------- cases
def _bounds(out, lo_z=LO[2], hi_z=HI_Z):
    cell = 0.6 / out[1]
    return (LO[0], LO[1], lo_z), (LO[0] + out[1] * cell, LO[1] + out[0] * cell, hi_z), cell


def _noise(rng, n, h, w):
    return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8), rng.integers(0, 256, (n, h, w), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def cases(shape, out):
    """[case] of one source shape and map shape: every camera with its ray-cast scene and with random depths salted with
    the values that must not count; the straight-down camera also with one constant depth (every pixel the same height:
    the index decides) and with heights exactly on, and one float32 off, lo_z and hi_z."""
    n, h, w = shape
    rng = np.random.default_rng(1000 * n + 10 * h + w + out[0])
    res = []
    for name, (pos, mat, fovy) in CAMERAS.items():
        cam = camera12(pos, mat, fovy_for(fovy, h, w), h, w)
        lo, hi, cell = _bounds(out)
        depth, rgb, seg = ray_cast(cam, n, h, w)
        res.append(dict(name=f"{name}: scene", cam=cam, bounds=(lo, hi), cell=cell, max_depth=99.0, out=out,
                        depth=depth, rgb=rgb, seg=seg))
        md = F(np.linalg.norm(np.asarray(pos) - np.array([0.5, -0.1, 0.45])))   # cuts through the middle of the box
        salt = np.array([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, NOTHING, md, np.nextafter(md, F(0)), np.nextafter(md, F(9))], F)
        depth = (md * (0.3 + 1.2 * rng.random((n, h, w)))).astype(F)
        mask = rng.random((n, h, w)) < 0.3
        depth[mask] = rng.choice(salt, size=int(mask.sum()))
        rgb, seg = _noise(rng, n, h, w)
        res.append(dict(name=f"{name}: salted", cam=cam, bounds=(lo, hi), cell=cell, max_depth=float(md), out=out,
                        depth=depth, rgb=rgb, seg=seg))
    pos, mat, fovy = CAMERAS["straight down"]
    cam = camera12(pos, mat, fovy_for(fovy, h, w), h, w)
    assert cam[6] == 0 and cam[7] == 0 and cam[8] == -1 and cam[11] == F(1.25)   # P[2] = 1.25 - d, exactly
    lo, hi, cell = _bounds(out, 0.375, 0.6875)                                      # both exact in float32
    rgb, seg = _noise(rng, n, h, w)
    res.append(dict(name="straight down: constant depth", cam=cam, bounds=(lo, hi), cell=cell, max_depth=99.0, out=out,
                    depth=np.full((n, h, w), 0.75, F), rgb=rgb, seg=seg))
    d_lo, d_hi = F(1.25 - 0.375), F(1.25 - 0.6875)
    edge = np.array([d_lo, d_hi, np.nextafter(d_lo, F(2)), np.nextafter(d_lo, F(0)), np.nextafter(d_hi, F(2)),
                     np.nextafter(d_hi, F(0))], F)
    res.append(dict(name="straight down: on the bounds", cam=cam, bounds=(lo, hi), cell=cell, max_depth=99.0, out=out,
                    depth=rng.choice(edge, size=(n, h, w)), rgb=rgb, seg=seg))
    for c in res:
        for k in ("depth", "rgb", "seg", "cam"):
            c[k].setflags(write=False)
    return res


# ----------------------------------------------------------------------------------------------------------- statement
def grid32(bounds, cell):
    """lo, hi float32 [3] and inv_cell float32, rounded as perception does."""
    return np.asarray(bounds[0], np.float64).astype(F), np.asarray(bounds[1], np.float64).astype(F), F(1.0 / float(cell))


def numpy_world(depth, cam):
    """The world point of every pixel, [x, y, z] float32 [n, h, w] each: P = pos + d (A (u, v, 1)), op by op."""
    n, h, w = depth.shape
    u, v = np.arange(w, dtype=F)[None, None, :], np.arange(h, dtype=F)[None, :, None]
    P = []
    with np.errstate(all="ignore"):
        for k in range(3):
            t0 = cam[3 * k] * u
            t1 = cam[3 * k + 1] * v
            s = t0 + t1
            s = s + cam[3 * k + 2]
            m = depth * s
            P.append(cam[9 + k] + m)
    return P


def numpy_points(depth, cam, lo, hi, inv_cell, max_depth, out):
    """Per pixel (cx, cy, hz float32 [n, h, w], valid bool): the statement up to the competition for a cell."""
    P = numpy_world(depth, cam)
    with np.errstate(all="ignore"):
        cx, cy = np.floor((P[0] - lo[0]) * inv_cell), np.floor((P[1] - lo[1]) * inv_cell)
        hz = P[2] - lo[2]
        valid = ((depth > 0) & (depth < F(max_depth)) & (cx >= 0) & (cx < out[1]) & (cy >= 0) & (cy < out[0])
                 & (P[2] >= lo[2]) & (P[2] <= hi[2]))
    assert cx.dtype == cy.dtype == hz.dtype == F
    return cx, cy, hz, valid


def numpy_heightmap(depth, rgb, seg, cam, bounds, cell, max_depth, out):
    """(hmap float32 [n, rows, columns], cmap uint8 [.., 3] or None, smap uint8 or None, src int32): every cell takes the
    valid pixel with the largest hz, among equal hz the smallest index -- the largest key (bits(hz) << 32) | ~index."""
    n, h, w = depth.shape
    lo, hi, inv_cell = grid32(bounds, cell)
    cx, cy, hz, valid = numpy_points(depth, cam, lo, hi, inv_cell, max_depth, out)
    cells = out[0] * out[1]
    hmap, src = np.zeros((n, cells), F), np.full((n, cells), -1, np.int32)
    for e in range(n):
        idx = np.nonzero(valid[e].ravel())[0]
        cell_of = cy[e].ravel()[idx].astype(np.int64) * out[1] + cx[e].ravel()[idx].astype(np.int64)
        bits = hz[e].ravel()[idx].view(np.uint32).astype(np.uint64)
        assert (bits < 2 ** 31).all()                      # hz >= +0
        keys = np.zeros(cells, np.uint64)
        np.maximum.at(keys, cell_of, (bits << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx.astype(np.uint64)))
        filled = keys != 0
        src[e][filled] = (np.uint64(0xFFFFFFFF) - (keys[filled] & np.uint64(0xFFFFFFFF))).astype(np.int32)
        hmap[e][filled] = (keys[filled] >> np.uint64(32)).astype(np.uint32).view(F)
    pick = np.maximum(src, 0)
    cmap = smap = None
    if rgb is not None:
        cmap = np.take_along_axis(rgb.reshape(n, h * w, 3), pick[..., None].astype(np.int64), axis=1)
        cmap = np.where((src >= 0)[..., None], cmap, 0).astype(np.uint8).reshape(n, out[0], out[1], 3)
    if seg is not None:
        smap = np.take_along_axis(seg.reshape(n, h * w), pick.astype(np.int64), axis=1)
        smap = np.where(src >= 0, smap, 255).astype(np.uint8).reshape(n, out[0], out[1])
    return hmap.reshape(n, out[0], out[1]), cmap, smap, src.reshape(n, out[0], out[1])


_STATEMENTS = {}


def statement(case):
    """numpy_heightmap of a case of ``cases`` with rgb and seg, computed once."""
    if id(case) not in _STATEMENTS:
        _STATEMENTS[id(case)] = numpy_heightmap(case["depth"], case["rgb"], case["seg"], case["cam"], case["bounds"],
                                                case["cell"], case["max_depth"], case["out"])
    return _STATEMENTS[id(case)]
