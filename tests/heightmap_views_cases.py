"""The numpy statement of the fused heightmap (perception.heightmap_views, mre_heightmap_views; include/mre.h) and the
multi-view cases the CPU and GPU tests run it on.  The statement is tests/heightmap_cases.numpy_heightmap per view, then the
merge: per cell the largest key (bits(hz) << 32) | ~(view << 28 | src) among the views that filled it -- the largest height,
the lowest view among equal heights.  Cameras, ray caster and salted depths are heightmap_cases' own.

A case is a dict: name, n, views [dict(depth, rgb, seg, cam)], bounds (lo, hi), cell, max_depth, out (rows, columns).
``statement(case)`` -> (hmap, cmap, smap, src, view, tie): the five outputs and the cells two or more views filled with the
same height bits (where a permutation of the views may change view, src, cmap and smap)."""
import functools

import numpy as np

from tests import heightmap_cases as HC

F = np.float32
NAMES = ("overhead", "oblique", "oblique rolled")
# n, (h, w) of each of the three views, map rows x columns: the single-view shapes of heightmap_cases, the fourth with views
# of different size, the last with the sizes of the reference's three cameras
SHAPES = [(1, ((1, 4),) * 3, (1, 1)), (2, ((3, 8),) * 3, (5, 7)), (3, ((24, 32),) * 3, (33, 47)),
          (3, ((48, 64), (32, 32), (24, 40)), (70, 130)), (2, ((48, 64),) * 3, (160, 120)), (2, ((48, 64),) * 3, (4, 3)),
          (1, ((480, 640), (640, 640), (640, 640)), (320, 240))]
IDS = [f"{n}x" + "+".join(f"{h}x{w}" for h, w in dict.fromkeys(sizes)) + f"-{out[0]}x{out[1]}" for n, sizes, out in SHAPES]
MID = SHAPES[2]


@functools.lru_cache(maxsize=None)
def scene_view(name, n, h, w):
    """The ray-cast scene of heightmap_cases seen through camera ``name`` at h x w: dict(depth, rgb, seg, cam), read-only."""
    pos, mat, fovy = HC.CAMERAS[name]
    cam = HC.camera12(pos, mat, HC.fovy_for(fovy, h, w), h, w)
    depth, rgb, seg = HC.ray_cast(cam, n, h, w)
    v = dict(depth=depth, rgb=rgb, seg=seg, cam=cam)
    for a in v.values():
        a.setflags(write=False)
    return v


def _single(name, n, h, w, out):
    """The case ``name`` of heightmap_cases.cases at this shape."""
    return [c for c in HC.cases((n, h, w), out) if c["name"] == name][0]


def _view_of(case):
    return {k: case[k] for k in ("depth", "rgb", "seg", "cam")}


def _case(name, n, views, out, bounds=None, cell=None, max_depth=99.0):
    lo, hi, c = HC._bounds(out)
    return dict(name=name, n=n, views=list(views), bounds=(lo, hi) if bounds is None else bounds,
                cell=c if cell is None else cell, max_depth=max_depth, out=out)


@functools.lru_cache(maxsize=None)
def cases(n, sizes, out):
    """The two cases of one shape: the three cameras on their ray-cast scenes, and on the salted depths of
    heightmap_cases.cases under the overhead view's max_depth."""
    scene = _case("scene", n, [scene_view(name, n, h, w) for name, (h, w) in zip(NAMES, sizes)], out)
    salted = [_single(f"{name}: salted", n, h, w, out) for name, (h, w) in zip(NAMES, sizes)]
    return [scene, _case("salted", n, [_view_of(c) for c in salted], out, max_depth=salted[0]["max_depth"])]


@functools.lru_cache(maxsize=None)
def further():
    """name -> case, at 3 envs and a 33 x 47 map: the same view twice, a view that sees nothing between two that do, one
    constant depth straight down in two sizes, one view, and eight."""
    n, sizes, out = MID
    h, w = sizes[0]
    over, obl, rolled = (scene_view(name, n, h, w) for name in NAMES)
    const = [_single("straight down: constant depth", n, hh, ww, out) for hh, ww in ((h, w), (2 * h, 2 * w))]
    eight = [scene_view(name, n, h, w) for name in HC.CAMERAS] + [scene_view("oblique", n, 32, 32),
                                                                  scene_view("overhead", n, 2 * h, 2 * w)]
    assert len(eight) == 8
    return {"twice": _case("twice", n, [obl, obl], out),
            "nothing in the middle": _case("nothing in the middle", n, [over, scene_view("sees nothing", n, h, w), rolled], out),
            "constant depth": _case("constant depth", n, [_view_of(c) for c in const], out, bounds=const[0]["bounds"],
                                    cell=const[0]["cell"]),
            "one view": _case("one view", n, [obl], out),
            "eight views": _case("eight views", n, eight, out)}


def single_statement(case, i, rgb=True, seg=True):
    """numpy_heightmap of view i of a case, alone."""
    v = case["views"][i]
    return HC.numpy_heightmap(v["depth"], v["rgb"] if rgb else None, v["seg"] if seg else None, v["cam"], case["bounds"],
                              case["cell"], case["max_depth"], case["out"])


def merge(singles):
    """(hmap, cmap, smap, src, view, tie) of the single-view maps [(hmap, cmap, smap, src)], lowest view first."""
    assert 1 <= len(singles) <= 8
    best = np.zeros(singles[0][0].shape, np.uint64)
    keys = []
    for i, (hmap, _, _, src) in enumerate(singles):
        assert (src < 2 ** 28).all()
        low = np.uint64(0xFFFFFFFF) - ((np.uint64(i) << np.uint64(28)) | np.maximum(src, 0).astype(np.uint64))
        key = np.where(src >= 0, (hmap.view(np.uint32).astype(np.uint64) << np.uint64(32)) | low, np.uint64(0))
        keys.append(key)
        best = np.maximum(best, key)
    filled = best != 0
    view = np.full(best.shape, 255, np.uint8)
    out = [np.zeros_like(singles[0][0]), None if singles[0][1] is None else np.zeros_like(singles[0][1]),
           None if singles[0][2] is None else np.full_like(singles[0][2], 255), np.full_like(singles[0][3], -1)]
    same = np.zeros(best.shape, np.int32)
    for i, (single, key) in enumerate(zip(singles, keys)):
        won = filled & (key == best)
        view[won] = i
        for o, s in zip(out, single):
            if o is not None:
                o[won] = s[won]
        same += (filled & ((key >> np.uint64(32)) == (best >> np.uint64(32))) & (key != 0)).astype(np.int32)
    return out[0], out[1], out[2], out[3], view, same >= 2


_STATEMENTS = {}


def statement(case):
    """The fused statement of a case with rgb and seg, computed once."""
    if id(case) not in _STATEMENTS:
        _STATEMENTS[id(case)] = merge([single_statement(case, i) for i in range(len(case["views"]))])
    return _STATEMENTS[id(case)]
