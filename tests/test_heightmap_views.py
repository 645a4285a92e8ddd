"""CPU tests of the fused heightmap (perception.heightmap_views, mre_heightmap_views; csrc/mre_heightmap_point.h) against
the numpy statement of tests/heightmap_views_cases.py, bit for bit:

  * the cases themselves, on the numpy statement alone: every view wins cells, the fused map fills more than any one view,
    cells are tied between views;
  * heightmap_views and heightmap_views_reference on CPU tensors: every output of every case, no cell left out;
  * one view is heightmap; a permutation of the views changes nothing but the winners of tied cells;
  * hm_key_view, the very text the kernel runs, compiled by g++ into tests/heightmap_views_host: it orders (hz, view, index)
    as the statement does;
  * the argument rules of mre_heightmap_views that need no device to refuse a call.
"""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import heightmap_cases as HC
from tests import heightmap_views_cases as VC

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "heightmap_views_host", "heightmap_views_host.cpp")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _torch_views(case, device="cpu", rgb=True, seg=True, order=None):
    order = range(len(case["views"])) if order is None else order
    t = lambda a: torch.from_numpy(a.copy()).to(device)
    return [(t(v["depth"]), t(v["rgb"]) if rgb else None, t(v["seg"]) if seg else None, v["cam"])
            for v in (case["views"][i] for i in order)]


def _kw(case):
    return dict(bounds=case["bounds"], cell=case["cell"], max_depth=case["max_depth"])


def _same(r, want, rgb, seg, what):
    hmap, cmap, smap, src, view = want[:5]
    assert r.height.dtype == torch.float32 and r.src.dtype == torch.int32 and r.view.dtype == torch.uint8
    assert np.array_equal(_bits(r.height.cpu().numpy()), _bits(hmap)), what
    assert np.array_equal(r.src.cpu().numpy(), src), what
    assert np.array_equal(r.view.cpu().numpy(), view), what
    if rgb:
        assert r.colour.dtype == torch.uint8 and np.array_equal(r.colour.cpu().numpy(), cmap), what
    else:
        assert r.colour is None
    if seg:
        assert r.seg.dtype == torch.uint8 and np.array_equal(r.seg.cpu().numpy(), smap), what
    else:
        assert r.seg is None


@pytest.mark.parametrize("n,sizes,out", VC.SHAPES, ids=VC.IDS)
def test_the_cases_exercise_what_they_are_meant_to(n, sizes, out):
    """On the numpy statement alone, before anything is compared with it."""
    scene = VC.cases(n, sizes, out)[0]
    hmap, cmap, smap, src, view, tie = VC.statement(scene)
    singles = [VC.single_statement(scene, i) for i in range(3)]
    filled = [int((s[3] >= 0).sum()) for s in singles]
    print(VC.IDS[VC.SHAPES.index((n, sizes, out))], "filled per view", filled, "fused", int((src >= 0).sum()), "of", src.size,
          "won per view", [int((view == i).sum()) for i in range(3)], "tied", int(tie.sum()))
    assert ((view == 255) == (src == -1)).all() and (view[src >= 0] < 3).all()
    if out == (1, 1):
        return
    assert all((view == i).any() for i in range(3))            # every view wins a cell
    if out != (4, 3):                                         # (there one view already fills the map)
        assert (src >= 0).sum() > max(filled)
    else:
        assert (src >= 0).all()
    assert tie.any()                                          # the tie rule decides somewhere


def test_the_counts_of_the_two_documented_shapes():
    """The filled cells DESIGN.md 8f.11 quotes for the 24 x 32 and the three-camera shapes."""
    for shape, per_view, fused in ((VC.SHAPES[2], [360, 198, 117], 645), (VC.SHAPES[6], [75195, 39275, 41586], 76355)):
        scene = VC.cases(*shape)[0]
        assert [int((VC.single_statement(scene, i)[3] >= 0).sum()) for i in range(3)] == per_view
        assert int((VC.statement(scene)[3] >= 0).sum()) == fused
    assert int(VC.statement(VC.cases(*VC.SHAPES[6])[0])[5].sum()) == 23408


@pytest.mark.parametrize("n,sizes,out", VC.SHAPES, ids=VC.IDS)
def test_heightmap_views_on_cpu_tensors_equals_the_numpy_statement(n, sizes, out):
    from mujoco_robot_environments_amd import perception as P
    for i, c in enumerate(VC.cases(n, sizes, out)):
        want = VC.statement(c)
        got = P.heightmap_views(_torch_views(c), **_kw(c))
        assert isinstance(got, P.FusedHeightMap) and got.height.shape == (n,) + out
        _same(got, want, True, True, c["name"])
        _same(P.heightmap_views_reference(_torch_views(c), **_kw(c)), want, True, True, c["name"])
        with_rgb, with_seg = [(False, False), (True, False), (False, True)][(i + n) % 3]
        _same(P.heightmap_views(_torch_views(c, rgb=with_rgb, seg=with_seg), **_kw(c)), want, with_rgb, with_seg, c["name"])


def test_the_further_cases_on_cpu_tensors():
    from mujoco_robot_environments_amd import perception as P
    cases = VC.further()
    for c in cases.values():
        _same(P.heightmap_views(_torch_views(c), **_kw(c)), VC.statement(c), True, True, c["name"])
    hmap, cmap, smap, src, view, tie = VC.statement(cases["twice"])
    assert (src >= 0).sum() > 100 and (view[src >= 0] == 0).all() and tie[src >= 0].all()
    one = VC.single_statement(cases["twice"], 0)
    assert all(np.array_equal(a, b) for a, b in zip((_bits(hmap), cmap, smap, src), (_bits(one[0]),) + one[1:]))
    # a view that sees nothing wins nothing, and the others are as they are without it
    c = cases["nothing in the middle"]
    hmap, cmap, smap, src, view, tie = VC.statement(c)
    assert (VC.single_statement(c, 1)[3] == -1).all() and not (view == 1).any() and (view == 2).any()
    without = VC.merge([VC.single_statement(c, 0), VC.single_statement(c, 2)])
    assert np.array_equal(_bits(hmap), _bits(without[0])) and np.array_equal(src, without[3])
    assert np.array_equal(cmap, without[1]) and np.array_equal(smap, without[2])
    assert np.array_equal(view, np.where(without[4] == 1, 2, without[4]))
    # one height everywhere: view 0 wins every cell it reaches, with the first of the cell's pixels
    c = cases["constant depth"]
    hmap, cmap, smap, src, view, tie = VC.statement(c)
    first = VC.single_statement(c, 0)
    assert c["views"][0]["depth"].shape != c["views"][1]["depth"].shape
    assert (first[3] >= 0).sum() > 100 and (view[first[3] >= 0] == 0).all() and np.array_equal(src[view == 0], first[3][view == 0])
    assert len(np.unique(_bits(hmap)[src >= 0])) == 1 and tie[first[3] >= 0].any()
    v0 = c["views"][0]
    cx, cy, hz, valid = HC.numpy_points(v0["depth"], v0["cam"], *HC.grid32(c["bounds"], c["cell"]), c["max_depth"], c["out"])
    w = v0["depth"].shape[2]
    seen = {}
    for e, v, u in zip(*np.nonzero(valid)):
        seen.setdefault((e, int(cy[e, v, u]), int(cx[e, v, u])), v * w + u)
    assert all(src[k] == i0 and view[k] == 0 for k, i0 in seen.items())
    assert (VC.statement(cases["eight views"])[4] == 7).any()


def test_one_view_is_heightmap():
    from mujoco_robot_environments_amd import perception as P
    c = VC.further()["one view"]
    d, rgb, seg, cam = _torch_views(c)[0]
    single = P.heightmap(d, rgb, seg, cam=cam, **_kw(c))
    for fn in (P.heightmap_views, P.heightmap_views_reference):
        got = fn([(d, rgb, seg, cam)], **_kw(c))
        assert torch.equal(got.height.view(torch.int32), single.height.view(torch.int32)) and torch.equal(got.src, single.src)
        assert torch.equal(got.colour, single.colour) and torch.equal(got.seg, single.seg)
        assert torch.equal(got.view == 0, single.src >= 0) and torch.equal(got.view == 255, single.src < 0)
        assert got[:4][0] is got.height and len(got) == 5   # HeightMap's fields first: maps[0 .. 3] index it alike


@pytest.mark.parametrize("n,sizes,out", VC.SHAPES[1:6], ids=VC.IDS[1:6])
def test_a_permutation_of_the_views_changes_tied_cells_only(n, sizes, out):
    from mujoco_robot_environments_amd import perception as P
    for c in VC.cases(n, sizes, out):
        hmap, cmap, smap, src, view, tie = VC.statement(c)
        singles = [VC.single_statement(c, i) for i in range(3)]
        holds = np.zeros((3,) + hmap.shape, bool)
        for order in itertools.permutations(range(3)):
            got = P.heightmap_views(_torch_views(c, order=order), **_kw(c))
            assert np.array_equal(_bits(got.height.numpy()), _bits(hmap)), (c["name"], order)
            back = np.append(np.asarray(order, np.uint8), [255] * 253).astype(np.uint8)   # position -> the view's own number
            back[255] = 255
            free = ~tie
            assert np.array_equal(back[got.view.numpy()][free], view[free]), (c["name"], order)
            assert np.array_equal(got.src.numpy()[free], src[free]) and np.array_equal(got.seg.numpy()[free], smap[free])
            assert np.array_equal(got.colour.numpy()[free], cmap[free])
            # and a tied cell goes to the first, in the new order, of the views that hold its height
            for k, i in enumerate(order):
                holds[k] = (singles[i][3] >= 0) & (_bits(singles[i][0]) == _bits(hmap))
            assert np.array_equal(got.view.numpy()[tie], holds.argmax(axis=0)[tie].astype(np.uint8)), (c["name"], order)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the host harness"
    exe = str(tmp_path_factory.mktemp("heightmap_views_host") / "heightmap_views_host")
    subprocess.check_call([gxx, "-O2", "-ffp-contract=off", "-std=c++17", SRC, "-o", exe])
    return exe


def test_the_kernels_key_on_the_host_orders_height_view_and_index(harness, tmp_path):
    f32 = lambda x: int(np.float32(x).view(np.uint32))
    top = 2 ** 28 - 1
    # in the order the statement ranks them, best first: height, then the lower view, then the lower index
    ranked = [(f32(0.3), 7, top), (f32(0.25), 0, 0), (f32(0.25), 0, 1), (f32(0.25), 0, top), (f32(0.25), 1, 0),
              (f32(0.25), 3, 12345), (f32(0.25), 7, 0), (f32(0.25), 7, top - 1), (f32(0.25), 7, top),
              (int(np.nextafter(np.float32(0.25), np.float32(0)).view(np.uint32)), 0, 0), (f32(1e-40), 2, 5), (0, 0, 0),
              (0, 0, 7), (0, 6, top), (0, 7, top)]
    fi, fo = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.asarray(ranked, np.uint32).tofile(fi)
    subprocess.check_call([harness, fi, fo])
    got = np.fromfile(fo, np.uint64).reshape(len(ranked), 4)
    keys = got[:, 0]
    assert (keys[:-1] > keys[1:]).all() and keys[-1] > 0          # strictly ordered, and no key is 0
    assert np.array_equal(got[:, 1], [r[1] for r in ranked]) and np.array_equal(got[:, 2], [r[2] for r in ranked])
    zero = [i for i, r in enumerate(ranked) if r[1] == 0]
    assert np.array_equal(got[zero, 0], got[zero, 3])              # view 0: the single-view key
    want = [(np.uint64(h) << np.uint64(32)) | np.uint64(0xFFFFFFFF - ((v << 28) | i)) for h, v, i in ranked]
    assert np.array_equal(keys, np.asarray(want, np.uint64))


def test_heightmap_views_rejects_bad_views():
    from mujoco_robot_environments_amd import perception as P
    c = VC.cases(*VC.SHAPES[1])[0]
    views = _torch_views(c)
    kw = _kw(c)
    d, rgb, seg, cam = views[0]
    bad = [[], views * 3, [(d, rgb, seg)], [(d[0], None, None, cam)], [(d, rgb[..., :2], seg, cam)], [(d, rgb, seg[:, :2], cam)],
           [views[0], (d[:1], rgb[:1], seg[:1], cam)], [views[0], (d, None, seg, cam)], [views[0], (d, rgb, None, cam)]]
    for v in bad:
        with pytest.raises(ValueError):
            P.heightmap_views(v, **kw)
        with pytest.raises(ValueError):
            P.heightmap_views_reference(v, **kw)
    for k in (dict(cell=0.0), dict(cell=float("nan")), dict(bounds=((0, 0, 1), (1, 1, 0))), dict(max_depth=0.0), dict(cell=1e-5)):
        with pytest.raises(ValueError):
            P.heightmap_views(views, **{**kw, **k})


def test_bad_arguments_are_refused_without_a_gpu():
    """The rules of mre_heightmap_views that are checked before any device call: MRE_ERR_ARG and a message that names it."""
    from mujoco_robot_environments_amd import lib as L
    L.build()
    lib = L.lib()
    p = 4096   # never dereferenced: every call below is refused on its scalars or on the pointers' own values
    ptrs = lambda *v: np.asarray(v, np.uint64)
    i32 = lambda *v: np.asarray(v, np.int32)
    cam = np.arange(24, dtype=np.float32)
    b = np.array([0, 0, 0, 1, 1, 1], np.float32)
    keep = dict(depth=ptrs(p, p), rgb=ptrs(p, p), seg=ptrs(p, p), height=i32(4, 4), width=i32(4, 4))
    good = dict(views=2, depth=keep["depth"].ctypes.data, rgb=None, seg=None, n=1, height=keep["height"].ctypes.data,
                width=keep["width"].ctypes.data, cam=cam.ctypes.data, bounds=b.ctypes.data, inv_cell=4.0, max_depth=99.0,
                out_h=4, out_w=4, hmap=p, cmap=None, smap=None, src=None, view=None)
    nan_b, swapped = b.copy(), b.copy()
    nan_b[4], swapped[[2, 5]] = np.nan, (1, 0)
    arrays = dict(h0=i32(4, 0), w0=i32(0, 4), big=i32(4, 16384), bigw=i32(4, 16384), odd=ptrs(p, p + 1), half=ptrs(p, p + 2),
                  hole=ptrs(p, 0), neg=i32(-1, 4))
    at = lambda k: arrays[k].ctypes.data
    rgb_ok, seg_ok = keep["rgb"].ctypes.data, keep["seg"].ctypes.data
    bad = [dict(views=0), dict(views=9), dict(views=-1), dict(n=-1), dict(height=at("h0")), dict(width=at("w0")),
           dict(height=at("neg")), dict(height=at("big"), width=at("bigw")), dict(height=None), dict(width=None),
           dict(out_h=0), dict(out_w=0), dict(out_h=4097), dict(out_w=4097), dict(inv_cell=0.0), dict(inv_cell=-1.0),
           dict(inv_cell=float("inf")), dict(inv_cell=float("nan")), dict(max_depth=0.0), dict(max_depth=float("inf")),
           dict(max_depth=float("nan")), dict(bounds=nan_b.ctypes.data), dict(bounds=swapped.ctypes.data), dict(bounds=None),
           dict(cam=None), dict(depth=None), dict(depth=at("hole")), dict(hmap=None), dict(depth=at("odd")), dict(depth=at("half")),
           dict(hmap=p + 2), dict(src=p + 2), dict(rgb=rgb_ok), dict(cmap=p), dict(seg=seg_ok), dict(smap=p),
           dict(rgb=at("hole"), cmap=p), dict(seg=at("hole"), smap=p)]
    assert 16384 * 16384 == 2 ** 28
    for kw in bad:
        a = {**good, **kw}
        rc = lib.mre_heightmap_views(None, *[a[k] for k in good])
        assert rc == -1, (kw, rc)   # MRE_ERR_ARG
        assert lib.mre_last_error().startswith(b"mre_heightmap_views"), kw
    # n = 0: MRE_OK, nothing launched -- with and without the optional outputs, at 1 and at 8 views
    assert lib.mre_heightmap_views(None, *[{**good, "n": 0}[k] for k in good]) == 0
    full = {**good, "n": 0, "rgb": rgb_ok, "seg": seg_ok, "cmap": p, "smap": p, "src": p, "view": p + 1}
    assert lib.mre_heightmap_views(None, *[full[k] for k in good]) == 0
    assert lib.mre_heightmap_views(None, *[{**good, "n": 0, "views": 1}[k] for k in good]) == 0
    eight = dict(depth=ptrs(*[p] * 8), height=i32(*[4] * 8), width=i32(*[16383] * 8), cam=np.zeros(96, np.float32))
    a = {**good, "n": 0, "views": 8, **{k: v.ctypes.data for k, v in eight.items()}}
    assert lib.mre_heightmap_views(None, *[a[k] for k in good]) == 0
