"""GPU tests of mre_seg_labels (csrc/mre_labels.hip) on synthetic images: the kernel against the per-env numpy statement
of tests/labels_cases.py, EXACTLY -- every integer, and the bits of zmin.  The shapes are the smallest at which each
mechanism of the kernel can break:

    1x1x1, 1x1x3        fewer pixels than one 16-byte vector: head / tail bytes only
    3x3x5, 3x7x17       odd h*w: env bases at every alignment, vectors straddle rows
    2x4x20, 2x2x1280    the camera's width rule (a multiple of 4) and its maximum width
    2x5x67, 1x130x64    more than one wave, more than one sweep of a workgroup, an image cut into pieces at n = 1
    3x480x640           the camera's frame
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import labels_cases as LC

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 1, 3), (3, 3, 5), (3, 7, 17), (2, 4, 20), (2, 2, 1280), (2, 5, 67), (1, 130, 64), (3, 480, 640)]
RANGES = [(12, 4), (0, 2), (248, 8), (255, 1)]
DEV = "cuda"


def _raw(seg, depth, n, h, w, id0, nid, stats, zmin):
    """mre_seg_labels on torch's current stream, pointers as given (ints or None); returns the status."""
    from mujoco_robot_environments_amd import lib as L
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.lib().mre_seg_labels(stream, seg, depth, n, h, w, id0, nid, stats, zmin)
    torch.cuda.synchronize()
    return rc


def _same(lab, seg, depth, id0, nid, what):
    stats, zmin = LC.numpy_labels(seg, depth, id0, nid)
    assert np.array_equal(lab.box.cpu().numpy(), stats[..., :4]), what
    assert np.array_equal(lab.count.cpu().numpy(), stats[..., 4]), what
    assert np.array_equal(lab.sum_xy.cpu().numpy(), stats[..., 5:7]), what
    if depth is None:
        assert lab.zmin is None
    else:
        assert np.array_equal(lab.zmin.cpu().numpy().view(np.uint32), zmin.view(np.uint32)), what


@pytest.mark.parametrize("id0,nid", RANGES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_the_numpy_statement_exactly(shape, id0, nid):
    from mujoco_robot_environments_amd import perception as P
    deps = LC.depths(*shape)
    dev_deps = [torch.from_numpy(d).to(DEV) for _, d in deps]
    for c, (name, seg) in enumerate(LC.contents(*shape, id0, nid)):
        t = torch.from_numpy(seg).to(DEV)
        _same(P.seg_labels(t, None, id0, nid), seg, None, id0, nid, (name, "no depth"))
        # every content with one depth image in turn; the label-rich ones with all three
        for j in (range(3) if name in ("interleaved", "rectangles", "one label everywhere") else [c % 3]):
            a = P.seg_labels(t, dev_deps[j], id0, nid)
            _same(a, seg, deps[j][1], id0, nid, (name, deps[j][0]))
            if name == "rectangles":   # a second call on the same input: the same bytes
                b = P.seg_labels(t, dev_deps[j], id0, nid)
                assert torch.equal(a.box, b.box) and torch.equal(a.count, b.count) and torch.equal(a.sum_xy, b.sum_xy)
                assert torch.equal(a.zmin.view(torch.int32), b.zmin.view(torch.int32))


def test_a_label_of_one_env_does_not_leak_into_its_neighbours():
    from mujoco_robot_environments_amd import perception as P
    seg = np.full((3, 7, 17), 1, np.uint8)
    seg[1, 2:5, 3:11] = 14
    lab = P.seg_labels(torch.from_numpy(seg).to(DEV))
    assert (lab.count.cpu().numpy() == [[0, 0, 0, 0], [0, 0, 24, 0], [0, 0, 0, 0]]).all()
    assert (lab.box[[0, 2]] == -1).all() and lab.box[1, 2].tolist() == [3, 2, 10, 4]


@pytest.mark.parametrize("shape", [(3, 3, 6), (2, 6, 67), (2, 7, 16)], ids=lambda s: "x".join(map(str, s)))
def test_guard_bytes_around_the_images_are_not_read(shape):
    """The images sit at an odd address (h * w is even, the view starts 1 + h * w bytes into an allocation) between guard
    bytes that hold the first label (depth: 0.0, below every real depth): a read outside seg[0 .. n*h*w) or
    depth[0 .. n*h*w) would show in the counts or in zmin."""
    n, h, w = shape
    id0, nid = 12, 4
    hw = h * w
    seg = LC.contents(n, h, w, id0, nid)[-1][1]
    depth = LC.depths(n, h, w)[0][1]
    buf = torch.full(((n + 2) * hw + 2,), id0, dtype=torch.uint8, device=DEV)
    view = buf[1 + hw: 1 + (n + 1) * hw]
    view.copy_(torch.from_numpy(seg).to(DEV).reshape(-1))
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    dbuf = torch.zeros(((n + 2) * hw + 2,), dtype=torch.float32, device=DEV)
    dview = dbuf[1 + hw: 1 + (n + 1) * hw]
    dview.copy_(torch.from_numpy(depth).to(DEV).reshape(-1))
    from mujoco_robot_environments_amd import perception as P
    lab = P.seg_labels(view.reshape(n, h, w), dview.reshape(n, h, w), id0, nid)
    _same(lab, seg, depth, id0, nid, "guarded")
    assert (buf[:1 + hw] == id0).all() and (buf[1 + (n + 1) * hw:] == id0).all()


def test_bad_arguments_return_err_arg_and_write_nothing():
    from mujoco_robot_environments_amd import lib as L
    n, h, w = 2, 4, 20
    seg = torch.full((n, h, w), 12, dtype=torch.uint8, device=DEV)
    dbuf = torch.ones((n * h * w + 1,), dtype=torch.float32, device=DEV)
    stats = torch.full((n, 8, 7), -77, dtype=torch.int64, device=DEV)
    zmin = torch.full((n, 8), -77.0, dtype=torch.float32, device=DEV)
    s, d, st, z = seg.data_ptr(), dbuf.data_ptr(), stats.data_ptr(), zmin.data_ptr()
    bad = [dict(nid=0), dict(nid=9), dict(id0=250, nid=7), dict(w=0), dict(h=0), dict(n=-1), dict(id0=-1),
           dict(zmin=None), dict(depth=None), dict(depth=d + 1), dict(depth=d + 2), dict(seg=None), dict(stats=None)]
    for kw in bad:
        a = dict(seg=s, depth=d, n=n, h=h, w=w, id0=12, nid=4, stats=st, zmin=z)
        a.update(kw)
        rc = _raw(a["seg"], a["depth"], a["n"], a["h"], a["w"], a["id0"], a["nid"], a["stats"], a["zmin"])
        assert rc == -1, (kw, rc)   # MRE_ERR_ARG
        assert L.lib().mre_last_error().startswith(b"mre_seg_labels")
        assert (stats == -77).all() and (zmin == -77.0).all(), kw
    assert _raw(s, d, 0, h, w, 12, 4, st, z) == 0   # n = 0: MRE_OK, nothing launched
    assert (stats == -77).all() and (zmin == -77.0).all()
    assert _raw(s, d, n, h, w, 12, 4, st, z) == 0   # and the good call writes every element it owns
    flat = stats.reshape(-1)[:n * 4 * 7].reshape(n, 4, 7).cpu().numpy()
    assert (flat[:, 0] == [0, 0, w - 1, h - 1, h * w, h * (w - 1) * w // 2, w * (h - 1) * h // 2]).all()
    assert (flat[:, 1:] == [-1, -1, -1, -1, 0, 0, 0]).all()
    zf = zmin.reshape(-1)[:n * 4].reshape(n, 4).cpu().numpy()
    assert (zf[:, 0] == 1.0).all() and np.isinf(zf[:, 1:]).all()
    assert (stats.reshape(-1)[n * 4 * 7:] == -77).all() and (zmin.reshape(-1)[n * 4:] == -77.0).all()


def test_a_strided_view_goes_through_the_wrapper_like_the_fallback():
    from mujoco_robot_environments_amd import perception as P
    seg = LC.contents(2, 12, 20, 12, 4)[-1][1]
    depth = LC.depths(2, 12, 20)[0][1]
    t, d = torch.from_numpy(seg).to(DEV), torch.from_numpy(depth).to(DEV)
    lab = P.seg_labels(t[:, ::2], d[:, ::2])
    ref = P.seg_labels_reference(torch.from_numpy(seg)[:, ::2], torch.from_numpy(depth)[:, ::2])
    assert not t[:, ::2].is_contiguous()
    assert torch.equal(lab.box.cpu(), ref.box) and torch.equal(lab.count.cpu(), ref.count)
    assert torch.equal(lab.sum_xy.cpu(), ref.sum_xy) and torch.equal(lab.zmin.cpu(), ref.zmin)
    cpu = P.seg_labels(torch.from_numpy(seg), torch.from_numpy(depth))   # a CPU tensor: the fallback, same values
    full = P.seg_labels(t, d)
    assert torch.equal(full.box.cpu(), cpu.box) and torch.equal(full.zmin.cpu(), cpu.zmin)
