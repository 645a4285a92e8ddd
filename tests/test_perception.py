"""CPU tests of the frame labels (mujoco_robot_environments_amd/perception.py): the torch fallback of seg_labels -- the
host-side statement of what mre_seg_labels computes -- against the per-env numpy statement of tests/labels_cases.py."""
import numpy as np
import pytest
import torch

from mujoco_robot_environments_amd import perception as P
from tests import labels_cases as LC


def _check(seg, depth, id0, nid, what):
    lab = P.seg_labels(torch.from_numpy(seg), None if depth is None else torch.from_numpy(depth), id0, nid)
    stats, zmin = LC.numpy_labels(seg, depth, id0, nid)
    assert lab.box.dtype == torch.int64 and lab.count.dtype == torch.int64 and lab.sum_xy.dtype == torch.int64
    assert tuple(lab.box.shape) == (seg.shape[0], nid, 4) and tuple(lab.sum_xy.shape) == (seg.shape[0], nid, 2)
    assert np.array_equal(lab.box.numpy(), stats[..., :4]), what
    assert np.array_equal(lab.count.numpy(), stats[..., 4]), what
    assert np.array_equal(lab.sum_xy.numpy(), stats[..., 5:7]), what
    if depth is None:
        assert lab.zmin is None
    else:
        assert lab.zmin.dtype == torch.float32
        assert np.array_equal(lab.zmin.numpy().view(np.uint32), zmin.view(np.uint32)), what
    return lab


@pytest.mark.parametrize("id0,nid", [(12, 4), (0, 2), (248, 8), (255, 1)])
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 3, 5), (2, 5, 67), (2, 48, 64)])
def test_seg_labels_on_cpu_tensors_match_the_numpy_statement(shape, id0, nid):
    for name, seg in LC.contents(*shape, id0, nid):
        for dname, depth in [("none", None)] + LC.depths(*shape):
            _check(seg, depth, id0, nid, (name, dname))


def test_seg_labels_of_a_strided_view_and_of_other_integer_types():
    seg = LC.contents(2, 12, 20, 12, 4)[-1][1]
    depth = LC.depths(2, 12, 20)[0][1]
    view = torch.from_numpy(seg)[:, ::2]
    lab = P.seg_labels(view, torch.from_numpy(depth)[:, ::2])
    stats, zmin = LC.numpy_labels(seg[:, ::2], depth[:, ::2], 12, 4)
    assert np.array_equal(lab.box.numpy(), stats[..., :4]) and np.array_equal(lab.count.numpy(), stats[..., 4])
    assert np.array_equal(lab.zmin.numpy(), zmin)
    lab32 = P.seg_labels(torch.from_numpy(seg.astype(np.int32)))
    assert np.array_equal(lab32.box.numpy(), LC.numpy_labels(seg, None, 12, 4)[0][..., :4])


def test_prop_bboxes_cases_through_the_labels():
    """The cases of test_host_logic.test_prop_bboxes_from_a_segmentation_image_on_cpu, through seg_labels and through
    prop_labels (which, given a segmentation image, must not touch the env)."""
    from mujoco_robot_environments_amd.tasks.rearrangement import BatchedRearrangementEnv, PROP_GEOM_ID0
    assert P.PROP_GEOM_ID0 == PROP_GEOM_ID0
    seg = torch.full((2, 48, 64), 1, dtype=torch.uint8)
    seg[0, 10:15, 20:31] = PROP_GEOM_ID0          # cube 0: rows 10..14, cols 20..30
    seg[0, 40:42, 3:5] = PROP_GEOM_ID0 + 2        # cube 2
    seg[1, 0:1, 63:64] = PROP_GEOM_ID0 + 3        # a single pixel in the corner
    lab = P.seg_labels(seg)
    out = BatchedRearrangementEnv.prop_labels(None, seg)
    for boxes in (lab.box.numpy(), out["bbox"], BatchedRearrangementEnv.prop_bboxes(None, seg)):
        assert boxes.shape == (2, 4, 4) and boxes.dtype == np.int64
        assert boxes[0, 0].tolist() == [20, 10, 30, 14]
        assert boxes[0, 2].tolist() == [3, 40, 4, 41]
        assert boxes[1, 3].tolist() == [63, 0, 63, 0]
        assert (boxes[0, 1] == -1).all() and (boxes[0, 3] == -1).all() and (boxes[1, :3] == -1).all()
    assert out["visible_pixels"].tolist() == [[55, 0, 4, 0], [0, 0, 0, 1]]
    assert out["nearest_depth"] is None
    assert out["centroid"][0, 0].tolist() == [25.0, 12.0] and out["centroid"][0, 2].tolist() == [3.5, 40.5]
    assert out["centroid"][1, 3].tolist() == [63.0, 0.0] and np.isnan(out["centroid"][0, 1]).all()
    depth = torch.full((2, 48, 64), 0.9)
    depth[0, 12, 25] = 0.55
    out = BatchedRearrangementEnv.prop_labels(None, seg, depth)
    assert out["nearest_depth"].dtype == np.float32
    assert out["nearest_depth"][0, 0] == np.float32(0.55) and out["nearest_depth"][0, 2] == np.float32(0.9)
    assert np.isinf(out["nearest_depth"][0, 1]) and np.isinf(out["nearest_depth"][1, :3]).all()


def test_centroid_is_nan_for_absent_labels():
    seg = torch.full((2, 4, 6), 255, dtype=torch.uint8)
    seg[1, 1:3, 2:5] = 13
    lab = P.seg_labels(seg)
    c = P.centroid(lab)
    assert c.dtype == torch.float64 and tuple(c.shape) == (2, 4, 2)
    assert torch.isnan(c[0]).all() and torch.isnan(c[1, [0, 2, 3]]).all()
    assert c[1, 1].tolist() == [3.0, 1.5]


def test_seg_labels_rejects_bad_label_ranges_and_shapes():
    seg = torch.zeros((1, 2, 2), dtype=torch.uint8)
    for id0, nid in [(12, 0), (12, 9), (250, 7), (-1, 2)]:
        with pytest.raises(ValueError):
            P.seg_labels(seg, None, id0, nid)
    with pytest.raises(ValueError):
        P.seg_labels(seg[0])
    with pytest.raises(ValueError):
        P.seg_labels(seg, torch.zeros((1, 2, 3)))
