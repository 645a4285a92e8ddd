"""Frame labels from the camera's images: the torch-facing wrapper of ``mre_seg_labels`` (include/mre.h,
csrc/mre_labels.hip).  For every env and every label of a small id range of a segmentation image it gives what the
reference's ``props_info`` takes from one (``get_bbox``, tasks/rearrangement.py:254-268: the PASCAL-VOC box of the
visible pixels) and what a caller needs beside it to label frames: the number of visible pixels (0 = hidden), the sums
of their coordinates (the centroid) and the smallest depth among them.  The kernel is enqueued on torch's current
stream; nothing here synchronises.  ``BatchedRearrangementEnv.prop_bboxes`` / ``prop_labels`` / ``props_info`` are the
users.
"""
from __future__ import annotations

import collections
import ctypes as C
from typing import Optional

import torch

from . import lib as _lib

PROP_GEOM_ID0 = 12   # geom ids of prop_0..3 in the compiled scene (tasks/rearrangement.py)
MAX_IDS = 8          # labels of one mre_seg_labels call

# box int64 [N, nid, (xmin, ymin, xmax, ymax)] (-1 where the label is absent), count int64 [N, nid],
# sum_xy int64 [N, nid, (sum of columns, sum of rows)], zmin float32 [N, nid] (+inf where absent) or None
SegLabels = collections.namedtuple("SegLabels", ["box", "count", "sum_xy", "zmin"])


def seg_labels_reference(seg: torch.Tensor, depth: Optional[torch.Tensor] = None, id0: int = PROP_GEOM_ID0,
                         nid: int = 4) -> SegLabels:
    """The semantics of ``seg_labels`` in plain torch, on whatever device ``seg`` is on, for any integer ``seg`` and
    any strides: the fallback of ``seg_labels`` and the host-side statement of what the kernel computes.  It
    materialises ``seg == label`` per label; use it for small batches and tests."""
    n, h, w = seg.shape
    dev = seg.device
    box = torch.full((n, nid, 4), -1, dtype=torch.int64, device=dev)
    count = torch.zeros((n, nid), dtype=torch.int64, device=dev)
    sum_xy = torch.zeros((n, nid, 2), dtype=torch.int64, device=dev)
    zmin = None if depth is None else torch.full((n, nid), float("inf"), dtype=torch.float32, device=dev)
    xs = torch.arange(w, dtype=torch.int64, device=dev)
    ys = torch.arange(h, dtype=torch.int64, device=dev)
    for k in range(nid):
        m = seg == (id0 + k)
        per_col, per_row = m.sum(dim=1), m.sum(dim=2)        # [n, w], [n, h] pixels of the label per column / row
        count[:, k] = per_col.sum(dim=1)
        sum_xy[:, k, 0] = (per_col * xs).sum(dim=1)
        sum_xy[:, k, 1] = (per_row * ys).sum(dim=1)
        if n and h and w:
            big = max(h, w)
            cols, rows = per_col > 0, per_row > 0
            b = torch.stack([torch.where(cols, xs, big).amin(dim=1), torch.where(rows, ys, big).amin(dim=1),
                             torch.where(cols, xs, -1).amax(dim=1), torch.where(rows, ys, -1).amax(dim=1)], dim=1)
            box[:, k] = torch.where((count[:, k] > 0)[:, None], b, box[:, k])
            if depth is not None:
                inf = torch.tensor(float("inf"), dtype=torch.float32, device=dev)
                zmin[:, k] = torch.where(m, depth.to(torch.float32), inf).amin(dim=(1, 2))
    return SegLabels(box, count, sum_xy, zmin)


def seg_labels(seg: torch.Tensor, depth: Optional[torch.Tensor] = None, id0: int = PROP_GEOM_ID0,
               nid: int = 4) -> SegLabels:
    """Box, pixel count, coordinate sums and nearest depth of the labels ``id0 .. id0 + nid - 1`` in every image of
    ``seg`` [N, H, W] (``depth`` [N, H, W] float32, finite and non-negative, or None): see ``SegLabels``.  A uint8
    CUDA ``seg`` is read once by ``mre_seg_labels`` (a non-contiguous view is made contiguous first); anything else is
    computed by ``seg_labels_reference`` with the same return values."""
    if seg.dim() != 3:
        raise ValueError("seg must be [N, H, W]")
    if depth is not None and tuple(depth.shape) != tuple(seg.shape):
        raise ValueError("depth must have seg's shape")
    if not (1 <= nid <= MAX_IDS and id0 >= 0 and id0 + nid <= 256):
        raise ValueError(f"labels {id0} .. {id0 + nid - 1}: at most {MAX_IDS} labels inside 0 .. 255")
    if not (seg.is_cuda and seg.dtype == torch.uint8):
        return seg_labels_reference(seg, depth, id0, nid)
    n, h, w = (int(x) for x in seg.shape)
    if h < 1 or w < 1 or h * w >= 2 ** 31:
        raise ValueError("images must have at least one pixel and fewer than 2^31")
    dev = seg.device
    seg = seg.contiguous()
    if depth is not None:
        depth = depth.to(device=dev, dtype=torch.float32).contiguous()
    stats = torch.empty((n, nid, 7), dtype=torch.int64, device=dev)
    zmin = None if depth is None else torch.empty((n, nid), dtype=torch.float32, device=dev)
    if n:
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(_lib.lib().mre_seg_labels(stream, seg.data_ptr(), None if depth is None else depth.data_ptr(),
                                                 n, h, w, int(id0), int(nid), stats.data_ptr(),
                                                 None if zmin is None else zmin.data_ptr()), "mre_seg_labels")
    return SegLabels(stats[..., 0:4], stats[..., 4], stats[..., 5:7], zmin)


def centroid(labels: SegLabels) -> torch.Tensor:
    """Mean (column, row) of every label's pixels: float64 [N, nid, 2], NaN where the label is absent."""
    cnt = labels.count.to(torch.float64)[..., None]
    nan = torch.full_like(cnt, float("nan"))
    return torch.where(cnt > 0, labels.sum_xy.to(torch.float64) / cnt, nan)
