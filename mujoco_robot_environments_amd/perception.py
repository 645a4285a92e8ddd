"""Frame labels and training inputs from the camera's images: the torch-facing wrappers of ``mre_seg_labels``
(include/mre.h, csrc/mre_labels.hip) and ``mre_heightmap`` (csrc/mre_heightmap.hip).

``seg_labels``: for every env and every label of a small id range of a segmentation image it gives what the
reference's ``props_info`` takes from one (``get_bbox``, tasks/rearrangement.py:254-268: the PASCAL-VOC box of the
visible pixels) and what a caller needs beside it to label frames: the number of visible pixels (0 = hidden), the sums
of their coordinates (the centroid) and the smallest depth among them.  ``BatchedRearrangementEnv.prop_bboxes`` /
``prop_labels`` / ``props_info`` are the users.

``heightmap``: the top-down orthographic height, colour and label maps a Transporter network is trained on, from the
depth / rgb / seg frames of every env (``BatchedRearrangementEnv.heightmap``); ``world_2_cell`` puts pick and place
points into the same map.

The kernels are enqueued on torch's current stream; nothing here synchronises.
"""
from __future__ import annotations

import collections
import ctypes as C
from typing import Optional

import numpy as np
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


# ---------------------------------------------------------------------------------------------------------- heightmaps
# height float32 [N, out_h, out_w] (0 where no pixel landed), colour uint8 [N, out_h, out_w, 3] (0) or None, seg uint8
# [N, out_h, out_w] (255) or None, src int32 [N, out_h, out_w]: the index v * W + u of the cell's source pixel, -1 where
# the cell is empty -- a filled cell may hold height 0.0, so src is what tells filled from empty
HeightMap = collections.namedtuple("HeightMap", ["height", "colour", "seg", "src"])
MAX_MAP = 4096   # rows / columns of a map at most


def heightmap_camera(pos, mat, fovy: float, h: int, w: int) -> np.ndarray:
    """The 12 floats ``heightmap`` takes for a pinhole camera at ``pos`` with rotation ``mat`` (camera to world, looking
    along its -z) and vertical field of view ``fovy`` degrees over ``h`` x ``w`` pixels: A = -R K^-1 row-major, with K of
    ``_get_camera_intrinsics`` (the reference's pixel_2_world, tasks/rearrangement.py:505-531), then ``pos``.  A is formed
    in float64 and rounded once; the world point of pixel (u, v) at depth d is pos + d * A (u, v, 1)."""
    f = (1.0 / np.tan(np.deg2rad(float(fovy)) / 2)) * h / 2.0
    K = np.array([[-f, 0, (w - 1) / 2], [0, f, (h - 1) / 2], [0, 0, 1]])
    A = -np.asarray(mat, np.float64).reshape(3, 3) @ np.linalg.inv(K)
    return np.concatenate([A.reshape(9), np.asarray(pos, np.float64).reshape(3)]).astype(np.float32)


def heightmap_shape(bounds, cell: float):
    """(rows, columns) of the map of ``bounds`` = (lo[3], hi[3]) at ``cell`` metres per cell: rows along y, columns along
    x, the last one partial when the extent is no multiple of the cell."""
    b = np.asarray(bounds, np.float64).reshape(2, 3)
    rows, cols = (max(1, int(np.ceil((b[1, k] - b[0, k]) / float(cell) - 1e-6))) for k in (1, 0))
    return rows, cols


def _grid(bounds, cell):
    """bounds and cell as the float32 values of the statement: lo[3], hi[3], inv_cell."""
    b = np.asarray(bounds, np.float64).reshape(2, 3).astype(np.float32)
    if not (np.isfinite(b).all() and (b[0] <= b[1]).all()):
        raise ValueError("bounds must be finite with lo <= hi")
    if not (np.isfinite(cell) and cell > 0):
        raise ValueError("cell must be positive and finite")
    return b[0], b[1], np.float32(1.0 / float(cell))


def _cells(P0, P1, lo, inv_cell):
    """(column, row) of world x / y as float tensors: floor((P - lo) * inv_cell), every operation rounded on its own."""
    return torch.floor((P0 - float(lo[0])) * float(inv_cell)), torch.floor((P1 - float(lo[1])) * float(inv_cell))


def heightmap_reference(depth: torch.Tensor, rgb: Optional[torch.Tensor] = None, seg: Optional[torch.Tensor] = None, *,
                        cam, bounds, cell: float, max_depth: float = 99.0) -> HeightMap:
    """The statement of ``heightmap`` (include/mre.h, mre_heightmap) in plain torch, float32 operation by operation, on
    whatever device ``depth`` is on and for any strides: the fallback of ``heightmap`` and, on the CPU, bit for bit
    what the kernel computes.  It materialises several int64 images per frame (in slices of about 2^24 pixels); use
    it for small batches and tests."""
    n, h, w = (int(x) for x in depth.shape)
    dev = depth.device
    cam = np.asarray(cam, np.float32).reshape(12)
    lo, hi, inv_cell = _grid(bounds, cell)
    out_h, out_w = heightmap_shape(bounds, cell)
    cells = out_h * out_w
    depth = depth.to(torch.float32)
    u = torch.arange(w, dtype=torch.float32, device=dev).view(1, 1, w)
    v = torch.arange(h, dtype=torch.float32, device=dev).view(1, h, 1)
    index = torch.arange(h * w, dtype=torch.int64, device=dev).view(1, h, w)
    keys = torch.zeros((n, cells), dtype=torch.int64, device=dev)
    step = max(1, (1 << 24) // (h * w))
    for e0 in range(0, n, step):
        d = depth[e0:e0 + step]
        P = []
        for k in range(3):
            t0 = float(cam[3 * k]) * u
            t1 = float(cam[3 * k + 1]) * v
            s = t0 + t1
            s = s + float(cam[3 * k + 2])
            m = d * s
            P.append(m + float(cam[9 + k]))
        cx, cy = _cells(P[0], P[1], lo, inv_cell)
        hz = P[2] - float(lo[2])
        valid = ((d > 0) & (d < float(np.float32(max_depth))) & (cx >= 0) & (cx < out_w) & (cy >= 0) & (cy < out_h)
                 & (P[2] >= float(lo[2])) & (P[2] <= float(hi[2])))
        # hz >= +0 orders like its bits: the largest key is the highest pixel, among equal heights the smallest index
        key = (hz.contiguous().view(torch.int32).to(torch.int64) << 32) | (0xFFFFFFFF - index)
        env = torch.arange(d.shape[0], dtype=torch.int64, device=dev).view(-1, 1, 1)
        where = (env * cells + cy.nan_to_num(0.0, 0.0, 0.0).clamp(0, out_h - 1).to(torch.int64) * out_w
                 + cx.nan_to_num(0.0, 0.0, 0.0).clamp(0, out_w - 1).to(torch.int64))
        keys[e0:e0 + step].view(-1).scatter_reduce_(0, where[valid], key.expand_as(valid)[valid], "amax", include_self=True)
    filled = keys != 0
    src = torch.where(filled, 0xFFFFFFFF - (keys & 0xFFFFFFFF), -1)
    height = torch.where(filled, (keys >> 32).to(torch.int32).view(torch.float32), 0.0).to(torch.float32)
    pick = src.clamp(min=0)
    colour = smap = None
    if rgb is not None:
        colour = torch.gather(rgb.reshape(n, h * w, 3), 1, pick[..., None].expand(-1, -1, 3))
        colour = torch.where(filled[..., None], colour, 0).to(rgb.dtype).view(n, out_h, out_w, 3)
    if seg is not None:
        smap = torch.where(filled, torch.gather(seg.reshape(n, h * w), 1, pick), 255).to(seg.dtype).view(n, out_h, out_w)
    return HeightMap(height.view(n, out_h, out_w), colour, smap, src.to(torch.int32).view(n, out_h, out_w))


def heightmap(depth: torch.Tensor, rgb: Optional[torch.Tensor] = None, seg: Optional[torch.Tensor] = None, *,
              cam, bounds, cell: float, max_depth: float = 99.0) -> HeightMap:
    """Top-down maps of ``bounds`` = (lo[3], hi[3]) at ``cell`` metres per cell from ``depth`` [N, H, W] (and ``rgb``
    [N, H, W, 3], ``seg`` [N, H, W]) seen through ``cam`` (``heightmap_camera``): every pixel with 0 < depth < max_depth
    is pushed back into the world, and cell (row along y, column along x) takes the highest point that lands in it
    inside the bounds, the first pixel among equal heights -- see ``HeightMap`` and include/mre.h for the exact
    statement.  The camera's "nothing hit" depth of 100 is cut by ``max_depth``.  CUDA float32 depth with uint8 rgb /
    seg is one launch of ``mre_heightmap`` (non-contiguous views are made contiguous first); anything else is
    computed by ``heightmap_reference`` with the same return values."""
    if depth.dim() != 3:
        raise ValueError("depth must be [N, H, W]")
    if rgb is not None and tuple(rgb.shape) != tuple(depth.shape) + (3,):
        raise ValueError("rgb must be [N, H, W, 3]")
    if seg is not None and tuple(seg.shape) != tuple(depth.shape):
        raise ValueError("seg must have depth's shape")
    cam = np.ascontiguousarray(np.asarray(cam, np.float32).reshape(12))
    lo, hi, inv_cell = _grid(bounds, cell)
    out_h, out_w = heightmap_shape(bounds, cell)
    if not (np.isfinite(max_depth) and max_depth > 0):
        raise ValueError("max_depth must be positive and finite")
    if out_h > MAX_MAP or out_w > MAX_MAP:
        raise ValueError(f"a map has at most {MAX_MAP} rows and columns")
    n, h, w = (int(x) for x in depth.shape)
    if h < 1 or w < 1 or h * w >= 2 ** 31:
        raise ValueError("images must have at least one pixel and fewer than 2^31")
    dev = depth.device
    on_device = depth.is_cuda and depth.dtype == torch.float32 and all(
        x is None or (x.device == dev and x.dtype == torch.uint8) for x in (rgb, seg))
    if not on_device:
        return heightmap_reference(depth, rgb, seg, cam=cam, bounds=bounds, cell=cell, max_depth=max_depth)
    depth = depth.contiguous()
    rgb = None if rgb is None else rgb.contiguous()
    seg = None if seg is None else seg.contiguous()
    height = torch.empty((n, out_h, out_w), dtype=torch.float32, device=dev)
    colour = None if rgb is None else torch.empty((n, out_h, out_w, 3), dtype=torch.uint8, device=dev)
    smap = None if seg is None else torch.empty((n, out_h, out_w), dtype=torch.uint8, device=dev)
    src = torch.empty((n, out_h, out_w), dtype=torch.int32, device=dev)
    if n:
        ptr = lambda t: None if t is None else t.data_ptr()
        b = np.ascontiguousarray(np.concatenate([lo, hi]), np.float32)
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(_lib.lib().mre_heightmap(stream, depth.data_ptr(), ptr(rgb), ptr(seg), n, h, w, cam.ctypes.data,
                                                b.ctypes.data, float(inv_cell), float(np.float32(max_depth)), out_h, out_w,
                                                height.data_ptr(), ptr(colour), ptr(smap), src.data_ptr()), "mre_heightmap")
    return HeightMap(height, colour, smap, src)


def world_2_cell(points, bounds, cell: float):
    """(column, row) of world points [..., 3] (or [..., 2]: x, y) in the map of ``bounds`` at ``cell``, by the float32
    statements of ``heightmap`` -- floor((x - lo_x) * inv_cell), floor((y - lo_y) * inv_cell) -- so that a pick or place
    position lands in the cell its own pixels land in.  int64 [..., 2], a torch tensor for a tensor and a numpy array for
    anything else; a point outside the bounds gives a cell outside 0 .. columns - 1, 0 .. rows - 1 (not clipped)."""
    lo, _, inv_cell = _grid(bounds, cell)
    is_tensor = isinstance(points, torch.Tensor)
    p = (points if is_tensor else torch.as_tensor(np.asarray(points, np.float64))).to(torch.float32)
    cx, cy = _cells(p[..., 0], p[..., 1], lo, inv_cell)
    out = torch.stack([cx, cy], dim=-1).to(torch.int64)
    return out if is_tensor else out.cpu().numpy()
