"""Frame labels, training inputs and the place decision from the camera's images: the torch-facing wrappers of
``mre_seg_labels`` (include/mre.h, csrc/mre_labels.hip), ``mre_heightmap`` (csrc/mre_heightmap.hip), ``mre_warp_maps``
(csrc/mre_warp.hip), ``mre_warp_inputs`` (csrc/mre_warp_inputs.hip) and ``mre_correlate`` (csrc/mre_correlate.hip).

``seg_labels``: for every env and every label of a small id range of a segmentation image it gives what the
reference's ``props_info`` takes from one (``get_bbox``, tasks/rearrangement.py:254-268: the PASCAL-VOC box of the
visible pixels) and what a caller needs beside it to label frames: the number of visible pixels (0 = hidden), the sums
of their coordinates (the centroid) and the smallest depth among them.  ``BatchedRearrangementEnv.prop_bboxes`` /
``prop_labels`` / ``props_info`` are the users.

``heightmap``: the top-down orthographic height, colour and label maps a Transporter network is trained on, from the
depth / rgb / seg frames of every env (``BatchedRearrangementEnv.heightmap``); ``world_2_cell`` puts pick and place
points into the same map.

``heightmap_views``: the same maps from several cameras in one launch of ``mre_heightmap_views``
(csrc/mre_heightmap_views.hip) -- every view's pixels compete for the cells, so that what one camera cannot see another
fills in; a ``FusedHeightMap`` also says which view every cell came from (``BatchedRearrangementEnv.heightmap_views``).

``warp_maps``: a nearest-neighbour affine gather of those maps, and on it what a Transporter learner does to every
sample: a random SE(2) perturbation of the map with its pick and place cells (``sample_perturbation``) and the rotated
crops around the pick cell (``crop_matrices``), together ``transporter_sample``
(``BatchedRearrangementEnv.transporter_sample``).

``warp_inputs``: the same gather written as the tensor a network consumes -- channels-first, normalised per channel
(``Channels``), float32 or bfloat16 -- by ``mre_warp_inputs`` (csrc/mre_warp_inputs.hip) in one launch, and on it
``transporter_batch`` (``BatchedRearrangementEnv.transporter_batch``): the perturbed scene, the rotated pick crops and the
label indices of a Transporter training batch, ready for a convolution.

``correlate``: what consumes the network's output -- a Transporter's place head: every env's scene features
cross-correlated with its own rotated crop features by ``mre_correlate`` (csrc/mre_correlate.hip, bf16 matrix cores), the
best (rotation, row, column) per env without the logits ever being written; ``decode_place`` and ``cell_2_world`` turn it
into cells, rotation bins and world positions (``BatchedRearrangementEnv.transporter_place``).

``place_loss``: what trains that head -- the softmax cross-entropy of every env's logits against a target cell
(``encode_place``) as a ``torch.autograd.Function`` over ``mre_correlate_loss``, ``mre_correlate_dlogits``,
``mre_correlate_grad_scene`` and ``mre_correlate_grad_kern`` (csrc/mre_correlate_grad.hip), without a logit stored;
``correlate_backward`` is the gradient pair alone, for any loss (``BatchedRearrangementEnv.transporter_loss``).

``attend`` and ``pick_loss``: the other head -- from the logits of an attention network the pick cell of every env
(``mre_attend``, csrc/mre_attend.hip: one read of the logits) and the loss that trains that network with its gradient
(``mre_attend_dlogits``); ``crop_matrices_device`` centres the rotated crops on pick cells that live on the device, so
that ``BatchedRearrangementEnv.transporter_act`` runs observation -> pick -> crops -> place without a synchronise.

The kernels are enqueued on torch's current stream; nothing here synchronises.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
import functools
from typing import Optional

import numpy as np
import torch

from . import lib as _lib
from . import rng

PROP_GEOM_ID0 = 12   # geom ids of prop_0..3 in the compiled scene (tasks/rearrangement.py)
MAX_IDS = 8          # labels of one mre_seg_labels call

# box int64 [N, nid, (xmin, ymin, xmax, ymax)] (-1 where the label is absent), count int64 [N, nid],
# sum_xy int64 [N, nid, (sum of columns, sum of rows)], zmin float32 [N, nid] (+inf where absent) or None
SegLabels = collections.namedtuple("SegLabels", ["box", "count", "sum_xy", "zmin"])


@contextlib.contextmanager
def _stream_on(dev):
    """torch's current stream on ``dev`` as the C ABI takes it, with ``dev`` the current device while a kernel is enqueued."""
    with torch.cuda.device(dev):
        yield C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ptr(t):
    """A tensor, or None, as the C ABI takes a pointer."""
    return None if t is None else t.data_ptr()


@functools.lru_cache(maxsize=64)
def _workspace_bytes(entry: str, *shape) -> int:   # what the library's ``entry`` (an ``mre_*_workspace``) asks for ``shape``
    nbytes = C.c_size_t(0)
    _lib.check(getattr(_lib.lib(), entry)(*shape, C.byref(nbytes)), entry)
    return int(nbytes.value)


def _workspace(entry: str, dev, *shape):
    """The workspace of a call: a ``torch.empty`` of ``_workspace_bytes(entry, *shape)`` bytes on ``dev``, and that number."""
    nbytes = _workspace_bytes(entry, *shape)
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev), nbytes


def _empty_if(on: bool, shape, dtype, dev):   # an output that is asked for, or None
    return torch.empty(shape, dtype=dtype, device=dev) if on else None


def _in_place(dtypes, *tensors) -> bool:   # what a kernel reads in place: contiguous CUDA tensors of one of ``dtypes``
    return all(t.is_cuda and t.dtype in dtypes and t.is_contiguous() for t in tensors)


def _maps_on_device(height, *companions) -> bool:
    """What the warp kernels read in place: a contiguous CUDA float32 ``height`` with contiguous uint8 companions (or None)
    on its device."""
    given = [x for x in companions if x is not None]
    return _in_place((torch.float32,), height) and _in_place((torch.uint8,), *given) and all(
        x.device == height.device for x in given)


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
        with _stream_on(dev) as stream:
            _lib.check(_lib.lib().mre_seg_labels(stream, seg.data_ptr(), _ptr(depth),
                                                 n, h, w, int(id0), int(nid), stats.data_ptr(),
                                                 _ptr(zmin)), "mre_seg_labels")
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


def _map_grid(bounds, cell, max_depth):
    """The checks of a map every entry makes: ``_grid``, then ``max_depth`` and the map's size.  lo[3], hi[3], inv_cell,
    rows, columns."""
    lo, hi, inv_cell = _grid(bounds, cell)
    out_h, out_w = heightmap_shape(bounds, cell)
    if not (np.isfinite(max_depth) and max_depth > 0):
        raise ValueError("max_depth must be positive and finite")
    if out_h > MAX_MAP or out_w > MAX_MAP:
        raise ValueError(f"a map has at most {MAX_MAP} rows and columns")
    return lo, hi, inv_cell, out_h, out_w


def _check_frames(depth, rgb, seg) -> None:
    """The shapes of one view's frames.  (The pixel limit is each entry's own, in its own place among the checks.)"""
    if depth.dim() != 3:
        raise ValueError("depth must be [N, H, W]")
    if rgb is not None and tuple(rgb.shape) != tuple(depth.shape) + (3,):
        raise ValueError("rgb must be [N, H, W, 3]")
    if seg is not None and tuple(seg.shape) != tuple(depth.shape):
        raise ValueError("seg must have depth's shape")


def _empty_maps(n, out_h, out_w, dev, colour: bool, seg: bool):
    """The four outputs of a launch, uninitialised: height, colour or None, seg or None, src."""
    return (torch.empty((n, out_h, out_w), dtype=torch.float32, device=dev),
            torch.empty((n, out_h, out_w, 3), dtype=torch.uint8, device=dev) if colour else None,
            torch.empty((n, out_h, out_w), dtype=torch.uint8, device=dev) if seg else None,
            torch.empty((n, out_h, out_w), dtype=torch.int32, device=dev))


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
    _check_frames(depth, rgb, seg)
    cam = np.ascontiguousarray(np.asarray(cam, np.float32).reshape(12))
    lo, hi, inv_cell, out_h, out_w = _map_grid(bounds, cell, max_depth)
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
    height, colour, smap, src = _empty_maps(n, out_h, out_w, dev, rgb is not None, seg is not None)
    if n:
        b = np.ascontiguousarray(np.concatenate([lo, hi]), np.float32)
        with _stream_on(dev) as stream:
            _lib.check(_lib.lib().mre_heightmap(stream, depth.data_ptr(), _ptr(rgb), _ptr(seg), n, h, w, cam.ctypes.data,
                                                b.ctypes.data, float(inv_cell), float(np.float32(max_depth)), out_h, out_w,
                                                height.data_ptr(), _ptr(colour), _ptr(smap), src.data_ptr()), "mre_heightmap")
    return HeightMap(height, colour, smap, src)


# ------------------------------------------------------------------------------------------ several views, one set of maps
# HeightMap's four fields, so that whatever indexes maps[0 .. 3] takes it as it is, then view uint8 [N, out_h, out_w]: the
# view whose pixel the cell holds, 255 where the cell is empty.  src is the pixel's index inside THAT view's image.
FusedHeightMap = collections.namedtuple("FusedHeightMap", ["height", "colour", "seg", "src", "view"])
MAX_VIEWS = 8              # MRE_HM_MAX_VIEWS
MAX_VIEW_PIXELS = 2 ** 28  # pixels of one view's image, exclusive


def _views_args(views, bounds, cell, max_depth):
    """The argument checks of ``heightmap_views``: [(depth, rgb, seg, cam float32 [12])] with every view of ``heightmap``'s
    shapes, the same number of frames, and rgb / seg in every view or in none."""
    views = [tuple(v) for v in views]
    if not 1 <= len(views) <= MAX_VIEWS:
        raise ValueError(f"1 to {MAX_VIEWS} views")
    _map_grid(bounds, cell, max_depth)
    res = []
    for v in views:
        if len(v) != 4:
            raise ValueError("a view is (depth, rgb, seg, cam)")
        depth, rgb, seg, cam = v
        _check_frames(depth, rgb, seg)
        h, w = int(depth.shape[1]), int(depth.shape[2])
        if h < 1 or w < 1 or h * w >= MAX_VIEW_PIXELS:
            raise ValueError("a view's images must have at least one pixel and fewer than 2^28")
        res.append((depth, rgb, seg, np.ascontiguousarray(np.asarray(cam, np.float32).reshape(12))))
    if len({int(v[0].shape[0]) for v in res}) != 1:
        raise ValueError("every view holds the same number of frames")
    for k, what in ((1, "rgb"), (2, "seg")):
        if len({v[k] is None for v in res}) != 1:
            raise ValueError(f"{what} is given for every view or for none")
    return res


def heightmap_views_reference(views, *, bounds, cell: float, max_depth: float = 99.0) -> FusedHeightMap:
    """The statement of ``heightmap_views`` (include/mre.h, mre_heightmap_views) as the composition it replaces:
    ``heightmap`` of every view of ``views`` = [(depth, rgb, seg, cam)], then the merge in plain torch on the first view's
    device -- a cell takes the view with the largest height among those that filled it, the lowest view among equal
    heights.  Bit for bit the statement on any device; the fallback of ``heightmap_views``."""
    views = _views_args(views, bounds, cell, max_depth)
    dev = views[0][0].device
    out = None
    for i, (depth, rgb, seg, cam) in enumerate(views):
        m = heightmap(depth, rgb, seg, cam=cam, bounds=bounds, cell=cell, max_depth=max_depth)
        m = HeightMap(*(None if x is None else x.to(dev) for x in m))
        filled = m.src >= 0
        which = torch.where(filled, i, 255).to(torch.uint8)
        if out is None:
            out = FusedHeightMap(m.height, m.colour, m.seg, m.src, which)
            continue
        # hz >= +0 orders like its bits; strictly higher only, so that the lower view keeps a tie
        take = filled & ((out.src < 0) | (m.height.view(torch.int32) > out.height.view(torch.int32)))
        out = FusedHeightMap(torch.where(take, m.height, out.height),
                             None if m.colour is None else torch.where(take[..., None], m.colour, out.colour),
                             None if m.seg is None else torch.where(take, m.seg, out.seg),
                             torch.where(take, m.src, out.src), torch.where(take, which, out.view))
    return out


def heightmap_views(views, *, bounds, cell: float, max_depth: float = 99.0) -> FusedHeightMap:
    """One set of top-down maps from several cameras: ``views`` is a sequence of up to 8 (depth [N, H, W], rgb
    [N, H, W, 3] or None, seg [N, H, W] or None, cam) -- what ``heightmap`` takes for one view; the views may differ in
    H x W, and rgb / seg are given for every view or for none.  Every view's pixels are binned as ``heightmap`` bins them
    and compete for the cells: a cell takes the highest point any view saw in it, the lowest view among equal heights,
    the first pixel inside that view -- the merge of the views' own ``heightmap`` outputs; see ``FusedHeightMap`` and
    include/mre.h.  CUDA float32 depths with uint8 rgb / seg, all on one device, are one launch of
    ``mre_heightmap_views`` (non-contiguous views are made contiguous first); anything else is computed by
    ``heightmap_views_reference`` with the same return values.  One view gives ``heightmap``'s maps."""
    views = _views_args(views, bounds, cell, max_depth)
    dev = views[0][0].device
    on_device = all(d.is_cuda and d.device == dev and d.dtype == torch.float32 and all(
        x is None or (x.device == dev and x.dtype == torch.uint8) for x in (rgb, seg)) for d, rgb, seg, _ in views)
    if not on_device:
        return heightmap_views_reference(views, bounds=bounds, cell=cell, max_depth=max_depth)
    views = [(d.contiguous(), None if rgb is None else rgb.contiguous(), None if seg is None else seg.contiguous(), cam)
             for d, rgb, seg, cam in views]
    lo, hi, inv_cell, out_h, out_w = _map_grid(bounds, cell, max_depth)
    n, nv = int(views[0][0].shape[0]), len(views)
    has_rgb, has_seg = views[0][1] is not None, views[0][2] is not None
    height, colour, smap, src = _empty_maps(n, out_h, out_w, dev, has_rgb, has_seg)
    which = torch.empty((n, out_h, out_w), dtype=torch.uint8, device=dev)
    if n:
        pointers = lambda k: (C.c_void_p * nv)(*[v[k].data_ptr() for v in views])
        sizes = np.ascontiguousarray([[v[0].shape[1], v[0].shape[2]] for v in views], np.int32).T.copy()
        cams = np.ascontiguousarray(np.stack([v[3] for v in views]), np.float32)
        b = np.ascontiguousarray(np.concatenate([lo, hi]), np.float32)
        with _stream_on(dev) as stream:
            _lib.check(_lib.lib().mre_heightmap_views(
                stream, nv, pointers(0), pointers(1) if has_rgb else None, pointers(2) if has_seg else None, n,
                sizes[0].ctypes.data, sizes[1].ctypes.data, cams.ctypes.data, b.ctypes.data, float(inv_cell),
                float(np.float32(max_depth)), out_h, out_w, height.data_ptr(), _ptr(colour), _ptr(smap), src.data_ptr(),
                which.data_ptr()), "mre_heightmap_views")
    return FusedHeightMap(height, colour, smap, src, which)


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


# ------------------------------------------------------------------------------------------- warped and cropped maps
# height float32 [S, out_h, out_w] (0 where the source cell does not exist), colour uint8 [S, out_h, out_w, 3] (0) or None,
# seg uint8 [S, out_h, out_w] (255) or None, source int32 [S, out_h, out_w]: row * in_w + column of the source cell inside
# its map, -1 where it does not exist, or None
WarpedMaps = collections.namedtuple("WarpedMaps", ["height", "colour", "seg", "source"])
# F float64 [N, 2, 3] (source cell -> perturbed cell), M float32 [N, 6] (its inverse: the mats of warp_maps), cells int64
# [N, K, 2] (the label cells moved by F), tries int64 [N] (the accepted attempt, from 1; -1: none, identity)
Perturbation = collections.namedtuple("Perturbation", ["F", "M", "cells", "tries"])
# maps: the perturbed WarpedMaps [N, rows, columns]; pick, place int64 [N, 2] (column, row) in them; crops: WarpedMaps of
# leading shape [N, n_rotations]; tries as in Perturbation
TransporterSample = collections.namedtuple("TransporterSample", ["maps", "pick", "place", "crops", "tries"])


def _affine(a, b, tx, c, d, ty) -> np.ndarray:
    """[[a, b, tx], [c, d, ty]] of broadcastable float64 arrays: [..., 2, 3]."""
    a, b, tx, c, d, ty = np.broadcast_arrays(a, b, tx, c, d, ty)
    return np.stack([np.stack([a, b, tx], axis=-1), np.stack([c, d, ty], axis=-1)], axis=-2)


def se2_forward(theta, shift, pivot) -> np.ndarray:
    """F = T(pivot + shift) R(theta) T(-pivot) in (column, row) cell coordinates, R = [[cos, -sin], [sin, cos]]: the
    rigid motion that turns a map by ``theta`` about ``pivot`` [..., 2] and then moves it by ``shift`` [..., 2].
    float64 [..., 2, 3]; element-wise arithmetic only, so a row does not depend on what else is in the batch."""
    theta = np.asarray(theta, np.float64)
    shift, pivot = np.asarray(shift, np.float64), np.asarray(pivot, np.float64)
    cos, sin = np.cos(theta), np.sin(theta)
    px, py = pivot[..., 0], pivot[..., 1]
    tx = px + shift[..., 0] - (cos * px - sin * py)
    ty = py + shift[..., 1] - (sin * px + cos * py)
    return _affine(cos, -sin, tx, sin, cos, ty)


def invert_affine(F) -> np.ndarray:
    """The inverse of affine maps ``F`` [..., 2, 3], float64 [..., 2, 3]: for a forward motion F (source -> output) it
    is the M of ``warp_maps`` (output -> source)."""
    F = np.asarray(F, np.float64)
    a, b, tx, c, d, ty = F[..., 0, 0], F[..., 0, 1], F[..., 0, 2], F[..., 1, 0], F[..., 1, 1], F[..., 1, 2]
    det = a * d - b * c
    ia, ib, ic, id_ = d / det, -b / det, -c / det, a / det
    return _affine(ia, ib, -(ia * tx + ib * ty), ic, id_, -(ic * tx + id_ * ty))


def affine_mats(M) -> np.ndarray:
    """Affine maps [..., 2, 3] as the float32 [S, 6] rows ``warp_maps`` takes: rounded to float32 once."""
    return np.ascontiguousarray(np.asarray(M, np.float64).reshape(-1, 6).astype(np.float32))


def transform_cells(F, cells) -> np.ndarray:
    """floor(F p + 0.5) for cells p = (column, row): int64.  ``F`` [..., 2, 3]; ``cells`` [..., 2], one cell per map, or
    [..., K, 2], K cells per map."""
    F, p = np.asarray(F, np.float64), np.asarray(cells, np.float64)
    single = p.ndim == F.ndim - 1
    if not single:
        F = F[..., None, :, :]
    x = F[..., 0, 0] * p[..., 0] + F[..., 0, 1] * p[..., 1] + F[..., 0, 2]
    y = F[..., 1, 0] * p[..., 0] + F[..., 1, 1] * p[..., 1] + F[..., 1, 2]
    return np.floor(np.stack([x, y], axis=-1) + 0.5).astype(np.int64)


def _quarter_exact(k: int, n: int):
    """cos and sin of 2 pi k / n, exactly 0 and +-1 at the quarter turns."""
    if (4 * k) % n == 0:
        q = (4 * k // n) % 4
        return (1.0, 0.0, -1.0, 0.0)[q], (0.0, 1.0, 0.0, -1.0)[q]
    a = 2.0 * np.pi * k / n
    return float(np.cos(a)), float(np.sin(a))


def crop_matrices(cells, n_rotations: int = 36, crop: int = 64):
    """The ``mats`` float32 [N * n_rotations, 6] and ``index`` int32 [N * n_rotations] of the rotated crops around the
    pivots ``cells`` [N, 2] (column, row): sample i * n_rotations + k is the crop x crop window centred on pivot i and
    turned by 2 pi k / n_rotations, M = T(p) R(2 pi k / n_rotations) T(-crop / 2, -crop / 2), read from map i.  At k = 0
    the entries are exactly 1, 0 and integers (crop even): the crop is the slice [p - crop / 2, p + crop / 2) of the
    zero-padded map.  Formed in float64 and rounded to float32 once."""
    p = np.asarray(cells, np.float64).reshape(-1, 2)
    if n_rotations < 1 or crop < 1:
        raise ValueError("n_rotations and crop must be at least 1")
    M = np.empty((len(p), n_rotations, 2, 3), np.float64)
    half = np.array([crop / 2.0, crop / 2.0])
    for k in range(n_rotations):
        cos, sin = _quarter_exact(k, n_rotations)
        R = np.array([[cos, -sin], [sin, cos]])
        M[:, k, :, :2] = R
        M[:, k, :, 2] = p - R @ half
    index = np.repeat(np.arange(len(p), dtype=np.int32), n_rotations)
    return affine_mats(M), index


def _warp_args(height, colour, seg, mats, index, out_shape):
    """The checked arguments of warp_maps / warp_maps_reference: (n, in_h, in_w, samples, out_h, out_w)."""
    if height.dim() != 3:
        raise ValueError("height must be [N, H, W]")
    if colour is not None and tuple(colour.shape) != tuple(height.shape) + (3,):
        raise ValueError("colour must be [N, H, W, 3]")
    if seg is not None and tuple(seg.shape) != tuple(height.shape):
        raise ValueError("seg must have height's shape")
    n, in_h, in_w = (int(x) for x in height.shape)
    if mats.dim() != 2 or mats.shape[1] != 6:
        raise ValueError("mats must be [S, 6] or [S, 2, 3]")
    samples = int(mats.shape[0])
    if index is None:
        if samples > n:
            raise ValueError("more samples than maps: give index, the source map of every sample")
    elif index.dim() != 1 or int(index.shape[0]) != samples:
        raise ValueError("index must be [S], one source map per row of mats")
    out_h, out_w = (in_h, in_w) if out_shape is None else (int(out_shape[0]), int(out_shape[1]))
    if not all(1 <= x <= MAX_MAP for x in (in_h, in_w, out_h, out_w)):
        raise ValueError(f"maps have between 1 and {MAX_MAP} rows and columns")
    return n, in_h, in_w, samples, out_h, out_w


def _as_mats(mats, dev):
    if isinstance(mats, torch.Tensor):
        m = mats.to(device=dev, dtype=torch.float32)
    else:
        m = torch.from_numpy(np.ascontiguousarray(np.asarray(mats, np.float32))).to(dev)
    return m.reshape(-1, 6).contiguous() if m.dim() == 3 and tuple(m.shape[1:]) == (2, 3) else m.contiguous()


def _as_index(index, dev):
    if index is None:
        return None
    if isinstance(index, torch.Tensor):
        return index.to(device=dev, dtype=torch.int32).contiguous()
    i = np.asarray(index)
    if i.size and (i.min() < -2 ** 31 or i.max() > 2 ** 31 - 1):
        raise ValueError("index must hold int32 values")
    return torch.from_numpy(np.ascontiguousarray(i.astype(np.int32))).to(dev)


def warp_maps_reference(height: torch.Tensor, colour: Optional[torch.Tensor] = None, seg: Optional[torch.Tensor] = None, *,
                        mats, index=None, out_shape=None, with_source: bool = True) -> WarpedMaps:
    """The statement of ``warp_maps`` (include/mre.h, mre_warp_maps) in plain torch, float32 operation by operation, on
    whatever device ``height`` is on and for any strides: the fallback of ``warp_maps`` and, on the CPU, bit for bit
    what the kernel computes.  It materialises int64 index images (in slices of about 2^24 cells); use it for small
    batches and tests."""
    dev = height.device
    mats, index = _as_mats(mats, dev), _as_index(index, dev)
    n, in_h, in_w, samples, out_h, out_w = _warp_args(height, colour, seg, mats, index, out_shape)
    hw = in_h * in_w
    c = torch.arange(out_w, dtype=torch.float32, device=dev).view(1, 1, out_w)
    r = torch.arange(out_h, dtype=torch.float32, device=dev).view(1, out_h, 1)
    e_all = torch.arange(samples, dtype=torch.int64, device=dev) if index is None else index.to(torch.int64)
    out_hz = torch.empty((samples, out_h, out_w), dtype=torch.float32, device=dev)
    out_c = None if colour is None else torch.empty((samples, out_h, out_w, 3), dtype=colour.dtype, device=dev)
    out_s = None if seg is None else torch.empty((samples, out_h, out_w), dtype=seg.dtype, device=dev)
    source = torch.empty((samples, out_h, out_w), dtype=torch.int32, device=dev) if with_source else None
    if n == 0 or samples == 0:
        return WarpedMaps(out_hz, out_c, out_s, source)
    flat_h = height.to(torch.float32).reshape(-1)
    flat_c = None if colour is None else colour.reshape(-1, 3)
    flat_s = None if seg is None else seg.reshape(-1)
    step = max(1, (1 << 24) // (out_h * out_w))
    for s0 in range(0, samples, step):
        m = mats[s0:s0 + step]
        e = e_all[s0:s0 + step].view(-1, 1, 1)
        k = [m[:, j].view(-1, 1, 1) for j in range(6)]
        a = k[0] * c
        b = k[1] * r
        x = a + b
        x = x + k[2]
        x = x + 0.5
        fx = torch.floor(x)
        a = k[3] * c
        b = k[4] * r
        y = a + b
        y = y + k[5]
        y = y + 0.5
        fy = torch.floor(y)
        valid = (e >= 0) & (e < n) & (fx >= 0) & (fx < in_w) & (fy >= 0) & (fy < in_h)
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        src = torch.where(valid, fy, zero).to(torch.int64) * in_w + torch.where(valid, fx, zero).to(torch.int64)
        where = torch.where(valid, e, 0) * hw + src
        out_hz[s0:s0 + step] = torch.where(valid, flat_h[where], zero)
        if out_c is not None:
            out_c[s0:s0 + step] = torch.where(valid[..., None], flat_c[where], 0).to(colour.dtype)
        if out_s is not None:
            out_s[s0:s0 + step] = torch.where(valid, flat_s[where], 255).to(seg.dtype)
        if source is not None:
            source[s0:s0 + step] = torch.where(valid, src, -1).to(torch.int32)
    return WarpedMaps(out_hz, out_c, out_s, source)


def warp_maps(height: torch.Tensor, colour: Optional[torch.Tensor] = None, seg: Optional[torch.Tensor] = None, *,
              mats, index=None, out_shape=None, with_source: bool = True) -> WarpedMaps:
    """A nearest-neighbour affine gather of the maps ``height`` [N, H, W] (and ``colour`` [N, H, W, 3], ``seg``
    [N, H, W]): output cell (row r, column c) of sample s takes the cell ``mats[s]`` (float32 [S, 6] or [S, 2, 3], OUTPUT
    cell -> SOURCE cell, numpy or tensor) sends it to, rounded to the nearest, in map ``index[s]`` (int32 [S]; None: map
    s, then S <= N) -- or 0 / (0, 0, 0) / 255 / source -1 where that cell or map does not exist.  See ``WarpedMaps`` and
    include/mre.h for the exact statement; ``out_shape`` = (rows, columns) defaults to the input's.  ``se2_forward`` /
    ``invert_affine`` / ``crop_matrices`` build the matrices.  Contiguous CUDA float32 height with uint8 colour / seg is
    one launch of ``mre_warp_maps`` on torch's current stream, without a synchronise; anything else is computed by
    ``warp_maps_reference`` with the same return values."""
    dev = height.device
    if not _maps_on_device(height, colour, seg):
        return warp_maps_reference(height, colour, seg, mats=mats, index=index, out_shape=out_shape,
                                   with_source=with_source)
    mats, index = _as_mats(mats, dev), _as_index(index, dev)
    n, in_h, in_w, samples, out_h, out_w = _warp_args(height, colour, seg, mats, index, out_shape)
    out_hz = torch.empty((samples, out_h, out_w), dtype=torch.float32, device=dev)
    out_c = None if colour is None else torch.empty((samples, out_h, out_w, 3), dtype=torch.uint8, device=dev)
    out_s = None if seg is None else torch.empty((samples, out_h, out_w), dtype=torch.uint8, device=dev)
    source = torch.empty((samples, out_h, out_w), dtype=torch.int32, device=dev) if with_source else None
    if n and samples:
        with _stream_on(dev) as stream:
            _lib.check(_lib.lib().mre_warp_maps(stream, height.data_ptr(), _ptr(colour), _ptr(seg), n, in_h, in_w, _ptr(index),
                                                mats.data_ptr(), samples, out_h, out_w, out_hz.data_ptr(), _ptr(out_c),
                                                _ptr(out_s), _ptr(source)), "mre_warp_maps")
    return WarpedMaps(out_hz, out_c, out_s, source)


def sample_perturbation(seed: int, env_ids, draw: int, cells, shape, max_theta: float = np.pi, max_shift=None,
                        max_tries: int = 16) -> Perturbation:
    """A random rigid motion of the map of every env that keeps the env's label cells inside it: see ``Perturbation``.
    ``cells`` int [N, K, 2] (column, row) are the label cells (pick, place), ``shape`` = (rows, columns) the map.  Attempt
    a = 0 .. max_tries - 1 of an env draws u = rng.uniform(seed, env id, draw * max_tries + a, 3): theta =
    (2 u0 - 1) max_theta about the map's centre ((columns - 1) / 2, (rows - 1) / 2), shift = (2 u1 - 1, 2 u2 - 1)
    max_shift cells (default: a quarter of the smaller side); the first attempt whose moved cells are all inside the map
    is taken.  A pure function of (seed, global env id, draw): the same whatever the order or the sharding of the envs.
    An env without an accepted attempt gets the identity and tries = -1.  The distribution is this project's choice."""
    ids = np.asarray(env_ids, np.int64).reshape(-1)
    n = len(ids)
    cells = np.asarray(cells, np.int64).reshape(n, -1, 2)
    rows, cols = int(shape[0]), int(shape[1])
    max_shift = min(rows, cols) / 4.0 if max_shift is None else float(max_shift)
    pivot = np.array([(cols - 1) / 2.0, (rows - 1) / 2.0])
    F = np.broadcast_to(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (n, 2, 3)).copy()
    moved, tries = cells.copy(), np.full(n, -1, np.int64)
    pending = np.arange(n)
    for attempt in range(int(max_tries)):
        if not len(pending):
            break
        u = rng.uniform(seed, ids[pending], [int(draw) * int(max_tries) + attempt], 3)[0]
        Fa = se2_forward((2.0 * u[:, 0] - 1.0) * float(max_theta), (2.0 * u[:, 1:3] - 1.0) * max_shift, pivot)
        q = transform_cells(Fa, cells[pending])
        ok = ((q[..., 0] >= 0) & (q[..., 0] < cols) & (q[..., 1] >= 0) & (q[..., 1] < rows)).all(axis=1)
        took = pending[ok]
        F[took], moved[took], tries[took] = Fa[ok], q[ok], attempt + 1
        pending = pending[~ok]
    return Perturbation(F, affine_mats(invert_affine(F)), moved, tries)


def _label_cells(pick_cells, place_cells, n: int) -> np.ndarray:
    """The pick and place cells of ``n`` envs (tensors or arrays [N, 2]) as ``sample_perturbation`` takes them: int64 [N, 2, 2]."""
    to_np = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    cells = np.stack([to_np(pick_cells), to_np(place_cells)], axis=1).astype(np.int64)
    if cells.shape != (n, 2, 2):
        raise ValueError("pick_cells and place_cells must be [N, 2]")
    return cells


def transporter_sample(maps, pick_cells, place_cells, *, seed: int, env_ids, draw: int, n_rotations: int = 36,
                       crop: int = 64) -> TransporterSample:
    """One Transporter training sample per env from its ``maps`` (a ``HeightMap`` / ``WarpedMaps``, or (height, colour,
    seg)): the maps under ``sample_perturbation(seed, env_ids, draw)`` of the pick and place cells ([N, 2] (column,
    row)), both cells moved with them, and ``n_rotations`` crops of ``crop`` x ``crop`` cells of the perturbed maps around
    the moved pick cell, crop k turned by 2 pi k / n_rotations (``crop_matrices``): see ``TransporterSample``.  Two
    launches of ``mre_warp_maps`` for CUDA maps."""
    height, colour, seg = maps[0], maps[1], maps[2]
    n = int(height.shape[0])
    cells = _label_cells(pick_cells, place_cells, n)
    pert =sample_perturbation(seed, env_ids, draw, cells, tuple(height.shape[1:3]))
    warped = warp_maps(height, colour, seg, mats=pert.M)
    mats, index = crop_matrices(pert.cells[:, 0], n_rotations, crop)
    flat = warp_maps(warped.height, warped.colour, warped.seg, mats=mats, index=index, out_shape=(crop, crop))
    crops = WarpedMaps(*[None if x is None else x.view((n, n_rotations) + tuple(x.shape[1:])) for x in flat])
    return TransporterSample(warped, pert.cells[:, 0], pert.cells[:, 1], crops, pert.tries)


# ------------------------------------------------------------------------------------------------- network inputs
SRC_RED, SRC_GREEN, SRC_BLUE, SRC_HEIGHT = 0, 1, 2, 3   # MRE_SRC_* of include/mre.h
MAX_CHANNELS = 8
_DTYPES = {torch.float32: 0, torch.bfloat16: 1}          # MRE_F32, MRE_BF16
# hi_z - lo_z of tasks.rearrangement.HEIGHTMAP_BOUNDS in metres (tests/test_warp_inputs.py holds the two together): the
# heights of the default maps lie in [0, HEIGHT_SPAN]
HEIGHT_SPAN = 0.3


class Channels(collections.namedtuple("Channels", ["sources", "scales", "biases"])):
    """The channels of a network input: channel k holds source ``sources[k]`` (0 red, 1 green, 2 blue, 3 height; they may
    repeat, in any order, 1 to 8 of them) of the gathered cell as a float32, times ``scales[k]``, plus ``biases[k]`` --
    two float32 operations, each rounded.  A cell whose source cell does not exist is a raw 0, so it holds the bias.
    Scales and biases are finite and are kept as the float32 values the kernel is given."""
    __slots__ = ()

    def __new__(cls, sources, scales=None, biases=None):
        src = tuple(int(x) for x in sources)
        one = lambda v, fill: np.broadcast_to(np.asarray(fill if v is None else v, np.float64), (len(src),))
        with np.errstate(over="ignore"):   # a value beyond float32 becomes an inf, which is refused below
            sc, bi = one(scales, 1.0).astype(np.float32), one(biases, 0.0).astype(np.float32)
        if not 1 <= len(src) <= MAX_CHANNELS:
            raise ValueError(f"between 1 and {MAX_CHANNELS} channels")
        if any(x not in (SRC_RED, SRC_GREEN, SRC_BLUE, SRC_HEIGHT) for x in src):
            raise ValueError("a channel's source is 0 (red), 1 (green), 2 (blue) or 3 (height)")
        if not (np.isfinite(sc).all() and np.isfinite(bi).all()):
            raise ValueError("scales and biases must be finite (as float32)")
        return super().__new__(cls, src, tuple(float(x) for x in sc), tuple(float(x) for x in bi))

    @classmethod
    def from_mean_std(cls, sources, mean, std, colour_unit: float = 1.0 / 255.0) -> "Channels":
        """Channels that hold (u - mean) / std, u the colour byte times ``colour_unit`` or the height: scale = unit / std
        and bias = -mean / std, formed in float64 and rounded to float32 once.  ``mean`` and ``std``: one per channel, or
        one for all."""
        src = np.asarray([int(x) for x in sources], np.int64)
        mean = np.broadcast_to(np.asarray(mean, np.float64), src.shape)
        std = np.broadcast_to(np.asarray(std, np.float64), src.shape)
        unit = np.where(src == SRC_HEIGHT, 1.0, float(colour_unit))
        return cls(src, unit / std, -mean / std)

    @property
    def uses_colour(self) -> bool:
        return any(x != SRC_HEIGHT for x in self.sources)


# every channel in [0, 1] on the default maps: colour bytes by 1 / 255, heights by 1 / HEIGHT_SPAN; RGBHHH is the six-channel
# input of Ravens' Transporter (the height three times)
CHANNELS_RGBH = Channels((0, 1, 2, 3), (1 / 255.0,) * 3 + (1 / HEIGHT_SPAN,))
CHANNELS_RGBHHH = Channels((0, 1, 2, 3, 3, 3), (1 / 255.0,) * 3 + (1 / HEIGHT_SPAN,) * 3)

# scene [N, C, rows, columns] and crops [N, n_rotations, C, crop, crop]: the network inputs; pick, place int64 [N, 2]
# (column, row) in the scene; pick_index, place_index int64 [N] = row * columns + column; rotation_index int64 [N];
# tries as in Perturbation
TransporterBatch = collections.namedtuple(
    "TransporterBatch", ["scene", "crops", "pick", "place", "pick_index", "place_index", "rotation_index", "tries"])


def _as_channels(channels) -> Channels:
    return channels if isinstance(channels, Channels) else Channels(*channels)


def _input_args(colour, channels, dtype) -> Channels:
    channels = _as_channels(channels)
    if dtype not in _DTYPES:
        raise ValueError("dtype must be torch.float32 or torch.bfloat16")
    if channels.uses_colour and colour is None:
        raise ValueError("a colour channel needs the colour map")
    return channels


def warp_inputs_reference(height: torch.Tensor, colour: Optional[torch.Tensor] = None, *, mats, index=None,
                          out_shape=None, channels=CHANNELS_RGBH, dtype=torch.float32) -> torch.Tensor:
    """The statement of ``warp_inputs`` (include/mre.h, mre_warp_inputs) in plain torch, float32 operation by operation,
    on whatever device ``height`` is on and for any strides: ``warp_maps_reference``, the colour bytes and the height as
    float32 planes, ``x * scale`` and ``+ bias`` as two operations, ``.to(dtype)``.  The fallback of ``warp_inputs`` and, on
    the CPU, bit for bit what the kernel computes."""
    channels = _input_args(colour, channels, dtype)
    w = warp_maps_reference(height, colour if channels.uses_colour else None, mats=mats, index=index, out_shape=out_shape,
                            with_source=False)
    dev = w.height.device
    planes = [w.height if s == SRC_HEIGHT else w.colour[..., s].to(torch.float32) for s in channels.sources]
    x = torch.stack(planes, dim=1)
    x = x * torch.tensor(channels.scales, dtype=torch.float32, device=dev).view(1, -1, 1, 1)
    x = x + torch.tensor(channels.biases, dtype=torch.float32, device=dev).view(1, -1, 1, 1)
    return x.to(dtype)


def warp_inputs(height: torch.Tensor, colour: Optional[torch.Tensor] = None, *, mats, index=None, out_shape=None,
                channels=CHANNELS_RGBH, dtype=torch.float32) -> torch.Tensor:
    """The gather of ``warp_maps`` -- the same ``mats``, ``index`` and ``out_shape``, the same source cell and the same
    empty cells, bit for bit -- as a network input [S, C, rows, columns] of ``dtype`` (float32 or bfloat16, rounded to
    nearest even): channel k is ``channels`` (a ``Channels``, or its three sequences) applied to the gathered colour byte or
    height, and to 0 where the source cell does not exist.  Contiguous CUDA float32 height with uint8 colour is one launch
    of ``mre_warp_inputs`` on torch's current stream, without a synchronise and with no intermediate; anything else is
    computed by ``warp_inputs_reference`` with the same result."""
    channels = _input_args(colour, channels, dtype)
    dev = height.device
    if not _maps_on_device(height, colour):
        return warp_inputs_reference(height, colour, mats=mats, index=index, out_shape=out_shape, channels=channels,
                                     dtype=dtype)
    mats, index = _as_mats(mats, dev), _as_index(index, dev)
    n, in_h, in_w, samples, out_h, out_w = _warp_args(height, colour, None, mats, index, out_shape)
    nc = len(channels.sources)
    out = torch.empty((samples, nc, out_h, out_w), dtype=dtype, device=dev)
    if n and samples:
        src = (C.c_int32 * nc)(*channels.sources)
        scale, bias = (C.c_float * nc)(*channels.scales), (C.c_float * nc)(*channels.biases)
        with _stream_on(dev) as stream:
            _lib.check(_lib.lib().mre_warp_inputs(
                stream, height.data_ptr(), colour.data_ptr() if channels.uses_colour else None, n, in_h, in_w,
                _ptr(index), mats.data_ptr(), samples, out_h, out_w, nc,
                C.addressof(src), C.addressof(scale), C.addressof(bias), _DTYPES[dtype], out.data_ptr()), "mre_warp_inputs")
    return out


def transporter_batch(maps, pick_cells, place_cells, *, seed: int, env_ids, draw: int, n_rotations: int = 36,
                      crop: int = 64, channels=CHANNELS_RGBH, dtype=torch.float32) -> TransporterBatch:
    """One Transporter training batch from the ``maps`` of the envs (a ``HeightMap`` / ``WarpedMaps``, or (height,
    colour)), as the tensors a network takes: see ``TransporterBatch``.  The motion is ``transporter_sample``'s -- the same
    ``sample_perturbation(seed, env_ids, draw)`` of the pick and place cells ([N, 2] (column, row)), so the same (seed, env
    id, draw) gives the same motion.  ``scene`` is ``warp_inputs`` of the source maps under that motion; ``crops`` is
    ``warp_inputs`` of the perturbed maps under ``crop_matrices`` around the moved pick cell.  The perturbed uint8 / float32
    maps are still made once by ``warp_maps``, because the crops gather from them (nearest of nearest is not nearest of the
    composition); the crops themselves are never written as bytes.  Three launches for CUDA maps.

    ``pick_index`` / ``place_index`` are row * columns + column of the moved cells: the class a softmax over the flattened
    scene is trained on (meaningful where the cell is inside the map, as it is where ``tries`` > 0).  ``rotation_index`` is
    0 for every env: the scripted demonstrator's ``gripper_rot`` is 0 for the pick and for the place, so the relative
    rotation bin a Transporter's place head is trained on is bin 0."""
    height, colour = maps[0], maps[1]
    channels = _input_args(colour, channels, dtype)
    n = int(height.shape[0])
    cells = _label_cells(pick_cells, place_cells, n)
    cols = int(height.shape[2])
    pert = sample_perturbation(seed, env_ids, draw, cells, tuple(height.shape[1:3]))
    kw = dict(channels=channels, dtype=dtype)
    scene = warp_inputs(height, colour, mats=pert.M, **kw)
    warped = warp_maps(height, colour if channels.uses_colour else None, mats=pert.M, with_source=False)
    mats, index = crop_matrices(pert.cells[:, 0], n_rotations, crop)
    crops = warp_inputs(warped.height, warped.colour, mats=mats, index=index, out_shape=(crop, crop), **kw)
    pick, place = pert.cells[:, 0], pert.cells[:, 1]
    return TransporterBatch(scene, crops.view((n, n_rotations) + tuple(crops.shape[1:])), pick, place,
                            pick[:, 1] * cols + pick[:, 0], place[:, 1] * cols + place[:, 0], np.zeros(n, np.int64),
                            pert.tries)


# ------------------------------------------------------------------------------------------- the place head
MAX_ROTATIONS, MAX_DEPTH, MAX_CROP = 64, 16, 64   # the limits of mre_correlate
# logits float32 or bfloat16 [N, R, rows, columns] or None; index int64 [N], the flat (r * rows + y) * columns + x of the
# largest float32 sum of every env (ties: the lowest), and value float32 [N], that sum; both None when not asked for
Correlation = collections.namedtuple("Correlation", ["logits", "index", "value"])


def _cells_in_range(rot, h, w) -> bool:   # the ranges of rotations, rows and columns that both heads take
    return 1 <= rot <= MAX_ROTATIONS and 1 <= h <= MAX_MAP and 1 <= w <= MAX_MAP and rot * h * w < 2 ** 31


def _correlate_args(scene, kernels, logits, best):
    if scene.dim() != 4 or kernels.dim() != 5:
        raise ValueError("scene must be [N, D, rows, columns] and kernels [N, R, D, crop, crop]")
    n, depth, h, w = (int(x) for x in scene.shape)
    rot, crop = int(kernels.shape[1]), int(kernels.shape[3])
    if tuple(kernels.shape) != (n, rot, depth, crop, crop):
        raise ValueError("kernels must be [N, R, D, crop, crop] with the N and D of scene")
    if not (1 <= rot <= MAX_ROTATIONS and 1 <= depth <= MAX_DEPTH and 2 <= crop <= MAX_CROP and crop % 2 == 0):
        raise ValueError("1 <= R <= 64, 1 <= D <= 16 and an even crop of 2 .. 64")
    if not _cells_in_range(rot, h, w):
        raise ValueError("1 <= rows, columns <= 4096 and R * rows * columns < 2^31")
    if logits not in (None, torch.float32, torch.bfloat16):
        raise ValueError("logits must be None, torch.float32 or torch.bfloat16")
    if logits is None and not best:
        raise ValueError("nothing asked for: logits is None and best is False")
    if kernels.device != scene.device:
        raise ValueError("scene and kernels must be on one device")
    return n, rot, depth, h, w, crop


def _logits_f32(scene, kernels, n, rot, depth, h, w, crop):
    """The conv2d line of ``correlate_reference``, differentiable: float32 [n, rot, h, w]"""
    x = scene.to(torch.float32).reshape(1, n * depth, h, w)
    k = kernels.to(torch.float32).reshape(n * rot, depth, crop, crop)
    if n == 0:   # (conv2d takes no empty group; the sums keep the empty result in the graph)
        return (x.sum() + k.sum()) * torch.zeros((0, rot, h, w), dtype=torch.float32, device=scene.device)
    return torch.nn.functional.conv2d(x, k, padding=crop // 2, groups=n)[..., :h, :w].reshape(n, rot, h, w)


_on_device = functools.partial(_in_place, (torch.bfloat16,))   # what the place head's kernels read in place


def correlate_reference(scene: torch.Tensor, kernels: torch.Tensor, *, logits=None, best: bool = True) -> Correlation:
    """The statement of ``correlate`` (include/mre.h, mre_correlate) in plain torch, on whatever device and for any
    strides and dtype: the grouped ``conv2d`` of the zero-padded scene with every env's own kernels in float32 from the
    given values, cut to the scene's cells; the best cell is the first occurrence of the largest float32 sum (a NaN
    counts as -inf).  The fallback of ``correlate``.  The order of its float32 additions is the library's, not the
    kernel's: integer-valued inputs (every partial sum below 2^24) make both exact."""
    n, rot, depth, h, w, crop = _correlate_args(scene, kernels, logits, best)
    out = _logits_f32(scene, kernels, n, rot, depth, h, w, crop)
    index = value = None
    if best:
        flat = out.reshape(n, rot * h * w)
        index = torch.where(torch.isnan(flat), torch.full_like(flat, float("-inf")), flat).argmax(dim=1)
        value = flat.gather(1, index[:, None])[:, 0]
    return Correlation(None if logits is None else out.to(logits).contiguous(), index, value)


def correlate(scene: torch.Tensor, kernels: torch.Tensor, *, logits=None, best: bool = True) -> Correlation:
    """A Transporter's place head: every env's ``scene`` features [N, D, rows, columns] cross-correlated with that env's
    own ``kernels`` [N, R, D, crop, crop] (the features of its R rotated crops; crop even, its index crop / 2 the pivot),
      logit[e, r, y, x] = sum over d, i, j of scene[e, d, y + i - crop/2, x + j - crop/2] * kernels[e, r, d, i, j]
    with cells outside the scene counting as 0, and per env the largest sum with its flat index -- a ``Correlation``.
    ``logits`` names the dtype the sums are written in (None: they are never written; 4096 envs x 36 x 320 x 240 of them
    are 45 GB); ``best`` asks for ``index`` and ``value``, which are taken from the float32 sums and are the same bits
    whether or not the logits are written.  ``decode_place`` turns ``index`` into cells and rotation bins.

    Contiguous CUDA bfloat16 inputs are one call of ``mre_correlate`` (csrc/mre_correlate.hip, bf16 matrix cores, float32
    accumulation) on torch's current stream with a ``torch.empty`` workspace, without a synchronise; anything else is
    computed by ``correlate_reference``.  No autograd: ``place_loss`` and ``correlate_backward`` are the training path."""
    n, rot, depth, h, w, crop = _correlate_args(scene, kernels, logits, best)
    if not _on_device(scene, kernels):
        return correlate_reference(scene, kernels, logits=logits, best=best)
    dev = scene.device
    out = _empty_if(logits is not None, (n, rot, h, w), logits, dev)
    index, value = _empty_if(best, (n,), torch.int64, dev), _empty_if(best, (n,), torch.float32, dev)
    if n:
        work, nbytes = _workspace("mre_correlate_workspace", dev, n, rot, h, w)
        with _stream_on(dev) as stream:
            _lib.check(_lib.lib().mre_correlate(
                stream, scene.detach().data_ptr(), kernels.detach().data_ptr(), n, rot, depth, h, w, crop,
                _DTYPES[logits if logits is not None else torch.float32], _ptr(out), _ptr(index), _ptr(value),
                work.data_ptr(), nbytes), "mre_correlate")
    return Correlation(out, index, value)


def decode_place(index, shape, n_rotations: int, check: bool = True):
    """The flat indices of ``correlate`` [N] over ``shape`` = (rows, columns) as (cells int64 [N, 2] (column, row), rotation
    bins int64 [N], angles float64 [N] = 2 pi bin / n_rotations, the turn of ``crop_matrices``' sample ``bin``).  Torch
    tensors for a tensor, numpy arrays for anything else.  ``check=False`` leaves out the range check, which reads the
    indices on the host: for indices a kernel has just written, which are in range, and which nothing should wait for."""
    rows, cols = int(shape[0]), int(shape[1])
    is_tensor = isinstance(index, torch.Tensor)
    idx = index.to(torch.int64) if is_tensor else torch.as_tensor(np.asarray(index, np.int64))
    if check and idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n_rotations * rows * cols):
        raise ValueError("an index outside n_rotations * rows * columns")
    bins = torch.div(idx, rows * cols, rounding_mode="floor")
    rest = idx - bins * (rows * cols)
    row = torch.div(rest, cols, rounding_mode="floor")
    cells = torch.stack([rest - row * cols, row], dim=-1)
    angles = bins.to(torch.float64) * (2.0 * np.pi / n_rotations)
    if is_tensor:
        return cells, bins, angles
    return cells.numpy(), bins.numpy(), angles.numpy()


def encode_place(cells, bins, shape):
    """The inverse of ``decode_place``: the flat index (bin * rows + row) * columns + column [N] of ``cells`` [N, 2]
    (column, row) at rotation ``bins`` [N] over ``shape`` = (rows, columns) -- the target ``place_loss`` takes.  A cell
    outside the map gives -1, which ``place_loss`` answers with NaN.  A torch tensor for tensors, a numpy array for
    anything else."""
    rows, cols = int(shape[0]), int(shape[1])
    is_tensor = isinstance(cells, torch.Tensor)
    c = cells.to(torch.int64) if is_tensor else torch.as_tensor(np.asarray(cells, np.int64))
    b = torch.as_tensor(bins if isinstance(bins, torch.Tensor) else np.asarray(bins, np.int64)).to(torch.int64).to(c.device)
    col, row = c[..., 0], c[..., 1]
    inside = (col >= 0) & (col < cols) & (row >= 0) & (row < rows) & (b >= 0)
    index = torch.where(inside, (b * rows + row) * cols + col, torch.full_like(col, -1))
    return index if is_tensor else index.numpy()


# ------------------------------------------------------------------------------------------- training the place head
def _place_args(scene, kernels):
    return _correlate_args(scene, kernels, None, True)


def _as_target(target, n, dev):
    t = torch.as_tensor(target).to(device=dev, dtype=torch.int64).contiguous()
    if tuple(t.shape) != (n,):
        raise ValueError("target must be [N]")
    return t


def _as_weight(weight, n, dev):
    if weight is None:
        return None
    w = torch.as_tensor(weight).to(device=dev, dtype=torch.float32).contiguous()
    if tuple(w.shape) != (n,):
        raise ValueError("weight must be [N]")
    return w


def place_loss_reference(scene: torch.Tensor, kernels: torch.Tensor, target, weight=None) -> torch.Tensor:
    """The statement of ``place_loss`` (include/mre.h, mre_correlate_loss) in plain float32 torch, on any device and for
    any dtype and strides, differentiable by torch itself: weight * (logsumexp of the env's R * rows * columns logits
    minus the logit at flat index ``target``), float32 [N]; NaN where ``target`` is outside, and the gradient is then that
    of the logsumexp alone.  The fallback of ``place_loss``."""
    n, rot, depth, h, w, crop = _place_args(scene, kernels)
    t = _as_target(target, n, scene.device)
    wgt = _as_weight(weight, n, scene.device)
    flat = _logits_f32(scene, kernels, n, rot, depth, h, w, crop).reshape(n, rot * h * w)
    inside = (t >= 0) & (t < rot * h * w)
    at = flat.gather(1, torch.where(inside, t, torch.zeros_like(t))[:, None])[:, 0]
    loss = torch.logsumexp(flat, dim=1) - torch.where(inside, at, torch.full_like(at, float("nan")))
    return _weighted(loss, wgt)


def _backward_args(scene, kernels, dlogits):
    n, rot, depth, h, w, crop = _place_args(scene, kernels)
    if tuple(dlogits.shape) != (n, rot, h, w) or dlogits.device != scene.device:
        raise ValueError("dlogits must be [N, R, rows, columns] on the device of scene")
    return n, rot, depth, h, w, crop


def correlate_backward_reference(scene: torch.Tensor, kernels: torch.Tensor, dlogits: torch.Tensor):
    """The statement of ``correlate_backward`` (include/mre.h, mre_correlate_grad_scene / _kern) in plain float32 torch:
    torch's own gradients of sum(dlogits * logits) through the ``conv2d`` of ``correlate_reference``, for any device,
    dtype and strides.  (grad_scene [N, D, rows, columns], grad_kernels [N, R, D, crop, crop]), float32."""
    n, rot, depth, h, w, crop = _backward_args(scene, kernels, dlogits)
    with torch.enable_grad():
        s = scene.detach().to(torch.float32).clone().requires_grad_(True)
        k = kernels.detach().to(torch.float32).clone().requires_grad_(True)
        out = _logits_f32(s, k, n, rot, depth, h, w, crop)
        gs, gk = torch.autograd.grad(out, (s, k), dlogits.detach().to(torch.float32))
    return gs, gk


def correlate_backward(scene: torch.Tensor, kernels: torch.Tensor, dlogits: torch.Tensor):
    """The gradients of sum(dlogits * logits) of ``correlate`` with respect to ``scene`` and ``kernels``, for any
    ``dlogits`` [N, R, rows, columns]: (grad_scene float32 [N, D, rows, columns], grad_kernels float32 [N, R, D, crop,
    crop]),
      grad_kernels[e, r, d, i, j] = sum over y, x of dlogits[e, r, y, x] * scene[e, d, y + i - crop/2, x + j - crop/2]
      grad_scene[e, d, v, u] = sum over r, i, j of dlogits[e, r, v - i + crop/2, u - j + crop/2] * kernels[e, r, d, i, j]
    with cells outside counting as 0.  Contiguous CUDA bfloat16 tensors are one call each of ``mre_correlate_grad_scene``
    and ``mre_correlate_grad_kern`` (csrc/mre_correlate_grad.hip: the forward's implicit GEMM with the operands in other
    roles) on torch's current stream with a ``torch.empty`` workspace they share (7 MB per env at the workload's shape),
    without a synchronise; anything else is computed by ``correlate_backward_reference``."""
    n, rot, depth, h, w, crop = _backward_args(scene, kernels, dlogits)
    if not _on_device(scene, kernels, dlogits):
        return correlate_backward_reference(scene, kernels, dlogits)
    return _grad_scene(scene, kernels, dlogits), _grad_kernels(scene, kernels, dlogits)


def _grad_call(name, g, other, out, shape):
    n, rot, depth, h, w, crop = shape
    if n:
        work, nbytes = _workspace("mre_correlate_grad_workspace", g.device, n, rot, depth, h, w, crop)
        with _stream_on(g.device) as stream:
            _lib.check(getattr(_lib.lib(), name)(stream, g.data_ptr(), other.data_ptr(), n, rot, depth, h, w, crop,
                                                 out.data_ptr(), work.data_ptr(), nbytes), name)
    return out


def _grad_scene(scene, kernels, g):
    shape = _place_args(scene, kernels)
    out = torch.empty(tuple(scene.shape), dtype=torch.float32, device=scene.device)
    return _grad_call("mre_correlate_grad_scene", g.detach(), kernels.detach(), out, shape)


def _grad_kernels(scene, kernels, g):
    shape = _place_args(scene, kernels)
    out = torch.empty(tuple(kernels.shape), dtype=torch.float32, device=scene.device)
    return _grad_call("mre_correlate_grad_kern", g.detach(), scene.detach(), out, shape)


# lse, target_logit and loss float32 [N] of mre_correlate_loss (unweighted)
PlaceLoss = collections.namedtuple("PlaceLoss", ["lse", "target_logit", "loss"])


def place_loss_forward(scene, kernels, target) -> PlaceLoss:
    """``mre_correlate_loss`` on contiguous CUDA bfloat16 ``scene`` and ``kernels`` and an int64 CUDA ``target`` [N]: the
    logsumexp of every env's logits, the logit at ``target`` and their difference, without a logit being stored."""
    n, rot, depth, h, w, crop = _place_args(scene, kernels)
    dev = scene.device
    out = torch.empty((3, n), dtype=torch.float32, device=dev)
    if n:
        work, nbytes = _workspace("mre_correlate_workspace", dev, n, rot, h, w)
        with _stream_on(dev) as stream:
            _lib.check(_lib.lib().mre_correlate_loss(
                stream, scene.detach().data_ptr(), kernels.detach().data_ptr(), n, rot, depth, h, w, crop, target.data_ptr(),
                out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), work.data_ptr(), nbytes), "mre_correlate_loss")
    return PlaceLoss(out[0], out[1], out[2])


def place_dlogits(scene, kernels, target, lse, weight=None) -> torch.Tensor:
    """``mre_correlate_dlogits``: g = weight * (softmax - one-hot of ``target``) as bfloat16 [N, R, rows, columns], from
    the ``lse`` of ``place_loss_forward``; the logits are computed again, not kept."""
    n, rot, depth, h, w, crop = _place_args(scene, kernels)
    g = torch.empty((n, rot, h, w), dtype=torch.bfloat16, device=scene.device)
    if n:
        with _stream_on(scene.device) as stream:
            _lib.check(_lib.lib().mre_correlate_dlogits(
                stream, scene.detach().data_ptr(), kernels.detach().data_ptr(), n, rot, depth, h, w, crop, target.data_ptr(),
                lse.data_ptr(), _ptr(weight), g.data_ptr()), "mre_correlate_dlogits")
    return g


def _weighted(x, weight):
    """``x`` times ``weight`` (None: 1): a head's loss, and in backward, of the incoming gradient, its dlogits' weight"""
    return x if weight is None else weight * x


class _PlaceLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scene, kernels, target, weight):
        out = place_loss_forward(scene, kernels, target)
        ctx.save_for_backward(scene, kernels, target, out.lse)
        ctx.weight = weight
        return _weighted(out.loss, weight)

    @staticmethod
    def backward(ctx, grad):
        scene, kernels, target, lse = ctx.saved_tensors
        g = place_dlogits(scene, kernels, target, lse, _weighted(grad.to(torch.float32), ctx.weight).contiguous())
        gs = _grad_scene(scene, kernels, g) if ctx.needs_input_grad[0] else None
        gk = _grad_kernels(scene, kernels, g) if ctx.needs_input_grad[1] else None
        return gs, gk, None, None


def place_loss(scene: torch.Tensor, kernels: torch.Tensor, target, weight=None) -> torch.Tensor:
    """The training loss of a Transporter's place head, float32 [N]: per env the softmax cross-entropy of the R * rows *
    columns logits of ``correlate`` against the cell ``target`` [N] (int64 flat index (r * rows + y) * columns + x, as
    ``encode_place`` makes it), times ``weight`` [N] (None: 1),
      loss[e] = weight[e] * (log sum over cells of exp(logit[e, cell]) - logit[e, target[e]])
    and NaN where ``target`` is outside (the gradient is then that of the logsumexp alone).  Differentiable with respect to
    ``scene`` and ``kernels``.

    Contiguous CUDA bfloat16 inputs take the kernels of csrc/mre_correlate_grad.hip on torch's current stream, without a
    synchronise and without a logit stored: forward is ``mre_correlate_loss`` and keeps scene, kernels, target and the
    logsumexp; backward computes the logits again for g = weight * grad * (softmax - one-hot) in bfloat16
    (``mre_correlate_dlogits``) and hands g to ``mre_correlate_grad_scene`` and ``mre_correlate_grad_kern``, whose float32
    results autograd casts to the inputs' dtype.  Anything else goes through ``place_loss_reference``."""
    n, rot, depth, h, w, crop = _place_args(scene, kernels)
    if not _on_device(scene, kernels):
        return place_loss_reference(scene, kernels, target, weight)
    return _PlaceLoss.apply(scene, kernels, _as_target(target, n, scene.device), _as_weight(weight, n, scene.device))


def cell_2_world(cells, bounds, cell: float):
    """World (x, y) of the centres of ``cells`` [..., 2] (column, row) of the map of ``bounds`` at ``cell``:
    lo + (c + 0.5) * cell in float64 -- the inverse of ``world_2_cell`` up to the cell.  A torch tensor for a tensor, a
    numpy array for anything else."""
    lo, _, _ = _grid(bounds, cell)
    is_tensor = isinstance(cells, torch.Tensor)
    c = (cells if is_tensor else torch.as_tensor(np.asarray(cells))).to(torch.float64)
    lo2 = torch.tensor([float(lo[0]), float(lo[1])], dtype=torch.float64, device=c.device)
    out = lo2 + (c + 0.5) * float(cell)
    return out if is_tensor else out.numpy()


# ------------------------------------------------------------------------------------------- the pick head
# index int64 [N], the flat (k * rows + y) * columns + x of the largest logit of every env (ties: the lowest), and value
# float32 [N], that logit (both None when not asked for); lse, target_logit and loss float32 [N] (None without a target)
Attention = collections.namedtuple("Attention", ["index", "value", "lse", "target_logit", "loss"])


def _attend_args(logits):
    if logits.dim() != 4:
        raise ValueError("logits must be [N, K, rows, columns]")
    n, rot, h, w = (int(x) for x in logits.shape)
    if not _cells_in_range(rot, h, w):
        raise ValueError("1 <= K <= 64, 1 <= rows, columns <= 4096 and K * rows * columns < 2^31")
    return n, rot, h, w


_logits_on_device = functools.partial(_in_place, tuple(_DTYPES))   # what the pick head's kernels read in place


def attend_reference(logits: torch.Tensor, target=None, best: bool = True) -> Attention:
    """The statement of ``attend`` (include/mre.h, mre_attend) in plain float32 torch, on any device and for any dtype and
    strides: the first occurrence of the largest logit (a NaN counts as -inf), and with ``target`` the logsumexp of the
    env's K * rows * columns logits, the logit at ``target`` and their difference (NaN where ``target`` is outside).
    -inf is a masked cell; an env of nothing else has lse = -inf and loss = NaN.  ``lse`` and ``loss`` are differentiable
    by torch itself, and an all -inf env then gets a zero gradient, as ``mre_attend_dlogits`` gives it.  The fallback of
    ``attend`` and ``pick_loss``."""
    n, rot, h, w = _attend_args(logits)
    flat = logits.to(torch.float32).reshape(n, rot * h * w)
    index = value = lse = at = loss = None
    if best:
        index = torch.where(torch.isnan(flat), torch.full_like(flat, float("-inf")), flat).detach().argmax(dim=1)
        value = flat.detach().gather(1, index[:, None])[:, 0]
    if target is not None:
        t = _as_target(target, n, logits.device)
        ninf = torch.full((n,), float("-inf"), dtype=torch.float32, device=logits.device)
        dead = (flat == float("-inf")).all(dim=1)
        lse = torch.where(dead, ninf, torch.logsumexp(torch.where(dead[:, None], torch.zeros_like(flat), flat), dim=1))
        inside = (t >= 0) & (t < rot * h * w)
        at = flat.gather(1, torch.where(inside, t, torch.zeros_like(t))[:, None])[:, 0]
        at = torch.where(inside, torch.where(dead, ninf, at), torch.full_like(at, float("nan")))
        loss = lse - at
    elif not best:
        raise ValueError("nothing asked for: target is None and best is False")
    return Attention(index, value, lse, at, loss)


def attend(logits: torch.Tensor, target=None, best: bool = True) -> Attention:
    """A Transporter's pick head: from the ``logits`` [N, K, rows, columns] of an attention network (K pick rotations, 1
    for a classic Transporter), per env the largest logit with its flat index (k * rows + y) * columns + x (``best``), and
    with ``target`` [N] (int64 flat indices, as ``encode_pick`` makes them) the softmax cross-entropy against that cell:
    ``lse``, ``target_logit`` and ``loss`` = lse - logit[target], NaN where ``target`` is outside.  An ``Attention``.
    -inf logits are masked cells.  ``decode_pick`` turns ``index`` into cells and rotation bins.

    Contiguous CUDA float32 or bfloat16 logits are one call of ``mre_attend`` (csrc/mre_attend.hip: one read of the
    logits, no float32 copy) on torch's current stream with a ``torch.empty`` workspace, without a synchronise; anything
    else is computed by ``attend_reference``.  No autograd on the device path: ``pick_loss`` is the training path."""
    n, rot, h, w = _attend_args(logits)
    if target is None and not best:
        raise ValueError("nothing asked for: target is None and best is False")
    if not _logits_on_device(logits):
        return attend_reference(logits, target, best)
    dev = logits.device
    t = None if target is None else _as_target(target, n, dev)
    index = _empty_if(best, (n,), torch.int64, dev)
    # the four float32 rows and, behind them, the workspace (a multiple of 16 bytes per env, 16 n bytes in): one allocation
    nbytes = _workspace_bytes("mre_attend_workspace", n, rot, h, w) if n else 0
    out = torch.empty((4 + nbytes // (4 * n) if n else 4, n), dtype=torch.float32, device=dev)
    rows = [out[k] if on else None for k, on in enumerate((best, t is not None, t is not None, t is not None))]
    if n:
        with _stream_on(dev) as stream:
            _lib.check(_lib.lib().mre_attend(stream, logits.data_ptr(), n, rot, h, w, _DTYPES[logits.dtype], _ptr(t), _ptr(index),
                                             *map(_ptr, rows), out.data_ptr() + 16 * n, nbytes), "mre_attend")
    return Attention(index, *rows)


def attend_dlogits(logits: torch.Tensor, target, lse: torch.Tensor, weight=None) -> torch.Tensor:
    """``mre_attend_dlogits``: g = weight * (softmax - one-hot of ``target``) in the logits' dtype and shape, from the
    ``lse`` of ``attend``; one read and one write.  ``logits`` must be what the kernels read in place (contiguous CUDA
    float32 or bfloat16: ``pick_loss_reference`` serves anything else), ``lse`` float32 [N] on its device; ``target`` [N] and
    ``weight`` [N] or None are brought to int64 and float32 there."""
    n, rot, h, w = _attend_args(logits)
    if not _logits_on_device(logits):
        raise ValueError("logits must be a contiguous CUDA float32 or bfloat16 tensor")
    dev = logits.device
    if lse.dtype != torch.float32 or lse.device != dev or tuple(lse.shape) != (n,):
        raise ValueError("lse must be float32 [N] on the device of logits")
    lse, target, weight = lse.contiguous(), _as_target(target, n, dev), _as_weight(weight, n, dev)
    g = torch.empty_like(logits)
    if n:
        with _stream_on(dev) as stream:
            _lib.check(_lib.lib().mre_attend_dlogits(
                stream, logits.data_ptr(), n, rot, h, w, _DTYPES[logits.dtype], target.data_ptr(), lse.data_ptr(),
                _ptr(weight), g.data_ptr()), "mre_attend_dlogits")
    return g


class _PickLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, weight):
        out = attend(logits, target, best=False)
        ctx.save_for_backward(logits, target, out.lse)
        ctx.weight = weight
        return _weighted(out.loss, weight)

    @staticmethod
    def backward(ctx, grad):
        logits, target, lse = ctx.saved_tensors
        return attend_dlogits(logits, target, lse, _weighted(grad.to(torch.float32), ctx.weight).contiguous()), None, None


def pick_loss_reference(logits: torch.Tensor, target, weight=None) -> torch.Tensor:
    """The statement of ``pick_loss`` in plain float32 torch (``attend_reference``), differentiable by torch itself:
    weight * (logsumexp of the env's logits minus the logit at ``target``), float32 [N]; NaN where ``target`` is outside,
    and the gradient is then that of the logsumexp alone.  The fallback of ``pick_loss``."""
    n = _attend_args(logits)[0]
    loss = attend_reference(logits, target, best=False).loss
    wgt = _as_weight(weight, n, logits.device)
    return _weighted(loss, wgt)


def pick_loss(logits: torch.Tensor, target, weight=None) -> torch.Tensor:
    """The training loss of a Transporter's pick head, float32 [N]: per env the softmax cross-entropy of the K * rows *
    columns ``logits`` against the cell ``target`` [N] (``encode_pick``), times ``weight`` [N] (None: 1); NaN where
    ``target`` is outside (the gradient is then that of the logsumexp alone).  Differentiable with respect to ``logits``.

    Contiguous CUDA float32 or bfloat16 logits take the kernels of csrc/mre_attend.hip on torch's current stream, without
    a synchronise: forward is ``mre_attend`` without the decision and keeps logits, target and the logsumexp (one float per
    env); backward is ``mre_attend_dlogits`` with weight * the incoming gradient, which writes the gradient in the logits'
    dtype in one read and one write.  Anything else goes through ``pick_loss_reference``."""
    n = _attend_args(logits)[0]
    if not _logits_on_device(logits):
        return pick_loss_reference(logits, target, weight)
    return _PickLoss.apply(logits, _as_target(target, n, logits.device), _as_weight(weight, n, logits.device))


def decode_pick(index, shape, n_rotations: int = 1, check: bool = True):
    """``decode_place`` under the pick head's name: pick and place share one index convention."""
    return decode_place(index, shape, n_rotations, check)


def encode_pick(cells, bins, shape):
    """``encode_place`` under the pick head's name: the target ``pick_loss`` takes."""
    return encode_place(cells, bins, shape)


@functools.lru_cache(maxsize=16)
def _crop_table(n_rotations: int, crop: int, device: str) -> torch.Tensor:
    """float64 [n_rotations, 6] on ``device``: (cos, -sin, (R @ half)_x, sin, cos, (R @ half)_y) by the expressions of
    ``crop_matrices``; built and uploaded once per (n_rotations, crop, device)"""
    half = np.array([crop / 2.0, crop / 2.0])
    table = np.empty((n_rotations, 6), np.float64)
    for k in range(n_rotations):
        cos, sin = _quarter_exact(k, n_rotations)
        R = np.array([[cos, -sin], [sin, cos]])
        table[k, [0, 1, 3, 4]] = R.reshape(4)
        table[k, [2, 5]] = R @ half
    return torch.from_numpy(table).to(device)


def crop_matrices_device(cells: torch.Tensor, n_rotations: int = 36, crop: int = 64):
    """``crop_matrices`` for pivots ``cells`` [N, 2] (column, row) that are a tensor, on its device and without a
    synchronise: (mats float32 [N * n_rotations, 6], index int32 [N * n_rotations]), bit for bit what ``crop_matrices``
    gives for the same cells.  The per-rotation entries and R @ half are formed on the host in float64 by the same
    expressions, once per (n_rotations, crop, device), and kept on the device; a call performs p - R @ half in float64 there,
    one correctly rounded operation, and rounds to float32 once: no copy from the host."""
    if n_rotations < 1 or crop < 1:
        raise ValueError("n_rotations and crop must be at least 1")
    p = cells.reshape(-1, 2).to(torch.float64)
    table = _crop_table(int(n_rotations), int(crop), str(p.device))
    mats = table[None].repeat(p.shape[0], 1, 1)
    mats[:, :, 2] = p[:, None, 0] - table[None, :, 2]
    mats[:, :, 5] = p[:, None, 1] - table[None, :, 5]
    index = torch.arange(p.shape[0], dtype=torch.int32, device=p.device).repeat_interleave(n_rotations)
    return mats.to(torch.float32).reshape(-1, 6).contiguous(), index
