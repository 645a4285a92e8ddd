"""The Transporter glue of ``BatchedRearrangementEnv``, this project's own (the reference has no heightmap and no Transporter
heads): top-down heightmaps of the rendered frames, training samples and batches, the decisions and losses of the pick and
place heads, one closed-loop decision, and the poses ``step()`` takes from a decision.  ``TransporterMixin`` is mixed into
the env, so that ``env.heightmap(...)`` and ``env.transporter_*(...)`` are methods of it; it reads the env's ``render``,
``render_views``, ``sort_colours``, ``env_ids`` and camera table.  The arithmetic is ``perception``'s.
"""
from __future__ import annotations

import collections

import numpy as np
import torch

from .. import perception
from ._camera import TABLE_TOP_Z
from ._env import home_quat

OVERHEAD = "overhead_camera/overhead_camera"
PICK_HEIGHT = 0.575     # tasks/rearrangement.py:362,405  ("hardcode for now :(")

# The box BatchedRearrangementEnv.heightmap covers by default, (lo, hi) in world metres: the reach of the arm over the
# table, from 1 cm BELOW the table top to 29 cm above it -- 320 rows (y) x 240 columns (x) at the default cell of 2.5 mm.
# This project's choice (the reference has no heightmap).  lo_z must sit below the table: the table's pixels come back
# from depth a float32 rounding above or below TABLE_TOP_Z, and a lo_z equal to it would cut the plane out of the map.
HEIGHTMAP_BOUNDS = ((0.2, -0.4, TABLE_TOP_Z - 0.01), (0.8, 0.4, TABLE_TOP_Z + 0.29))
# what BatchedRearrangementEnv.transporter_place decides for every env
PlaceDecision = collections.namedtuple("PlaceDecision", ["cells", "rotation", "angle", "xy", "value"])
# what BatchedRearrangementEnv.transporter_pick decides for every env: cells int64 [N, 2] (column, row), rotation bins int64
# [N], angles float64 [N] (radians), xy float64 [N, 2] (world) and the logit float32 [N], on the logits' device.  (`bins` and
# `angles` are what PlaceDecision, which is older, calls `rotation` and `angle`: transporter_act returns one of each.)
PickDecision = collections.namedtuple("PickDecision", ["cells", "bins", "angles", "xy", "value"])


def quat_mul(a, b) -> np.ndarray:
    """Hamilton product of quaternions (w, x, y, z) [..., 4]: the rotation b, then the rotation a."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    aw, ax, ay, az = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bw, bx, by, bz = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def transporter_poses(pick_xy, place_xy, place_angle, pick_quat=None, height: float = PICK_HEIGHT):
    """The two poses ``step()`` takes from a Transporter's decisions: (pick_pose, place_pose), float64 [N, 7] each
    (position, quaternion (w, x, y, z)).  ``pick_xy`` and ``place_xy`` [N, 2] are world positions, ``place_angle`` [N] the
    angle of the place head's rotation bin (``perception.decode_place``), ``pick_quat`` the gripper's orientation at the pick
    (default ``home_quat()``).

    The sign of the turn: crop k of ``crop_matrices`` reads the map at p + R(a) u for the offset u from its
    pivot, a = 2 pi k / n_rotations, R = [[cos, -sin], [sin, cos]] in (column, row) -- and column runs along world x, row
    along world y, so R(a) is a turn by +a about world z.  A point of the picked object at p + v therefore shows in crop k
    at u = R(-a) v: laid over the place cell c, crop k shows the object at c + R(-a) v, turned by -a.  The place quaternion
    is the pick quaternion turned about world z by -place_angle (taken into (-pi, pi])."""
    pick_xy, place_xy = np.asarray(pick_xy, np.float64).reshape(-1, 2), np.asarray(place_xy, np.float64).reshape(-1, 2)
    n = len(pick_xy)
    q0 = np.broadcast_to(home_quat() if pick_quat is None else np.asarray(pick_quat, np.float64), (n, 4))
    turn = -np.asarray(place_angle, np.float64).reshape(n)
    turn = turn - 2.0 * np.pi * np.floor(turn / (2.0 * np.pi) + 0.5)          # [-pi, pi)
    turn = np.where(turn == -np.pi, np.pi, turn)
    qz = np.stack([np.cos(turn / 2), np.zeros(n), np.zeros(n), np.sin(turn / 2)], axis=-1)
    z = np.full((n, 1), float(height))
    return np.concatenate([pick_xy, z, q0], axis=1), np.concatenate([place_xy, z, quat_mul(qz, q0)], axis=1)


def _decision(best, shape, n_rotations, cell, kind):
    """A head's ``best`` (index and value per env) over maps of ``shape`` = (rows, columns) as a ``kind`` of decision"""
    cells, bins, angles = perception.decode_place(best.index, shape, n_rotations, check=False)
    return kind(cells, bins, angles, perception.cell_2_world(cells, HEIGHTMAP_BOUNDS, cell), best.value)


def _cell_target(cells, bins, features):
    """The target a head's loss takes: ``cells`` [N, 2] at ``bins`` [N] over the maps of ``features``, on its device"""
    target = perception.encode_place(np.asarray(cells), np.asarray(bins), tuple(features.shape[2:]))
    return torch.from_numpy(target).to(features.device)


class TransporterMixin:
    """``heightmap``, ``heightmap_views`` and the ``transporter_*`` methods of BatchedRearrangementEnv."""

    def heightmap(self, depth=None, rgb=None, seg=None, camera: str = OVERHEAD, bounds=None, cell: float = 0.0025):
        """Top-down orthographic maps of every env, the inputs of a Transporter network: a ``perception.HeightMap`` of
        CUDA tensors -- height above ``bounds``' lo_z [N, rows, columns], colour [N, rows, columns, 3], seg
        [N, rows, columns] and the source pixel of every cell -- over ``bounds`` (default HEIGHTMAP_BOUNDS) at ``cell``
        metres per cell, row along world y and column along world x (``perception.world_2_cell`` maps a pick or place
        position to its cell).  The frames are the caller's (``depth`` [N, H, W] with optional ``rgb`` / ``seg``, as
        ``render`` returns them, seen from ``camera``) or one ``render`` of the current state when ``depth`` is not
        given; ``self`` is not touched when it is."""
        if depth is None:
            rgb, depth, seg = self.render(camera=camera)
        depth, rgb, seg, cam12 = self._view(camera, rgb, depth, seg)
        return perception.heightmap(depth, rgb, seg, cam=cam12, bounds=HEIGHTMAP_BOUNDS if bounds is None else bounds,
                                    cell=cell)

    def _view(self, camera: str, rgb, depth, seg):
        """The frames of ``camera`` as a view of ``perception.heightmap_views``: (depth, rgb, seg, cam12), tensors on the
        device of ``depth``."""
        depth = torch.as_tensor(depth)
        cam = self._cameras[camera]
        cam12 = perception.heightmap_camera(cam["pos"], cam["mat"], cam["fovy"], int(depth.shape[1]), int(depth.shape[2]))
        return (depth, None if rgb is None else torch.as_tensor(rgb).to(depth.device),
                None if seg is None else torch.as_tensor(seg).to(depth.device), cam12)

    def heightmap_views(self, cameras, frames=None, bounds=None, cell: float = 0.0025):
        """``heightmap`` from several cameras at once, a ``perception.FusedHeightMap``: every cell takes the highest point
        any of the named ``cameras`` saw in it (the first camera among equal heights), so that what the overhead camera
        cannot see -- side faces, what the arm or a tall prop hides -- is filled from the others; ``view`` says which
        camera a cell came from.  ``frames`` is a list of (rgb, depth, seg) per camera as ``render_views`` returns it
        (rgb / seg may be None, in every camera or in none), or None for one ``render_views`` of the current state;
        ``self`` is not touched when it is given.  One launch of ``mre_heightmap_views`` for CUDA frames."""
        cameras = list(cameras)
        if frames is None:
            frames = self.render_views(cameras)
        if len(frames) != len(cameras):
            raise ValueError("one (rgb, depth, seg) per camera")
        views = [self._view(name, rgb, depth, seg) for name, (rgb, depth, seg) in zip(cameras, frames)]
        return perception.heightmap_views(views, bounds=HEIGHTMAP_BOUNDS if bounds is None else bounds, cell=cell)

    def transporter_sample(self, seed: int, draw: int = 0, depth=None, rgb=None, seg=None, cell: float = 0.0025,
                           n_rotations: int = 36, crop: int = 64, camera: str = OVERHEAD, maps=None):
        """One Transporter training sample per env on the device, a ``perception.TransporterSample``: the maps of
        ``heightmap(depth, rgb, seg, cell=cell)`` under a random rigid motion keyed by (``seed``, global env id, ``draw``),
        the pick and place cells of ``sort_colours(peek=True)`` moved with them, and ``n_rotations`` rotated crops of
        ``crop`` x ``crop`` cells around the moved pick cell.  An env with nothing left to move has its home pose as
        both cells; ``tries`` is -1 (and the maps unperturbed) where no motion kept both cells inside the map.  No state
        of the env changes: no place draw is consumed.  ``maps`` (a ``HeightMap`` or ``FusedHeightMap`` at ``cell``, such
        as ``heightmap_views`` returns) takes the place of the ``heightmap`` call."""
        return perception.transporter_sample(*self._labelled_maps(maps, depth, rgb, seg, camera, cell), seed=seed,
                                             env_ids=self.env_ids, draw=draw, n_rotations=n_rotations, crop=crop)

    def _labelled_maps(self, maps, depth, rgb, seg, camera, cell):
        """What the ``transporter_*`` producers start from: (maps, pick cells, place cells) -- ``maps`` or, without them,
        ``heightmap(depth, rgb, seg, camera, cell)``, and the cells of ``sort_colours(peek=True)`` in them."""
        if maps is None:
            maps = self.heightmap(depth, rgb, seg, camera=camera, cell=cell)
        _, pick, place = self.sort_colours(peek=True)
        return (maps, perception.world_2_cell(pick[:, :3], HEIGHTMAP_BOUNDS, cell),
                perception.world_2_cell(place[:, :3], HEIGHTMAP_BOUNDS, cell))

    def transporter_batch(self, seed: int, draw: int = 0, depth=None, rgb=None, seg=None, cell: float = 0.0025,
                          n_rotations: int = 36, crop: int = 64, channels=perception.CHANNELS_RGBH,
                          dtype=torch.bfloat16, camera: str = OVERHEAD, maps=None):
        """One Transporter training batch on the device as the tensors a network takes, a
        ``perception.TransporterBatch``: ``scene`` [N, C, rows, columns] and ``crops`` [N, n_rotations, C, crop, crop],
        channels-first, normalised by ``channels`` (a ``perception.Channels``) and in ``dtype``, with the
        moved pick and place cells and their flat indices.  The steps of ``transporter_sample`` up to the cells -- the same
        maps, the same motion for the same (``seed``, global env id, ``draw``) -- then ``perception.transporter_batch``.  No
        state of the env changes.  ``maps``, when given, takes the place of the ``heightmap`` call."""
        return perception.transporter_batch(*self._labelled_maps(maps, depth, rgb, seg, camera, cell), seed=seed,
                                            env_ids=self.env_ids, draw=draw, n_rotations=n_rotations, crop=crop,
                                            channels=channels, dtype=dtype)

    def transporter_place(self, scene_features, crop_features, cell: float = 0.0025):
        """The place decision of a Transporter's place head for every env, on the device: ``scene_features`` [N, D, rows,
        columns] (the network's output on ``transporter_batch``'s ``scene``) correlated with ``crop_features`` [N, R, D,
        crop, crop] (its output on the rotated ``crops``) by ``perception.correlate``, the best cell and rotation bin of
        every env by ``perception.decode_place``, and that cell's centre in the world by ``perception.cell_2_world`` on
        ``HEIGHTMAP_BOUNDS`` at ``cell`` metres per cell.  A ``PlaceDecision``: cells int64 [N, 2] (column, row), rotation
        bins int64 [N], angles float64 [N] (radians), xy float64 [N, 2] and the values float32 [N], on the features'
        device.  No logits are written and no state of the env changes."""
        best = perception.correlate(scene_features, crop_features)
        return _decision(best, scene_features.shape[2:], int(crop_features.shape[1]), cell, PlaceDecision)

    def transporter_loss(self, scene_features, crop_features, batch, weight=None):
        """The training loss of a Transporter's place head for every env, float32 [N], on the device:
        ``perception.place_loss`` of ``scene_features`` [N, D, rows, columns] and ``crop_features`` [N, R, D, crop, crop]
        (the network's outputs on ``batch.scene`` and ``batch.crops``) against the target of ``batch``, a
        ``perception.TransporterBatch``: its moved place cell at its rotation bin (``perception.encode_place``).
        Differentiable with respect to both feature tensors; NaN for an env whose place cell lies outside the map (where
        ``batch.tries`` is 0).  No logits are written and no state of the env changes."""
        target = _cell_target(batch.place, batch.rotation_index, scene_features)
        return perception.place_loss(scene_features, crop_features, target, weight)

    def transporter_pick(self, logits, cell: float = 0.0025):
        """The pick decision of a Transporter's attention head for every env, on the device: the best cell and rotation bin
        of ``logits`` [N, K, rows, columns] (the network's output on the scene; K pick rotations, 1 for a classic
        Transporter; -inf masks a cell) by ``perception.attend`` and ``perception.decode_pick``, and that cell's centre in
        the world by ``perception.cell_2_world`` on ``HEIGHTMAP_BOUNDS`` at ``cell`` metres per cell.  A ``PickDecision`` on
        the logits' device; nothing synchronises and no state of the env changes."""
        return _decision(perception.attend(logits), logits.shape[2:], int(logits.shape[1]), cell, PickDecision)

    def transporter_pick_loss(self, logits, batch, weight=None):
        """The training loss of a Transporter's attention head for every env, float32 [N], on the device:
        ``perception.pick_loss`` of ``logits`` [N, K, rows, columns] (the network's output on ``batch.scene``) against the
        target of ``batch``, a ``perception.TransporterBatch``: its moved pick cell at rotation bin 0
        (``perception.encode_pick``).  Differentiable with respect to ``logits``.  An env whose pick cell lies outside the
        map has no label: its loss is NaN and its gradient that of the logsumexp alone, so the caller gives such envs
        ``weight`` 0 (the gradient is then exactly 0) and leaves them out of the sum.  No state of the env changes."""
        return perception.pick_loss(logits, _cell_target(batch.pick, np.zeros(len(batch.pick), np.int64), logits), weight)

    def transporter_act(self, attention, query, key, *, channels, dtype, n_rotations: int = 36, crop: int = 64,
                        cell: float = 0.0025, depth=None, rgb=None, seg=None, maps=None):
        """One decision of a Transporter policy for every env, from the observation to the two poses ``step()`` takes:
        (pick_pose [N, 7], place_pose [N, 7], ``PickDecision``, ``PlaceDecision``).  ``attention``, ``query`` and ``key`` are
        the caller's networks: ``attention(scene)`` -> pick logits [N, K, rows, columns], ``key(scene)`` -> [N, D, rows,
        columns] and ``query(crops)`` -> [N * n_rotations, D, crop, crop] on crops [N * n_rotations, C, crop, crop].

        ``heightmap(depth, rgb, seg, cell=cell)``; ``scene`` = one ``perception.warp_inputs`` of the maps under the identity
        (``channels``, ``dtype``); ``transporter_pick`` of ``attention(scene)``; ``perception.crop_matrices_device`` at the
        predicted cells and one ``warp_inputs`` for the rotated crops around them; ``transporter_place`` of ``key(scene)``
        and ``query(crops)``; ``transporter_poses``.  Everything up to the poses stays on the device and nothing waits for
        it; the poses are numpy because ``step()`` takes numpy.  The pick quaternion is ``home_quat()``, the place
        quaternion that turned about world z by the place decision (``transporter_poses`` has the sign).  No state of the env
        changes: the caller passes the poses to ``step()``.  ``maps``, when given (``heightmap_views``' for a policy that
        looks through several cameras), takes the place of the ``heightmap`` call."""
        if maps is None:
            maps = self.heightmap(depth, rgb, seg, cell=cell)
        height, colour = maps[0], maps[1]
        n, dev = int(height.shape[0]), height.device
        kw = dict(channels=channels, dtype=dtype)
        identity = torch.zeros((n, 6), dtype=torch.float32, device=dev)   # filled on the device: no copy from the host
        identity[:, 0] = 1.0
        identity[:, 4] = 1.0
        scene = perception.warp_inputs(height, colour, mats=identity, **kw)
        pick = self.transporter_pick(attention(scene), cell)
        mats, index = perception.crop_matrices_device(pick.cells, n_rotations, crop)
        crops = perception.warp_inputs(height, colour, mats=mats, index=index, out_shape=(crop, crop), **kw)
        features = query(crops)
        place = self.transporter_place(key(scene), features.reshape((n, n_rotations) + tuple(features.shape[1:])), cell)
        packed = torch.cat([pick.xy, place.xy, place.angle[:, None]], dim=1).cpu().numpy()   # the one wait
        pick_pose, place_pose = transporter_poses(packed[:, 0:2], packed[:, 2:4], packed[:, 4])
        return pick_pose, place_pose, pick, place
