"""RearrangementEnv on the MI355X batched physics step.

Drop-in shell of the reference's ``tasks/rearrangement.py`` (class RearrangementEnv,
:51-779): same constructor arguments, ``reset()`` / ``step(action_dict)`` 4-tuples and
observation shapes, ``pick`` / ``place`` scripted macros, ``sort_colours`` / ``prop_pick`` /
``prop_place`` demo helpers and camera maths -- with the inner loop
(``RobotArm.run_controller`` -> OSC + ``physics.step()``) executed by the HIP kernels for
``num_envs`` environments in lockstep.  ``BatchedRearrangementEnv`` carries a leading env
axis on every array; ``RearrangementEnv`` is the batch of one with reference shapes and
reference error behaviour (RuntimeError when a phase does not converge).

Observations: with ``render=True`` the batched overhead camera (csrc/mre_render.hip) renders
depth + RGB of every env and ``props_info`` boxes / ``pixel_2_world``
read the rendered segmentation / depth; with ``render=False`` (BASELINE configs[4]: "render
stubbed") they are zero images of the reference shapes and the pixel/world conversions use the
analytic pinhole model with the table plane for depth.

Solver: the reference sets timestep / gravity / nconmax / njmax only (tasks/rearrangement.py:77-80),
so its MuJoCo runs the default Newton solver -- the env's default here too (``solver="Newton"``);
``solver="PGS"`` selects the solver BASELINE.json's north_star prescribes for the bench.
"""
from __future__ import annotations

import collections
import enum
from typing import Dict, Optional

import numpy as np
import torch
from scipy.spatial.transform import Rotation as R

from .. import demo_logic, perception, placement, rng
from ..config import Cfg, colour_separator_task_config, default_config  # noqa: F401
from ..model import compile as _compile
from ..model import spec as _spec
from ..models.robot_arm import RobotArm
from ..physics import BatchedPhysics

try:  # dm_env is what the reference returns; fall back to an equivalent tuple
    import dm_env
    from dm_env import specs as _specs
    TimeStep, StepType = dm_env.TimeStep, dm_env.StepType
    _Array = _specs.Array
except Exception:  # pragma: no cover - dm_env absent on the target image
    class StepType(enum.IntEnum):
        FIRST = 0
        MID = 1
        LAST = 2

    TimeStep = collections.namedtuple("TimeStep", ["step_type", "reward", "discount", "observation"])

    class _Array:
        def __init__(self, shape, dtype, name=None):
            self.shape, self.dtype, self.name = tuple(shape), np.dtype(dtype), name

        def __repr__(self):
            return f"Array(shape={self.shape}, dtype={self.dtype}, name={self.name})"

DEFAULT_CONFIG = default_config()
TABLE_TOP_Z = 0.4
PICK_HEIGHT = 0.575     # tasks/rearrangement.py:362,405  ("hardcode for now :(")
PRE_PICK_HEIGHT = 0.9   # :364,408
PROP_GEOM_ID0 = 12      # geom ids of prop_0..3 in the compiled scene

PropsLabels = collections.namedtuple("PropsLabels", ["shape", "colour", "texture"])
# environment/props.py:13-20
COLOURS = {"red": (1.0, 0.0, 0.0), "green": (0.0, 1.0, 0.0), "blue": (0.0, 0.0, 1.0),
           "yellow": (1.0, 1.0, 0.0), "cyan": (0.0, 1.0, 1.0), "magenta": (1.0, 0.0, 1.0)}
COLOUR_NOISE = 0.1      # environment/props.py:274,290
OVERHEAD = "overhead_camera/overhead_camera"
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


def mat2quat(mat3x3) -> np.ndarray:
    """mujoco.mju_mat2Quat: (w, x, y, z)."""
    return _compile.m2q(np.asarray(mat3x3, np.float64).reshape(3, 3))


def home_quat() -> np.ndarray:
    """mju_mat2Quat(R.from_euler('xyz',[0,180,0])) (tasks/rearrangement.py:391-393)."""
    return mat2quat(R.from_euler("xyz", [0, 180, 0], degrees=True).as_matrix())


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


class BatchedRearrangementEnv:
    """num_envs independent RearrangementEnv instances stepped in lockstep on one GPU."""

    def __init__(self, cfg: Optional[Cfg] = None, num_envs: int = 1, viewer=None, device: int = 0,
                 seed: Optional[int] = None, env_id_offset: int = 0, env_ids=None, render: bool = False,
                 solver: str = "Newton", torque_law=None):
        self._cfg = cfg if cfg is not None else DEFAULT_CONFIG
        self.torque_law = torque_law   # law(terms, target) -> tau run in place of the in-kernel OSC (models/robot_arm.py)
        cfg = self._cfg
        self.num_envs = int(num_envs)
        self.has_viewer = False  # no viewer on a headless GPU batch (tasks/rearrangement.py:64-70)
        # global env ids key every random draw; explicit ids may repeat (envs sharing a scene)
        self.env_ids = (np.arange(env_id_offset, env_id_offset + self.num_envs) if env_ids is None
                        else np.asarray(env_ids, np.int64).reshape(self.num_envs))
        self._explicit_ids = env_ids is not None
        self.seed = int(cfg.task.initializers.seed if seed is None else seed)
        ac = cfg.robots.arm.actuator_config
        lim = [float(ac[ac.joint_actuator_mapping[f"joint{i + 1}"]].ctrlrange.split()[1]) for i in range(7)]
        scene = _spec.default_scene(dict(physics_dt=cfg.physics_dt, gravity=cfg.gravity, motor_ctrlrange=lim,
                                         home=cfg.robots.arm.default_configurations.home, solver=solver))
        self._model = _compile.compile_scene(scene)
        self._physics = BatchedPhysics(self.num_envs, model=self._model, device=device)
        # ---- props: count / size / colour per env (environment/props.py:583-639)
        pc = cfg.arena.props
        u = rng.uniform(self.seed ^ 0xC0105, self.env_ids, [0], 12)[0]
        if pc.min_objects == pc.max_objects:
            self.nprops = np.full(self.num_envs, pc.min_objects, np.int32)
        else:  # np.random.randint(min, max): max exclusive
            self.nprops = (pc.min_objects + np.floor(u[:, 0] * (pc.max_objects - pc.min_objects))).astype(np.int32)
        assert self.nprops.max() <= 4, "the compiled scene has 4 cube slots"
        size = pc.min_object_size + (pc.max_object_size - pc.min_object_size) * u[:, 1:5]
        self.prop_half_size = np.repeat(size[:, :, None], 3, axis=2)
        self.prop_colours = []
        for i in range(self.num_envs):
            cols = []
            for p in range(int(self.nprops[i])):
                cols.append(pc.colours[p] if p <= 1 else pc.colours[int(u[i, 5 + p] * len(pc.colours)) % len(pc.colours)])
            self.prop_colours.append(cols)
        self._physics.set_props(self.nprops, self.prop_half_size)
        # ---- cameras (config/arena/cameras/*.yaml); only the pose / fovy constants are needed
        self._cameras = {}
        for cam in cfg.arena.cameras:
            q = np.asarray(cam.quat, np.float64)
            q = q / np.linalg.norm(q)
            self._cameras[f"{cam.name}/{cam.name}"] = dict(pos=np.asarray(cam.pos, np.float64),
                                                           mat=_compile.q2m(q), fovy=float(cam.fovy),
                                                           height=int(cam.height), width=int(cam.width))
            if cam.name == "overhead_camera":
                self.overhead_camera_height, self.overhead_camera_width = int(cam.height), int(cam.width)
        # ---- overhead camera images (mre_render): cube albedo = colour + noise (props.py:288-291),
        # table grey (tasks/rearrangement.py:91), robot hulls dark
        self.render_observations = bool(render)
        un = rng.uniform(self.seed ^ 0xC0FFEE, self.env_ids, [0], 12)[0].reshape(self.num_envs, 4, 3)
        self.prop_rgb = np.zeros((self.num_envs, 4, 3), np.uint8)
        self.prop_rgba = np.ones((self.num_envs, 4, 4))
        for i in range(self.num_envs):
            for p, c in enumerate(self.prop_colours[i]):
                rgbf = np.clip(np.asarray(COLOURS.get(c, (0.5, 0.5, 0.5))) + COLOUR_NOISE * (2 * un[i, p] - 1), 0.0, 1.0)
                self.prop_rgba[i, p, :3] = rgbf
                self.prop_rgb[i, p] = np.round(rgbf * 255)
        geom_rgb = np.full((int(self._model["ngeom"][0]), 3), 0.25, np.float32)
        geom_rgb[1] = 0.5
        self._physics.set_render_colours(self.prop_rgb, geom_rgb)
        self._reset_count = 0
        self._place_count = 0
        self._place_counts = np.zeros(self.num_envs, np.int64)  # prop_place calls per env (RNG key)
        self._zones = None  # [N, 4, 4] colour zone of every cube (set when the colours are drawn)
        # pose of the reference's mocap target body (tasks/rearrangement.py:130-140; simulation_tuning_mode)
        self.mocap_pos = np.tile(np.array([0.4, 0.0, 0.6]), (self.num_envs, 1))
        self.mocap_quat = np.tile(home_quat(), (self.num_envs, 1))
        self._robot: Optional[RobotArm] = None
        self.mode = None
        self.eef_home_pose = None
        self.last_converged = np.ones(self.num_envs, bool)
        self.placement_failed = np.zeros(self.num_envs, bool)   # reset(): PropPlacer found no pose for a cube
        self.not_settled = np.zeros(self.num_envs, bool)
        self.failed_phase = np.full(self.num_envs, "", dtype=object)

    # ------------------------------------------------------------------ misc
    def close(self) -> None:
        self._physics.close()

    @property
    def physics(self) -> BatchedPhysics:
        return self._physics

    @property
    def model(self) -> dict:
        """tasks/rearrangement.py:219-221: the compiled model (arrays of model/compile.py; there is no MjModel)."""
        return self._model

    @property
    def data(self) -> BatchedPhysics:
        """tasks/rearrangement.py:223-225: the batched state holder (qpos / qvel / ctrl / contacts accessors)."""
        return self._physics

    def _zeros_obs(self):
        h, w = self.overhead_camera_height, self.overhead_camera_width
        n = self.num_envs
        rgb = np.broadcast_to(np.zeros((1, 1, 1, 1), np.uint8), (n, h, w, 3))
        depth = np.broadcast_to(np.zeros((1, 1, 1), np.float32), (n, h, w))
        return {"overhead_camera/rgb": rgb, "overhead_camera/depth": depth}

    def render(self, rgb: bool = True, depth: bool = True, seg: bool = True, camera: str = OVERHEAD):
        """Overhead camera images of every env's current state as CUDA tensors (rgb uint8 [N,H,W,3],
        depth float32 [N,H,W], seg uint8 [N,H,W]: 12 + p = cube p, 1 table, 2..11 and 16..19 robot, 255 nothing):
        the batched form of the reference's renderer / depth_renderer / seg_renderer passes
        (tasks/rearrangement.py:254-280, 460-478)."""
        cam = self._cameras[camera]
        return self._physics.render(cam["pos"], cam["mat"], cam["fovy"], self.overhead_camera_height,
                                    self.overhead_camera_width, rgb=rgb, depth=depth, seg=seg)

    def add_camera(self, name: str, pos, quat, fovy: float, height: int, width: int) -> str:
        """Register a further fixed camera, as the reference's ``add_camera`` does at build time (environment/cameras.py):
        ``pos`` and ``quat`` (w, x, y, z) in the world, ``fovy`` degrees, ``height`` x ``width`` pixels.  Returns the key
        ``"name/name"`` that ``render``, ``render_views``, ``heightmap`` and ``heightmap_views`` take.  The overhead set-up
        can so carry the two obliques of config/arena/cameras/rearrangement.yaml beside its own camera."""
        key = f"{name}/{name}"
        if key in self._cameras:
            raise ValueError(f"camera {key} exists")
        if int(height) < 1 or int(width) < 1:
            raise ValueError("height and width must be at least 1")
        q = np.asarray(quat, np.float64).reshape(4)
        self._cameras[key] = dict(pos=np.asarray(pos, np.float64).reshape(3), mat=_compile.q2m(q / np.linalg.norm(q)),
                                  fovy=float(fovy), height=int(height), width=int(width))
        return key

    def render_views(self, cameras, rgb: bool = True, depth: bool = True, seg: bool = True):
        """``render`` through each of the named ``cameras`` at that camera's own configured size: a list of
        (rgb, depth, seg), one per camera in the order given.  (``render`` itself renders every camera at the overhead
        camera's size.)"""
        out = []
        for name in cameras:
            cam = self._cameras[name]
            out.append(self._physics.render(cam["pos"], cam["mat"], cam["fovy"], cam["height"], cam["width"], rgb=rgb,
                                            depth=depth, seg=seg))
        return out

    def prop_bboxes(self, seg=None) -> np.ndarray:
        """PASCAL-VOC boxes [N, 4 cubes, (xmin, ymin, xmax, ymax)] of the VISIBLE pixels of every cube
        in the segmentation image (get_bbox, tasks/rearrangement.py:254-268); -1 where a cube is not
        in view or not in use.  One pass over the image on the device (perception.seg_labels) for a CUDA
        ``seg`` or the env's own render; ``self`` is not touched when ``seg`` is given."""
        import torch
        if seg is None:
            seg = self.render(rgb=False, depth=False)[2]
        box = perception.seg_labels(torch.as_tensor(seg), None, PROP_GEOM_ID0, 4).box
        return box.contiguous().cpu().numpy()

    def prop_labels(self, seg=None, depth=None) -> dict:
        """What a frame says about every cube slot, as numpy arrays: ``bbox`` int64 [N, 4, 4] (prop_bboxes),
        ``visible_pixels`` int64 [N, 4] (0: the cube is hidden, out of view or not in use), ``centroid`` float64
        [N, 4, (x, y)] of the visible pixels (NaN where there are none) and ``nearest_depth`` float32 [N, 4], the
        smallest depth among them (+inf where there are none; None when ``seg`` is given without ``depth``).
        The images are the caller's (CUDA or CPU tensors [N, H, W]) or one ``render(rgb=False)`` of the current state
        when neither is given; ``self`` is not touched when ``seg`` is given."""
        import torch
        if seg is None:
            _, d, seg = self.render(rgb=False, depth=depth is None)
            depth = d if depth is None else depth
        seg = torch.as_tensor(seg)
        lab = perception.seg_labels(seg, None if depth is None else torch.as_tensor(depth).to(seg.device), PROP_GEOM_ID0, 4)
        return {"bbox": lab.box.contiguous().cpu().numpy(), "visible_pixels": lab.count.contiguous().cpu().numpy(),
                "centroid": perception.centroid(lab).cpu().numpy(),
                "nearest_depth": None if lab.zmin is None else lab.zmin.cpu().numpy()}

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

    def _compute_observation(self):
        if not self.render_observations:
            return self._zeros_obs()
        rgb, depth, _ = self.render(seg=False)
        return {"overhead_camera/rgb": rgb, "overhead_camera/depth": depth}

    def observation_spec(self):
        h, w = self.overhead_camera_height, self.overhead_camera_width
        return {"overhead_camera/depth": _Array(shape=(h, w), dtype=np.float32),
                "overhead_camera/rgb": _Array(shape=(h, w, 3), dtype=np.float32)}  # (sic: :448; images are uint8)

    def action_spec(self) -> Dict[str, _Array]:
        return {"pose": _Array(shape=(7,), dtype=np.float64),
                "pixel_coords": _Array(shape=(2,), dtype=np.int64),
                "gripper_rot": _Array(shape=(1,), dtype=np.float64)}

    # ----------------------------------------------------------------- reset
    def reset(self) -> TimeStep:
        """Physics.reset, arm to home, PropPlacer (sample + settle), new RobotArm
        (tasks/rearrangement.py:297-337)."""
        ws = self._cfg.task.initializers.workspace
        self._physics.reset()
        if self._explicit_ids:
            self._physics.set_env_ids(self.env_ids)
        else:
            self._physics.set_env_id_offset(int(self.env_ids[0]))
        # PropPlacer: contact-based rejection sampling, then settle with the robot frozen; every env
        # stops by itself (>= 0.3 s, <= 2 s, max|qvel| < 1e-3 and max|qacc| < 1e-2) inside the kernel
        self._physics.place_props(self.seed + 104729 * self._reset_count, ws.min_pose, ws.max_pose,
                                  settle_steps=300)
        self._reset_count += 1
        # mre_place_props flags the envs whose rejection sampling ran out of attempts (MRE_ST_PLACEMENT_FAILED) or whose
        # cubes never came to rest (MRE_ST_NOT_SETTLED) and returns MRE_OK.  The reference raises
        # RuntimeError(_REJECTION_SAMPLING_FAILED) out of reset() (prop_initializer.py:230-233) and the data-generation loop
        # drops the episode: a batch of one raises likewise, a batch carries the mask so that sort_colours() and
        # BatchedEpisodeLogger leave those envs out.
        st = self._physics.status()
        self.placement_failed = (st & 16) != 0
        self.not_settled = (st & 8) != 0
        if self.num_envs == 1 and self.placement_failed[0]:
            raise RuntimeError("Failed to find a non-colliding pose for some props")
        steps = int(np.abs(self._physics.settle_steps()).max())
        cp = self._cfg.robots.arm.controller_config.controller_params
        mm = self._cfg.robots.end_effector.controller_config.controller
        self._robot = RobotArm(self._physics, controller_params=cp, gripper_cfg=mm, torque_law=self.torque_law)
        self._robot.time = steps * self._physics.timestep
        pose0 = np.atleast_2d(self._robot.eef_pose).copy()
        pose0[:, 0] -= 0.1  # reference shifts x although the comment says "up" (App. D.5)
        self.eef_home_pose = pose0
        self.mode = "pick"
        self.last_converged[:] = True
        self.failed_phase[:] = ""
        return TimeStep(step_type=StepType.FIRST, reward=0.0, discount=0.0,
                        observation=self._compute_observation())

    # ------------------------------------------------------------------ step
    def step(self, action_dict) -> TimeStep:
        observation = self._compute_observation()  # rendered BEFORE acting (App. D.1)
        if self.mode == "pick":
            self.pick(action_dict["pose"])
            self.mode = "place"
        else:
            self.place(action_dict["pose"])
            self.mode = "pick"
        return TimeStep(step_type=StepType.MID, reward=0.0, discount=0.0, observation=observation)

    def _phase(self, name: str, duration: float):
        conv = np.atleast_1d(self._robot.run_controller(duration))
        newly = (~conv) & (self.failed_phase == "")
        self.failed_phase[newly] = name
        self.last_converged &= conv
        return conv

    def interactive_tuning(self, mocap_pos=None, mocap_quat=None):
        """One tick of the reference's tuning loop (tasks/rearrangement.py:753-779): the OSC target follows
        the mocap body (position + [0, 0, 0.175], its quaternion, zero velocities), the arm and gripper commands
        are computed once and held for 5 physics steps.  There is no viewer to drag a mocap body here, so its
        pose is state of the env (``mocap_pos`` [N, 3] / ``mocap_quat`` [N, 4], initialised like the reference's
        body at (0.4, 0, 0.6), gripper down) that the caller may move, per env, through the arguments."""
        if mocap_pos is not None:
            self.mocap_pos[:] = np.asarray(mocap_pos, np.float64)
        if mocap_quat is not None:
            self.mocap_quat[:] = np.asarray(mocap_quat, np.float64)
        self._robot.arm_controller.set_target(position=self.mocap_pos + np.array([0.0, 0.0, 0.175]),
                                              quat=self.mocap_quat, velocity=np.zeros(3),
                                              angular_velocity=np.zeros(3))
        # compute_control_output() + 5 x (set_control, step) = one control tick of the fused launch
        self._physics.run_controller(1, self._robot.control_steps)
        for _ in range(self._robot.control_steps):
            self._robot.time += self._robot.timestep

    def time_limit_exceeded(self) -> bool:
        """tasks/rearrangement.py:216-217 (the reference reads a module-level ``cfg.time_limit`` that its config
        tree does not define; absent means no limit)."""
        return self._robot.time >= float(self._cfg.get("time_limit", float("inf")))

    def _pose2d(self, pose):
        pose = np.asarray(pose)
        return pose.reshape(self.num_envs, 7) if pose.ndim == 1 else pose

    def pick(self, pose):
        """Scripted pick (tasks/rearrangement.py:358-399): pre-pick 2 s, descend 2 s,
        close 1 s, lift 2 s, home 2 s."""
        pose[..., 2] = PICK_HEIGHT  # in-place, like the reference
        p = self._pose2d(pose).astype(np.float64)
        pre = p.copy()
        pre[:, 2] = PRE_PICK_HEIGHT
        c = self._robot.arm_controller
        c.set_target(position=pre[:, :3], velocity=np.zeros(3), quat=pre[:, 3:], angular_velocity=np.zeros(3))
        self._phase("Failed to move arm to pre pick position", 2.0)
        c.set_target(position=p[:, :3])
        self._phase("Failed to move arm to pick position", 2.0)
        self._robot.end_effector_controller.status = "max"
        self._phase("Failed to close gripper", 1.0)
        c.set_target(position=pre[:, :3])
        self._phase("Failed to move arm to pre grasp position", 2.0)
        c.set_target(position=self.eef_home_pose, quat=home_quat())
        self._phase("Failed to move arm to home position", 2.0)

    def place(self, pose):
        """Scripted place (tasks/rearrangement.py:401-440)."""
        pose[..., 2] = PICK_HEIGHT
        p = self._pose2d(pose).astype(np.float64)
        pre = p.copy()
        pre[:, 2] = PRE_PICK_HEIGHT
        c = self._robot.arm_controller
        c.set_target(position=pre[:, :3], quat=pre[:, 3:])
        self._phase("Failed to move arm to pre place position", 2.0)
        c.set_target(position=p[:, :3])
        self._phase("Failed to move arm to place position", 2.0)
        self._robot.end_effector_controller.status = "min"
        self._phase("Failed to open gripper", 1.0)
        c.set_target(position=pre[:, :3])
        self._phase("Failed to move arm to pre place position", 2.0)
        c.set_target(position=self.eef_home_pose, quat=home_quat())
        self._phase("Failed to move arm to home position", 2.0)

    # ---------------------------------------------------------------- camera
    def _get_camera_intrinsics(self, camera_name, h, w, inverse=False):
        fov = self._cameras[camera_name]["fovy"]
        f = (1.0 / np.tan(np.deg2rad(fov) / 2)) * self.overhead_camera_height / 2.0
        return np.array([[-f, 0, (w - 1) / 2], [0, f, (h - 1) / 2], [0, 0, 1]])

    def _get_camera_extrinsics(self, camera_name):
        cam = self._cameras[camera_name]
        ext = np.eye(4)
        ext[:3, :3] = cam["mat"].T
        ext[:3, 3] = -cam["mat"].T @ cam["pos"]
        return ext

    def world_2_pixel(self, camera_name, coords):
        """tasks/rearrangement.py:533-548 (coords [3] or [N,3])."""
        K = self._get_camera_intrinsics(camera_name, self.overhead_camera_height, self.overhead_camera_width)
        E = self._get_camera_extrinsics(camera_name)
        c = np.atleast_2d(np.asarray(coords, np.float64))
        cam = (E @ np.concatenate([c, np.ones((len(c), 1))], axis=1).T).T
        cam = cam[:, :3] / cam[:, 3:4]
        img = (K @ cam.T).T
        img = img[:, :2] / img[:, 2:3]
        out = np.round(img).astype(np.int32)
        return out[0] if np.asarray(coords).ndim == 1 else out

    def pixel_2_world(self, camera_name, coords, env: int = 0):
        """tasks/rearrangement.py:505-531: the pixel's rendered depth pushed back through the pinhole
        model (env selects the image of a batch).  Without rendering the depth is that of the table
        plane: the pixel ray intersected with z = table top."""
        K = self._get_camera_intrinsics(camera_name, self.overhead_camera_height, self.overhead_camera_width)
        E = self._get_camera_extrinsics(camera_name)
        coords = np.asarray(coords, np.float64)
        ray_c = np.linalg.inv(K) @ np.concatenate([coords, np.ones(1)])
        cam = self._cameras[camera_name]
        if self.render_observations:
            rc = np.round(coords).astype(np.int32)  # coords_rounded (:509)
            mask = np.zeros(self.num_envs, np.uint8)
            mask[env] = 1
            _, dimg, _ = self._physics.render(cam["pos"], cam["mat"], cam["fovy"], self.overhead_camera_height,
                                              self.overhead_camera_width, rgb=False, seg=False, mask=mask)
            depth = float(dimg[env, rc[1], rc[0]])
        else:
            d_w = cam["mat"] @ (-ray_c)  # camera looks along -z
            depth = (TABLE_TOP_Z - cam["pos"][2]) / d_w[2]
        camc = np.concatenate([ray_c * (-depth), np.ones(1)])
        w = np.linalg.inv(E) @ camc
        return w[:3] / w[3]

    def pixel_2_world_batch(self, camera_name, coords, depth=None) -> np.ndarray:
        """pixel_2_world for one pixel per env: coords [N, 2] (x, y) -> world points [N, 3] float64, row i equal to
        ``pixel_2_world(camera_name, coords[i], env=i)``.  With rendering on, the depths are one gather from ``depth``
        [N, H, W] (the caller's, e.g. the observation's, or one render of the batch); without, the table-plane ray.
        A pixel outside the image raises ValueError."""
        h, w = self.overhead_camera_height, self.overhead_camera_width
        K = self._get_camera_intrinsics(camera_name, h, w)
        E = self._get_camera_extrinsics(camera_name)
        coords = np.asarray(coords, np.float64)
        if coords.shape != (self.num_envs, 2):
            raise ValueError(f"coords must be [{self.num_envs}, 2]")
        rc = np.round(coords).astype(np.int64)  # coords_rounded (:509)
        if (rc < 0).any() or (rc[:, 0] >= w).any() or (rc[:, 1] >= h).any():
            raise ValueError(f"pixel outside the {w} x {h} image")
        ray_c = (np.linalg.inv(K) @ np.concatenate([coords, np.ones((self.num_envs, 1))], axis=1).T).T
        cam = self._cameras[camera_name]
        if self.render_observations:
            if depth is None:
                depth = self._physics.render(cam["pos"], cam["mat"], cam["fovy"], h, w, rgb=False, seg=False)[1]
            if tuple(depth.shape) != (self.num_envs, h, w):
                raise ValueError(f"depth must be [{self.num_envs}, {h}, {w}]")
            if hasattr(depth, "cpu"):
                import torch
                env = torch.arange(self.num_envs, device=depth.device)
                d = depth[env, torch.as_tensor(rc[:, 1], device=depth.device), torch.as_tensor(rc[:, 0], device=depth.device)]
                d = d.cpu().numpy().astype(np.float64)
            else:
                d = np.asarray(depth)[np.arange(self.num_envs), rc[:, 1], rc[:, 0]].astype(np.float64)
        else:
            d_w = (cam["mat"] @ (-ray_c).T).T  # camera looks along -z
            d = (TABLE_TOP_Z - cam["pos"][2]) / d_w[:, 2]
        camc = np.concatenate([ray_c * (-d[:, None]), np.ones((self.num_envs, 1))], axis=1)
        wp = (np.linalg.inv(E) @ camc.T).T
        return wp[:, :3] / wp[:, 3:4]

    def get_camera_params(self, camera_name):
        return {"intrinsics": self._get_camera_intrinsics(camera_name, self.overhead_camera_height, self.overhead_camera_width),
                "extrinsics": self._get_camera_extrinsics(camera_name)}

    def get_camera_metadata(self):
        K = self._get_camera_intrinsics("overhead_camera/overhead_camera", self.overhead_camera_height, self.overhead_camera_width)
        E = self._get_camera_extrinsics("overhead_camera/overhead_camera")
        quat = R.from_matrix(E[:3, :3]).as_quat()
        # NB the reference reads the translation from row 3 of the 4x4 (always 0,0,0): kept (:563-565)
        return {"intrinsics": {"fx": K[0, 0], "fy": K[1, 1], "cx": K[0, 2], "cy": K[1, 2]},
                "extrinsics": {"x": E[3, 0], "y": E[3, 1], "z": E[3, 2],
                               "qx": quat[0], "qy": quat[1], "qz": quat[2], "qw": quat[3]}}

    # ------------------------------------------------------------ demo logic
    def props_info_env(self, i: int, prop_pose: Optional[np.ndarray] = None, bboxes: Optional[np.ndarray] = None) -> dict:
        """props_info of env i (tasks/rearrangement.py:227-295); keys are geom ids.  With rendering
        enabled the bounding boxes come from the segmentation image like the reference's (visible
        pixels, empty array when out of view); otherwise from the projected cube corners."""
        if prop_pose is None:
            prop_pose = self._physics.sites()[2]
        if bboxes is None and self.render_observations:
            bboxes = self.prop_bboxes()
        info = {}
        for p in range(int(self.nprops[i])):
            pos = prop_pose[i, p, :3].astype(np.float64)
            qw = prop_pose[i, p, 3:7].astype(np.float64)
            mat = _compile.q2m(qw / np.linalg.norm(qw))
            half = self.prop_half_size[i, p]
            corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * half
            px = self.world_2_pixel("overhead_camera/overhead_camera", pos + corners @ mat.T)
            bbox = np.array([px[:, 0].min(), px[:, 1].min(), px[:, 0].max(), px[:, 1].max()])
            if bboxes is not None:
                bbox = bboxes[i, p] if bboxes[i, p, 0] >= 0 else np.array([])
            info[PROP_GEOM_ID0 + p] = {
                "prop_name": f"prop_{p}", "position": pos,
                "orientation": R.from_matrix(mat).as_quat(),  # scipy (x,y,z,w) like the reference
                "rgba": self.prop_rgba[i, p].copy(), "bbox": bbox,
                "labels": PropsLabels("cube", self.prop_colours[i][p], "plain")}
        return info

    def props_info(self) -> dict:
        """props_info_env for the whole batch, as arrays over [N envs, 4 cube slots]: ``position`` [N, 4, 3],
        ``orientation`` [N, 4, 4] (scipy order x, y, z, w), ``rgba`` [N, 4, 4], ``bbox`` int64 [N, 4, 4],
        ``visible_pixels`` int64 [N, 4] and ``in_use`` bool [N, 4] (slot p < nprops).  Slot p of env i agrees with
        ``props_info_env(i)[PROP_GEOM_ID0 + p]`` wherever in_use is set; the scalar call's empty bbox (cube not in view)
        is -1 here, like every entry of a slot not in use (position and orientation: NaN).  With rendering on, boxes and
        visible pixel counts come from ONE segmentation render of the batch; without, boxes are the projected cube
        corners and visible_pixels is -1 (not known).  (RearrangementEnv, the batch of one, keeps the reference's
        ``props_info`` property: the dict of props_info_env(0).)"""
        n = self.num_envs
        in_use = np.arange(4)[None, :] < np.asarray(self.nprops)[:, None]
        pose = self._physics.sites()[2].astype(np.float64)
        qw = np.where(in_use[..., None], pose[..., 3:7], np.array([1.0, 0.0, 0.0, 0.0]))
        qw = qw / np.linalg.norm(qw, axis=2, keepdims=True)
        mat = np.moveaxis(_compile.q2m(np.moveaxis(qw.reshape(n * 4, 4), 1, 0)), 2, 0)   # [N * 4, 3, 3]
        position = np.where(in_use[..., None], pose[..., :3], np.nan)
        orientation = np.where(in_use[..., None], R.from_matrix(mat).as_quat().reshape(n, 4, 4), np.nan)
        if self.render_observations:
            lab = self.prop_labels(self.render(rgb=False, depth=False)[2])
            bbox = np.where(in_use[..., None], lab["bbox"], -1)
            visible = np.where(in_use, lab["visible_pixels"], 0)
        else:
            bbox = np.full((n, 4, 4), -1, np.int64)
            visible = np.full((n, 4), -1, np.int64)
            unit = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
            for i, p in zip(*np.nonzero(in_use)):
                px = self.world_2_pixel("overhead_camera/overhead_camera",
                                        position[i, p] + (unit * self.prop_half_size[i, p]) @ mat[4 * i + p].T)
                bbox[i, p] = [px[:, 0].min(), px[:, 1].min(), px[:, 0].max(), px[:, 1].max()]
        return {"position": position, "orientation": orientation, "rgba": self.prop_rgba.copy(), "bbox": bbox,
                "visible_pixels": visible, "in_use": in_use}

    def prop_pick_env(self, i: int, prop_id: int, info: Optional[dict] = None) -> np.ndarray:
        """tasks/rearrangement.py:579-595."""
        info = info or self.props_info_env(i)
        obj_pose, obj_quat = info[prop_id]["position"], info[prop_id]["orientation"]
        m = R.from_quat(obj_quat).as_matrix()
        rz = abs(np.rad2deg(np.arctan2(m[1, 0], m[0, 0])))
        rz = min([rz, rz - 90])
        grasp = mat2quat(R.from_euler("xyz", [0, 180, rz], degrees=True).as_matrix())
        return np.concatenate([obj_pose, grasp])

    def prop_place_env(self, i: int, prop_id: int, min_pose=None, max_pose=None, info: Optional[dict] = None):
        """Collision-free place pose (tasks/rearrangement.py:597-665): uniform samples in the bounds,
        the cube moved there and physics.forward() evaluated on the device (mre_prop_place), rejected
        while a contact with a geom other than the table has dist <= 0.05."""
        ws = self._cfg.task.initializers.workspace
        lo = np.asarray(ws.min_pose if min_pose is None else min_pose, np.float64)
        hi = np.asarray(ws.max_pose if max_pose is None else max_pose, np.float64)
        prop = np.full(self.num_envs, -1, np.int32)
        prop[i] = prop_id - PROP_GEOM_ID0
        bounds = np.zeros((self.num_envs, 6))
        bounds[i, :3], bounds[i, 3:] = lo, hi
        pose, att = self._physics.prop_place(self.seed + 1, prop, bounds, self._place_counts * demo_logic.MAX_PLACE_ATTEMPTS,
                                             demo_logic.MAX_PLACE_ATTEMPTS, demo_logic.PLACE_CLEARANCE)
        if att[i] <= 0:
            raise Exception("Failed to find collision free place pose.")
        self._place_counts[i] += 1
        return pose[i]

    def sort_colours_env(self, i: int, info: Optional[dict] = None):
        """tasks/rearrangement.py:700-751 for env i."""
        info = info or self.props_info_env(i)
        task = self._cfg.task
        for prop_id, a in info.items():
            tl = task.target_locations[task.colour_target_map[a["labels"].colour]]
            lo = np.array([tl["location"][0] - tl["size"][0] / 2, tl["location"][1] - tl["size"][1] / 2, 0.4])
            hi = np.array([tl["location"][0] + tl["size"][0] / 2, tl["location"][1] + tl["size"][1] / 2, 0.4])
            x, y, _ = a["position"]
            if not (lo[0] <= x <= hi[0] and lo[1] <= y <= hi[1]):
                return True, self.prop_pick_env(i, prop_id, info), self.prop_place_env(i, prop_id, lo, hi, info)
        return False, None, None

    def sort_colours(self, peek: bool = False):
        """Batched sort_colours on the device (mre_sort_colours: selection, prop_pick and the
        prop_place rejection loop of tasks/rearrangement.py:700-751 run per env in one launch pair):
        (in_progress[N], pick_pose[N,7], place_pose[N,7]); envs with nothing left to do (or whose place
        sampling failed, recorded in ``failed_phase``) get their home pose as a no-op target."""
        if self._zones is None:
            lo, hi = demo_logic.target_bounds(self._cfg.task, self.prop_colours, 4)
            self._zones = np.concatenate([lo[..., :2], hi[..., :2]], axis=2)
        which, pick, place, att = self._physics.sort_colours(self.seed, self._place_counts, self._zones,
                                                             demo_logic.MAX_PLACE_ATTEMPTS, demo_logic.PLACE_CLEARANCE)
        prog = (which >= 0) & (att > 0) & ~self.placement_failed
        failed = (which >= 0) & (att < 0) & ~self.placement_failed
        if not peek:   # (peek: only asks which envs still have a cube to move; consumes no place draws)
            self._place_counts[prog] += 1
            self.failed_phase[failed] = "Failed to find collision free place pose."
        idle = ~prog
        home = np.atleast_2d(self.eef_home_pose)
        pick[idle, :3] = place[idle, :3] = home[idle] if len(home) == self.num_envs else home[0]
        pick[idle, 3:] = place[idle, 3:] = home_quat()
        return prog, pick, place

    def random_pick_and_place(self):
        """tasks/rearrangement.py:667-698 (always the first prop), batched."""
        poses = self._physics.sites()[2]
        ws = self._cfg.task.initializers.workspace
        pick = np.zeros((self.num_envs, 7))
        place = np.zeros((self.num_envs, 7))
        u = rng.uniform(self.seed + 2, self.env_ids, [self._place_count], 3)[0]
        self._place_count += 1
        for i in range(self.num_envs):
            info = self.props_info_env(i, poses)
            first = list(info.keys())[0]
            m = R.from_quat(info[first]["orientation"]).as_matrix()
            rz = np.rad2deg(np.arctan2(m[1, 0], m[0, 0]))
            grasp = mat2quat(R.from_euler("xyz", [0, 180, rz], degrees=True).as_matrix())
            pick[i] = np.concatenate([info[first]["position"], grasp])
            place[i] = np.concatenate([np.asarray(ws.min_pose) + (np.asarray(ws.max_pose) - np.asarray(ws.min_pose)) * u[i], grasp])
        return pick, place


class RearrangementEnv(BatchedRearrangementEnv):
    """Batch of one with the reference's shapes and error behaviour
    (signature: tasks/rearrangement.py:54-58)."""

    def __init__(self, viewer=None, cfg: Optional[Cfg] = None, device: int = 0, render: bool = True,
                 solver: str = "Newton"):
        super().__init__(cfg=cfg, num_envs=1, viewer=viewer, device=device, render=render, solver=solver)

    def _compute_observation(self):
        o = super()._compute_observation()
        return {k: (v[0].cpu().numpy() if hasattr(v, "cpu") else v[0]) for k, v in o.items()}

    def _phase(self, name, duration):
        conv = super()._phase(name, duration)
        if not conv[0]:  # tasks/rearrangement.py:371-399,413-440
            raise RuntimeError(name)
        return conv

    @property
    def props_info(self) -> dict:
        return self.props_info_env(0)

    def prop_pick(self, prop_id):
        return self.prop_pick_env(0, prop_id)

    def prop_place(self, prop_id, min_pose=None, max_pose=None):
        return self.prop_place_env(0, prop_id, min_pose, max_pose)

    def sort_colours(self):
        return self.sort_colours_env(0)

    def random_pick_and_place(self):
        a, b = super().random_pick_and_place()
        return a[0], b[0]

    def reset(self):
        ts = super().reset()
        self.eef_home_pose = self.eef_home_pose[0]
        return ts

    def pick(self, pose):
        self.eef_home_pose = np.atleast_2d(self.eef_home_pose)
        try:
            super().pick(pose)
        finally:
            self.eef_home_pose = self.eef_home_pose[0]

    def place(self, pose):
        self.eef_home_pose = np.atleast_2d(self.eef_home_pose)
        try:
            super().place(pose)
        finally:
            self.eef_home_pose = self.eef_home_pose[0]
