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
from typing import Optional

import numpy as np
import torch
from scipy.spatial.transform import Rotation as R

from .. import demo_logic, perception, rng
from ..config import Cfg, colour_separator_task_config, default_config  # noqa: F401
from ..model import compile as _compile
from ..model import spec as _spec
from . import _camera
from ._camera import TABLE_TOP_Z  # noqa: F401
from ._env import BatchedEnv, _actuator_cfg, home_quat, mat2quat
from ._timestep import StepType, TimeStep, _Array  # noqa: F401
from ._transporter import (HEIGHTMAP_BOUNDS, OVERHEAD, PICK_HEIGHT, PickDecision, PlaceDecision,  # noqa: F401
                           TransporterMixin, quat_mul, transporter_poses)

DEFAULT_CONFIG = default_config()
PRE_PICK_HEIGHT = 0.9   # tasks/rearrangement.py:364,408
PROP_GEOM_ID0 = 12      # geom ids of prop_0..3 in the compiled scene

PropsLabels = collections.namedtuple("PropsLabels", ["shape", "colour", "texture"])
# environment/props.py:13-20
COLOURS = {"red": (1.0, 0.0, 0.0), "green": (0.0, 1.0, 0.0), "blue": (0.0, 0.0, 1.0),
           "yellow": (1.0, 1.0, 0.0), "cyan": (0.0, 1.0, 1.0), "magenta": (1.0, 0.0, 1.0)}
COLOUR_NOISE = 0.1      # environment/props.py:274,290
# the five phases of a scripted pick and of a scripted place: what ``failed_phase`` (and the RuntimeError of a batch of one)
# says when the arm has not converged by the end of the phase
PICK_PHASES = ("Failed to move arm to pre pick position", "Failed to move arm to pick position", "Failed to close gripper",
               "Failed to move arm to pre grasp position", "Failed to move arm to home position")
PLACE_PHASES = ("Failed to move arm to pre place position", "Failed to move arm to place position", "Failed to open gripper",
                "Failed to move arm to pre place position", "Failed to move arm to home position")


class BatchedRearrangementEnv(TransporterMixin, BatchedEnv):
    """num_envs independent RearrangementEnv instances stepped in lockstep on one GPU."""

    def __init__(self, cfg: Optional[Cfg] = None, num_envs: int = 1, viewer=None, device: int = 0,
                 seed: Optional[int] = None, env_id_offset: int = 0, env_ids=None, render: bool = False,
                 solver: str = "Newton", torque_law=None):
        cfg = cfg if cfg is not None else DEFAULT_CONFIG
        scene = _spec.default_scene(dict(physics_dt=cfg.physics_dt, gravity=cfg.gravity, solver=solver,
                                         motor_ctrlrange=_actuator_cfg(cfg.robots.arm.actuator_config)["motor_ctrlrange"],
                                         home=cfg.robots.arm.default_configurations.home))
        # (the mocap body of the reference's tuning mode starts at (0.4, 0, 0.6), gripper down: tasks/rearrangement.py:130-140)
        super().__init__(cfg, scene, num_envs, device, render, mocap_pos=[0.4, 0.0, 0.6], mocap_quat=home_quat())
        self.torque_law = torque_law   # law(terms, target) -> tau run in place of the in-kernel OSC (models/robot_arm.py)
        # global env ids key every random draw; explicit ids may repeat (envs sharing a scene)
        self.env_ids = (np.arange(env_id_offset, env_id_offset + self.num_envs) if env_ids is None
                        else np.asarray(env_ids, np.int64).reshape(self.num_envs))
        self._explicit_ids = env_ids is not None
        self.seed = int(cfg.task.initializers.seed if seed is None else seed)
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
        # ---- overhead camera images (mre_render): cube albedo = colour + noise (props.py:288-291),
        # table grey (tasks/rearrangement.py:91), robot hulls dark
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
        self.mode = None
        self.last_converged = np.ones(self.num_envs, bool)
        self.placement_failed = np.zeros(self.num_envs, bool)   # reset(): PropPlacer found no pose for a cube
        self.not_settled = np.zeros(self.num_envs, bool)
        self.failed_phase = np.full(self.num_envs, "", dtype=object)

    # ---------------------------------------------------------------- images
    @property
    def overhead_camera_height(self) -> int:
        return self.camera_height

    @property
    def overhead_camera_width(self) -> int:
        return self.camera_width

    def render(self, rgb: bool = True, depth: bool = True, seg: bool = True, camera: str = OVERHEAD):
        """Overhead camera images of every env's current state as CUDA tensors (rgb uint8 [N,H,W,3],
        depth float32 [N,H,W], seg uint8 [N,H,W]: 12 + p = cube p, 1 table, 2..11 and 16..19 robot, 255 nothing):
        the batched form of the reference's renderer / depth_renderer / seg_renderer passes
        (tasks/rearrangement.py:254-280, 460-478)."""
        return self._render(self._cameras[camera], self.camera_height, self.camera_width, rgb=rgb, depth=depth, seg=seg)

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
        self._cameras[key] = _camera.camera(pos, quat, fovy, height, width)
        return key

    def render_views(self, cameras, rgb: bool = True, depth: bool = True, seg: bool = True):
        """``render`` through each of the named ``cameras`` at that camera's own configured size: a list of
        (rgb, depth, seg), one per camera in the order given.  (``render`` itself renders every camera at the overhead
        camera's size.)"""
        views = [self._cameras[name] for name in cameras]
        return [self._render(cam, cam["height"], cam["width"], rgb=rgb, depth=depth, seg=seg) for cam in views]

    def prop_bboxes(self, seg=None) -> np.ndarray:
        """PASCAL-VOC boxes [N, 4 cubes, (xmin, ymin, xmax, ymax)] of the VISIBLE pixels of every cube
        in the segmentation image (get_bbox, tasks/rearrangement.py:254-268); -1 where a cube is not
        in view or not in use.  One pass over the image on the device (perception.seg_labels) for a CUDA
        ``seg`` or the env's own render; ``self`` is not touched when ``seg`` is given."""
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
        if seg is None:
            _, d, seg = self.render(rgb=False, depth=depth is None)
            depth = d if depth is None else depth
        seg = torch.as_tensor(seg)
        lab = perception.seg_labels(seg, None if depth is None else torch.as_tensor(depth).to(seg.device), PROP_GEOM_ID0, 4)
        return {"bbox": lab.box.contiguous().cpu().numpy(), "visible_pixels": lab.count.contiguous().cpu().numpy(),
                "centroid": perception.centroid(lab).cpu().numpy(),
                "nearest_depth": None if lab.zmin is None else lab.zmin.cpu().numpy()}

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
        self._new_robot(torque_law=self.torque_law).time = steps * self._physics.timestep
        self._eef_home = np.atleast_2d(self._robot.eef_pose).copy()
        self._eef_home[:, 0] -= 0.1  # reference shifts x although the comment says "up" (App. D.5)
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
        are computed once and held for the robot's ``control_steps`` (5) physics steps.  The mocap pose is state of the env
        (``mocap_pos`` [N, 3] / ``mocap_quat`` [N, 4]) that the caller may move, per env, through the arguments."""
        self._mocap_tick(mocap_pos, mocap_quat, 0.175, self._robot.control_steps)

    def time_limit_exceeded(self) -> bool:
        """tasks/rearrangement.py:216-217 (the reference reads a module-level ``cfg.time_limit`` that its config
        tree does not define; absent means no limit)."""
        return self._robot.time >= float(self._cfg.get("time_limit", float("inf")))

    def _pose2d(self, pose):
        pose = np.asarray(pose)
        return pose.reshape(self.num_envs, 7) if pose.ndim == 1 else pose

    def _scripted(self, pose, gripper: str, phases, **approach):
        """The five-phase macro that ``pick`` and ``place`` are (tasks/rearrangement.py:358-440): above the pose 2 s, down
        to it 2 s, the gripper to ``gripper`` 1 s, back up 2 s, home 2 s.  ``phases`` names what ``failed_phase`` says for
        each, ``approach`` is what the first target sets beside position and orientation."""
        pose[..., 2] = PICK_HEIGHT  # in-place, like the reference
        p = self._pose2d(pose).astype(np.float64)
        pre = p.copy()
        pre[:, 2] = PRE_PICK_HEIGHT
        c = self._robot.arm_controller
        c.set_target(position=pre[:, :3], quat=pre[:, 3:], **approach)
        self._phase(phases[0], 2.0)
        c.set_target(position=p[:, :3])
        self._phase(phases[1], 2.0)
        self._robot.end_effector_controller.status = gripper
        self._phase(phases[2], 1.0)
        c.set_target(position=pre[:, :3])
        self._phase(phases[3], 2.0)
        c.set_target(position=self._eef_home, quat=home_quat())
        self._phase(phases[4], 2.0)

    def pick(self, pose):
        """Scripted pick (tasks/rearrangement.py:358-399): pre-pick 2 s, descend 2 s,
        close 1 s, lift 2 s, home 2 s."""
        self._scripted(pose, "max", PICK_PHASES, velocity=np.zeros(3), angular_velocity=np.zeros(3))

    def place(self, pose):
        """Scripted place (tasks/rearrangement.py:401-440)."""
        self._scripted(pose, "min", PLACE_PHASES)

    # ---------------------------------------------------------------- camera
    def _get_camera_intrinsics(self, camera_name, h, w, inverse=False):
        # (the focal length is the overhead camera's, whatever h: kept)
        return _camera.intrinsics(self._cameras[camera_name], self.overhead_camera_height, h, w)

    def _get_camera_extrinsics(self, camera_name):
        return _camera.extrinsics(self._cameras[camera_name])

    def _camera_matrices(self, camera_name):
        return (self._get_camera_intrinsics(camera_name, self.overhead_camera_height, self.overhead_camera_width),
                self._get_camera_extrinsics(camera_name))

    def world_2_pixel(self, camera_name, coords):
        """tasks/rearrangement.py:533-548 (coords [3] or [N,3])."""
        return _camera.world_2_pixel(*self._camera_matrices(camera_name), coords)

    def pixel_2_world(self, camera_name, coords, env: int = 0):
        """tasks/rearrangement.py:505-531: the pixel's rendered depth pushed back through the pinhole
        model (env selects the image of a batch).  Without rendering the depth is that of the table
        plane: the pixel ray intersected with z = table top."""
        K, E = self._camera_matrices(camera_name)
        coords = np.asarray(coords, np.float64)
        rays = _camera.pixel_rays(K, coords)
        cam = self._cameras[camera_name]
        if self.render_observations:
            rc = np.round(coords).astype(np.int32)  # coords_rounded (:509)
            mask = np.zeros(self.num_envs, np.uint8)
            mask[env] = 1
            _, dimg, _ = self._render(cam, self.overhead_camera_height, self.overhead_camera_width, rgb=False, seg=False,
                                      mask=mask)
            depth = float(dimg[env, rc[1], rc[0]])
        else:
            depth = _camera.plane_depth(cam, rays)
        return _camera.unproject(E, rays, depth)

    def pixel_2_world_batch(self, camera_name, coords, depth=None) -> np.ndarray:
        """pixel_2_world for one pixel per env: coords [N, 2] (x, y) -> world points [N, 3] float64, row i equal to
        ``pixel_2_world(camera_name, coords[i], env=i)``.  With rendering on, the depths are one gather from ``depth``
        [N, H, W] (the caller's, e.g. the observation's, or one render of the batch); without, the table-plane ray.
        A pixel outside the image raises ValueError."""
        h, w = self.overhead_camera_height, self.overhead_camera_width
        K, E = self._camera_matrices(camera_name)
        coords = np.asarray(coords, np.float64)
        if coords.shape != (self.num_envs, 2):
            raise ValueError(f"coords must be [{self.num_envs}, 2]")
        rc = np.round(coords).astype(np.int64)  # coords_rounded (:509)
        if (rc < 0).any() or (rc[:, 0] >= w).any() or (rc[:, 1] >= h).any():
            raise ValueError(f"pixel outside the {w} x {h} image")
        rays = _camera.pixel_rays(K, coords)
        cam = self._cameras[camera_name]
        if self.render_observations:
            if depth is None:
                depth = self._render(cam, h, w, rgb=False, seg=False)[1]
            if tuple(depth.shape) != (self.num_envs, h, w):
                raise ValueError(f"depth must be [{self.num_envs}, {h}, {w}]")
            if hasattr(depth, "cpu"):
                env = torch.arange(self.num_envs, device=depth.device)
                d = depth[env, torch.as_tensor(rc[:, 1], device=depth.device), torch.as_tensor(rc[:, 0], device=depth.device)]
                d = d.cpu().numpy().astype(np.float64)
            else:
                d = np.asarray(depth)[np.arange(self.num_envs), rc[:, 1], rc[:, 0]].astype(np.float64)
        else:
            d = _camera.plane_depth(cam, rays)
        return _camera.unproject(E, rays, d)

    def get_camera_params(self, camera_name):
        K, E = self._camera_matrices(camera_name)
        return {"intrinsics": K, "extrinsics": E}

    def get_camera_metadata(self):
        return _camera.metadata(*self._camera_matrices(OVERHEAD))

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
            if bboxes is not None:
                bbox = bboxes[i, p] if bboxes[i, p, 0] >= 0 else np.array([])
            else:
                bbox = _camera.corner_box(*self._camera_matrices(OVERHEAD), pos, mat, self.prop_half_size[i, p])
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
            K, E = self._camera_matrices(OVERHEAD)
            for i, p in zip(*np.nonzero(in_use)):
                bbox[i, p] = _camera.corner_box(K, E, position[i, p], mat[4 * i + p], self.prop_half_size[i, p])
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
        pick[idle, :3] = place[idle, :3] = self._eef_home[idle]
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

    @property
    def eef_home_pose(self):
        """[3], as the reference has it (the batch keeps [1, 3])."""
        return None if self._eef_home is None else self._eef_home[0]
