"""What the four task envs share -- ``RearrangementEnv`` (tasks/rearrangement.py) and, through tasks/_arm_task.py, ``BaseEnv``,
``PushEnv`` and ``LasaDrawEnv``: the compiled scene and its ``BatchedPhysics``, the camera table of the config, the named
camera of the observations, the one render call, the observation and its specs, the ``RobotArm`` of a reset and the mocap
tick of ``interactive_tuning``.  Everything carries a leading env axis; the batch-of-one classes take it off.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
from scipy.spatial.transform import Rotation as R

from ..model import compile as _compile
from ..models.robot_arm import RobotArm
from ..physics import BatchedPhysics
from . import _camera
from ._timestep import _Array


def mat2quat(mat3x3) -> np.ndarray:
    """mujoco.mju_mat2Quat: (w, x, y, z)."""
    return _compile.m2q(np.asarray(mat3x3, np.float64).reshape(3, 3))


def home_quat() -> np.ndarray:
    """mju_mat2Quat(R.from_euler('xyz',[0,180,0])) (tasks/rearrangement.py:391-393)."""
    return mat2quat(R.from_euler("xyz", [0, 180, 0], degrees=True).as_matrix())


def _actuator_cfg(ac) -> Dict:
    """robots.arm.actuator_config (motor.yaml | position.yaml) -> the scene builder's actuator arguments."""
    if ac.type == "motor":
        lim = [float(ac[ac.joint_actuator_mapping[f"joint{i + 1}"]].ctrlrange.split()[1]) for i in range(7)]
        return dict(actuator="motor", motor_ctrlrange=lim)
    rows = []
    for i in range(7):
        j = ac[ac.joint_actuator_mapping[f"joint{i + 1}"]]
        cr = tuple(float(x) for x in str(j.ctrlrange).split())
        fr = tuple(float(x) for x in str(j.forcerange).split())
        bias = tuple(float(x) for x in str(j.biasprm).split())
        rows.append((cr, fr[1], float(j.gainprm), -bias[2]))
        assert bias[0] == 0.0 and bias[1] == -float(j.gainprm), "position actuator: biasprm = 0 -kp -kv"
    return dict(actuator="position", position_actuators=rows)


class BatchedEnv:
    """num_envs instances of one scene, stepped in lockstep on one GPU."""

    CAMERA = "overhead_camera"   # the camera of the observations, by its name in cfg.arena.cameras

    def __init__(self, cfg, scene: dict, num_envs: int, device: int, render: bool, mocap_pos, mocap_quat):
        self._cfg = cfg
        self.num_envs = int(num_envs)
        self.has_viewer = False  # no viewer on a headless GPU batch (tasks/rearrangement.py:64-70)
        self._model = _compile.compile_scene(scene)
        self._physics = BatchedPhysics(self.num_envs, model=self._model, device=device)
        # cameras (config/arena/cameras/*.yaml): only the pose / fovy / size constants are needed
        self._cameras = {f"{c.name}/{c.name}": _camera.camera(c.pos, c.quat, c.fovy, c.height, c.width) for c in cfg.arena.cameras}
        self._camera_key = f"{self.CAMERA}/{self.CAMERA}"
        if self._camera_key not in self._cameras:
            raise ValueError(f"config has no camera named {self.CAMERA}")
        self.camera_height, self.camera_width = (self._cameras[self._camera_key][k] for k in ("height", "width"))
        self.render_observations = bool(render)
        # pose of the reference's mocap target body (simulation_tuning_mode), one per env: state the caller may move
        self.mocap_pos = np.tile(np.asarray(mocap_pos, np.float64), (self.num_envs, 1))
        self.mocap_quat = np.tile(np.asarray(mocap_quat, np.float64), (self.num_envs, 1))
        self._robot: Optional[RobotArm] = None
        self._eef_home = None   # [N, 3] from reset()

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

    @property
    def eef_home_pose(self):
        """Where the end effector stood after the last ``reset()``, [N, 3] (None before the first)."""
        return self._eef_home

    # ------------------------------------------------------- images and specs
    def _render(self, cam: dict, height: int, width: int, **kw):
        """Every image of the envs: ``BatchedPhysics.render`` through ``cam`` (an entry of ``_cameras``) at height x width."""
        return self._physics.render(cam["pos"], cam["mat"], cam["fovy"], height, width, **kw)

    def _compute_observation(self):
        h, w, n = self.camera_height, self.camera_width, self.num_envs
        if self.render_observations:
            rgb, depth, _ = self.render(seg=False)
        else:  # (render stubbed: zero images of the reference's shapes)
            rgb = np.broadcast_to(np.zeros((1, 1, 1, 1), np.uint8), (n, h, w, 3))
            depth = np.broadcast_to(np.zeros((1, 1, 1), np.float32), (n, h, w))
        return {f"{self.CAMERA}/rgb": rgb, f"{self.CAMERA}/depth": depth}

    def observation_spec(self):
        h, w = self.camera_height, self.camera_width
        return {f"{self.CAMERA}/depth": _Array(shape=(h, w), dtype=np.float32),
                f"{self.CAMERA}/rgb": _Array(shape=(h, w, 3), dtype=np.float32)}  # (sic: :448; images are uint8)

    def action_spec(self) -> Dict[str, _Array]:
        return {"pose": _Array(shape=(7,), dtype=np.float64),
                "pixel_coords": _Array(shape=(2,), dtype=np.int64),
                "gripper_rot": _Array(shape=(1,), dtype=np.float64)}

    # ------------------------------------------------------ robot and ticks
    def _new_robot(self, **kw) -> RobotArm:
        """The RobotArm of a reset, on the controller and gripper settings of the config."""
        cp = self._cfg.robots.arm.controller_config.controller_params
        mm = self._cfg.robots.end_effector.controller_config.controller
        self._robot = RobotArm(self._physics, controller_params=cp, gripper_cfg=mm, **kw)
        return self._robot

    def _advance_clock(self, steps: int) -> None:
        for _ in range(steps):   # (one addition per physics step, as RobotArm's own loop counts them)
            self._robot.time += self._robot.timestep

    def _osc_tick(self, position, quat, velocity, steps: int) -> None:
        """One control tick of the fused launch: compute_control_output() once on the OSC target given, then
        ``steps`` x (set_control, step)."""
        self._robot.arm_controller.set_target(position=position, quat=quat, velocity=velocity,
                                              angular_velocity=np.zeros(3))
        self._physics.run_controller(1, steps)
        self._advance_clock(steps)

    def _mocap_tick(self, mocap_pos, mocap_quat, z_offset: float, steps: int) -> None:
        """One tick of the reference's tuning loop (tasks/rearrangement.py:753-779): the OSC target follows the mocap body
        (its position + [0, 0, z_offset], its quaternion, zero velocities) and the command is held for ``steps`` physics
        steps.  There is no viewer to drag a mocap body here, so the caller moves it, per env, through the arguments."""
        if mocap_pos is not None:
            self.mocap_pos[:] = np.asarray(mocap_pos, np.float64)
        if mocap_quat is not None:
            self.mocap_quat[:] = np.asarray(mocap_quat, np.float64)
        self._osc_tick(self.mocap_pos + np.array([0.0, 0.0, z_offset]), self.mocap_quat, np.zeros(3), steps)
