"""Shared body of the reference's three small environments -- ``BaseEnv`` (tasks/base.py), ``PushEnv``
(tasks/push.py) and ``LasaDrawEnv`` (tasks/lasa_draw.py) -- batched over ``num_envs`` and run on the SAME
step kernels as ``RearrangementEnv``.

Their hot path is the same five-substep pattern (tasks/base.py:228-254, tasks/push.py:339-363,
tasks/lasa_draw.py:300-370): one OSC torque (or one joint-position command) held for five
``physics.step()`` calls.  ``step()`` itself only renders, as in the reference.

The kernels are compiled for one body topology (arm + 2F-85 + four cube slots).  A task without a gripper
(push, lasa) is embedded in it: ``model/spec.py:other_task_scene`` hangs an INERT copy of the gripper
(no mass, no geoms, no springs) below the attachment body, so the arm rows of the mass matrix, the bias
forces and every contact are those of the arm-only model; ``tests/test_other_tasks.py`` checks in the fp64
oracle that the embedded model and the task's own body tree give the same arm and block trajectories.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
from scipy.spatial.transform import Rotation as R

from ..config import Cfg
from ..model import spec as _spec
from ._env import BatchedEnv, _actuator_cfg  # noqa: F401  (_actuator_cfg: imported from here by the tests)
from ._timestep import StepType, TimeStep


class BatchedArmTaskEnv(BatchedEnv):
    """num_envs independent instances of one of the small tasks, stepped in lockstep on one GPU."""

    TASK = "base"
    CAMERA = "overhead_camera"
    MOCAP_POS = (0.4, 0.0, 0.2)
    TARGET_OFFSET = 0.175
    HAS_GRIPPER = True
    TICK_STEPS = 5   # physics steps one command is held for (tasks/base.py:228-254 and its copies), whatever the config says

    def __init__(self, cfg: Cfg, num_envs: int = 1, viewer=None, device: int = 0, render: bool = False,
                 solver: str = "Newton", scene_cfg: Optional[dict] = None):
        sc = dict(physics_dt=cfg.physics_dt, gravity=cfg.gravity, solver=solver,
                  home=cfg.robots.arm.default_configurations.home)
        sc.update(_actuator_cfg(cfg.robots.arm.actuator_config))
        sc.update(scene_cfg or {})
        self.position_actuators = sc["actuator"] == "position"
        self._scene = _spec.other_task_scene(self.TASK, sc)
        # the reference's mocap target body; R.as_quat() is (x, y, z, w) and is handed to MuJoCo's
        # (w, x, y, z) unconverted there: reproduced
        mq = R.from_euler("xyz", [180, 180, 0], degrees=True).as_quat()
        super().__init__(cfg, self._scene, num_envs, device, render, mocap_pos=self.MOCAP_POS, mocap_quat=mq / np.linalg.norm(mq))
        self.nprops = np.full(self.num_envs, 1 if self.TASK == "push" else 0, np.int32)
        self.prop_half_size = np.full((self.num_envs, 4, 3), 0.025 if self.TASK == "push" else 0.0155)
        self._physics.set_props(self.nprops, self.prop_half_size)
        names = self._model["_names"]["geoms"]
        geom_rgb = np.full((len(names), 3), 0.25, np.float32)
        for g, n in enumerate(names):
            if n.startswith("table"):
                geom_rgb[g] = 1.0      # tasks/push.py:90, tasks/lasa_draw.py:93: white tables
            if n == "tool_cylinder":
                geom_rgb[g] = (0.02, 0.302, 0.4)
        if self.TASK == "push":      # green -> red gradient of the eight slabs (tasks/push.py:103-116)
            for k in range(8):
                t = k / 7.0
                geom_rgb[names.index(f"table_{k + 1}")] = (t, 1.0 - t, 0.0)
        prop_rgb = np.full((self.num_envs, 4, 3), 128, np.uint8)   # push block: rgba 0.5 0.5 0.5
        self._physics.set_render_colours(prop_rgb, geom_rgb)

    # ---------------------------------------------------------------- images
    def render(self, rgb: bool = True, depth: bool = True, seg: bool = False, camera: Optional[str] = None):
        """Images of every env through a named camera (default: the one of the observations) at its own size."""
        cam = self._cameras[camera or self._camera_key]
        return self._render(cam, cam["height"], cam["width"], rgb=rgb, depth=depth, seg=seg)

    # ----------------------------------------------------------------- reset
    def _initial_qpos(self, qpos: np.ndarray) -> None:
        """Task-specific initial state written into qpos [N, 43] (arm already at home)."""

    def reset(self, arm_configuration=None) -> TimeStep:
        """physics.reset(), arm to the home (or given) configuration, a new RobotArm
        (tasks/base.py:150-190, tasks/push.py:241-283, tasks/lasa_draw.py:207-244)."""
        self._physics.reset()
        qpos, qvel = self._physics.get_state()
        qpos, qvel = qpos.copy(), qvel.copy()
        if arm_configuration is not None:
            qpos[:, :7] = np.asarray(arm_configuration, np.float32)
        self._initial_qpos(qpos)
        self._physics.set_state(qpos, qvel)
        self._new_robot(gripper=self.HAS_GRIPPER, strict=False)
        self._eef_home = np.atleast_2d(self._robot.eef_pose).copy()
        return TimeStep(step_type=StepType.FIRST, reward=0.0, discount=0.0, observation=self._compute_observation())

    def step(self, action_dict=None) -> TimeStep:
        """tasks/base.py:192-203 and its copies: the observation, nothing else."""
        return TimeStep(step_type=StepType.MID, reward=0.0, discount=0.0, observation=self._compute_observation())

    # ------------------------------------------------------------- hot path
    def interactive_tuning(self, mocap_pos=None, mocap_quat=None) -> None:
        """One pass of the tuning loop: the OSC target follows the mocap body (+ TARGET_OFFSET in z), the
        command is computed once and held for five physics steps."""
        if self.position_actuators:
            raise RuntimeError("interactive_tuning drives motors through the OSC torque law; "
                               "this env was built with position actuators")
        self._mocap_tick(mocap_pos, mocap_quat, self.TARGET_OFFSET, self.TICK_STEPS)
