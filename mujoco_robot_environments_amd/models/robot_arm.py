"""RobotArm: mirror of the reference's ``models/robot_arm.py`` over a batch of envs.

``run_controller(duration)`` is THE hot loop (reference models/robot_arm.py:61-94): per
5 ms control tick one OSC torque + one gripper command, then ``control_steps`` physics
steps.  Here the whole call is ONE kernel launch (mre_run_controller); the number of ticks
replicates the reference's ``while physics.data.time - start_time < duration`` test on an
fp64 clock advanced by the timestep once per physics step, and -- as in the reference,
where ``gripper_converged`` can never become True with a gripper attached (:65,86-88) --
the loop always runs the full duration.

``torque_law``: a callable ``law(terms, target) -> tau [N, 7]`` (controllers/torch_osc.py) that replaces the in-kernel
law.  ``run_controller`` then runs the reference's loop tick by tick on the device: the arm's Jacobian, mass matrix and
bias force are exported (``BatchedPhysics.arm_dynamics``), the law and the MinMax command make the control, which is
held for ``control_steps`` physics steps, and convergence is tested on the new state and latched -- one export per
tick, which serves the test of tick t and the law of tick t + 1.  It returns the flags as the in-kernel path does, with
one difference: the status bit MRE_ST_NOT_CONVERGED (1) is the in-kernel loop's and is NOT set here."""
from __future__ import annotations

import numpy as np

from ..controllers import OSC, MinMax


class RobotArm:
    def __init__(self, physics, controller_params=None, gripper_cfg=None, gripper: bool = True, strict: bool = True,
                 torque_law=None):
        self.physics = physics
        self.torque_law = torque_law
        self.arm_controller = OSC(physics, controller_config=controller_params)
        self.end_effector = "robotiq_2f85" if gripper else None
        mm = dict(min_val=0.0, max_val=255.0)
        if gripper_cfg is not None:
            mm = dict(min_val=float(gripper_cfg.get("min_val", 0.0)), max_val=float(gripper_cfg.get("max_val", 255.0)))
        self.end_effector_controller = MinMax(num_envs=physics.num_envs, physics=physics, **mm)
        control_dt = 0.005 if controller_params is None else float(controller_params["control_dt"])
        self.timestep = physics.timestep
        # robot_arm.py:53
        self.control_steps = int(control_dt // self.timestep)
        if self.control_steps < 1 and strict:
            raise ValueError("control_dt < physics_dt gives control_steps = 0: the reference's "
                             "run_controller would never advance time (SURVEY.md App. D.9)")
        self.time = 0.0  # physics.data.time (fp64, += timestep per step)

    @property
    def eef_pose(self):
        """site_xpos of the gripper pinch site (robot_arm.py:55-58)."""
        tcp, _, _ = self.physics.sites()
        return tcp[0].astype(np.float64) if self.physics.num_envs == 1 else tcp.astype(np.float64)

    def ticks_for(self, duration: float) -> int:
        t, start, ticks = self.time, self.time, 0
        while t - start < duration:
            for _ in range(self.control_steps):
                t += self.timestep
            ticks += 1
        return ticks

    def run_controller(self, duration: float):
        if self.control_steps < 1:  # LasaDrawEnv's config (physics_dt 0.01 > control_dt 0.005): the reference spins forever
            raise ValueError("control_steps = 0: run_controller would never advance time (SURVEY.md App. D.9)")
        ticks = self.ticks_for(duration)
        if self.torque_law is None:
            conv = self.physics.run_controller(ticks, self.control_steps)
        else:
            conv = self._run_torque_law(ticks)
        for _ in range(ticks * self.control_steps):
            self.time += self.timestep
        return bool(conv[0]) if self.physics.num_envs == 1 else conv

    def _run_torque_law(self, ticks: int) -> np.ndarray:
        """models/robot_arm.py:69-88 with ``torque_law`` in the place of OSC.compute_control_output()."""
        import torch
        from ..controllers.torch_osc import TorchOSC, target_tensors
        phys, law = self.physics, self.torque_law
        test = law if hasattr(law, "converged") else TorchOSC.from_osc(self.arm_controller)
        target = target_tensors(self.arm_controller, phys.device)
        grip = np.broadcast_to(np.asarray(self.end_effector_controller.compute_control_output(), np.float32), (phys.num_envs,))
        grip = torch.from_numpy(grip.copy()).to(phys.device)[:, None]
        conv = torch.zeros(phys.num_envs, dtype=torch.bool, device=phys.device)
        terms = phys.arm_dynamics("eef")
        for _ in range(ticks):
            tau = law(terms, target)
            phys.set_control(torch.cat([tau.to(torch.float32), grip], dim=1))
            phys.step(self.control_steps)
            terms = phys.arm_dynamics("eef")
            conv |= test.converged(terms, target)
        return conv.cpu().numpy()
