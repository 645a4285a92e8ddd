#!/usr/bin/env python3
"""Candidate torque LAWS for the absent ``mujoco_controllers.osc.OSC`` (VERDICT "next round" item 6):
the scripted ``pick()`` of the data-generation loop at osc.yaml's own gains, once per law, each law a few lines of torch
over the arm's exported Jacobian / mass matrix / bias force (``BatchedPhysics.arm_dynamics``, controllers/torch_osc.py)
run through ``BatchedRearrangementEnv(torque_law=...)``.  Reported per law: "held after home" -- the envs whose picked
cube is still in the gripper when the arm is back at its home pose -- and the phases that converged; beside it the cost
of the loop: ms per control tick of the torch loop against the in-kernel one (mre_run_controller).

    python examples/controller_laws.py --envs 64
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mujoco_robot_environments_amd.controllers.torch_osc import TorchOSC  # noqa: E402
from mujoco_robot_environments_amd.tasks.rearrangement import BatchedRearrangementEnv, colour_separator_task_config  # noqa: E402

GAINS = [350.0, 20.0, 500.0, 100.0, 200.0, 30.0]   # osc.yaml:5-15: kp, kd of position / orientation / nullspace


class JointSpaceDamping(TorchOSC):
    """The task force is the P-term alone; damping acts on the joints, through the mass matrix: - M (kd_p qd)."""
    def __call__(self, terms, target):
        t = self._target(terms, target)
        ep, eo = self.errors(terms, t)
        F = torch.cat([self._gain(0, terms) * ep, self._gain(2, terms) * eo], dim=1)
        qd = terms.qvel.to(self.dtype)
        damp = (terms.mass.to(self.dtype) @ (self._gain(1, terms) * qd)[:, :, None])[:, :, 0]
        return self.project(terms, F, self.nullspace_torque(terms)) - damp


class DampingOutsideLambda(TorchOSC):
    """The D-term is a task-space force that is NOT multiplied by the task inertia: J' (L F_p + F_d)."""
    def __call__(self, terms, target):
        t = self._target(terms, target)
        ep, eo = self.errors(terms, t)
        Fp = torch.cat([self._gain(0, terms) * ep, self._gain(2, terms) * eo], dim=1)
        Fd = self.task_force(terms, t) - Fp
        Jt = terms.jac.to(self.dtype).transpose(1, 2)
        return self.project(terms, Fp, self.nullspace_torque(terms)) + (Jt @ Fd[:, :, None])[:, :, 0]


class DampingRatio(TorchOSC):
    """kd is a damping RATIO: the D-gain is 2 kd sqrt(kp) (position, orientation and nullspace alike)."""
    def _gain(self, k, terms):
        g = super()._gain(k, terms)
        return 2.0 * g * torch.sqrt(super()._gain(k - 1, terms)) if k % 2 else g


def laws():
    return [("in-kernel law (mre_run_controller)", None),
            ("the same law in torch (TorchOSC)", TorchOSC(gains=GAINS)),
            ("damping in joint space", JointSpaceDamping(gains=GAINS)),
            ("D-term not multiplied by Lambda", DampingOutsideLambda(gains=GAINS)),
            ("kd as a damping ratio", DampingRatio(gains=GAINS)),
            ("position gains 200 / 30", TorchOSC(gains=[200.0, 30.0] + GAINS[2:]))]


def run(law, n_envs, solver):
    """reset, sort_colours, pick(): (envs acting, held after home [N], converged phases per env [N], seconds, ticks)."""
    env = BatchedRearrangementEnv(cfg=colour_separator_task_config(), num_envs=n_envs, solver=solver, torque_law=law)
    env.reset()
    acting, pick_pose, _ = env.sort_colours()
    phys = env.physics
    nconv = np.zeros(n_envs, int)
    inner = env._phase

    def phase(name, duration):
        conv = inner(name, duration)
        nconv[:] += conv
        return conv
    env._phase = phase
    phys.sync()
    t0 = time.perf_counter()
    env.pick(pick_pose)
    phys.sync()
    seconds = time.perf_counter() - t0
    props = phys.sites()[2]
    held = (props[:, :, 2] > 0.5).any(axis=1)     # a cube above 0.5 m at the home pose: in the gripper
    ticks = sum(env._robot.ticks_for(d) for d in (2.0, 2.0, 1.0, 2.0, 2.0))
    bad = int(((phys.status() & 2) != 0).sum())
    env.close()
    return acting, held, nconv, seconds, ticks, bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--solver", default="Newton")
    args = ap.parse_args()
    print(f"scripted pick() on {args.envs} scenes, osc.yaml gains {GAINS}, solver {args.solver}")
    ref = None
    for name, law in laws():
        acting, held, nconv, seconds, ticks, bad = run(law, args.envs, args.solver)
        n = int(acting.sum())
        line = (f"{name:38s} held after home {int((held & acting).sum()):3d} / {n}   all 5 phases converged "
                f"{int(((nconv == 5) & acting).sum()):3d} / {n}   {1e3 * seconds / ticks:6.3f} ms per tick ({ticks} ticks)")
        if bad:
            line += f"   non-finite state in {bad} envs"
        if ref is None:
            ref = held
        elif isinstance(law, TorchOSC) and type(law) is TorchOSC and law.gains.tolist() == GAINS:
            line += f"   envs whose outcome differs from the in-kernel law's: {int((held != ref)[acting].sum())}"
        print(line, flush=True)


if __name__ == "__main__":
    main()
