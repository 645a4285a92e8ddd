#!/usr/bin/env python3
"""A Transporter policy acting in the batched env it would be trained on, from the render to the arm's motion:
BatchedRearrangementEnv.transporter_act -- heightmap, scene tensor, the attention network and the pick head
(perception.attend -> csrc/mre_attend.hip), rotated crops around the predicted pick cells
(perception.crop_matrices_device), the key and query networks and the place head (perception.correlate) -- then
step(pick pose) and step(place pose).  One shared random Conv2d stands in for each of the three networks.

    python examples/transporter_rollout.py --num-envs 64
Prints the decisions of the first --show envs and how many envs' controllers converged in both steps.  The networks are
random, so the decisions mean nothing; with trained weights the same lines evaluate a policy: reset -> transporter_act ->
step -> step.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mujoco_robot_environments_amd import perception  # noqa: E402
from mujoco_robot_environments_amd.tasks.rearrangement import (  # noqa: E402
    BatchedRearrangementEnv, colour_separator_task_config)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=64)
    ap.add_argument("--cell", type=float, default=0.0025, help="metres per cell of the maps")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--rotations", type=int, default=36)
    ap.add_argument("--crop", type=int, default=64)
    ap.add_argument("--features", type=int, default=3, help="channels of the key and query feature maps (1 .. 16)")
    ap.add_argument("--show", type=int, default=8, help="envs whose decisions are printed")
    args = ap.parse_args()
    env = BatchedRearrangementEnv(cfg=colour_separator_task_config(), num_envs=args.num_envs, render=True)
    env.reset()
    channels, dtype, dev = perception.CHANNELS_RGBH, torch.bfloat16, "cuda"
    torch.manual_seed(args.seed)
    conv = lambda out: torch.nn.Conv2d(len(channels.sources), out, 3, padding=1).to(device=dev, dtype=dtype)
    attention, key, query = conv(1), conv(args.features), conv(args.features)
    with torch.no_grad():
        pick_pose, place_pose, pick, place = env.transporter_act(
            attention, query, key, channels=channels, dtype=dtype, n_rotations=args.rotations, crop=args.crop, cell=args.cell)
    pc, qc = pick.cells.cpu().numpy(), place.cells.cpu().numpy()
    angle = np.rad2deg(place.angle.cpu().numpy())
    for i in range(min(args.show, env.num_envs)):
        print(f"env {i:4d}: pick row {pc[i, 1]:3d} column {pc[i, 0]:3d} -> x {pick_pose[i, 0]:.4f} y {pick_pose[i, 1]:.4f}; "
              f"place row {qc[i, 1]:3d} column {qc[i, 0]:3d} crop turned {angle[i]:5.1f} deg -> x {place_pose[i, 0]:.4f} "
              f"y {place_pose[i, 1]:.4f} quat {np.round(place_pose[i, 3:], 3).tolist()}")
    env.step({"pose": pick_pose})
    env.step({"pose": place_pose})
    print(f"{int(env.last_converged.sum())} of {env.num_envs} envs converged in every phase of the pick and the place")
    env.close()


if __name__ == "__main__":
    main()
