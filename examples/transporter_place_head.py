#!/usr/bin/env python3
"""A Transporter's place decision on the device, from the render to a world pose: the network-ready batch of every env
(BatchedRearrangementEnv.transporter_batch), one shared random Conv2d on the scene and on the rotated crops as a stand-in
for the two feature networks, and the place head itself (BatchedRearrangementEnv.transporter_place ->
perception.correlate -> csrc/mre_correlate.hip): every env's scene features correlated with its own crop features on the
bf16 matrix cores, the best (rotation, row, column), and that cell's centre in the world.

    python examples/transporter_place_head.py --num-envs 64
Prints the shapes, the decisions of the first --show envs beside the scripted place pose, and how many logits were never
written.  The network is random, so the decisions mean nothing; with trained weights the same lines evaluate a policy in the
batched env: render -> heightmap -> transporter_batch -> network -> transporter_place -> place().
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mujoco_robot_environments_amd import perception  # noqa: E402
from mujoco_robot_environments_amd.tasks.rearrangement import (  # noqa: E402
    BatchedRearrangementEnv, HEIGHTMAP_BOUNDS, colour_separator_task_config)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=64)
    ap.add_argument("--cell", type=float, default=0.0025, help="metres per cell of the maps")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--rotations", type=int, default=36)
    ap.add_argument("--crop", type=int, default=64)
    ap.add_argument("--features", type=int, default=3, help="channels of the feature maps (1 .. 16)")
    ap.add_argument("--show", type=int, default=8, help="envs whose decisions are printed")
    args = ap.parse_args()
    env = BatchedRearrangementEnv(cfg=colour_separator_task_config(), num_envs=args.num_envs, render=True)
    env.reset()
    b = env.transporter_batch(args.seed, cell=args.cell, n_rotations=args.rotations, crop=args.crop)
    n, c, rows, cols = b.scene.shape
    torch.manual_seed(args.seed)
    net = torch.nn.Conv2d(c, args.features, 3, padding=1).to(device=b.scene.device, dtype=b.scene.dtype)
    with torch.no_grad():
        scene_features = net(b.scene)
        crop_features = net(b.crops.reshape(n * args.rotations, c, args.crop, args.crop)).reshape(
            n, args.rotations, args.features, args.crop, args.crop)
    print(f"{n} envs: scene features {tuple(scene_features.shape)}, crop features {tuple(crop_features.shape)} "
          f"{crop_features.dtype} on {crop_features.device}")
    d = env.transporter_place(scene_features, crop_features, cell=args.cell)
    _, _, place = env.sort_colours(peek=True)
    scripted = perception.world_2_cell(place[:, :3], HEIGHTMAP_BOUNDS, args.cell)
    cells, bins, xy, value = d.cells.cpu().numpy(), d.rotation.cpu().numpy(), d.xy.cpu().numpy(), d.value.cpu().numpy()
    angle = np.rad2deg(d.angle.cpu().numpy())
    for i in range(min(args.show, n)):
        print(f"env {i:4d}: place row {cells[i, 1]:3d} column {cells[i, 0]:3d} turned {angle[i]:5.1f} deg (bin {bins[i]:2d}) "
              f"-> x {xy[i, 0]:.4f} y {xy[i, 1]:.4f}, logit {value[i]:.3f}; scripted place: row {scripted[i, 1]:3d} "
              f"column {scripted[i, 0]:3d}")
    logits = n * args.rotations * rows * cols
    print(f"{logits:.3g} logits ({4 * logits / 2 ** 30:.2f} GiB in float32) were summed on the matrix cores and never written: "
          f"{2.0 * logits * args.features * args.crop ** 2 / 1e12:.2f} TFLOP per call")
    env.close()


if __name__ == "__main__":
    main()
