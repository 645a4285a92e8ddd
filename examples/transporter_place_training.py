#!/usr/bin/env python3
"""Training a Transporter's place head on the device: the network-ready batch of every env
(BatchedRearrangementEnv.transporter_batch), one shared Conv2d on the scene and on the rotated crops as a stand-in for the
two feature networks, the place loss (BatchedRearrangementEnv.transporter_loss -> perception.place_loss ->
csrc/mre_correlate_grad.hip): the softmax cross-entropy of every env's rotations x rows x columns logits against its moved
place cell, without a logit stored, and both gradients back into the Conv2d -- and a few SGD steps on that one fixed batch.

    python examples/transporter_place_training.py --num-envs 16 --steps 5
Prints the mean loss of every step: it starts near log(rotations x rows x columns) and falls as the network begins to
overfit the batch.  With a data loader around transporter_batch(seed, draw) the same lines train a policy.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mujoco_robot_environments_amd.tasks.rearrangement import BatchedRearrangementEnv, colour_separator_task_config  # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=16)
    ap.add_argument("--cell", type=float, default=0.0025, help="metres per cell of the maps")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--rotations", type=int, default=36)
    ap.add_argument("--crop", type=int, default=64)
    ap.add_argument("--features", type=int, default=3, help="channels of the feature maps (1 .. 16)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--lr", type=float, default=0.2)
    args = ap.parse_args()
    env = BatchedRearrangementEnv(cfg=colour_separator_task_config(), num_envs=args.num_envs, render=True)
    env.reset()
    b = env.transporter_batch(args.seed, cell=args.cell, n_rotations=args.rotations, crop=args.crop)
    n, c, rows, cols = b.scene.shape
    labelled = torch.from_numpy(np.asarray(b.tries) > 0).to(b.scene.device)   # the place cell is inside the map
    torch.manual_seed(args.seed)
    # float32 master weights; the features are made in the batch's bfloat16
    net = torch.nn.Conv2d(c, args.features, 3, padding=1).to(b.scene.device)
    opt = torch.optim.SGD(net.parameters(), lr=args.lr)
    print(f"{n} envs ({int(labelled.sum())} labelled), {args.rotations * rows * cols} logits each; "
          f"log of that: {np.log(args.rotations * rows * cols):.3f}")
    for step in range(args.steps):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            scene_features = net(b.scene)
            # the crop features divided by the length of a logit's sum: a logit is then a mean of products and starts O(1)
            crop_features = net(b.crops.reshape(n * args.rotations, c, args.crop, args.crop)).reshape(
                n, args.rotations, args.features, args.crop, args.crop) / (args.features * args.crop ** 2)
        loss = env.transporter_loss(scene_features.contiguous(), crop_features.contiguous(), b)[labelled].mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        print(f"step {step}: loss {loss.item():.4f}")
    env.close()


if __name__ == "__main__":
    main()
