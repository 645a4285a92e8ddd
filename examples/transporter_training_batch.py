#!/usr/bin/env python3
"""One Transporter training batch on the device: the orthographic maps of every env (BatchedRearrangementEnv.heightmap),
perturbed by a random rigid motion with their pick and place cells, and the rotated crops around the moved pick cell
(BatchedRearrangementEnv.transporter_sample -> perception.warp_maps -> csrc/mre_warp.hip).

    python examples/transporter_training_batch.py --num-envs 64
Renders the envs after reset(), builds the maps and takes one sample per env.  Prints the shapes, the attempts the
perturbation took, and for the first --show envs that have a cube to move: the pick cell before and after the motion with
the label the maps hold there, and the memory of the batch.

    python examples/transporter_training_batch.py --num-envs 64 --inputs
also takes the same batch as the tensors a network consumes (BatchedRearrangementEnv.transporter_batch ->
perception.warp_inputs -> csrc/mre_warp_inputs.hip): channels-first, normalised, bfloat16.  Prints their shapes, dtypes and
the smallest and largest value of every channel, and feeds the scene through one torch.nn.Conv2d: nothing else is needed.
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=64)
    ap.add_argument("--cell", type=float, default=0.0025, help="metres per cell of the maps")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--draw", type=int, default=0, help="which perturbation of the stream (seed, env id, draw)")
    ap.add_argument("--rotations", type=int, default=36)
    ap.add_argument("--crop", type=int, default=64)
    ap.add_argument("--show", type=int, default=8, help="envs whose pick cells are printed")
    ap.add_argument("--inputs", action="store_true", help="also take the batch as network-ready tensors and run a convolution on it")
    args = ap.parse_args()
    env = BatchedRearrangementEnv(cfg=colour_separator_task_config(), num_envs=args.num_envs, render=True)
    env.reset()
    rgb, depth, seg = env.render()
    maps = env.heightmap(depth, rgb, seg, cell=args.cell)
    s = env.transporter_sample(args.seed, args.draw, depth, rgb, seg, cell=args.cell, n_rotations=args.rotations,
                               crop=args.crop)
    n, rows, cols = s.maps.height.shape
    print(f"{n} envs: maps {tuple(s.maps.height.shape)} + colour {tuple(s.maps.colour.shape)} + label, "
          f"crops {tuple(s.crops.height.shape)} + colour {tuple(s.crops.colour.shape)} + label")
    took = s.tries[s.tries > 0]
    print(f"perturbation (seed {args.seed}, draw {args.draw}): {len(took)} envs accepted after {took.mean() if len(took) else 0:.2f} "
          f"attempts on average (most {took.max() if len(took) else 0}), {int((s.tries < 0).sum())} kept the identity")
    in_progress, pick, _ = env.sort_colours(peek=True)
    before = perception.world_2_cell(pick[:, :3], HEIGHTMAP_BOUNDS, args.cell)
    label0, label1 = maps.seg.cpu().numpy(), s.maps.seg.cpu().numpy()
    centre = s.crops.seg[:, 0, args.crop // 2, args.crop // 2].cpu().numpy()
    shown = 0
    for i in np.nonzero(in_progress & (s.tries > 0))[0]:
        (c0, r0), (c1, r1) = before[i], s.pick[i]
        was = label0[i, r0, c0] if 0 <= c0 < cols and 0 <= r0 < rows else -1
        print(f"env {i:4d}: pick row {r0:3d} column {c0:3d} (label {was:3d}) -> row {r1:3d} column {c1:3d} "
              f"(label {label1[i, r1, c1]:3d}; centre of crop 0: {centre[i]:3d}) after {s.tries[i]} attempts; "
              f"place -> row {s.place[i, 1]:3d} column {s.place[i, 0]:3d}")
        shown += 1
        if shown >= args.show:
            break
    tensors = [t for m in (s.maps, s.crops) for t in m if t is not None]
    print(f"one batch: {sum(t.numel() * t.element_size() for t in tensors) / 2 ** 20:.1f} MiB on {tensors[0].device} "
          f"({sum(t.numel() * t.element_size() for t in s.crops if t is not None) / 2 ** 20:.1f} MiB of it crops)")
    if args.inputs:
        show_inputs(env, args, depth, rgb, seg, s)
    env.close()


def show_inputs(env, args, depth, rgb, seg, sample):
    import torch
    b = env.transporter_batch(args.seed, args.draw, depth, rgb, seg, cell=args.cell, n_rotations=args.rotations, crop=args.crop,
                              channels=perception.CHANNELS_RGBHHH)
    assert np.array_equal(b.pick, sample.pick) and np.array_equal(b.tries, sample.tries)   # the motion of the sample above
    print(f"network inputs: scene {tuple(b.scene.shape)} {b.scene.dtype}, crops {tuple(b.crops.shape)} {b.crops.dtype} on "
          f"{b.scene.device}; pick_index {b.pick_index.shape} {b.pick_index.dtype}, rotation_index all {int(b.rotation_index.max())}")
    names = ["red", "green", "blue", "height"]
    for k, src in enumerate(perception.CHANNELS_RGBHHH.sources):
        sc, cr = b.scene[:, k].float(), b.crops[:, :, k].float()
        print(f"  channel {k} ({names[src]:6s}): scene {float(sc.min()):.4f} .. {float(sc.max()):.4f}, "
              f"crops {float(cr.min()):.4f} .. {float(cr.max()):.4f}")
    conv = torch.nn.Conv2d(b.scene.shape[1], 8, 3).to(device=b.scene.device, dtype=b.scene.dtype)
    with torch.no_grad():
        y = conv(b.scene)
    print(f"Conv2d({b.scene.shape[1]}, 8, 3)(scene) -> {tuple(y.shape)} {y.dtype}, finite: {bool(torch.isfinite(y).all())}")


if __name__ == "__main__":
    main()
