#!/usr/bin/env python3
"""Training inputs of a Transporter network from the batched camera: top-down orthographic height, colour and label maps
of every env (BatchedRearrangementEnv.heightmap -> csrc/mre_heightmap.hip), and the pick / place labels of the scripted
demonstrator (sort_colours) as cells of those maps (perception.world_2_cell).

    python examples/transporter_heightmaps.py --num-envs 64
Renders the envs after reset(), builds the maps on the device, and prints for the first --show envs that have a cube to
move: the cell of the pick pose, the height and the label the map holds there, and the cell of the place pose.

    python examples/transporter_heightmaps.py --num-envs 64 --views
The same from three cameras fused into one set of maps (BatchedRearrangementEnv.heightmap_views ->
csrc/mre_heightmap_views.hip): the overhead camera plus the two obliques of the reference's arena/cameras/rearrangement
group, each rendered at its own size; also prints the cells each camera fills alone, the cells of the fused maps and how
many of them each camera won.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mujoco_robot_environments_amd import config, perception  # noqa: E402
from mujoco_robot_environments_amd.tasks.rearrangement import (  # noqa: E402
    BatchedRearrangementEnv, HEIGHTMAP_BOUNDS, OVERHEAD, colour_separator_task_config)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=64)
    ap.add_argument("--cell", type=float, default=0.0025, help="metres per cell of the maps")
    ap.add_argument("--show", type=int, default=8, help="envs whose pick / place cells are printed")
    ap.add_argument("--views", action="store_true", help="fuse the overhead camera with the reference's two oblique cameras")
    args = ap.parse_args()
    env = BatchedRearrangementEnv(cfg=colour_separator_task_config(), num_envs=args.num_envs, render=True)
    env.reset()
    if args.views:
        obliques = config.compose(overrides=["arena/cameras=rearrangement", "arena/props=colour_splitter"]).arena.cameras
        cameras = [OVERHEAD] + [env.add_camera(c.name, c.pos, c.quat, c.fovy, c.height, c.width) for c in obliques]
        frames = env.render_views(cameras)
        maps = env.heightmap_views(cameras, frames, cell=args.cell)
        n, rows, cols = maps.height.shape
        for k, (name, (rgb, depth, seg)) in enumerate(zip(cameras, frames)):
            alone = env.heightmap(depth, rgb, seg, camera=name, cell=args.cell)
            print(f"view {k} {name}: {depth.shape[1]} x {depth.shape[2]} frames fill {int((alone.src >= 0).sum())} cells alone "
                  f"and win {int((maps.view == k).sum())} of the fused maps'")
        print(f"{n} envs: {len(cameras)} views fused -> {rows} x {cols} maps at {args.cell * 1000:g} mm per cell, "
              f"{int((maps.src >= 0).sum())} of {n * rows * cols} cells filled")
    else:
        rgb, depth, seg = env.render()
        maps = env.heightmap(depth, rgb, seg, cell=args.cell)
        n, rows, cols = maps.height.shape
        filled = (maps.src >= 0).float().mean().item()
        print(f"{n} envs: {depth.shape[1]} x {depth.shape[2]} frames -> {rows} x {cols} maps of {HEIGHTMAP_BOUNDS[0]} .. "
              f"{HEIGHTMAP_BOUNDS[1]} at {args.cell * 1000:g} mm per cell, {100 * filled:.1f} % of the cells filled")
    in_progress, pick, place = env.sort_colours(peek=True)
    pick_cell = perception.world_2_cell(pick[:, :3], HEIGHTMAP_BOUNDS, args.cell)
    place_cell = perception.world_2_cell(place[:, :3], HEIGHTMAP_BOUNDS, args.cell)
    height, label = maps.height.cpu().numpy(), maps.seg.cpu().numpy()
    shown = 0
    for i in np.nonzero(in_progress)[0]:
        (pc, pr), (qc, qr) = pick_cell[i], place_cell[i]
        inside = 0 <= pc < cols and 0 <= pr < rows
        at = f"height {height[i, pr, pc] * 1000:6.1f} mm above lo_z, label {label[i, pr, pc]:3d}" if inside else "outside the map"
        print(f"env {i:4d}: pick ({pick[i, 0]:.3f}, {pick[i, 1]:+.3f}) -> row {pr:3d} column {pc:3d}: {at}; "
              f"place ({place[i, 0]:.3f}, {place[i, 1]:+.3f}) -> row {qr:3d} column {qc:3d}")
        shown += 1
        if shown >= args.show:
            break
    print(f"{int(in_progress.sum())} of {n} envs have a cube to move")
    env.close()


if __name__ == "__main__":
    main()
