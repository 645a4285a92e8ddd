"""Time of the fused multi-view heightmaps (mre_heightmap_views) on rendered frames, against the composition a user has
without them.

    python tools/bench_heightmap_views.py [--envs 4096] [--iters 10] [--out profiles/r19a_bench_heightmap_views.json]
Renders one frame of `--envs` bench scenes (bench.setup_envs) through the configured overhead camera (480 x 640) and the two
obliques of the reference's arena/cameras/rearrangement group (640 x 640 each), and times on those frames, in this process:

  fused           perception.heightmap_views of the three views: one launch
  composition     perception.heightmap_views_reference on the device: three mre_heightmap launches, then the merge in torch
  one_view        perception.heightmap of the overhead view (mre_heightmap), beside
  one_view_fused  perception.heightmap_views of the overhead view alone

One untimed repeat of every candidate, then three timed repeats with the candidates alternating inside each; the median and
the range are reported.  Times are HIP events around `--iters` calls on torch's stream.  `--envs` is halved until the frames
and one candidate's outputs fit the device's free memory; the JSON says what was used.  The fused kernel's roofline is HBM:
it must read every depth pixel of every view once (4 B), rgb + seg of the winners (4 B per filled cell) and write 13 B per
cell (4 height, 3 colour, 1 label, 4 source index, 1 view).  What it reads beyond that is reported per view as source pixels
scanned per image pixel, from bench_heightmap's numpy model of the source rectangles.  The condition: the
fused kernel's slowest repeat is faster than the composition's fastest.  Prints one JSON line and writes it to --out.
"""
import argparse, json, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_PEAK_GBS = 8000.0   # the figure tools/bench_render.py divides by


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cell", type=float, default=0.0025)
    ap.add_argument("--out", default=os.path.join("profiles", "r19a_bench_heightmap_views.json"))
    args = ap.parse_args()
    import torch, bench
    from bench_heightmap import scanned_pixels
    assert torch.cuda.is_available(), "bench_heightmap_views needs a GPU"
    from mujoco_robot_environments_amd import config, lib as L, perception as P, rng
    from mujoco_robot_environments_amd.model import compile as MC
    from mujoco_robot_environments_amd.physics import BatchedPhysics
    from mujoco_robot_environments_amd.tasks.rearrangement import HEIGHTMAP_BOUNDS
    overhead = config.compose(overrides=["arena/props=colour_splitter"]).arena.cameras
    obliques = config.compose(overrides=["arena/cameras=rearrangement", "arena/props=colour_splitter"]).arena.cameras
    cameras = list(overhead) + list(obliques)
    out = P.heightmap_shape(HEIGHTMAP_BOUNDS, args.cell)
    # frames (8 B a pixel) plus the maps of the composition: three single-view sets, the fused set and the merge's temporaries
    per_env = sum(8 * int(c.height) * int(c.width) for c in cameras) + 8 * 13 * out[0] * out[1]
    N, asked = args.envs, args.envs
    while N > 1 and N * per_env > 0.6 * torch.cuda.mem_get_info()[0]:
        N //= 2
    phys = BatchedPhysics(N); ids = np.arange(N)
    bench.setup_envs(phys, 0, ids)
    phys.set_render_colours((rng.uniform(7, ids, [0], 12)[0].reshape(N, 4, 3) * 255).astype(np.uint8), None)
    views = []
    for c in cameras:
        q = np.asarray(c.quat, np.float64); Rc = MC.q2m(q / np.linalg.norm(q)); pos = np.asarray(c.pos, np.float64)
        h, w = int(c.height), int(c.width)
        rgb, depth, seg = phys.render(pos, Rc, float(c.fovy), h, w)
        views.append((depth, rgb, seg, P.heightmap_camera(pos, Rc, float(c.fovy), h, w)))
    torch.cuda.synchronize()
    kw = dict(bounds=HEIGHTMAP_BOUNDS, cell=args.cell)
    d0, rgb0, seg0, cam0 = views[0]
    cands = {"fused": lambda: P.heightmap_views(views, **kw), "composition": lambda: P.heightmap_views_reference(views, **kw),
             "one_view": lambda: P.heightmap(d0, rgb0, seg0, cam=cam0, **kw), "one_view_fused": lambda: P.heightmap_views(views[:1], **kw)}
    # the same answer first
    a, b = cands["fused"](), cands["composition"]()
    equal = all(bool(torch.equal(x.view(torch.uint8), y.view(torch.uint8))) for x, y in zip(a, b))
    filled = int((a.src >= 0).sum())
    won = [int((a.view == k).sum()) for k in range(len(views))]
    del b
    alone = [int((P.heightmap(d, None, None, cam=cam, **kw).src >= 0).sum()) for d, _, _, cam in views]
    a1, b1 = cands["one_view_fused"](), cands["one_view"]()
    equal_one = all(bool(torch.equal(x.view(torch.uint8), y.view(torch.uint8))) for x, y in zip(a1[:4], b1))
    filled_one = int((b1.src >= 0).sum())
    del a, a1, b1
    peak = {}
    for name, fn in cands.items():   # the untimed repeat of every candidate, and its peak memory above the resident frames
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn(); torch.cuda.synchronize()
        peak[name] = int(torch.cuda.max_memory_allocated() - base)
    ms = {name: [] for name in cands}
    for _ in range(3):
        for name, fn in cands.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record(); torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.iters)
    med = {name: statistics.median(v) for name, v in ms.items()}
    cells = float(N) * out[0] * out[1]
    pixels = [float(N) * v[0].shape[1] * v[0].shape[2] for v in views]
    moved = {"fused": 4.0 * sum(pixels) + 4.0 * filled + 13.0 * cells, "one_view_fused": 4.0 * pixels[0] + 4.0 * filled_one + 13.0 * cells,
             "one_view": 4.0 * pixels[0] + 4.0 * filled_one + 12.0 * cells}
    scanned = [scanned_pixels(v[3], HEIGHTMAP_BOUNDS, args.cell, out, v[0].shape[1], v[0].shape[2])[0] / float(v[0].shape[1] * v[0].shape[2])
               for v in views]
    res = {"metric": "fused height / colour / label / source / view maps of a batch frame seen through three cameras",
           "envs": N, "envs_asked": asked, "cameras": [c.name for c in cameras],
           "resolutions": [[int(v[0].shape[1]), int(v[0].shape[2])] for v in views], "map": list(out), "cell": args.cell,
           "iters": args.iters, "source_hash": L.source_hash(), "equal_composition": equal, "one_view_equal_mre_heightmap": equal_one,
           "filled_cells_per_view": alone, "filled_cells_fused": filled, "cells_won_per_view": won, "cells": int(cells),
           "source_pixels_scanned_per_image_pixel": scanned,
           "ms": med, "ms_range": {name: [min(v), max(v)] for name, v in ms.items()}, "ms_repeats": ms,
           "speedup_vs_composition": med["composition"] / med["fused"],
           "condition": "the fused kernel's slowest repeat beats the composition's fastest",
           "condition_held": bool(max(ms["fused"]) < min(ms["composition"])),
           "one_view_fused_over_mre_heightmap": med["one_view_fused"] / med["one_view"],
           "peak_memory_bytes_above_frames": peak,
           "roofline": {name: {"bound": "hbm", "algorithmic_bytes": moved[name], "achieved": moved[name] / (med[name] * 1e-3) / 1e9,
                               "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": moved[name] / (med[name] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                               "kernel": "k_heightmap" if name == "one_view" else "k_heightmap_views"} for name in moved}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    phys.close()


if __name__ == "__main__":
    main()
