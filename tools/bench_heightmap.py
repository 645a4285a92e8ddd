"""Time of the orthographic heightmaps (mre_heightmap) on rendered frames, against the torch statement of the same maps.

    python tools/bench_heightmap.py [--envs 4096] [--iters 10] [--out profiles/r12a_bench_heightmap.json]
Renders one frame of `--envs` bench scenes (bench.setup_envs) at 480 x 640 from the configured overhead camera and times,
on those frames and in this process: the kernel with rgb and seg (all four maps), the kernel on depth alone, and
`perception.heightmap_reference` on the same device -- plain torch, what a user has without the kernel.  The torch
statement is timed on `--ref-envs` of the frames (it materialises int64 images) and scaled to the batch.  Three repeats,
the candidates alternating inside each; the median repeat is reported.  Times are HIP events around `--iters` calls on
torch's stream.  The kernel's roofline is HBM: it must read every depth pixel once (4 B) and rgb + seg of the winners
(4 B per filled cell), and write 12 B per cell (4 height, 3 colour, 1 label, 4 source index).  What it reads beyond that
-- neighbouring tiles scan the pixels their boxes share through parallax -- is reported as source pixels scanned per
image pixel, from a numpy model of the kernel's source rectangles (`scanned_pixels`).  Prints one JSON line and writes
it to --out.
"""
import argparse, json, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0   # the figure tools/bench_render.py divides by
TILE = 64               # HM_TILE of csrc/mre_heightmap.h


def scanned_pixels(cam, bounds, cell, out, h, w, tile=TILE):
    """Source pixels the workgroups of one env scan (tile_rect of csrc/mre_heightmap.hip, in float64), as
    (total, [(u0, u1, v0, v1) or None per tile, row-major])."""
    cam = np.asarray(cam, np.float64)
    A, pos = cam[:9].reshape(3, 3), cam[9:]
    inv = np.linalg.inv(A)
    lo, hi = np.asarray(bounds[0], np.float64), np.asarray(bounds[1], np.float64)
    total, rects = 0, []
    for ty in range(-(-out[0] // tile)):
        for tx in range(-(-out[1] // tile)):
            xs = lo[0] + np.array([tx * tile, min((tx + 1) * tile, out[1])]) * cell
            ys = lo[1] + np.array([ty * tile, min((ty + 1) * tile, out[0])]) * cell
            q = np.array([inv @ (np.array([x, y, z]) - pos) for x in xs for y in ys for z in (lo[2], hi[2])])
            if (q[:, 2] >= 1e-3).all():
                u, v = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
                r = (max(np.floor(u.min()) - 2, 0), min(np.ceil(u.max()) + 2, w - 1),
                     max(np.floor(v.min()) - 2, 0), min(np.ceil(v.max()) + 2, h - 1))
            else:
                r = (0, w - 1, 0, h - 1)
            if r[0] <= r[1] and r[2] <= r[3]:
                rects.append(tuple(int(x) for x in r))
                total += (rects[-1][1] - rects[-1][0] + 1) * (rects[-1][3] - rects[-1][2] + 1)
            else:
                rects.append(None)
    return total, rects


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--ref-envs", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cell", type=float, default=0.0025)
    ap.add_argument("--tile", type=int, default=TILE,
                    help="HM_TILE of the library being timed (a diagnostic build with -DMRE_HM_TILE=32 loaded through MRE_LIB)")
    ap.add_argument("--out", default=os.path.join("profiles", "r12a_bench_heightmap.json"))
    args = ap.parse_args()
    import torch, bench
    assert torch.cuda.is_available(), "bench_heightmap needs a GPU"
    from mujoco_robot_environments_amd.model import compile as MC
    from mujoco_robot_environments_amd.physics import BatchedPhysics
    from mujoco_robot_environments_amd.tasks.rearrangement import HEIGHTMAP_BOUNDS
    from mujoco_robot_environments_amd import lib as L, perception as P, rng
    N, H, W, R = args.envs, 480, 640, min(args.ref_envs, args.envs)
    phys = BatchedPhysics(N); ids = np.arange(N)
    bench.setup_envs(phys, 0, ids)
    phys.set_render_colours((rng.uniform(7, ids, [0], 12)[0].reshape(N, 4, 3) * 255).astype(np.uint8), None)
    q = np.array([0.707, 0, 0, -0.707]); pos = np.array([0.7, 0, 1.3]); Rc = MC.q2m(q / np.linalg.norm(q))
    rgb, depth, seg = phys.render(pos, Rc, 61.0, H, W)
    torch.cuda.synchronize()
    kw = dict(cam=P.heightmap_camera(pos, Rc, 61.0, H, W), bounds=HEIGHTMAP_BOUNDS, cell=args.cell)
    out = P.heightmap_shape(HEIGHTMAP_BOUNDS, args.cell)

    cands = {"kernel": lambda: P.heightmap(depth, rgb, seg, **kw), "kernel_depth_only": lambda: P.heightmap(depth, **kw),
             "torch_statement": lambda: P.heightmap_reference(depth[:R], rgb[:R], seg[:R], **kw)}
    # the same answer first, on the frames the torch statement is timed on
    a, b = P.heightmap(depth[:R], rgb[:R], seg[:R], **kw), cands["torch_statement"]()
    equal = bool(torch.equal(a.height.view(torch.int32), b.height.view(torch.int32)) and torch.equal(a.colour, b.colour)
                 and torch.equal(a.seg, b.seg) and torch.equal(a.src, b.src))
    filled = int((cands["kernel"]().src >= 0).sum())
    del a, b
    peak = {}
    for name, fn in cands.items():   # warm-up of every candidate, and its peak memory above the resident frames
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn(); torch.cuda.synchronize()
        peak[name] = int(torch.cuda.max_memory_allocated() - base)
        fn(); torch.cuda.synchronize()
    ms = {name: [] for name in cands}
    for _ in range(3):
        for name, fn in cands.items():
            iters = args.iters if name != "torch_statement" else max(1, args.iters // 5)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record(); torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / iters * (N / R if name == "torch_statement" else 1.0))
    med = {name: statistics.median(v) for name, v in ms.items()}
    cells = float(N) * out[0] * out[1]
    moved = {"kernel": 4.0 * N * H * W + 4.0 * filled + 12.0 * cells, "kernel_depth_only": 4.0 * N * H * W + 8.0 * cells}
    scanned = scanned_pixels(kw["cam"], HEIGHTMAP_BOUNDS, args.cell, out, H, W, args.tile)[0]
    res = {"metric": "orthographic height / colour / label / source maps of a batch frame",
           "envs": N, "resolution": [H, W], "map": list(out), "cell": args.cell, "iters": args.iters,
           "source_hash": L.source_hash(), "tile": args.tile, "source_pixels_scanned_per_image_pixel": scanned / float(H * W),
           "equal_torch_statement": equal, "torch_statement_envs_timed": R, "filled_cells": filled,
           "ms": med, "ms_repeats": ms, "speedup_vs_torch_statement": med["torch_statement"] / med["kernel"],
           "peak_memory_bytes_above_frames": peak,
           "roofline": {name: {"bound": "hbm", "algorithmic_bytes": moved[name],
                               "achieved": moved[name] / (med[name] * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": moved[name] / (med[name] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                               "kernel": "k_heightmap"} for name in moved}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    phys.close()


if __name__ == "__main__":
    main()
