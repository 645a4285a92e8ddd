"""Time of the frame labels (mre_seg_labels) on rendered frames, against the torch formula prop_bboxes used before it.

    python tools/bench_labels.py [--envs 4096] [--iters 20] [--out profiles/r08a_bench_labels.json]
Renders one frame of `--envs` bench scenes (bench.setup_envs) at 480 x 640 and times, on those frames and in this
process: the kernel without depth (boxes, counts, sums), the kernel with depth (+ nearest depth), and the torch formula
(boxes only).  Three repeats, the three candidates alternating inside each; the median repeat is reported.  Times are
HIP events around `--iters` calls on torch's stream.  The kernel's roofline is HBM: it reads every segmentation byte
once (1 B / pixel) and, with depth, 4 more bytes for each pixel that carries a label; what it writes is 60 B per env and
label.  Prints one JSON line and writes it to --out.
"""
import argparse, json, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0   # the figure tools/bench_render.py divides by


def torch_prop_bboxes(seg):
    """prop_bboxes before the kernel (kept here as the baseline): per cube a [N, H, W] mask, two any() reductions over
    it and four arg-max passes over int copies of their results."""
    import torch
    n, h, w = seg.shape
    out = torch.full((n, 4, 4), -1, dtype=torch.int64, device=seg.device)
    for p in range(4):
        m = seg == (12 + p)
        cols, rows = m.any(dim=1), m.any(dim=2)
        vis = cols.any(dim=1)
        box = torch.stack([cols.int().argmax(dim=1), rows.int().argmax(dim=1),
                           w - 1 - cols.flip(1).int().argmax(dim=1), h - 1 - rows.flip(1).int().argmax(dim=1)], dim=1)
        out[:, p] = torch.where(vis[:, None], box, out[:, p])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--out", default=os.path.join("profiles", "r08a_bench_labels.json"))
    args = ap.parse_args()
    import torch, bench
    assert torch.cuda.is_available(), "bench_labels needs a GPU"
    from mujoco_robot_environments_amd.model import compile as MC
    from mujoco_robot_environments_amd.physics import BatchedPhysics
    from mujoco_robot_environments_amd import lib as L, perception as P, rng
    N, H, W = args.envs, args.height, args.width
    phys = BatchedPhysics(N); ids = np.arange(N)
    bench.setup_envs(phys, 0, ids)
    phys.set_render_colours((rng.uniform(7, ids, [0], 12)[0].reshape(N, 4, 3) * 255).astype(np.uint8), None)
    q = np.array([0.707, 0, 0, -0.707]); Rc = MC.q2m(q / np.linalg.norm(q))
    _, depth, seg = phys.render(np.array([0.7, 0, 1.3]), Rc, 61.0, H, W, rgb=False)
    torch.cuda.synchronize()

    cands = {"kernel": lambda: P.seg_labels(seg), "kernel_depth": lambda: P.seg_labels(seg, depth),
             "torch_formula": lambda: torch_prop_bboxes(seg)}
    # the same answer first, at the size that is timed
    lab = P.seg_labels(seg, depth)
    boxes_equal = bool(torch.equal(lab.box, cands["torch_formula"]()))
    label_pixels = int(lab.count.sum())
    peak = {}
    for name, fn in cands.items():   # warm-up of every candidate, and its peak memory above the resident frames
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn(); torch.cuda.synchronize()
        peak[name] = int(torch.cuda.max_memory_allocated() - base)
        fn(); fn(); torch.cuda.synchronize()
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
    read = {"kernel": float(N) * H * W, "kernel_depth": float(N) * H * W + 4.0 * label_pixels}
    res = {"metric": "frame labels of a batch frame: boxes, visible pixels, centroid sums (+ nearest depth)",
           "envs": N, "resolution": [H, W], "iters": args.iters, "source_hash": L.source_hash(),
           "boxes_equal_torch_formula": boxes_equal, "label_pixels": label_pixels,
           "ms": med, "ms_repeats": ms, "speedup_vs_torch_formula": med["torch_formula"] / med["kernel"],
           "peak_memory_bytes_above_frames": peak,
           "roofline": {name: {"bound": "hbm", "algorithmic_bytes_read": read[name],
                               "achieved": read[name] / (med[name] * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": read[name] / (med[name] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                               "kernel": "k_labels_init + k_seg_labels"} for name in read}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    phys.close()


if __name__ == "__main__":
    main()
