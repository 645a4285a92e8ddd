"""Time of the warped and cropped maps (mre_warp_maps) of a Transporter training batch, against the torch statement.

    python tools/bench_warp.py [--envs 4096] [--iters 10] [--out profiles/r13a_bench_warp.json]
Two workloads on `--envs` maps of 320 x 240 cells (height float32, colour uint8 x 3, label uint8; synthetic content made on
the device: a gather's time does not depend on the values, only on the matrices):
  (a) perturb   every map under its own rigid motion (perception.sample_perturbation) to 320 x 240;
  (b) crops     36 rotated crops of 64 x 64 cells per map around a pick cell (perception.crop_matrices).
Each is timed with all three maps and with the height map alone, always with the source index, and against
`perception.warp_maps_reference` on the same device -- plain torch, what a user has without the kernel.  The torch
statement is timed on `--ref-envs` of the maps (it materialises int64 index images) and scaled to the batch.  Three repeats,
the candidates alternating inside each; the median repeat is reported.  Times are HIP events around `--iters` calls on
torch's stream.  The kernel's roofline is HBM: per output cell it must write 12 B (4 height, 3 colour, 1 label, 4 source
index; 8 B for the height alone) and, where the source cell exists, read 8 B (4 B).  What a launch moves beyond that is
what rocprofv3 --pmc FETCH_SIZE WRITE_SIZE shows.  Prints one JSON line and writes it to --out.
"""
import argparse, json, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0   # the figure tools/bench_render.py divides by


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--ref-envs", type=int, default=128)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rotations", type=int, default=36)
    ap.add_argument("--crop", type=int, default=64)
    ap.add_argument("--only", default="", help="run one candidate once and exit (for a counter pass): e.g. perturb/kernel")
    ap.add_argument("--out", default=os.path.join("profiles", "r13a_bench_warp.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_warp needs a GPU"
    from mujoco_robot_environments_amd import lib as L, perception as P
    N, H, W, R, K, CR = args.envs, 320, 240, min(args.ref_envs, args.envs), args.rotations, args.crop
    dev = "cuda"
    g = torch.Generator(device=dev); g.manual_seed(0)
    height = torch.rand((N, H, W), generator=g, device=dev) * 0.3
    colour = torch.randint(0, 256, (N, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
    seg = torch.randint(0, 20, (N, H, W), generator=g, device=dev, dtype=torch.uint8)
    rs = np.random.default_rng(0)
    cells = np.stack([rs.integers(60, 180, (N, 2)), rs.integers(80, 240, (N, 2))], axis=2)   # pick, place (column, row)
    pert = P.sample_perturbation(0, np.arange(N), 0, cells, (H, W))
    cmats, cindex = P.crop_matrices(pert.cells[:, 0], K, CR)
    pm = torch.from_numpy(pert.M).to(dev)
    cm, ci = torch.from_numpy(cmats).to(dev), torch.from_numpy(cindex).to(dev)
    work = {"perturb": dict(mats=pm, index=None, out_shape=(H, W), ref=R, scale=N / R),
            "crops": dict(mats=cm, index=ci, out_shape=(CR, CR), ref=R * K, scale=N / R)}
    cands = {}
    for name, w in work.items():
        kw = dict(mats=w["mats"], index=w["index"], out_shape=w["out_shape"])
        r = w["ref"]
        rkw = dict(mats=w["mats"][:r], index=None if w["index"] is None else w["index"][:r], out_shape=w["out_shape"])
        cands[name + "/kernel"] = lambda kw=kw: P.warp_maps(height, colour, seg, **kw)
        cands[name + "/kernel_height_only"] = lambda kw=kw: P.warp_maps(height, **kw)
        cands[name + "/torch_statement"] = lambda rkw=rkw: P.warp_maps_reference(height[:R], colour[:R], seg[:R], **rkw)
        cands[name + "/torch_statement_height_only"] = lambda rkw=rkw: P.warp_maps_reference(height[:R], **rkw)
    if args.only:
        cands[args.only](); torch.cuda.synchronize()
        cands[args.only](); torch.cuda.synchronize()
        return
    equal, valid = {}, {}
    for name, w in work.items():   # the same answer first, on the samples the torch statement is timed on
        r = w["ref"]
        a = P.warp_maps(height[:R], colour[:R], seg[:R], mats=w["mats"][:r],
                        index=None if w["index"] is None else w["index"][:r], out_shape=w["out_shape"])
        b = cands[name + "/torch_statement"]()
        equal[name] = bool(torch.equal(a.height.view(torch.int32), b.height.view(torch.int32)) and torch.equal(a.colour, b.colour)
                           and torch.equal(a.seg, b.seg) and torch.equal(a.source, b.source))
        del a, b
        full = cands[name + "/kernel"]()
        valid[name] = int((full.source >= 0).sum())
        del full
    peak = {}
    for name, fn in cands.items():   # warm-up of every candidate, and its peak memory above the resident maps
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn(); torch.cuda.synchronize()
        peak[name] = int(torch.cuda.max_memory_allocated() - base)
        fn(); torch.cuda.synchronize()
    ms = {name: [] for name in cands}
    for _ in range(3):
        for name, fn in cands.items():
            is_ref = "torch" in name
            iters = max(1, args.iters // 5) if is_ref else args.iters
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record(); torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / iters * (work[name.split("/")[0]]["scale"] if is_ref else 1.0))
    med = {name: statistics.median(v) for name, v in ms.items()}
    out_cells = {"perturb": float(N) * H * W, "crops": float(N) * K * CR * CR}
    roof = {}
    for name in work:
        for kind, rd, wr in (("kernel", 8.0, 12.0), ("kernel_height_only", 4.0, 8.0)):
            moved = wr * out_cells[name] + rd * valid[name]
            t = med[f"{name}/{kind}"] * 1e-3
            roof[f"{name}/{kind}"] = {"bound": "hbm", "algorithmic_bytes": moved, "achieved": moved / t / 1e9, "peak": HBM_PEAK_GBS,
                                      "unit": "GB/s", "frac": moved / t / 1e9 / HBM_PEAK_GBS, "kernel": "k_warp_maps"}
    res = {"metric": "warped (a: perturb) and cropped (b: crops) height / colour / label maps of a Transporter batch",
           "envs": N, "map": [H, W], "rotations": K, "crop": CR, "iters": args.iters, "source_hash": L.source_hash(),
           "maps": "synthetic, made on the device", "equal_torch_statement": equal,
           "torch_statement_envs_timed": R, "torch_statement_scaled_by": N / R,
           "output_cells": out_cells, "valid_cells": valid, "ms": med, "ms_repeats": ms,
           "speedup_vs_torch_statement": {n: med[n + "/torch_statement"] / med[n + "/kernel"] for n in work},
           "speedup_vs_torch_statement_height_only": {n: med[n + "/torch_statement_height_only"] / med[n + "/kernel_height_only"]
                                                      for n in work},
           "peak_memory_bytes_above_maps": peak, "roofline": roof}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
