"""Time of the network-ready tensors (mre_warp_inputs) of a Transporter training batch, against what a user had before it:
mre_warp_maps followed by the torch conversion lines.

    python tools/bench_warp_inputs.py [--envs 4096] [--iters 20] [--out profiles/r14a_bench_warp_inputs.json]
Two workloads on `--envs` maps of 320 x 240 cells (height float32, colour uint8 x 3; synthetic content made on the device: a
gather's time does not depend on the values, only on the matrices):
  (a) scenes   every map under its own rigid motion (perception.sample_perturbation) to 320 x 240;
  (b) crops    36 rotated crops of 64 x 64 cells per map around the moved pick cell (perception.crop_matrices),
each at CHANNELS_RGBH and CHANNELS_RGBHHH, in float32 and bfloat16: eight legs.  In every leg two candidates:
  kernel     perception.warp_inputs: one launch, no intermediate;
  two_step   perception.warp_maps (the kernel of the parent commit) and then, on the device,
             x = cat([colour.float(), height[..., None] (x 3)], -1).permute(0, 3, 1, 2).contiguous();
             x = (x - mean) / std;  x.to(dtype)
             on `--ref-envs` of the maps, scaled to the batch (every pass of it is linear in the samples).
Three repeats, the candidates alternating inside each; HIP events around `--iters` calls on torch's stream, after one untimed
call that leaves the candidate's blocks in torch's allocator; the median repeat is reported and all three are kept.  A leg
passes when the slowest repeat of the kernel is faster than the fastest repeat of the two-step path.  The kernel's roofline is
HBM: per output cell it must write channels x element size and, where the source cell exists, read 8 B (4 B of height and
the 3 B of colour counted as 4, as DESIGN.md 8f.6 counts them).  Before timing, the kernel is held to
perception.warp_inputs_reference on the first maps, and once per dtype the LAST sample of the RGBHHH crop tensor (3.6e9
elements: the far end of the 64-bit output offsets) is held to it too.
Prints one JSON line and writes it to --out.
"""
import argparse, json, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0   # the figure tools/bench_warp.py divides by


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--ref-envs", type=int, default=4096, help="maps the two-step path is timed on (scaled to --envs)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rotations", type=int, default=36)
    ap.add_argument("--crop", type=int, default=64)
    ap.add_argument("--only", default="", help="run one candidate twice and exit (for a counter pass): e.g. crops/RGBH/bf16/kernel")
    ap.add_argument("--out", default=os.path.join("profiles", "r14a_bench_warp_inputs.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_warp_inputs needs a GPU"
    from mujoco_robot_environments_amd import lib as L, perception as P
    N, H, W, R, K, CR = args.envs, 320, 240, min(args.ref_envs, args.envs), args.rotations, args.crop
    dev = "cuda"
    g = torch.Generator(device=dev); g.manual_seed(0)
    height = torch.rand((N, H, W), generator=g, device=dev) * 0.3
    colour = torch.randint(0, 256, (N, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
    rs = np.random.default_rng(0)
    cells = np.stack([rs.integers(60, 180, (N, 2)), rs.integers(80, 240, (N, 2))], axis=2)   # pick, place (column, row)
    pert = P.sample_perturbation(0, np.arange(N), 0, cells, (H, W))
    cmats, cindex = P.crop_matrices(pert.cells[:, 0], K, CR)
    pm = torch.from_numpy(pert.M).to(dev)
    cm, ci = torch.from_numpy(cmats).to(dev), torch.from_numpy(cindex).to(dev)
    work = {"scenes": dict(mats=pm, index=None, out_shape=(H, W), ref=R),
            "crops": dict(mats=cm, index=ci, out_shape=(CR, CR), ref=R * K)}
    chans = {"RGBH": P.CHANNELS_RGBH, "RGBHHH": P.CHANNELS_RGBHHH}
    dtypes = {"f32": torch.float32, "bf16": torch.bfloat16}
    scale = N / R

    def two_step(rkw, ch, dtype):
        # what a user writes after warp_maps: mean and std such that (u - mean) / std is the channel set's u * scale + bias
        nh = len(ch.sources) - 3
        std = torch.tensor([1.0 / s for s in ch.scales], device=dev).view(1, -1, 1, 1)
        mean = torch.tensor([-b / s for b, s in zip(ch.biases, ch.scales)], device=dev).view(1, -1, 1, 1)

        def fn():
            w = P.warp_maps(height[:R], colour[:R], with_source=False, **rkw)
            x = torch.cat([w.colour.float()] + [w.height.unsqueeze(-1)] * nh, dim=-1).permute(0, 3, 1, 2).contiguous()
            x = (x - mean) / std
            return x.to(dtype)
        return fn

    cands, legs = {}, []
    for name, w in work.items():
        kw = dict(mats=w["mats"], index=w["index"], out_shape=w["out_shape"])
        r = w["ref"]
        rkw = dict(mats=w["mats"][:r], index=None if w["index"] is None else w["index"][:r], out_shape=w["out_shape"])
        for cn, ch in chans.items():
            for dn, dt in dtypes.items():
                leg = f"{name}/{cn}/{dn}"
                legs.append(leg)
                cands[leg + "/kernel"] = lambda kw=kw, ch=ch, dt=dt: P.warp_inputs(height, colour, channels=ch, dtype=dt, **kw)
                cands[leg + "/two_step"] = two_step(rkw, ch, dt)
    if args.only:
        cands[args.only](); torch.cuda.synchronize()
        cands[args.only](); torch.cuda.synchronize()
        return
    bits = lambda t: t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)
    # the same answer first: the statement on the first maps, and the far end of the largest tensor
    E = min(32, N)
    equal, far_end = {}, {}
    for leg in legs:
        name, cn, dn = leg.split("/")
        w, r = work[name], E * (K if name == "crops" else 1)
        kw = dict(mats=w["mats"][:r], index=None if w["index"] is None else w["index"][:r], out_shape=w["out_shape"],
                  channels=chans[cn], dtype=dtypes[dn])
        a, b = P.warp_inputs(height[:E], colour[:E], **kw), P.warp_inputs_reference(height[:E], colour[:E], **kw)
        equal[leg] = bool(torch.equal(bits(a), bits(b)))
        del a, b
    for dn, dt in dtypes.items():
        full = cands[f"crops/RGBHHH/{dn}/kernel"]()
        want = P.warp_inputs_reference(height[N - 1:], colour[N - 1:], mats=cm[-1:], index=[0], out_shape=(CR, CR),
                                       channels=P.CHANNELS_RGBHHH, dtype=dt)
        far_end[dn] = {"elements": int(full.numel()), "last_sample_equals_statement": bool(torch.equal(bits(full[-1:]), bits(want)))}
        del full, want
    valid = {}
    for name, w in work.items():
        src = P.warp_maps(height, mats=w["mats"], index=w["index"], out_shape=w["out_shape"]).source
        valid[name] = int((src >= 0).sum())
        del src
    peak = {}
    for cname, fn in cands.items():   # warm-up of every candidate, and its peak memory above the resident maps
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn(); torch.cuda.synchronize()
        peak[cname] = int(torch.cuda.max_memory_allocated() - base)
        fn(); torch.cuda.synchronize()
    ms = {cname: [] for cname in cands}
    for _ in range(3):
        for cname, fn in cands.items():
            # one untimed call first: the candidates differ in the sizes they allocate, and the timed window must find
            # its blocks in torch's cache instead of asking the driver for gigabytes
            torch.cuda.empty_cache()
            fn(); torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record(); torch.cuda.synchronize()
            ms[cname].append(e0.elapsed_time(e1) / args.iters * (scale if cname.endswith("two_step") else 1.0))
    med = {cname: statistics.median(v) for cname, v in ms.items()}
    out_cells = {"scenes": float(N) * H * W, "crops": float(N) * K * CR * CR}
    roof, ratio, passes = {}, {}, {}
    for leg in legs:
        name, cn, dn = leg.split("/")
        k, t = ms[leg + "/kernel"], ms[leg + "/two_step"]
        moved = len(chans[cn].sources) * (2.0 if dn == "bf16" else 4.0) * out_cells[name] + 8.0 * valid[name]
        sec = med[leg + "/kernel"] * 1e-3
        roof[leg] = {"bound": "hbm", "algorithmic_bytes": moved, "achieved": moved / sec / 1e9, "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": moved / sec / 1e9 / HBM_PEAK_GBS, "kernel": "k_warp_inputs"}
        ratio[leg] = {"median": med[leg + "/two_step"] / med[leg + "/kernel"], "at_least": min(t) / max(k), "at_most": max(t) / min(k),
                      "kernel_spread": max(k) / min(k) - 1.0, "two_step_spread": max(t) / min(t) - 1.0}
        passes[leg] = bool(max(k) < min(t))
    res = {"metric": "network-ready scenes (a) and pick crops (b) of a Transporter batch: one launch against warp_maps + torch",
           "envs": N, "map": [H, W], "rotations": K, "crop": CR, "iters": args.iters, "source_hash": L.source_hash(),
           "maps": "synthetic, made on the device", "equal_torch_statement": equal, "far_end": far_end,
           "two_step_envs_timed": R, "two_step_scaled_by": scale, "output_cells": out_cells, "valid_cells": valid,
           "ms": med, "ms_repeats": ms, "two_step_over_kernel": ratio,
           "kernel_slowest_repeat_beats_two_step_fastest": passes, "peak_memory_bytes_above_maps": peak, "roofline": roof}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ok = all(passes.values()) and all(equal.values()) and all(v["last_sample_equals_statement"] for v in far_end.values())
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
