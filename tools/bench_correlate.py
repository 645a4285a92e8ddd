"""Time of the Transporter place head (mre_correlate: correlate every env's crops with its scene, best cell per env) at the
workload this project measures, against what a user has without it: torch's grouped conv2d and an argmax.

    python tools/bench_correlate.py [--torch | --torch-only] [--out profiles/r16a_bench_correlate.json]
Workload: R 36 rotations, depth 3, scenes of 320 x 240, crops of 64 x 64, random bfloat16 features made on the device.
  kernel legs   n = 64, 512 and 4096 with best_* only; n = 64 and 512 with float32 logits as well;
  torch legs    (--torch; run last) n = 8, 64, 512, ... as far as --torch-max: in each, alternating with the kernel on the
                same features,
                    conv2d(scene.reshape(1, n D, H, W), kernels.reshape(n R, D, c, c), padding=c // 2, groups=n)[..., :H, :W]
                in bfloat16 on the device, then .flatten(1).argmax(1).  A size whose time, extrapolated linearly from the
                size before, would pass its limit is skipped and recorded as such, and so is every size after a leg that
                failed (no solver, out of memory) or ran out of time.
Every leg runs in a process of its own under its own time limit; this process never opens the GPU, and after a leg that
died or timed out it starts nothing more.  In a leg: the kernel's best_index on the first 8 envs is held to the argmax of
perception.correlate_reference on the same features (float32, on the CPU); one untimed call; three repeats, the candidates alternating inside
each, HIP events on torch's stream around `iters` calls; the median repeat is reported and all three are kept.  The
condition: in every leg where torch ran, the kernel's slowest repeat beats torch's fastest.
Recorded without a threshold: useful TFLOP/s = 2 n R H W D c^2 per call, issued TFLOP/s with R padded to 48 (three MFMA
row tiles), both as shares of the dense bfloat16 rate of the MI355X (about 2.5 PFLOP/s).
Prints one JSON line and writes it to --out.
"""
import argparse, json, os, statistics, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

R, D, H, W, CROP = 36, 3, 320, 240, 64
PEAK_TFLOPS = 2500.0


def flops(n, rot=R):
    return 2.0 * n * rot * H * W * D * CROP * CROP


def child(args):
    import torch
    assert torch.cuda.is_available(), "bench_correlate needs a GPU"
    from mujoco_robot_environments_amd import perception as P
    n, dev = args.n, "cuda"
    g = torch.Generator(device=dev); g.manual_seed(n)
    scene = torch.randn((n, D, H, W), generator=g, device=dev).to(torch.bfloat16)
    kern = torch.randn((n, R, D, CROP, CROP), generator=g, device=dev).to(torch.bfloat16)
    logits = {"none": None, "f32": torch.float32}[args.logits]
    kernel = lambda: P.correlate(scene, kern, logits=logits)

    def torch_leg():
        x = torch.nn.functional.conv2d(scene.reshape(1, n * D, H, W), kern.reshape(n * R, D, CROP, CROP), padding=CROP // 2, groups=n)
        return x[..., :H, :W].reshape(n, R, H, W).flatten(1).argmax(1)

    cands = {"kernel": kernel}
    if args.with_torch:
        cands["torch"] = torch_leg
    e8 = min(8, n)
    got = P.correlate(scene[:e8], kern[:e8]).index
    want = P.correlate_reference(scene[:e8].cpu(), kern[:e8].cpu()).index   # on the CPU: a known cost, no solver search
    res = {"n": n, "logits": args.logits, "iters": args.iters, "best_index_equals_reference_on_first_envs": bool(torch.equal(got.cpu(), want))}
    del want
    if args.with_torch:   # what torch's bfloat16 convolution answers on those envs, for the record: its sums are rounded
        res["torch_argmax_equals_kernel_on_first_envs"] = bool(torch.equal(torch_leg()[:e8], kernel().index[:e8]))
    ms = {c: [] for c in cands}
    for fn in cands.values():   # one untimed call each
        fn(); torch.cuda.synchronize()
    for _ in range(3):
        for c, fn in cands.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record(); torch.cuda.synchronize()
            ms[c].append(e0.elapsed_time(e1) / args.iters)
    res["ms_repeats"] = ms
    res["ms"] = {c: statistics.median(v) for c, v in ms.items()}
    sec = res["ms"]["kernel"] * 1e-3
    res["useful_tflops"], res["issued_tflops"] = flops(n) / sec / 1e12, flops(n, 48) / sec / 1e12
    res["useful_share_of_peak"], res["issued_share_of_peak"] = res["useful_tflops"] / PEAK_TFLOPS, res["issued_tflops"] / PEAK_TFLOPS
    if args.with_torch:
        res["kernel_slowest_repeat_beats_torch_fastest"] = bool(max(ms["kernel"]) < min(ms["torch"]))
        res["torch_over_kernel"] = res["ms"]["torch"] / res["ms"]["kernel"]
    print("RESULT " + json.dumps(res))


def run_leg(n, logits, iters, with_torch, limit):
    """One leg in a process of its own: (result dict or None, a word on how it ended)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--n", str(n), "--logits", logits, "--iters", str(iters)]
    if with_torch:
        cmd.append("--with-torch")
    print("leg n=%d logits=%s torch=%s starts (limit %d s)" % (n, logits, with_torch, limit), file=sys.stderr, flush=True)
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return None, "time limit of %d s" % limit
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            res = json.loads(line[7:])
            print("leg n=%d logits=%s torch=%s: %s ms" % (n, logits, with_torch, res["ms"]), file=sys.stderr, flush=True)
            return res, "ok"
    return None, "exit status %d: %s" % (p.returncode, p.stderr.strip().splitlines()[-1][:200] if p.stderr.strip() else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--torch", action="store_true", help="also time torch's grouped conv2d + argmax, last")
    ap.add_argument("--torch-only", action="store_true", help="keep the kernel legs already in --out and run the torch legs alone")
    ap.add_argument("--torch-max", type=int, default=512, help="largest n of a torch leg")
    ap.add_argument("--torch-limit", type=int, default=150, help="seconds a torch leg may take")
    ap.add_argument("--limit", type=int, default=120, help="seconds a kernel leg may take")
    ap.add_argument("--out", default=os.path.join("profiles", "r16a_bench_correlate.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--logits", default="none", choices=("none", "f32"))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--with-torch", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    from mujoco_robot_environments_amd import lib as L
    legs, skipped, alive = {}, {}, True
    if args.torch_only:
        with open(args.out) as f:
            before = json.load(f)
        legs = {k: v for k, v in before["legs"].items() if k.startswith("kernel/")}
        skipped = {k: v for k, v in before["not_run"].items() if k.startswith("kernel/")}
    for n, logits, iters in () if args.torch_only else ((64, "none", 20), (512, "none", 4), (4096, "none", 2), (64, "f32", 20), (512, "f32", 4)):
        name = "kernel/n%d/%s" % (n, logits)
        if not alive:
            skipped[name] = "not started: a leg before it died"
            continue
        res, how = run_leg(n, logits, iters, False, args.limit)
        if res is None:
            skipped[name], alive = how, False
        else:
            legs[name] = res
    if args.torch or args.torch_only:
        last, n = None, 8
        while n <= args.torch_max:
            name = "torch/n%d" % n
            # a leg makes 2 + 3 * iters calls of each candidate
            iters = 5 if n <= 64 else 2
            if not alive:
                skipped[name] = "not started: a leg before it died or found no way to run"
            elif last is not None and last[1] * 1e-3 * (n / last[0]) * (2 + 3 * iters) > 0.5 * args.torch_limit:
                skipped[name] = "not started: %.0f ms at n = %d extrapolates past the leg's limit" % (last[1], last[0])
            else:
                res, how = run_leg(n, "none", iters, True, args.torch_limit)
                if res is None:
                    skipped[name], alive = how, False
                else:
                    legs[name], last = res, (n, res["ms"]["torch"])
            n *= 8
    passes = {k: v["kernel_slowest_repeat_beats_torch_fastest"] for k, v in legs.items() if k.startswith("torch/")}
    equal = {k: v["best_index_equals_reference_on_first_envs"] for k, v in legs.items()}
    out = {"metric": "Transporter place head: correlate 36 rotated 64 x 64 crops with a 320 x 240 scene per env, best cell",
           "rotations": R, "depth": D, "map": [H, W], "crop": CROP, "peak_tflops_dense_bf16": PEAK_TFLOPS,
           "flop_per_env_useful": flops(1), "source_hash": L.source_hash(), "legs": legs, "not_run": skipped,
           "best_index_equals_reference_on_first_envs": equal, "kernel_slowest_repeat_beats_torch_fastest": passes}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    kernel_legs = [k for k in legs if k.startswith("kernel/")]
    sys.exit(0 if len(kernel_legs) == 5 and all(equal.values()) and all(passes.values()) else 1)


if __name__ == "__main__":
    main()
