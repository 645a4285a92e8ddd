"""Copy one round's rocprofv3 outputs from gpurun_out/ (scratch) into profiles/ (tracked).

usage: [BENCH_STEPS=200 BENCH_WARMUP=20] python tools/summarize_profiles.py TAG SOLVER STATS_DIR FETCH_DIR WRITE_DIR SQ_DIR FLOP_DIR [BUILD NOTE]
  BENCH_STEPS / BENCH_WARMUP: the --steps / --warmup the profiled bench.py command ran with (default: bench.py's own
  200 / 20; the driver's end-of-round run uses 20 / 5).  They are recorded in the summary, and files of a
  non-default pair carry the suffix _s<steps>w<warmup>: bench.py only quotes counters taken at ITS arguments, on
  ITS sources (the summary records lib.source_hash()).
  SOLVER    : PGS (kernel mre::k_step, files TAG_*) or Newton (mre::k_step_newton, files TAG_*_newton)
  STATS_DIR : rocprofv3 --kernel-trace --stats --output-format csv -d STATS_DIR -- python bench.py ...
  FETCH_DIR / WRITE_DIR / SQ_DIR / FLOP_DIR : the separate --pmc passes (never combined with traces
  other than --kernel-trace); FLOP_DIR (SQ_INSTS_VALU_{ADD,MUL,FMA,TRANS}_F32/F64) may be "-"; MFMA_DIR (environment:
  the SQ_INSTS_VALU_MFMA_MOPS_F32 pass) is optional.
Writes profiles/TAG_kernel_stats.csv and TAG_pmc_summary.json (per-launch means; FETCH_SIZE / WRITE_SIZE are KiB on gfx950).
"""
import csv
import glob
import json
import os
import shutil
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# bench.py's default cut (round 5): QUEUE launches -- the warm-up window is one launch of the queue kernel, the timed
# window ceil(K / 200) launches of all 4096 envs (csrc/mre_env.h: mre_env::queue_ticks).  PER_TICK=1: the launches of
# rounds 1-5 (bench.py --fused 1: one launch per tick and env group).
PER_TICK = os.environ.get("PER_TICK", "0") == "1"
KERNELS = ({"PGS": "mre::k_step(", "Newton": "mre::k_step_newton("} if PER_TICK else
           {"PGS": "mre::k_step_queue(", "Newton": "mre::k_step_queue_newton("})
KERNEL = KERNELS["PGS"]
GROUPS = int(os.environ.get("MRE_GROUPS", "4"))   # env groups per tick (csrc/mre_sched.cpp: one launch per group)
STEPS = int(os.environ.get("BENCH_STEPS", "200"))
WARMUP_TICKS = int(os.environ.get("BENCH_WARMUP", "20"))
QUEUE_TICKS = int(os.environ.get("MRE_QUEUE_TICKS", "200"))
if PER_TICK:
    WARMUP = WARMUP_TICKS * GROUPS  # the kernel's dispatches that belong to the untimed warm-up ticks
    TIMED = STEPS * GROUPS
    ENVS_PER_LAUNCH, TICKS_PER_LAUNCH = 4096 // GROUPS, 1.0
else:
    # bench.py's warm-up window on a fresh handle: a queue launch from 8 ticks on (nothing measured yet says the regime is
    # light: csrc/mre_policy.h, window_wants_queue), per-tick launches below
    WARMUP = (WARMUP_TICKS + QUEUE_TICKS - 1) // QUEUE_TICKS if WARMUP_TICKS >= 8 else 0
    TIMED = (STEPS + QUEUE_TICKS - 1) // QUEUE_TICKS
    ENVS_PER_LAUNCH, TICKS_PER_LAUNCH = 4096, STEPS / float(TIMED)


def one(pattern):
    f = sorted(glob.glob(pattern, recursive=True))
    if not f:
        raise SystemExit(f"nothing matches {pattern}")
    return f[0]


def counter_rows(d):
    path = one(os.path.join(d, "**", "*counter_collection.csv"))
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if r["Kernel_Name"].startswith(KERNEL)]
    # the first WARMUP dispatches of the kernel are the bench's untimed warm-up launches
    ids = sorted({int(r["Dispatch_Id"]) for r in rows})
    keep = set(ids[WARMUP:WARMUP + TIMED]) if len(ids) > WARMUP else set(ids)   # the timed window's launches only
    return path, [r for r in rows if int(r["Dispatch_Id"]) in keep]


def main():
    global KERNEL
    tag, solver, stats_d, fetch_d, write_d, sq_d, flop_d = sys.argv[1:8]
    note = sys.argv[8] if len(sys.argv) > 8 else ""
    KERNEL = KERNELS[solver]
    sfx = "" if solver == "PGS" else "_newton"
    if (STEPS, WARMUP_TICKS) != (200, 20):
        sfx += f"_s{STEPS}w{WARMUP_TICKS}"
    sys.path.insert(0, ROOT)
    from mujoco_robot_environments_amd import lib as _lib
    out = os.environ.get("PROFILES_OUT", os.path.join(ROOT, "profiles"))   # (PROFILES_OUT: summarise on the GPU box into gpurun_out/, the raw CSVs stay there)
    os.makedirs(out, exist_ok=True)
    shutil.copy(one(os.path.join(stats_d, "**", "*kernel_stats.csv")), os.path.join(out, f"{tag}_kernel_stats{sfx}.csv"))
    summary = {
        "command": f"rocprofv3 --pmc <COUNTERS> --kernel-trace --output-format csv -- python bench.py --solver {solver} "
                   f"--steps {STEPS} --warmup {WARMUP_TICKS} --no-cpu-baseline ({WARMUP} warm-up launches dropped, {TIMED} timed launches averaged; separate passes: FETCH_SIZE | WRITE_SIZE | SQ_* | "
                   "SQ_INSTS_VALU_*_F32/F64 + MFMA)",
        "bench_steps": STEPS, "bench_warmup": WARMUP_TICKS, "source_hash": _lib.source_hash(),
        "kernel": KERNEL.rstrip("("),
        "launch": (f"1 env group of 1 control tick = 5 physics steps x {ENVS_PER_LAUNCH} envs ({GROUPS} launches per tick; "
                   "the counter passes serialise the dispatches, so launch durations in these passes are those of one group alone on the GPU)") if PER_TICK else
                  (f"1 queue launch = {TICKS_PER_LAUNCH:.0f} control ticks x 5 physics steps x {ENVS_PER_LAUNCH} envs on 2048 persistent waves; the counter "
                   "passes serialise the dispatches: the large kernel's waiting launch (k_step_queue_large) leaves after its bounded wait, this "
                   "kernel then runs alone, and the large kernel's second launch behind it steps the envs handed over -- a few of 4096, not counted here"),
        "envs_per_launch": ENVS_PER_LAUNCH, "ticks_per_launch": TICKS_PER_LAUNCH, "build": note}
    passes = [("fetch", fetch_d), ("write", write_d), ("sq", sq_d)]
    if flop_d != "-":
        passes.append(("flop", flop_d))
    if os.environ.get("MFMA_DIR"):
        passes.append(("mfma", os.environ["MFMA_DIR"]))
    for name, d in passes:
        path, rows = counter_rows(d)
        if not rows:
            print(f"no rows of {KERNEL} in {path}")
            continue
        # (the per-dispatch rows stay under gpurun_out/: only the per-launch means below are read afterwards, and two
        #  generations of raw CSVs were 29 MB of every snapshot pushed to the GPU box)
        acc = defaultdict(list)
        dur = {}
        for r in rows:
            acc[r["Counter_Name"]].append(float(r["Counter_Value"]))
            dur[r["Dispatch_Id"]] = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        summary[f"avg_launch_ms_in_{name}_pass"] = sum(dur.values()) / len(dur)
        summary[f"launches_in_{name}_pass"] = len(dur)
        for k, v in sorted(acc.items()):
            summary[f"{k}_per_launch"] = sum(v) / len(v)
        summary["LDS_Block_Size"] = int(rows[0]["LDS_Block_Size"])
        summary["VGPR_Count"] = int(rows[0]["VGPR_Count"])
        summary["Accum_VGPR_Count"] = int(rows[0]["Accum_VGPR_Count"])
        summary["Scratch_Size"] = int(rows[0]["Scratch_Size"])
    # MI355X_MICROARCH.md: on gfx950 FETCH_SIZE reads half the bytes of a streaming read, and "other access widths are
    # uncalibrated: calibrate on a known byte count in your own access pattern".  tools/pmc_calibrate.hip did, for the
    # step kernels' pattern (one wave moves one row of 44 floats): FETCH_SIZE x 1.22, WRITE_SIZE x 0.917; dword- and
    # 16-B-per-lane streaming reads both x 2.0, streaming writes exact (profiles/*_pmc_calibration.json).
    cal = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_calibration.json")))
    f_read, f_write, f_read_stream = 1.0, 1.0, 2.0
    if cal:
        with open(cal[-1]) as f:
            c = json.load(f)
        f_read = c.get("FETCH_SIZE k_rows44", {}).get("factor") or 1.0
        f_write = c.get("WRITE_SIZE k_rows44", {}).get("factor") or 1.0
        f_read_stream = c.get("FETCH_SIZE k_read_dword", {}).get("factor") or 2.0
        summary["calibration"] = {"file": os.path.basename(cal[-1]), "read_rows": f_read, "write_rows": f_write, "read_streaming": f_read_stream}
    summary["hbm_read_bytes_per_launch"] = summary["FETCH_SIZE_per_launch"] * 1024.0 * f_read
    summary["hbm_write_bytes_per_launch"] = summary["WRITE_SIZE_per_launch"] * 1024.0 * f_write
    summary["traffic_bytes_per_launch"] = summary["hbm_read_bytes_per_launch"] + summary["hbm_write_bytes_per_launch"]
    # upper bound: every read counted like a streaming one
    summary["traffic_bytes_per_launch_upper"] = summary["FETCH_SIZE_per_launch"] * 1024.0 * f_read_stream + summary["hbm_write_bytes_per_launch"]
    g = lambda k: summary.get(f"SQ_INSTS_VALU_{k}_per_launch", 0.0)
    if "SQ_INSTS_VALU_per_launch" in summary:
        # VALU issue: a wave64 VALU instruction holds its SIMD for 4 cycles; 1024 SIMDs at 2.4 GHz
        t = summary["avg_launch_ms_in_sq_pass"] * 1e-3
        summary["valu_issue_util_in_sq_pass"] = summary["SQ_INSTS_VALU_per_launch"] * 4.0 / (1024 * 2.4e9 * t)
    if "SQ_INSTS_VALU_FMA_F32_per_launch" in summary:
        # counted FLOPs: every counted wave instruction at its full 64 lanes (exec masks are not
        # visible to the counter), FMA = 2
        summary["counted_flop_f32_per_launch"] = 64.0 * (g("ADD_F32") + g("MUL_F32") + g("TRANS_F32") + 2.0 * g("FMA_F32"))
        summary["counted_flop_f64_per_launch"] = 64.0 * (g("ADD_F64") + g("MUL_F64") + 2.0 * g("FMA_F64"))
    if "SQ_INSTS_VALU_MFMA_MOPS_F32_per_launch" in summary:
        # matrix-core work of the Newton Hessian (v_mfma_f32_16x16x4_f32).  MI355X_MICROARCH.md: the MOPS counters
        # count in units of 512 flops per wave instruction
        summary["mfma_flop_f32_per_launch"] = 512.0 * summary["SQ_INSTS_VALU_MFMA_MOPS_F32_per_launch"]
    summary["note"] = ("FETCH_SIZE/WRITE_SIZE are in KiB; traffic = FETCH_SIZE x read_rows + WRITE_SIZE x write_rows with the factors "
                       "calibrated on a known byte count in this kernel's access pattern (tools/pmc_calibrate.hip: one wave moves "
                       "one row of 44 floats); traffic_bytes_per_launch_upper counts every read like a streaming one (x 2).")
    with open(os.path.join(out, f"{tag}_pmc_summary{sfx}.json"), "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
