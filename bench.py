#!/usr/bin/env python3
"""bench.py -- env-steps/s of the batched RearrangementEnv physics step on MI355X.

Workload (BASELINE.json configs[1]): 4096 parallel RearrangementEnv per GPU
(per-env 2..4 cubes, half size U(0.015,0.016)), random actions resampled every
control tick (5 physics steps of 1 ms), inputs resident in HBM.
One bench "step" = one control tick = 5 env-steps x 4096 envs.  The timed window of K ticks is handed to the library
in ONE call (mre_rollout_ticks), which steps it as QUEUE launches (round 5): persistent waves, one (env, tick) per pass,
the env furthest behind first -- no per-tick barrier, so a slow tick of one env delays nobody else; `per_tick_launches`
times the same ticks the old way (one launch per tick and env group) in the same run.
With --gpus N (launched through torch.distributed.run, one rank per GPU) every
rank owns 4096 envs (weak scaling: 32768 envs at N=8, configs[3]); there is no
data-path collective, only the end-of-rollout all_gather of the final state.

Prints ONE JSON line (rank 0) with the driver contract fields plus
  "roofline":     HBM roofline of the step kernel (algorithmic bytes / time; bound "hbm" as north_star asks), with
                  "issue_occupancy" (VALU issue slots taken -- what actually limits the kernel) beside it
  "queue":        the queue launches of the window (count, waves, envs handed to the large kernel inside a launch)
A plain run times the headline solver's window and nothing else.  --full adds every other measurement below (and
"flop" in the roofline: algorithmic FLOPs counted on the CPU restatement vs the lanes the device issues):
  "per_tick_launches": the same ticks stepped as one launch per tick and env group
  "default_regime": the same workload timed a second time in the same run over ticks 200..400 (arms on the table,
                  cubes knocked about: the heavy regime), whatever --steps / --warmup the headline window used
  "pgs":          the same two windows with north_star's PGS (<= 100 sweeps); the headline is the solver whose parity
                  tests hold the 1e-4 bar as a hard assertion (Newton, which is also what the reference's MuJoCo runs)
  "pick_place":   the second leg, BASELINE.json configs[2]: the loop the reference actually runs -- one scripted pick +
                  place per env through mre_run_controller with osc.yaml's gains (18 000 env-steps per env), env-steps/s,
                  converged fraction and constraint high-water marks per phase, capacity promotions
  "cpu_baseline": the fp64 CPU oracle ("port" of the same pipeline, NOT MuJoCo) timed
                  on this host's cores on a bounded sample of the same workload.
--dump-outputs DIR writes the final state of the headline window (what a caller of the rollout reads back) as .npy files.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

ENVS_PER_GPU = 4096
CONTROL_STEPS = 5
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec
WS_MIN, WS_MAX = (0.35, -0.4, 0.43), (0.55, 0.4, 0.435)  # config/task/rearrangement.yaml:4-6


def algorithmic_bytes_per_env_step(nprops: np.ndarray) -> float:
    """4*(2*nq + 4*nv + nu) bytes with nq = 15+7n, nv = 15+6n, nu = 8."""
    n = nprops.astype(np.float64)
    return float(np.mean(4.0 * (2 * (15 + 7 * n) + 4 * (15 + 6 * n) + 8)))


def baseline_metric():
    """BASELINE.json's metric string (the repo root travels with the bench)."""
    try:
        with open(os.path.join(ROOT, "BASELINE.json")) as f:
            return json.load(f)["metric"]
    except Exception:
        return "env steps/sec (whole node), RearrangementEnv batch=4096 at 1/2/4/8 MI355X"


def pmc_summary(solver, steps, warmup):
    """The committed counter passes that describe THIS run: profiles/rNNx_pmc_summary[_newton][_s<K>w<W>].json taken by
    tools/measure_round.sh with the same --steps / --warmup (the constraint mix, hence every counter, depends on which
    ticks are timed) on the same sources (lib.source_hash()).  The counters cannot be read from inside the process, so
    per-launch figures are carried over -- but only from a pass that matches; otherwise (None, reason)."""
    import glob
    import re
    from mujoco_robot_environments_amd import lib as _lib
    sfx = "_pmc_summary" + ("" if solver == "PGS" else "_newton") + ("" if (steps, warmup) == (200, 20) else f"_s{steps}w{warmup}") + ".json"
    files = sorted(f for f in glob.glob(os.path.join(ROOT, "profiles", "*" + sfx))
                   if re.fullmatch(r"r\d\d[a-z]" + re.escape(sfx), os.path.basename(f)))
    if not files:
        return None, f"no counter passes at --steps {steps} --warmup {warmup} under profiles/"
    with open(files[-1]) as f:
        d = json.load(f)
    name = os.path.basename(files[-1])
    if (d.get("bench_steps"), d.get("bench_warmup")) != (steps, warmup):
        return None, f"{name} was taken at --steps {d.get('bench_steps')} --warmup {d.get('bench_warmup')}"
    if d.get("source_hash") != _lib.source_hash():
        return None, f"{name} was taken on other kernel sources ({d.get('source_hash')}, now {_lib.source_hash()})"
    return d, name


def issue_occupancy(d, name, avg_launch_s, envs_per_launch=ENVS_PER_GPU, ticks_per_launch=1.0):
    """What actually limits the kernel: VALU issue slots (an occupancy of the issue ports by executed instructions,
    useful or not -- NOT a roofline fraction; the flop object says how much of it is algorithmic work).  A wave64 VALU instruction occupies its
    SIMD for 4 cycles (16 lanes per SIMD), so  util = SQ_INSTS_VALU * 4 / (SIMDs * clock * time).
    ``avg_launch_s``: wall time per launch (tick time / launches per tick): launches of different env groups
    overlap on the GPU, so their individual durations do not add up to the time the SIMDs were available."""
    n = d.get("SQ_INSTS_VALU_per_launch")
    if not n or avg_launch_s <= 0:
        return None
    # counters were taken on launches of that many envs x control ticks
    scale = envs_per_launch * ticks_per_launch / (float(d.get("envs_per_launch", ENVS_PER_GPU)) * float(d.get("ticks_per_launch", 1)))
    n *= scale
    simds, clock = 256 * 4, 2.4e9  # MI355X_MICROARCH.md: 256 CUs x 4 SIMDs, 2.4 GHz peak engine clock
    out = {"valu_insts_per_launch": n, "cycles_per_wave64_inst": 4, "simds": simds, "clock_hz": clock,
           "util": n * 4.0 / (simds * clock * avg_launch_s), "source": name}
    fl = d.get("counted_flop_f32_per_launch")
    if fl:
        fl *= scale
        # counted FLOPs (SQ_INSTS_VALU_{ADD,MUL,TRANS,FMA}_F32 x 64 lanes, FMA = 2) against the FP32 vector peak
        # of MI355X_MICROARCH.md (157.3 TFLOP/s); idle lanes of a wave count as work, so this is an upper bound
        mf = d.get("mfma_flop_f32_per_launch")
        out["counted_flop"] = {"f32_per_launch": fl, "f64_per_launch": d.get("counted_flop_f64_per_launch"),
                               "mfma_f32_per_launch": mf * scale if mf is not None else None,   # SQ_INSTS_VALU_MFMA_MOPS_F32 x 512
                               "tflops": fl / avg_launch_s / 1e12, "peak_tflops": 157.3,
                               "frac": fl / avg_launch_s / 1e12 / 157.3}
    return out


def setup_envs(phys, seed, env_ids, settle_steps=300):
    from mujoco_robot_environments_amd import placement, rng
    nprops, sizes = rng.prop_params(seed, env_ids)
    phys.set_env_id_offset(int(env_ids[0]))
    phys.set_props(nprops, sizes)
    phys.reset()
    # PropPlacer: rejection sampling + settle with the robot frozen (prop_initializer.py:164-283)
    phys.place_props(seed, WS_MIN, WS_MAX, settle_steps=settle_steps)
    return nprops, sizes


def cpu_baseline(seed, budget_s=12.0, nenv=64):
    """Oracle (CPU restatement) on this host: same scene / action law, OpenMP over envs."""
    from mujoco_robot_environments_amd import placement, rng
    from mujoco_robot_environments_amd.model import compile as MC
    from oracle import oracle as O
    A = MC.compile_scene()
    m = O.Model(MC.to_blob(A))
    ids = np.arange(nenv)
    nprops, sizes = rng.prop_params(seed, ids)
    pose, _ = placement.sample_poses(seed, ids, nprops, sizes, WS_MIN, WS_MAX)
    envs = []
    for i in range(nenv):
        e = O.Env(m, int(nprops[i]), sizes[i])
        q = e.arr("qpos")
        q[:7] = A["home_qpos"]
        for p in range(int(nprops[i])):
            q[15 + 7 * p: 22 + 7 * p] = pose[i, p]
        e.freeze_robot(True)
        e.forward()
        envs.append(e)
    # a 1-GPU box grants a 16-core CPU share (more threads only oversubscribe the cgroup)
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    threads = max(1, min(avail, 16))
    O.batch_step(m, envs, None, 300, threads)  # settle
    for e in envs:
        e.freeze_robot(False)
        e.set_solver("Newton")     # the headline's solver (MuJoCo's default: what the reference's CPU path runs)
    ticks, t0 = 0, time.perf_counter()
    while True:
        acts = rng.random_actions(seed, ids, [ticks])[0]
        O.batch_step(m, envs, acts, CONTROL_STEPS, threads)
        ticks += 1
        if time.perf_counter() - t0 > budget_s:
            break
    dt = time.perf_counter() - t0
    finite = sum(bool(np.isfinite(e.arr("qpos")[:43]).all()) for e in envs)
    # the same loop on ONE thread (SURVEY section 8d asks for both), a few seconds on the first 4 envs
    t1, ticks1 = time.perf_counter(), 0
    while time.perf_counter() - t1 < 4.0:
        acts = rng.random_actions(seed, ids[:4], [ticks + ticks1])[0]
        O.batch_step(m, envs[:4], acts, CONTROL_STEPS, 1)
        ticks1 += 1
    dt1 = time.perf_counter() - t1
    # the oracle's PGS <= 100 sweeps (north_star's solver), same envs, a few seconds
    for e in envs:
        e.set_solver("PGS")
    t2, ticks2 = time.perf_counter(), 0
    while time.perf_counter() - t2 < 4.0:
        acts = rng.random_actions(seed, ids, [ticks + ticks1 + ticks2])[0]
        O.batch_step(m, envs, acts, CONTROL_STEPS, threads)
        ticks2 += 1
    dt2 = time.perf_counter() - t2
    return {"finite_envs": finite, "value": nenv * ticks * CONTROL_STEPS / dt, "unit": "env-steps/s", "cores": threads,
            "pgs_value": nenv * ticks2 * CONTROL_STEPS / dt2,
            "pgs_sample": f"the same envs right after the Newton sample (ticks {ticks + ticks1}..{ticks + ticks1 + ticks2}: arms on the "
                          "table, the heaviest regime; from rest the PGS oracle runs at twice this rate)",
            "kind": "port", "sample": f"{nenv} envs x {ticks} ticks x {CONTROL_STEPS} steps, fp64 oracle "
            f"(Newton, same scene / actions as the headline), OpenMP {threads} threads, {dt:.1f} s",
            "single_thread_value": 4 * ticks1 * CONTROL_STEPS / dt1}


def mujoco_probe(seed, budget_s=6.0, nenv=4):
    """if ``import mujoco`` happens to succeed on this host, run genuine
    mj_step on the MJCF this repo emits from its own spec (tools/emit_mjcf.py) -- same scenes, same action
    law -- time it and report how far the oracle is from it.  Never a dependency: absent -> {"mujoco": None}."""
    try:
        import mujoco
    except Exception as e:  # ModuleNotFoundError on this image
        return {"mujoco": None, "reason": f"{type(e).__name__}: {e}"}
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import emit_mjcf
    from mujoco_robot_environments_amd import placement, rng
    from mujoco_robot_environments_amd.model import compile as MC
    from oracle import oracle as O
    A = MC.compile_scene()
    om = O.Model(MC.to_blob(A))
    ids = np.arange(nenv)
    nprops, sizes = rng.prop_params(seed, ids)
    pose, _ = placement.sample_poses(seed, ids, nprops, sizes, WS_MIN, WS_MAX)
    out = {"mujoco": mujoco.__version__}
    for solver in ("Newton", "PGS"):
        worst, steps, t_mj = 0.0, 0, 0.0
        for i in range(nenv):
            n = int(nprops[i])
            m = mujoco.MjModel.from_xml_string(emit_mjcf.emit(nprops=n, prop_sizes=sizes[i], solver=solver))
            d = mujoco.MjData(m)
            e = O.Env(om, n, sizes[i])
            e.set_solver(solver)
            q = e.arr("qpos")
            q[:7] = A["home_qpos"]
            for p in range(n):
                q[15 + 7 * p: 22 + 7 * p] = pose[i, p]
            d.qpos[:] = q[:15 + 7 * n]
            e.forward()
            mujoco.mj_forward(m, d)
            for t in range(200):
                a = rng.random_actions(seed, ids[i:i + 1], [t])[0, 0]
                d.ctrl[:] = a
                e.arr("ctrl")[:] = a
                t0 = time.perf_counter()
                for _ in range(CONTROL_STEPS):
                    mujoco.mj_step(m, d)
                t_mj += time.perf_counter() - t0
                e.step(CONTROL_STEPS)
                steps += CONTROL_STEPS
                worst = max(worst, float(np.abs(d.qpos - e.arr("qpos")[:15 + 7 * n]).max()))
                if t_mj > budget_s:
                    break
        out[solver] = {"oracle_vs_mujoco_max_dqpos": worst, "mujoco_steps_per_s_1_thread": steps / max(t_mj, 1e-9),
                       "sample": f"{nenv} envs, {steps} steps"}
    return out


def counted_flops(seed, windows, nenv=16):
    """algorithmic FLOPs per env-step COUNTED on the CPU restatement (tools/count_flops.py: the oracle's
    source compiled with an operation-counting `double`), for the tick windows this run times.  A child process: the
    counting library replaces the plain oracle library, which this process may already hold."""
    import subprocess
    cmd = [sys.executable, os.path.join(ROOT, "tools", "count_flops.py"), "--nenv", str(nenv), "--seed", str(seed),
           "--windows", ",".join(f"{a}:{b}" for a, b in windows)]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        return json.loads(out.stdout.strip().splitlines()[-1])
    except Exception as e:  # the line must still be printed
        return {"error": f"{type(e).__name__}: {e}"}


def attach_flop_roofline(run, flops, solver, window, n_local):
    """roofline.flop: algorithmic work (counted on the oracle, this run's tick window) against what the device issues
    (lane-inclusive counter figure of the matching PMC pass, if there is one) and against the FP32 vector peak."""
    w = (flops.get(solver) or {}).get(window)
    if not w:
        run["roofline"]["flop"] = {"unavailable": flops.get("error", f"no count for {solver} {window}")}
        return
    alg = w["arith_per_env_step"]
    occ = run["roofline"].get("issue_occupancy") or {}
    cf = occ.get("counted_flop") or {}
    dev = None
    if cf.get("f32_per_launch"):
        per = run["roofline"]["envs_per_launch"] * run["roofline"].get("ticks_per_launch", 1.0) * CONTROL_STEPS
        dev = (cf["f32_per_launch"] + (cf.get("f64_per_launch") or 0.0) + (cf.get("mfma_f32_per_launch") or 0.0)) / per
    run["roofline"]["flop"] = {
        "algorithmic_per_env_step": alg, "special_per_env_step": w["special_per_env_step"], "per_stage": w["per_stage"],
        "counted_per_env_step": dev, "lane_efficiency": (alg / dev) if dev else None,
        "frac_of_157TF": alg * run["value"] / 157.3e12, "peak_tflops": 157.3,
        "source": f"tools/count_flops.py on {flops.get('nenv')} envs of this workload, ticks {window} (MuJoCo-dense pipeline: "
                  "multiplications by structural zeros of the dense Jacobian are counted, as MuJoCo executes them at nv < 60); "
                  "counted_per_env_step = SQ_INSTS_VALU_*_F32/F64 x 64 lanes (+ MFMA) of the matching counter pass"}


def pick_place_leg(n_envs, device, solver="Newton"):
    """BASELINE.json configs[2] -- the loop the reference actually runs: n_envs RearrangementEnv with
    arena/props=colour_splitter + task=rearrangement_w_targets, every env executing ONE scripted pick (9 s) + place (9 s)
    towards its first misplaced cube (tasks/rearrangement.py:358-440, :700-751) through mre_run_controller (in-kernel OSC,
    osc.yaml's own gains): 18 000 env-steps per env.  Timed: the two env.step() calls (10 scripted phases, each cut into
    launches of 50 ticks), state resident in HBM; reset / sort_colours are outside the timed region."""
    from mujoco_robot_environments_amd.tasks.rearrangement import BatchedRearrangementEnv, colour_separator_task_config
    cfg = colour_separator_task_config()
    env = BatchedRearrangementEnv(cfg=cfg, num_envs=n_envs, device=device, render=False, solver=solver)
    env.reset()
    in_progress, pick_pose, place_pose = env.sort_colours()
    phys = env.physics
    phys.sync()
    fb0 = phys.fallback_stats()
    q0 = phys.queue_info()
    phases = []
    inner = env._phase

    def phase(name, duration):
        conv = inner(name, duration)
        li = phys.launch_info()
        q = lambda a: [int(np.quantile(a, x)) for x in (0.5, 0.9, 0.99, 1.0)]   # noqa: E731
        phases.append({"phase": name.replace("Failed to ", ""), "seconds": duration, "converged_frac": float(np.mean(conv)),
                       # high-water marks of the phase's LAST launch (50 ticks) over envs: median / 90 % / 99 % / max
                       # (compact capacities 32 contacts / 112 rows / 62 robot rows / 8 cube-cube; large 48 / 160 / 100 / 16)
                       "ncon": q(li["ncon"]), "nefc": q(li["nefc"]), "nrrow": q(li["nrrow"]), "npp": q(li["npp"]),
                       "large_envs": phys.fallback_stats()["large_envs"]})
        return conv
    env._phase = phase
    cube0 = phys.qpos()[:, 15:18].copy()
    phys.profile_enable(True)
    t0 = time.perf_counter()
    env.step({"pose": pick_pose, "pixel_coords": None, "gripper_rot": 0.0})
    held = phys.qpos()[:, 17] > 0.55          # the first cube of the envs that act is the picked one only by chance: report per `which` below
    env.step({"pose": place_pose, "pixel_coords": None, "gripper_rot": 0.0})
    phys.sync()
    elapsed = time.perf_counter() - t0
    kern_ms, launches = phys.profile_read()
    phys.profile_enable(False)
    fb1 = phys.fallback_stats()
    q1 = phys.queue_info()
    status = phys.status()
    still = env.sort_colours(peek=True)[0]
    nprops = env.nprops
    steps = 18000
    alg = algorithmic_bytes_per_env_step(nprops) * n_envs * steps
    out = {"workload": "configs[2]: colour_splitter + rearrangement_w_targets, one scripted pick + place per env through "
                       "mre_run_controller (in-kernel OSC, osc.yaml gains), 18000 env-steps per env",
           "solver": solver, "envs": n_envs, "value": n_envs * steps / elapsed, "unit": "env-steps/s", "seconds": elapsed,
           "envs_acting": int(in_progress.sum()), "phases": phases,
           "all_phases_converged_frac": float(np.mean(env.last_converged[in_progress])) if in_progress.any() else None,
           "cube_moved_frac": float(np.mean(np.linalg.norm(phys.qpos()[in_progress, 15:17] - cube0[in_progress, :2], axis=1) > 0.02)) if in_progress.any() else None,
           "envs_done_after_the_pair": int((~still).sum()),
           "capacity_fallback": {k: fb1[k] - fb0[k] if k != "large_envs" else fb1[k] for k in fb1},
           "queue_launches": q1["launches"] - q0["launches"], "queue_handovers": q1["handovers"] - q0["handovers"],
           "nan_envs": int(((status & 2) != 0).sum()), "overflow_envs": int(((status & 4) != 0).sum()),
           "roofline": {"bound": "hbm", "achieved": alg / elapsed / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": alg / elapsed / 1e9 / HBM_PEAK_GBS, "traffic": None,
                        "kernel": ("mre::k_step_queue_newton + mre::k_step_queue_large_newton" if solver == "Newton" else "mre::k_step_queue + mre::k_step_queue_large")
                                  if q1["launches"] > q0["launches"] else
                                  ("mre::k_step_newton + mre::k_step_large_newton" if solver == "Newton" else "mre::k_step + mre::k_step_large"),
                        "kernel_ms_sum": kern_ms, "launches": launches,
                        "note": "queue launches of 100 ticks over all envs (mre_run_controller; without the queue: launches of 50 ticks per env "
                                "group); the compact and the large kernel of a launch run side by side; per-kernel averages: "
                                "profiles/r05*_kernel_stats_pickplace.csv"}}
    del held
    env.close()
    return out


def spawn_ranks(args) -> int:
    """`python bench.py --gpus N` outside torch.distributed.run: start the N ranks as fresh child
    processes BEFORE this process touches the GPU (never re-exec a process that holds the device),
    relay their output and exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


def timed_run(phys, seq, K, W, F, world, backend, dist, torch, n_local, dist_on=None, gather=True):
    """W untimed warm-up ticks, then exactly K timed ticks between barrier + synchronize pairs."""
    dist_on = world > 1 if dist_on is None else dist_on

    def barrier():
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()
        phys.sync()

    # one library call per window: mre_rollout_ticks cuts the K ticks into launches of F ticks (default 1: one launch
    # per tick and env group, as the reference's loop steps tick by tick) and enqueues them all, staying up to four
    # launches ahead of every group; MRE_BENCH_PER_TICK_CALLS=1 restores one Python call per tick (rounds 1-4)
    if os.environ.get("MRE_BENCH_PER_TICK_CALLS") == "1":
        for k in range(0, W, max(F, 1)):
            phys.rollout(seq[k:k + max(F, 1)], control_steps=CONTROL_STEPS)
    elif W > 0:
        phys.rollout(seq[0:W], control_steps=CONTROL_STEPS, ticks_per_launch=F)   # (F = 0: the library's cut, see main)
    barrier()
    phys.profile_enable(True)
    timed_run.queue0 = phys.queue_info()   # (queue launches / hand-overs of the timed window only)
    t0 = time.perf_counter()
    if os.environ.get("MRE_BENCH_PER_TICK_CALLS") == "1":
        for k in range(W, W + K, max(F, 1)):
            phys.rollout(seq[k:k + max(F, 1)], control_steps=CONTROL_STEPS)
    else:
        phys.rollout(seq[W:W + K], control_steps=CONTROL_STEPS, ticks_per_launch=F)
    gather_ms = 0.0
    if dist_on and gather:
        # end-of-rollout gather (the only collective of the job): final qpos/qvel/status
        phys.sync()
        tg = time.perf_counter()
        from mujoco_robot_environments_amd import distributed as D
        # rows packed ON THE DEVICE (mre_pack_final_state) and handed to all_gather_into_tensor as they are; only the
        # gloo rehearsal (CPU tensors) takes them through the host
        fin = phys.pack_final_state()
        if backend != "nccl":
            fin = fin.cpu()
        out = D.gather_final_state(fin)
        assert out.shape[0] == world * n_local
        torch.cuda.synchronize()
        gather_ms = (time.perf_counter() - tg) * 1e3
    barrier()
    elapsed = time.perf_counter() - t0
    kern_ms, launches = phys.profile_read()
    phys.profile_enable(False)
    if dist_on:
        t = torch.tensor([elapsed], dtype=torch.float64, device=phys.device if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    return elapsed, kern_ms, launches, gather_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--envs-per-gpu", type=int, default=ENVS_PER_GPU)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-second-window", action="store_true",
                    help="skip the default_regime window (ticks 200..400): profiling passes, whose per-kernel averages must "
                         "describe the headline window's launches only (tools/measure_round.sh)")
    ap.add_argument("--no-pick-place", action="store_true",
                    help="skip the second leg (configs[2]: one scripted pick + place per env through mre_run_controller)")
    ap.add_argument("--pick-place-only", action="store_true", help="profiling passes: run only the configs[2] leg")
    ap.add_argument("--fused", type=int, default=0,
                    help="control ticks per kernel launch; 0 (default) = the library's cut of the window handed over in one call: queue "
                         "launches (persistent waves, the env furthest behind first: include/mre.h mre_get_queue_info) when the batch "
                         "exceeds the GPU's wave slots, else one launch; 1 = one launch per tick and env group (rounds 1-5)")
    ap.add_argument("--solver", choices=["both", "PGS", "Newton"], default="both",
                    help="both (default): Newton is the headline line (MuJoCo's default, what the reference runs, and the "
                         "path whose parity tests hold north_star's bar); with --full, north_star's PGS <= 100 sweeps is timed "
                         "on the same start state and actions and printed beside it in `pgs` / `value_by_solver`")
    ap.add_argument("--full", action="store_true",
                    help="every measurement beside the headline window: PGS next to Newton, the per-tick launches, the "
                         "default_regime window, the pick_place leg, the CPU baseline with counted FLOPs and the MuJoCo probe "
                         "(each still subject to the --no-* options)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the headline window's final state (qpos, qvel as float64, status as float32) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_ranks(args))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    # rehearsal knobs (1-GPU box): MRE_BENCH_DEVICE pins every rank to one device and
    # MRE_BENCH_BACKEND=gloo replaces RCCL (two ranks cannot share a device under RCCL)
    backend = os.environ.get("MRE_BENCH_BACKEND", "nccl")
    if "MRE_BENCH_DEVICE" in os.environ:
        local_rank = int(os.environ["MRE_BENCH_DEVICE"])
    torch.cuda.set_device(local_rank)
    # MRE_BENCH_FORCE_DIST=1 (under torch.distributed.run --nproc-per-node 1): the multi-rank code path -- RCCL init
    # bound to the device, barriers, the device-tensor all_gather_into_tensor, the MAX all_reduce of the time -- with a
    # world of one, so that those lines have run on a GPU before the first 8-GPU job (tests/test_gpu_api.py)
    dist_on = world > 1 or os.environ.get("MRE_BENCH_FORCE_DIST") == "1"
    if dist_on:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)

    from mujoco_robot_environments_amd import rng
    from mujoco_robot_environments_amd.physics import BatchedPhysics
    n_local = args.envs_per_gpu
    if args.pick_place_only:
        solver = "Newton" if args.solver == "both" else args.solver
        print(json.dumps({"metric": baseline_metric(), "pick_place": pick_place_leg(n_local, local_rank, solver)}))
        return
    env_ids = np.arange(rank * n_local, (rank + 1) * n_local)  # global ids: results independent of sharding
    phys = BatchedPhysics(n_local, device=local_rank)
    nprops, _ = setup_envs(phys, args.seed, env_ids)
    qp0, qv0 = phys.get_state()
    ws0 = phys.get_warmstart()

    K, W, F = args.steps, args.warmup, max(0, args.fused)
    assert F == 0 or (K % F == 0 and W % F == 0), "--fused must divide --steps and --warmup"
    acts = rng.random_actions(args.seed, env_ids, np.arange(W + K)).astype(np.float32)
    seq = torch.from_numpy(acts).to(phys.device).contiguous()  # resident in HBM before timing
    bytes_per_tick = algorithmic_bytes_per_env_step(nprops) * n_local * CONTROL_STEPS   # one control tick of the whole batch
    total_env_steps = world * n_local * K * CONTROL_STEPS
    pmc = (F == 0 and n_local == ENVS_PER_GPU)   # (the committed counter passes describe the default cut)

    second_window = args.full and not args.no_second_window
    K2, W2 = 200, 200   # the second window of every --full run: ticks 200 .. 400, the heavy regime
    need = max(W + K, W2 + K2) if second_window else (W + K)
    if acts.shape[0] < need:
        acts2 = rng.random_actions(args.seed, env_ids, np.arange(need)).astype(np.float32)
        seq_all = torch.from_numpy(acts2).to(phys.device).contiguous()
    else:
        seq_all = seq

    outputs = {}

    def run(solver):
        phys.set_solver(solver)
        phys.reset()
        phys.set_state(qp0, qv0)
        phys.set_warmstart(ws0)
        phys.sync()
        elapsed, kern_ms, launches, gather_ms = timed_run(phys, seq, K, W, F, world, backend, dist, torch, n_local, dist_on)
        if args.dump_outputs and not outputs:
            # the headline window's result as its caller reads it back, before any other leg touches the state
            qpos, qvel = phys.get_state_f64()
            outputs.update(qpos=qpos, qvel=qvel, status=phys.status().astype(np.float32))
        q0 = timed_run.queue0
        status, stats = phys.status(), phys.solver_stats()
        fb = phys.fallback_stats()
        q1 = phys.queue_info()
        queue = q1["launches"] > q0["launches"]
        avg_launch_s = (kern_ms / max(launches, 1)) * 1e-3
        if queue:
            # queue launches (csrc/mre_api.cpp, mre_env::qgroup): ONE launch covers all envs and up to 200 control ticks;
            # its persistent waves take the env furthest behind, one tick at a time.  Launches do not overlap.
            per_tick = launches / float(K)
            envs_per_launch, ticks_per_launch = n_local, K / float(max(launches, 1))
            kname = "mre::k_step_queue" if solver == "PGS" else "mre::k_step_queue_newton"
        else:
            # the library steps the batch as env groups on separate streams (launches of different groups overlap on
            # the GPU, csrc/mre_api.cpp launch_step): one tick = `per_tick` launches of N / per_tick envs each
            per_tick = max(1, round(launches / max(K // max(F, 1), 1)))
            envs_per_launch, ticks_per_launch = n_local // per_tick, float(max(F, 1))
            kname = "mre::k_step" if solver == "PGS" else "mre::k_step_newton"
        bytes_per_launch = bytes_per_tick * (envs_per_launch / float(n_local)) * ticks_per_launch
        wall_per_launch_s = elapsed / max(launches, 1)
        # the group launches of a tick (and of consecutive ticks) overlap on the GPU, so their individual durations
        # are not additive: the bandwidth the path achieves is the window's algorithmic bytes over the window's wall time
        # (= bytes per launch over wall time per launch); the per-launch form is kept beside it.  Queue launches do not
        # overlap: the two agree up to the host's gap between launches.
        achieved = bytes_per_launch / wall_per_launch_s / 1e9
        achieved_per_launch = bytes_per_launch / avg_launch_s / 1e9
        # counter-derived figures only from passes taken at these arguments on these sources (else null + the reason)
        summ, summ_name = pmc_summary(solver, K, W) if pmc else (None, "counters describe the default cut (--fused 0) at 4096 envs per GPU")
        if summ is not None and summ.get("kernel") != kname:
            summ, summ_name = None, f"{summ_name} describes {summ.get('kernel')}, this run's kernel is {kname}"
        traffic = occ = None
        wait_note = ""
        if summ is not None:
            traffic = summ.get("traffic_bytes_per_launch")
            scale = envs_per_launch * ticks_per_launch / (float(summ.get("envs_per_launch", ENVS_PER_GPU)) * float(summ.get("ticks_per_launch", 1)))
            if traffic is not None:
                traffic *= scale
            occ = issue_occupancy(summ, summ_name, wall_per_launch_s, envs_per_launch, ticks_per_launch)
            if summ.get("SQ_WAIT_ANY_per_launch") and summ.get("SQ_WAVE_CYCLES_per_launch"):
                wait_note = (f"; waves parked in s_waitcnt {100.0 * summ['SQ_WAIT_ANY_per_launch'] / summ['SQ_WAVE_CYCLES_per_launch']:.0f} % "
                             f"of their cycles (SQ_WAIT_ANY / SQ_WAVE_CYCLES, {summ_name})")
        # the same start state and ticks stepped the old way -- one launch per tick and env group (rounds 1-5) -- beside
        # the headline: what the queue launches are worth, measured in this very run
        per_tick_leg = None
        if queue and second_window:
            phys.reset()
            phys.set_state(qp0, qv0)
            phys.set_warmstart(ws0)
            phys.sync()
            elp, _, lp, _ = timed_run(phys, seq, K, W, 1, world, backend, dist, torch, n_local, dist_on, gather=False)
            per_tick_leg = {"value": total_env_steps / elp, "ms_per_step": elp / K * 1e3, "launches": lp,
                            "note": "one launch per tick and env group (--fused 1: the scheme of rounds 1-5), same start state, same ticks; "
                                    "final states are bit-identical to the headline's (tests/test_gpu_properties.py)"}
        # the same start state again, timed over ticks 200 .. 400 (no gather, no counters: a second clock on the workload)
        second = None
        if second_window:
            phys.reset()
            phys.set_state(qp0, qv0)
            phys.set_warmstart(ws0)
            phys.sync()
            el2, kern2, launches2, _ = timed_run(phys, seq_all, K2, W2, F, world, backend, dist, torch, n_local, dist_on, gather=False)
            st2 = phys.solver_stats()
            second = {"ticks": f"{W2}:{W2 + K2}", "value": world * n_local * K2 * CONTROL_STEPS / el2,
                      "ms_per_step": el2 / K2 * 1e3, "avg_launch_ms": kern2 / max(launches2, 1),
                      "mean_ncon": float(st2[:, 0].mean()), "mean_nefc": float(st2[:, 1].mean()),
                      "mean_solver_iters": float(st2[:, 2].mean()),
                      "note": "same start state and action stream, ticks 200..400: arms on the table, cubes knocked about"}
        return {
            "solver": solver, "value": total_env_steps / elapsed, "ms_per_step": elapsed / K * 1e3, "gather_ms": gather_ms,
            "default_regime": second, "per_tick_launches": per_tick_leg,
            "queue": {"in_use": queue, "launches": q1["launches"] - q0["launches"], "waves": q1["waves"],
                      "handovers": q1["handovers"] - q0["handovers"],
                      "note": "envs a queue launch handed to the large kernel's waves itself (capacity fallback inside the launch)"},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                         "traffic": traffic, "traffic_source": summ_name if summ is not None else None,
                         "kernel": kname, "avg_launch_ms": avg_launch_s * 1e3, "launches": launches,
                         "launches_per_tick": per_tick, "envs_per_launch": envs_per_launch, "ticks_per_launch": ticks_per_launch,
                         "algorithmic_bytes_per_launch": bytes_per_launch,
                         "wall_ms_per_launch": wall_per_launch_s * 1e3,
                         "achieved_per_overlapping_launch": achieved_per_launch,
                         "issue_occupancy": occ, "issue_occupancy_unavailable": None if occ is not None else summ_name,
                         "launch_note": ("a launch is one QUEUE launch: all envs, `ticks_per_launch` control ticks, persistent waves "
                                         "(csrc/mre_kernels.hip step_body<QUEUE>); avg_launch_ms is its own duration (HIP events on its stream; "
                                         "rocprofv3 --stats agrees), wall_ms_per_launch the window's wall time per launch; the large kernel's "
                                         "few waves (k_step_queue_large) run beside it for the envs that outgrow the compact capacities")
                                        if queue else
                                        ("a tick is stepped as `launches_per_tick` env-group launches on prioritised streams that "
                                         "overlap each other and the next tick's (csrc/mre_api.cpp launch_step): avg_launch_ms is one "
                                         "group launch's own duration (HIP events; rocprofv3 --stats agrees), wall_ms_per_launch the "
                                         "window's wall time divided by its launches; achieved / frac use the wall time"),
                         "note": ("HBM is not what limits this path (SURVEY 8d): an env's state stays in LDS across the 5 fused steps and "
                                  "the algorithmic traffic is < 1e-2 of peak by construction. " +
                                  ("PGS: VALU issue inside the 100 fixed sweeps (issue_occupancy)" if solver == "PGS" else
                                   "Newton: dependent LDS round trips at 2 waves / SIMD (issue_occupancy)") + wait_note +
                                  "; flop = algorithmic work counted on the CPU restatement against the FP32 vector peak")},
            "health": {"nan_envs": int(((status & 2) != 0).sum()), "overflow_envs": int(((status & 4) != 0).sum()),
                       "mean_ncon": float(stats[:, 0].mean()), "mean_nefc": float(stats[:, 1].mean()),
                       "mean_solver_iters": float(stats[:, 2].mean()), "max_solver_iters": int(stats[:, 2].max()),
                       "solver_iters_histogram": np.bincount(np.minimum(stats[:, 2], 10), minlength=11).tolist(),
                       "capacity_fallback": fb},
        }

    order = (["Newton", "PGS"] if args.full else ["Newton"]) if args.solver == "both" else [args.solver]
    runs = {s: run(s) for s in order}
    head = runs[order[0]]
    if args.dump_outputs:
        # one set per rank (its own global env ids): a multi-rank job writes <name>_rank<r>.npy
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, a in outputs.items():
            np.save(os.path.join(args.dump_outputs, name + ("" if world == 1 else f"_rank{rank}") + ".npy"), a)
    res = {
        "metric": baseline_metric(),
        "value": head["value"], "unit": "env-steps/s", "n_gpus": world, "steps": K, "warmup": W,
        "ms_per_step": head["ms_per_step"], "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "configs[1]: 4096 parallel RearrangementEnv per GPU (2-4 cubes), random "
                   "actions every 5 ms tick, 5 x 1 ms physics steps per bench step",
                   "envs_per_gpu": n_local, "control_steps": CONTROL_STEPS,
                   "ticks_per_launch": F if F > 0 else "library's cut of the window (one call): " + (
                       f"queue launches of {head['roofline']['ticks_per_launch']:.0f} ticks" if head["queue"]["in_use"] else
                       "one launch per tick and env group (a window shorter than 32 ticks: csrc/mre_api.cpp queue_min_ticks)"),
                   "solver": ("PGS<=100 sweeps, tol 1e-8 (north_star)" if head["solver"] == "PGS"
                              else "Newton<=100 iterations, tol 1e-8 (MuJoCo's default: what the reference runs, "
                                   "tasks/rearrangement.py:77-80 sets no solver)"),
                   "solver_note": "the headline is the solver whose parity tests hold north_star's bar (1e-4 on all 43 qpos "
                                  "coordinates over 1000 steps) as a hard assertion in 64 / 64 envs; north_star's PGS <= 100 sweeps "
                                  "is timed on the same start state and actions in `pgs` with --full (63 / 64: DESIGN.md section 7)",
                   "integrator": "implicitfast"},
        "control_ticks_per_s": head["value"] / CONTROL_STEPS,
        "pick_place_macro_steps_per_s": head["value"] / 18000.0,
        "roofline": head["roofline"], "default_regime": head["default_regime"], "health": head["health"],
        "queue": head["queue"], "per_tick_launches": head["per_tick_launches"],
        "gather_ms": head["gather_ms"],
        # which solver `value` is, and both solvers' numbers at the top level: the step from BENCH_r03 (PGS headline,
        # 5.34 M at --steps 20 --warmup 5 / 4.65 M default) to BENCH_r04 (Newton headline) was a solver switch, not a
        # speed-up; PGS itself LOST 4 % / 21 % in round 4 to the fp64 block update of robot contacts
        "headline_solver": head["solver"],
        "value_by_solver": {s_: r_["value"] for s_, r_ in runs.items()},
        "default_regime_by_solver": {s_: (r_["default_regime"] or {}).get("value") for s_, r_ in runs.items()},
    }
    for s_, key in (("PGS", "pgs"), ("Newton", "newton")):
        if s_ in runs and runs[s_] is not head:
            res[key] = runs[s_]
    if rank == 0 and world == 1 and args.full and not args.no_pick_place:
        phys.close()
        try:
            res["pick_place"] = pick_place_leg(n_local, local_rank, order[0])
            if res["pick_place"].get("queue_launches") and not args.no_second_window:
                # the same leg with the launches of rounds 1-5 (50 ticks per env group, overflow -> host re-run), in this run
                prev = os.environ.get("MRE_QUEUE")
                os.environ["MRE_QUEUE"] = "0"
                try:
                    old = pick_place_leg(n_local, local_rank, order[0])
                finally:
                    if prev is None:
                        del os.environ["MRE_QUEUE"]
                    else:
                        os.environ["MRE_QUEUE"] = prev
                res["pick_place"]["without_queue_launches"] = {k: old[k] for k in ("value", "seconds", "capacity_fallback", "all_phases_converged_frac",
                                                                                    "envs_done_after_the_pair")}
        except Exception as e:  # the headline line must still be printed
            res["pick_place"] = {"error": f"{type(e).__name__}: {e}"}
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(args.seed)
        flops = counted_flops(args.seed, [(W, W + K)] + ([] if args.no_second_window else [(W2, W2 + K2)]))
        res["cpu_baseline"]["counted_flops"] = flops
        for s_, r_ in runs.items():
            attach_flop_roofline(r_, flops, s_, f"{W}:{W + K}", n_local)
        probe = mujoco_probe(args.seed)
        res["mujoco"] = probe["mujoco"]          # version string, or null: MuJoCo is not on this host
        res["mujoco_probe"] = probe
    elif rank == 0:
        res["cpu_baseline"] = None
        res["mujoco"] = None
    if dist_on:
        res["distributed"] = {"backend": backend, "world": world, "gathered_rows": world * n_local}
    if rank == 0:
        print(json.dumps(res))
    if dist_on:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
