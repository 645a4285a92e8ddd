"""Episode-shard logging rate: the host encoder against the device encoder, same process, same seeded episodes.

    python tools/bench_shards.py [--num-envs 1024] [--max-steps 2] [--repeats 1] [--host-envs K]

Runs BatchedRearrangementEnv(render=True) for --max-steps pick / place pairs with EVERY env logged, once per path and
repeat, alternating host, device, host, ...:
  host    the observations are handed to BatchedEpisodeLogger as numpy arrays (one device-to-host copy of the batch,
          outside the clock): dataset.py encodes every byte on the host -- the logger as it was before the device path
  device  the CUDA tensors are handed over: csrc/mre_records.hip packs and checksums, the host frames and writes
The clock is a host clock around reset() / step() of the logger (each followed by a device synchronise) and around
flush() + close().  --host-envs limits the HOST path to the first K envs when all of them would take too long; rates
are per byte written, so they stay comparable.  Prints one JSON line.

Kernel share of HBM peak (device path): the bytes the encode kernels must move per frame -- the rgb row read twice
(count, pack), its packed length written, the depth row read -- over the kernel time from device events, against the
8.0 TB/s of MI355X_MICROARCH.md.  The logger's sizing pass reads the rgb rows once more than that; its time is inside
the kernel time, its bytes are not in the numerator.
"""
import argparse
import collections
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
TimeStep = collections.namedtuple("TimeStep", ["step_type", "reward", "discount", "observation"])


def run(path: str, args, out_dir: str) -> dict:
    import torch
    from mujoco_robot_environments_amd import dataset as D
    from mujoco_robot_environments_amd.tasks.rearrangement import BatchedRearrangementEnv, colour_separator_task_config
    N = args.num_envs
    cfg = colour_separator_task_config()
    env = BatchedRearrangementEnv(cfg=cfg, num_envs=N, seed=args.seed, solver="Newton", render=True)
    H, W = env.overhead_camera_height, env.overhead_camera_width
    cam = "overhead_camera/overhead_camera"
    writer = D.EpisodeWriter(out_dir, "colour_splitter", H, W, max_episodes_per_file=cfg.dataset.max_episodes_per_file)
    logged = N if path == "device" or args.host_envs is None else min(N, args.host_envs)

    class FirstEnvs:   # what the logger asks of its env, for the first `logged` envs (--host-envs; otherwise all)
        num_envs = logged
        get_camera_metadata = staticmethod(env.get_camera_metadata)

    ts = env.reset()
    FirstEnvs.placement_failed = env.placement_failed[:logged]
    log = D.BatchedEpisodeLogger(FirstEnvs(), writer, time_kernels=(path == "device"))

    def hand_over(ts):
        if path == "device":
            return ts
        o = ts.observation
        return TimeStep(ts.step_type, ts.reward, ts.discount,
                        {k: o[k][:logged].cpu().numpy() for k in ("overhead_camera/rgb", "overhead_camera/depth")})

    t_steps = 0.0

    def timed(fn, *a):
        nonlocal t_steps
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn(*a)
        torch.cuda.synchronize()
        t_steps += time.perf_counter() - t

    timed(log.reset, hand_over(ts))
    frames = int(log.mask.sum())
    for _ in range(args.max_steps):
        in_progress, pick, place = env.sort_colours()
        for pose in (pick, place):
            a = {"pose": pose.copy(), "pixel_coords": env.world_2_pixel(cam, pose[:, :3]), "gripper_rot": 0.0}
            ts = env.step(a)
            active = in_progress[:logged]
            a = {k: (v[:logged] if isinstance(v, np.ndarray) else v) for k, v in a.items()}
            timed(log.step, a, hand_over(ts), active)
            frames += int((log.mask & active).sum())
    kernel_ms = log.kernel_ms() if path == "device" else None
    t = time.perf_counter()
    log.flush()
    info = writer.close()
    t_flush = time.perf_counter() - t
    env.close()
    nbytes = int(info["splits"][0]["numBytes"])
    res = {"envs_logged": logged, "frames": frames, "bytes_written": nbytes, "seconds": t_steps + t_flush,
           "seconds_in_reset_and_step": t_steps, "seconds_in_flush_and_close": t_flush,
           "GB_per_s": nbytes / (t_steps + t_flush) / 1e9, "frames_encoded_on_device": log.frames_encoded_on_device}
    if path == "device":
        rb, db = H * W * 3, H * W * 4
        packed = nbytes - frames * db            # all but the depth bytes (and a few hundred bytes per episode) is packed rgb
        must_move = 2 * frames * rb + packed + frames * db
        res.update({"kernel_ms_total": kernel_ms, "kernel_us_per_frame": 1e3 * kernel_ms / frames,
                    "kernel_bytes_must_move": must_move, "kernel_GB_per_s": must_move / (kernel_ms * 1e-3) / 1e9,
                    "kernel_frac_of_hbm_peak": must_move / (kernel_ms * 1e-3) / HBM_PEAK, "hbm_peak_GB_per_s": HBM_PEAK / 1e9,
                    "seconds_copy_and_host_in_step": t_steps - kernel_ms * 1e-3, "host_memory_pinned": log._arena.pin})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--max-steps", type=int, default=2, help="pick / place pairs per episode")
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--host-envs", type=int, default=None, help="host path: log the first K envs only")
    ap.add_argument("--dir", default=None, help="where the shards go (default: a temporary directory); removed afterwards")
    args = ap.parse_args()
    runs = {"host": [], "device": []}
    for _ in range(args.repeats):
        for path in ("host", "device"):
            d = tempfile.mkdtemp(prefix=f"shards_{path}_", dir=args.dir)
            try:
                runs[path].append(run(path, args, d))
            finally:
                shutil.rmtree(d, ignore_errors=True)
    best = {p: min(r, key=lambda x: x["seconds"]) for p, r in runs.items()}
    print(json.dumps({"metric": "episode-shard logging rate, device encode over host encode", "unit": "x",
                      "value": best["device"]["GB_per_s"] / best["host"]["GB_per_s"],
                      "num_envs": args.num_envs, "max_steps": args.max_steps, "repeats": args.repeats,
                      "host": best["host"], "device": best["device"],
                      "seconds_all_runs": {p: [x["seconds"] for x in r] for p, r in runs.items()}}))


if __name__ == "__main__":
    main()
