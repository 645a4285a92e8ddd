"""Episode-shard logging rate: the host encoder against the device encoder, same process, same seeded episodes.

    python tools/bench_shards.py [--num-envs 1024] [--max-steps 2] [--repeats 1] [--host-envs K] [--no-read]

Runs BatchedRearrangementEnv(render=True) for --max-steps pick / place pairs with EVERY env logged, once per path and
repeat, alternating host, device, host, ...:
  host    the observations are handed to BatchedEpisodeLogger as numpy arrays (one device-to-host copy of the batch,
          outside the clock): dataset.py encodes every byte on the host -- the logger as it was before the device path
  device  the CUDA tensors are handed over: csrc/mre_records.hip packs and checksums, the host frames and writes
The clock is a host clock around reset() / step() of the logger (each followed by a device synchronise) and around
flush() + close().  --host-envs limits the HOST path to the first K envs when all of them would take too long; rates
are per byte written, so they stay comparable.  Prints one JSON line.

Read leg (after the write legs, same process): the device path's directory is written once more and read back with
dataset.read_episodes (host: every byte parsed in Python / numpy) and dataset.read_episodes_device (the file goes to the
device once, csrc/mre_records.hip unpacks the rgb lists and checks the CRCs), alternating host, device, ... --repeats
times (at least 3).  --host-envs limits the HOST reader to the first K episodes; rates are per shard byte read (record
framing included), so they stay comparable.  A host clock around each whole read; the device reader's tensors are each
consumed by a device reduction, with one synchronise at the end.  read.kernel_ms is from device events around the unpack
and the CRC launches of a run of its own (the events are not in the timed runs); read.hbm_frac is the bytes those kernels
must move -- the packed rgb read twice (count, unpack), the unpacked rgb written once, every payload read once for its
CRC -- over that time, against the same 8.0 TB/s.

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


def _shard_bytes(directory: str, episodes=None):
    """(bytes of the shard files, episodes in them); with `episodes`, of the first shards that hold that many."""
    from mujoco_robot_environments_amd import dataset as D
    total = count = 0
    for n in sorted(os.listdir(directory)):
        if "tfrecord" not in n:
            continue
        recs = list(D.scan_records(os.path.join(directory, n)))
        for _, length, _ in recs:
            if episodes is not None and count >= episodes:
                return total, count
            total += D.record_bytes(length)
            count += 1
    return total, count


def read_leg(directory: str, args) -> dict:
    import itertools
    import torch
    from mujoco_robot_environments_amd import dataset as D
    all_bytes, episodes = _shard_bytes(directory)
    k_host = episodes if args.host_envs is None else min(episodes, args.host_envs)
    host_bytes, _ = _shard_bytes(directory, k_host)

    def host_read():
        t = time.perf_counter()
        acc = 0
        for ep in itertools.islice(D.read_episodes(directory), k_host):
            obs = ep["steps"]["observation"]
            acc += int(obs["overhead_camera/rgb"].sum()) + int(obs["overhead_camera/depth"].shape[0])
        return time.perf_counter() - t, acc

    def device_read(timer=None):
        torch.cuda.synchronize()
        t = time.perf_counter()
        acc = torch.zeros((), dtype=torch.float64, device="cuda")
        frames = 0
        for ep in D.read_episodes_device(directory, timer=timer):
            obs = ep["steps"]["observation"]
            acc += obs["overhead_camera/rgb"].sum() + obs["overhead_camera/depth"].sum()
            frames += int(obs["overhead_camera/rgb"].shape[0])
        torch.cuda.synchronize()
        return time.perf_counter() - t, frames

    device_read()                                              # warm-up: pinned memory, the allocator, the code objects
    repeats = max(3, args.repeats)
    t_host, t_dev, frames = [], [], 0
    for _ in range(repeats):
        t_host.append(host_read()[0])
        t, frames = device_read()
        t_dev.append(t)
    timer = D.ReadTimer()
    device_read(timer)
    ms_unpack, ms_crc = timer.kernel_ms()
    must_move = 2 * timer.packed_bytes + timer.unpacked_bytes + timer.crc_bytes
    ms = ms_unpack + ms_crc
    # where the device reader's time goes, one more pass in pieces: the file read alone, the upload alone
    names = sorted(n for n in os.listdir(directory) if "tfrecord" in n)
    biggest = max(os.path.getsize(os.path.join(directory, n)) for n in names)
    pinned = torch.empty(biggest, dtype=torch.uint8, pin_memory=True)
    dev = torch.empty(biggest, dtype=torch.uint8, device="cuda")
    t_file = t_up = 0.0
    for n in names:
        t = time.perf_counter()
        with open(os.path.join(directory, n), "rb") as f:
            got = f.readinto(pinned.numpy())
        t_file += time.perf_counter() - t
        t = time.perf_counter()
        dev[:got].copy_(pinned[:got], non_blocking=True)
        torch.cuda.synchronize()
        t_up += time.perf_counter() - t
    return {"episodes": episodes, "frames": frames, "shard_bytes": all_bytes, "host_episodes": k_host,
            "host_shard_bytes": host_bytes, "repeats": repeats,
            "host_gb_s": host_bytes / min(t_host) / 1e9, "device_gb_s": all_bytes / min(t_dev) / 1e9,
            "host_gb_s_all": [host_bytes / x / 1e9 for x in t_host], "device_gb_s_all": [all_bytes / x / 1e9 for x in t_dev],
            "host_seconds": t_host, "device_seconds": t_dev,
            "kernel_ms": ms, "kernel_ms_unpack": ms_unpack, "kernel_ms_crc": ms_crc,
            "kernel_bytes_must_move": must_move, "hbm_frac": must_move / (ms * 1e-3) / HBM_PEAK,
            "hbm_frac_unpack": (2 * timer.packed_bytes + timer.unpacked_bytes) / (ms_unpack * 1e-3) / HBM_PEAK,
            "hbm_frac_crc": timer.crc_bytes / (ms_crc * 1e-3) / HBM_PEAK,
            "device_seconds_file_read_alone": t_file, "device_seconds_upload_alone": t_up,
            "hbm_peak_GB_per_s": HBM_PEAK / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--max-steps", type=int, default=2, help="pick / place pairs per episode")
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--host-envs", type=int, default=None, help="host path: log the first K envs only")
    ap.add_argument("--no-read", action="store_true", help="skip the read leg")
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
    read = None
    if not args.no_read:
        d = tempfile.mkdtemp(prefix="shards_read_", dir=args.dir)
        try:
            run("device", args, d)
            read = read_leg(d, args)
        finally:
            shutil.rmtree(d, ignore_errors=True)
    print(json.dumps({"metric": "episode-shard logging rate, device encode over host encode", "unit": "x",
                      "value": best["device"]["GB_per_s"] / best["host"]["GB_per_s"],
                      "num_envs": args.num_envs, "max_steps": args.max_steps, "repeats": args.repeats,
                      "host": best["host"], "device": best["device"], "read": read,
                      "seconds_all_runs": {p: [x["seconds"] for x in r] for p, r in runs.items()}}))


if __name__ == "__main__":
    main()
