"""Bad calls of the handle entries of the C ABI on a LIVE handle, for tests/test_gpu_handle_refusals.py and
tests/golden/make_handle_records.py: every value check that an entry makes after it has found its handle, what it answers
(return code and mre_last_error() text) and in which order the checks come.

The handle holds 3 envs and has not settled anything yet (mre_get_settle_steps).  Every entry with more than one check gets
one call that is wrong in two ways; mre_set_fallback, mre_set_solver, mre_step and mre_pack_final_state have a single check
after the NULL checks of tests/handle_null_cases.py.  The last row is one mre_step(e, 1, 0): after all the refusals the
handle still steps.
"""
import ctypes as C

import numpy as np
import torch

N = 3
INF, NAN = float("inf"), float("nan")
CAM_POS = np.array([0.45, 0.0, 1.6], np.float32)
CAM_MAT = np.eye(3, dtype=np.float32).reshape(-1)


def cases(h):
    """[(id, entry point, argument tuple)] for the live handle ``h``, in a fixed order, and what keeps the buffers alive"""
    dev = lambda nbytes: torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")
    host = lambda nbytes: np.zeros(nbytes + 64, np.uint8)
    keep = dict(d_rgb=dev(N * 4 * 8 * 3), d_depth=dev(N * 4 * 8 * 4), d_seg=dev(N * 4 * 8), d_out=dev(N * 128 * 4),
                d_seq=dev(4 * N * 8 * 4), d_trace=dev(10 * N * 88 * 4), h_any=host(1 << 14), pos=CAM_POS, mat=CAM_MAT)
    d = {k: v.data_ptr() for k, v in keep.items() if k.startswith("d_")}
    assert all(p % 16 == 0 for p in d.values())
    H = keep["h_any"].ctypes.data
    pos, mat = CAM_POS.ctypes.data, CAM_MAT.ctypes.data
    out = []

    def table(entry, names, good, bad):
        for what, kw in bad:
            assert set(kw) <= set(names), (entry, what)
            out.append((f"{entry}: {what}", entry, (h,) + tuple({**good, **kw}[k] for k in names)))

    table("mre_render", ["cam_pos", "cam_mat", "fovy", "height", "width", "rgb", "depth", "seg", "mask"],
          dict(cam_pos=pos, cam_mat=mat, fovy=45.0, height=4, width=8, rgb=d["d_rgb"], depth=d["d_depth"], seg=d["d_seg"], mask=None), [
        ("width 6", dict(width=6)), ("width 1284", dict(width=1284)), ("height 0", dict(height=0)), ("fovy 0", dict(fovy=0.0)),
        ("fovy 180", dict(fovy=180.0)), ("host rgb", dict(rgb=H)), ("host depth", dict(depth=H)), ("host seg", dict(seg=H)),
        ("depth misaligned", dict(depth=d["d_depth"] + 4)), ("rgb misaligned", dict(rgb=d["d_rgb"] + 1)),
        ("seg misaligned", dict(seg=d["d_seg"] + 2)),
        ("two: height 0 and host rgb", dict(height=0, rgb=H)), ("two: host seg and depth misaligned", dict(seg=H, depth=d["d_depth"] + 4)),
        ("two: depth misaligned and rgb misaligned", dict(depth=d["d_depth"] + 8, rgb=d["d_rgb"] + 2)),
        ("two: null cam_pos and width 6", dict(cam_pos=None, width=6)),
    ])
    table("mre_set_fallback", ["mode"], {}, [("mode 3", dict(mode=3)), ("mode -1", dict(mode=-1))])
    table("mre_set_solver", ["solver"], {}, [("solver 1", dict(solver=1))])
    table("mre_get_arm_dynamics", ["site", "out"], dict(site=0, out=d["d_out"]), [
        ("site 2", dict(site=2)), ("host pointer", dict(out=H)), ("out off by 4 bytes", dict(out=d["d_out"] + 4)),
        ("two: site 2 and host pointer", dict(site=2, out=H)), ("two: null out and site -1", dict(site=-1, out=None)),
    ])
    table("mre_pack_final_state", ["out"], {}, [("host pointer", dict(out=H))])
    table("mre_rollout_ticks", ["ctrl_seq", "nticks", "control_steps", "flags", "ticks_per_launch"],
          dict(ctrl_seq=d["d_seq"], nticks=4, control_steps=5, flags=0, ticks_per_launch=2), [
        ("host pointer", dict(ctrl_seq=H)), ("control_steps 0", dict(control_steps=0)), ("nticks -1", dict(nticks=-1)),
        ("two: control_steps 0 and host pointer", dict(control_steps=0, ctrl_seq=H)),
    ])
    table("mre_rollout", ["ctrl_seq", "nticks", "control_steps", "flags"],
          dict(ctrl_seq=d["d_seq"], nticks=4, control_steps=5, flags=0), [("host pointer", dict(ctrl_seq=H))])
    table("mre_step", ["nsubsteps", "flags"], dict(flags=0), [("nsubsteps -1", dict(nsubsteps=-1))])
    table("mre_set_trace", ["out", "nenv", "max_steps"], dict(out=d["d_trace"], nenv=N, max_steps=10), [
        ("nenv 0", dict(nenv=0)), ("nenv N + 1", dict(nenv=N + 1)), ("max_steps 0", dict(max_steps=0)), ("host buffer", dict(out=H)),
        ("two: host buffer and nenv 0", dict(out=H, nenv=0)), ("two: nenv 0 and max_steps 0", dict(nenv=0, max_steps=0)),
    ])
    gains = np.tile(np.array([350, 20, 500, 100, 200, 30], np.float32), (N, 1))

    def bad_gains(**at):
        g = gains.copy()
        for k, v in at.items():
            g[int(k[1]), int(k[2])] = v
        keep[f"gains{len(keep)}"] = g
        return g.ctypes.data
    table("mre_osc_configure_env", ["gains", "null_q", "thr"], dict(null_q=None, thr=None), [
        ("a negative gain", dict(gains=bad_gains(g12=-1.0))), ("an infinite gain", dict(gains=bad_gains(g20=INF))),
        ("a NaN gain", dict(gains=bad_gains(g05=NAN))), ("two: a NaN gain and a negative gain", dict(gains=bad_gains(g01=NAN, g23=-2.0))),
    ])
    table("mre_get_settle_steps", ["steps"], {}, [("before any settle", dict(steps=H)),
                                                  ("two: null steps before any settle", dict(steps=None))])
    table("mre_place_props", ["mask", "seed", "ws_min", "ws_max", "max_attempts", "settle_steps"],
          dict(mask=None, seed=7, ws_min=H, ws_max=H + 64, max_attempts=100, settle_steps=0), [
        ("max_attempts 0", dict(max_attempts=0)), ("two: max_attempts 0 and null ws_max", dict(max_attempts=0, ws_max=None)),
    ])
    table("mre_prop_place", ["seed", "prop", "bounds", "tick", "max_attempts", "max_dist", "pose", "attempts"],
          dict(seed=7, prop=H, bounds=H + 64, tick=H + 512, max_attempts=10, max_dist=0.05, pose=H + 1024, attempts=H + 2048), [
        ("max_attempts 0", dict(max_attempts=0)), ("two: max_attempts -1 and null pose", dict(max_attempts=-1, pose=None)),
    ])
    table("mre_sort_colours", ["seed", "call_counts", "zones", "max_attempts", "max_dist", "which", "pick", "place", "attempts"],
          dict(seed=7, call_counts=H, zones=H + 64, max_attempts=10, max_dist=0.05, which=H + 1024, pick=H + 2048, place=H + 3072,
               attempts=H + 4096), [
        ("max_attempts 0", dict(max_attempts=0)), ("two: max_attempts 0 and null which", dict(max_attempts=0, which=None)),
    ])
    table("mre_run_controller", ["nticks", "control_steps", "converged_out"], dict(nticks=6, control_steps=5, converged_out=None), [
        ("nticks -1", dict(nticks=-1)), ("control_steps 0", dict(control_steps=0)),
        ("two: nticks -1 and control_steps 0", dict(nticks=-1, control_steps=0)),
    ])
    out.append(("mre_step: one step after the refusals", "mre_step", (h, 1, 0)))
    assert len({c[0] for c in out}) == len(out)
    return out, keep


def answers(L, blob):
    """[[id, return code, message]] of ``cases()`` on a fresh handle of the loaded library ``L``; a call that returns 0 sets
    no message, so its message is recorded as empty."""
    h = C.c_void_p()
    assert L.mre_create(blob, len(blob), N, 0, C.byref(h)) == 0, L.mre_last_error()
    try:
        table, keep = cases(h)
        res = []
        for what, entry, args in table:
            rc = int(getattr(L, entry)(*args))
            res.append([what, rc, L.mre_last_error().decode() if rc else ""])
        assert L.mre_sync(h) == 0, L.mre_last_error()
        del keep
        return res
    finally:
        L.mre_destroy(h)
