"""One fixed script over every handle entry of the C ABI (include/mre.h) that produces output, and ``digests(L, model, run)``,
which runs it on a loaded library and returns [label, CRC-32C (mre_crc32c) of the output's bytes] rows.  The record
tests/golden/handle_bytes.json is made by tests/golden/make_handle_records.py with the library of the commit BEFORE a change
to the host side of the handle entries: such a change touches no kernel and no launch argument, so it keeps every byte.

The script runs on a handle of 3 envs (odd, so that a wrong row stride shows) and on a handle of 1, with Newton and with
PGS (RUNS).  The PGS runs take the model with 10 sweeps per step instead of 100: under PGS resting cubes never pass the
settle test, so each settling placement goes through all of its ten rounds of 2 s of physics -- the path that rewinds the
clock and flags the envs, 20 000 steps at 0.75 ms with 100 sweeps.  Only bytes the ABI specifies are hashed: the pad
columns of qpos / qvel / warm-start rows are left out, contact rows count up to |count|, pick / place rows only where a cube
was selected and a pose found, mre_get_launch_info without its duration bits and mre_get_queue_info without the waves of
the card.  Images are 4 x 8 (and once 8 x 4, so that the cached background is reallocated), no call steps more than 6 ticks.
The script ends with placements that cannot succeed (one draw per cube; a workspace of a single point), so that the envs
dropped from a search and the MRE_ST_PLACEMENT_FAILED flag are in the record too.
"""
import ctypes as C

import numpy as np
import torch

MRE_SOLVER_PGS, MRE_SOLVER_NEWTON = 0, 2
# (id, envs, solver, opt_iterations of the model or None = as compiled)
RUNS = [("3 envs, Newton", 3, MRE_SOLVER_NEWTON, None), ("3 envs, PGS", 3, MRE_SOLVER_PGS, 10),
        ("1 env, Newton", 1, MRE_SOLVER_NEWTON, None), ("1 env, PGS", 1, MRE_SOLVER_PGS, 10)]
WS_MIN, WS_MAX = np.array([0.35, -0.4, 0.43], np.float32), np.array([0.55, 0.4, 0.435], np.float32)
CAM_A = (np.array([0.45, 0.0, 1.6], np.float32), np.eye(3, dtype=np.float32).reshape(-1), 45.0)
CAM_B = (np.array([0.5, 0.1, 1.4], np.float32), np.array([0, -1, 0, 1, 0, 0, 0, 0, 1], np.float32), 60.0)


class _Run:
    def __init__(self, L, h, n):
        self.L, self.h, self.n, self.rows, self.keep = L, h, n, [], []

    def call(self, entry, *args):
        rc = getattr(self.L, entry)(self.h, *args)
        assert rc == 0, (entry, rc, self.L.mre_last_error())

    def p(self, a):
        """the address of a host array (kept alive until the run ends)"""
        assert isinstance(a, np.ndarray) and a.flags["C_CONTIGUOUS"]
        self.keep.append(a)
        return a.ctypes.data

    def rec(self, label, a):
        raw = np.ascontiguousarray(a).tobytes()
        self.rows.append([label, int(self.L.mre_crc32c(raw, len(raw)))])

    def dev(self, shape, dtype, fill=0):
        t = torch.full(shape, fill, dtype=dtype, device="cuda")
        torch.cuda.synchronize()   # (the handle's stream is not torch's)
        self.keep.append(t)
        return t

    def read(self, t):
        self.call("mre_sync")
        return t.cpu().numpy()

    def state(self, tag):
        n = self.n
        q, v, w = np.zeros((n, 44), np.float32), np.zeros((n, 40), np.float32), np.zeros((n, 40), np.float32)
        q64, v64 = np.zeros((n, 43)), np.zeros((n, 39))
        c, t, st = np.zeros((n, 8), np.float32), np.zeros(n), np.zeros(n, np.uint32)
        self.call("mre_get_state", self.p(q), self.p(v))
        self.call("mre_get_state_f64", self.p(q64), self.p(v64))
        self.call("mre_get_warmstart", self.p(w))
        self.call("mre_get_ctrl", self.p(c))
        self.call("mre_get_time", self.p(t))
        self.call("mre_get_status", self.p(st))
        for name, a in (("qpos", q[:, :43]), ("qvel", v[:, :39]), ("qpos f64", q64), ("qvel f64", v64), ("warm start", w[:, :39]),
                        ("ctrl", c), ("time", t), ("status", st)):
            self.rec(f"{tag}: {name}", a)
        return q, v, q64, v64

    def telemetry(self, tag):
        n = self.n
        stats, info = np.zeros((n, 4), np.int32), np.zeros((n, 4), np.int32)
        fb, qi = (C.c_longlong * 4)(), (C.c_longlong * 5)()
        self.call("mre_get_solver_stats", self.p(stats))
        self.call("mre_get_launch_info", self.p(info))
        self.call("mre_get_fallback_stats", fb)
        self.call("mre_get_queue_info", qi)
        info[:, 1] &= 0xFFFF   # (the upper half is the env's duration)
        self.rec(f"{tag}: solver stats", stats)
        self.rec(f"{tag}: launch info", info)
        self.rec(f"{tag}: fallback stats", np.array(list(fb), np.int64))
        self.rec(f"{tag}: queue info", np.array([qi[0], qi[2], qi[3], qi[4]], np.int64))

    def place(self, tag, mask, seed, settle, max_attempts=100, ws=(WS_MIN, WS_MAX)):
        self.call("mre_place_props", None if mask is None else self.p(mask), seed, self.p(ws[0]), self.p(ws[1]), max_attempts, settle)
        self.state(tag)
        if settle > 0:
            steps = np.zeros(self.n, np.int32)
            self.call("mre_get_settle_steps", self.p(steps))
            self.rec(f"{tag}: settle steps", steps)

    def render(self, tag, cam, mask, height=4, width=8):
        n = self.n
        rgb = self.dev((n, height, width, 3), torch.uint8, 0xDE)
        depth, seg = self.dev((n, height, width), torch.float32, -1.0), self.dev((n, height, width), torch.uint8, 0xDE)
        self.call("mre_render", self.p(cam[0]), self.p(cam[1]), cam[2], height, width, rgb.data_ptr(), depth.data_ptr(),
                  seg.data_ptr(), None if mask is None else self.p(mask))
        for name, t in (("rgb", rgb), ("depth", depth), ("seg", seg)):
            self.rec(f"{tag}: {name}", self.read(t))


def _script(r):
    n, p = r.n, r.p
    rng = np.random.default_rng(20240 + n)
    m1, m2 = np.array([1, 0, 1][:n], np.uint8), np.array([0, 1, 0][:n], np.uint8)
    # ---- scene parameters, the state after mre_create's reset
    nprops = np.array([4, 3, 2][:n], np.int32)
    sizes = np.full((n, 4, 3), 0.0155, np.float32) + np.float32(0.001) * np.arange(n, dtype=np.float32)[:, None, None]
    r.call("mre_set_props", p(nprops), p(sizes))
    r.call("mre_sync")
    q, v, q64, v64 = r.state("created")
    # ---- state in and out: float64 (low-order words), then float32 (they are cleared)
    q64 = q64.copy()
    v64 = v64.copy()
    q64[:, :7] += 1e-3 * rng.standard_normal((n, 7)) + 1e-10
    v64[:, :7] += 1e-2 * rng.standard_normal((n, 7))
    r.call("mre_set_state_f64", p(q64), p(v64))
    r.state("set_state_f64")
    r.call("mre_set_state_f64", p(q64 + 1e-9), None)
    r.state("set_state_f64, qpos alone")
    q[:, :7] += np.float32(1e-3)
    r.call("mre_set_state", p(q), None)
    r.call("mre_sync")
    r.state("set_state, qpos alone")
    v[:, :7] = np.float32(0.01)
    r.call("mre_set_state", p(q), p(v))
    r.call("mre_sync")
    r.state("set_state")
    r.call("mre_set_warmstart", p((0.1 * rng.standard_normal((n, 40))).astype(np.float32)))
    r.call("mre_set_ctrl", p((0.05 * rng.standard_normal((n, 8))).astype(np.float32)))
    r.call("mre_sync")
    r.state("set_warmstart, set_ctrl")
    # ---- reset, placement without and with settling, reset and placement under a mask
    r.call("mre_reset", None)
    r.state("reset")
    r.place("place_props", None, 11, 0)
    r.place("place_props, settling", None, 12, 150)
    r.call("mre_reset", p(m2))
    r.state("reset, mask")
    r.place("place_props, settling, mask", m2, 13, 150)
    r.place("place_props, other mask", m1, 14, 0)
    r.telemetry("after the placements")
    # ---- stepping: a traced step, rollouts as one launch and as launches of 2 and 3 ticks
    trace = r.dev((5, n, 88), torch.float32)
    r.call("mre_set_trace", trace.data_ptr(), n, 5)
    r.call("mre_step", 5, 0)
    r.rec("step: trace", r.read(trace))
    r.call("mre_set_trace", None, 0, 0)
    r.state("step")
    r.telemetry("step")
    seq = torch.tensor((0.1 * rng.standard_normal((6, n, 8))).astype(np.float32), device="cuda").contiguous()
    torch.cuda.synchronize()
    r.keep.append(seq)
    r.call("mre_rollout", seq.data_ptr(), 4, 5, 0)
    r.state("rollout, one launch")
    r.call("mre_rollout_ticks", seq.data_ptr(), 4, 5, 0, 2)
    r.state("rollout, launches of 2")
    r.call("mre_rollout_ticks", seq.data_ptr(), 6, 5, 0, 3)
    r.state("rollout of 6, launches of 3")
    r.telemetry("rollouts")
    # ---- the controller: targets with every optional array absent once and under a mask, each read through the torque law
    def sites(tag):
        tcp, eef, props = np.zeros((n, 3), np.float32), np.zeros((n, 7), np.float32), np.zeros((n, 4, 7), np.float32)
        r.call("mre_get_sites", p(tcp), p(eef), p(props))
        for name, a in (("tcp", tcp), ("eef", eef), ("props", props)):
            r.rec(f"{tag}: {name}", a)
        return eef

    def torques(tag):
        tau, grip = np.zeros((n, 7), np.float32), np.zeros(n, np.float32)
        r.call("mre_osc_compute", p(tau), p(grip))
        r.rec(f"{tag}: tau", tau)
        r.rec(f"{tag}: grip", grip)
    eef = sites("get_sites")
    pos = np.ascontiguousarray(eef[:, :3] + np.array([0.02, -0.01, 0.03], np.float32))
    quat = np.ascontiguousarray(eef[:, 3:])
    vel = np.full((n, 3), 0.01, np.float32)
    ang = np.full((n, 3), -0.02, np.float32)
    for tag, args in (("all", (pos, quat, vel, ang, None)), ("no pos", (None, quat, vel + 1, ang, None)),
                      ("no quat", (pos + 0.01, None, vel, ang, None)), ("no vel", (pos, quat, None, ang + 1, None)),
                      ("no angvel", (pos, quat, vel, None, None)), ("mask", (pos - 0.02, quat, vel, ang, m1)),
                      ("back", (pos, quat, 0 * vel, 0 * ang, None))):
        r.call("mre_osc_set_target", *(None if a is None else p(np.ascontiguousarray(a, a.dtype)) for a in args))
        torques(f"osc_set_target, {tag}")
    r.call("mre_gripper_set", p(m1))
    conv = np.full(n, 7, np.uint8)
    r.call("mre_run_controller", 6, 5, p(conv))
    r.rec("run_controller: converged", conv)
    r.state("run_controller")
    r.call("mre_run_controller", 2, 5, None)
    r.state("run_controller, no flags")
    torques("osc_compute")
    sites("get_sites after the controller")
    for site in (0, 1):
        dyn = r.dev((n, 128), torch.float32, -1.0)
        r.call("mre_get_arm_dynamics", site, dyn.data_ptr())
        r.rec(f"get_arm_dynamics, site {site}", r.read(dyn))
    # ---- contacts
    count, rows3 = np.zeros(n, np.int32), np.zeros((n, 32, 3), np.float32)
    r.call("mre_get_contacts", p(count), p(rows3))
    r.rec("get_contacts: count", count)
    r.rec("get_contacts: rows", np.concatenate([rows3[i, :abs(int(count[i]))].reshape(-1) for i in range(n)]))
    for active in (0, 1):
        count, rows15 = np.zeros(n, np.int32), np.zeros((n, 32, 15), np.float32)
        r.call("mre_get_contacts_full", active, p(count), p(rows15))
        r.rec(f"get_contacts_full, active_only {active}: count", count)
        r.rec(f"get_contacts_full, active_only {active}: rows",
              np.concatenate([rows15[i, :abs(int(count[i]))].reshape(-1) for i in range(n)]))
    # ---- pose search: prop_place, sort_colours
    prop, tick = np.array([0, 1, -1][:n], np.int32), np.array([0, 5, 9][:n], np.int32)
    bounds = np.tile(np.array([0.35, -0.3, 0.45, 0.55, 0.3, 0.5]), (n, 1))
    pose, attempts = np.zeros((n, 7)), np.zeros(n, np.int32)
    r.call("mre_prop_place", 21, p(prop), p(bounds), p(tick), 20, 0.05, p(pose), p(attempts))
    r.rec("prop_place: attempts", attempts)
    r.rec("prop_place: pose", pose[attempts > 0])
    zones = np.zeros((n, 4, 4))
    for k in range(4):
        zones[:, k] = [0.3, -0.4 + 0.2 * k, 0.6, -0.2 + 0.2 * k]
    calls = np.array([0, 1, 2][:n], np.int32)
    which, pick, place, attempts = np.zeros(n, np.int32), np.zeros((n, 7)), np.zeros((n, 7)), np.zeros(n, np.int32)
    r.call("mre_sort_colours", 22, p(calls), p(zones), 20, 0.05, p(which), p(pick), p(place), p(attempts))
    r.rec("sort_colours: which", which)
    r.rec("sort_colours: attempts", attempts)
    r.rec("sort_colours: pick", pick[which >= 0])
    r.rec("sort_colours: place", place[(which >= 0) & (attempts > 0)])
    # ---- controller parameters: shared, per env, shared again; each followed by a tick
    gains = np.array([300, 25, 450, 90, 150, 20], np.float32)
    null_q = np.array([0.1, -0.7, 0.0, -2.3, 0.0, 1.5, 0.7], np.float32)
    thr = np.array([4e-3, 60e-3], np.float32)
    r.call("mre_osc_configure", p(gains), p(null_q), p(thr), 1)
    r.call("mre_run_controller", 1, 5, None)
    r.state("osc_configure")
    genv = np.ascontiguousarray(np.tile(gains, (n, 1)) * (1 + 0.1 * np.arange(n, dtype=np.float32))[:, None])
    r.call("mre_osc_configure_env", p(genv), None, p(np.ascontiguousarray(np.tile(thr, (n, 1)))))
    r.call("mre_run_controller", 1, 5, None)
    r.state("osc_configure_env")
    r.call("mre_osc_configure_env", None, p(np.ascontiguousarray(np.tile(null_q, (n, 1)))), None)
    r.call("mre_run_controller", 1, 5, None)
    r.state("osc_configure_env, null_q alone")
    r.call("mre_osc_configure", None, None, None, 0)
    r.call("mre_run_controller", 1, 5, None)
    r.state("osc_configure, nothing but pinv_always")
    # ---- global env ids: explicit, replaced, an offset; each followed by a placement
    LLP = C.POINTER(C.c_longlong)
    for tag, ids in (("set_env_ids", [10, 10, 12]), ("set_env_ids, replaced", [3, 4, 3])):
        a = np.array(ids[:n], np.int64)
        r.keep.append(a)
        r.call("mre_set_env_ids", a.ctypes.data_as(LLP))
        r.place(tag, None, 15, 0)
    r.call("mre_set_env_id_offset", 100)
    r.place("set_env_id_offset", None, 15, 0)
    r.call("mre_set_env_ids", a.ctypes.data_as(LLP))
    r.call("mre_set_env_ids", None)
    r.place("set_env_ids, NULL", None, 15, 0)
    # ---- a caller's dispatch order
    r.call("mre_set_env_order", p(np.array([2, 0, 1][:n] if n == 3 else [0], np.int32)))
    r.call("mre_step", 5, 0)
    r.state("set_env_order")
    r.call("mre_set_env_order", None)
    # ---- the camera: every branch of the cached background, then colours
    r.render("render", CAM_A, None)
    r.render("render, same camera", CAM_A, None)
    r.render("render, mask", CAM_A, m1)
    r.render("render, camera changed", CAM_B, None)
    r.render("render, camera changed back", CAM_A, None)
    r.render("render, camera changed under a mask", CAM_B, m2)
    r.render("render, 8 x 4", CAM_B, None, 8, 4)
    r.render("render, 4 x 8 again, mask", CAM_A, m1)
    prgb = np.ascontiguousarray((40 * np.arange(n * 12) % 256).astype(np.uint8).reshape(n, 4, 3))
    grgb = np.ascontiguousarray((np.arange(60, dtype=np.float32) / 60).reshape(20, 3))
    r.call("mre_set_render_colours", p(prgb), p(grgb))
    r.render("render, colours", CAM_A, None)
    r.call("mre_set_render_colours", None, p(np.ascontiguousarray(grgb[::-1])))
    r.render("render, geom colours alone", CAM_A, None)
    # ---- the packed final state, the capacity modes, the profile's launch count, a foreign stream
    final = r.dev((n, 83), torch.float32, -1.0)
    r.call("mre_pack_final_state", final.data_ptr())
    r.rec("pack_final_state", r.read(final))
    for mode in (2, 0, 1):
        r.call("mre_set_fallback", mode)
        r.call("mre_step", 5, 0)
        r.state(f"set_fallback {mode}")
        r.telemetry(f"set_fallback {mode}")
    r.call("mre_profile_enable", 1)
    r.call("mre_step", 5, 0)
    r.render("render while profiling", CAM_A, None)
    ms, launches = C.c_float(), C.c_int()
    r.call("mre_profile_read", C.byref(ms), C.byref(launches))
    r.call("mre_profile_enable", 0)
    r.rec("profile_read: launches", np.array([launches.value], np.int32))
    r.call("mre_wait_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
    r.call("mre_step", 1, 0)
    r.state("wait_stream, step")
    # ---- placements that fail (last, so that the flags they leave touch no other row): a single draw per cube, then a
    # workspace of one point, where the second cube of every env has nowhere to go -- without and with settling
    point = (np.array([0.45, 0.0, 0.43], np.float32), np.array([0.45, 0.0, 0.43], np.float32))
    r.place("place_props, one attempt", None, 17, 0, max_attempts=1)
    r.place("place_props, no room", None, 18, 0, max_attempts=3, ws=point)
    r.call("mre_reset", None)
    r.place("place_props, no room, mask, settling", m1, 19, 150, max_attempts=2, ws=point)
    assert r.L.mre_num_envs(r.h) == n and r.L.mre_stream(r.h) and r.L.mre_get_solver(r.h) in (MRE_SOLVER_PGS, MRE_SOLVER_NEWTON)


def digests(L, model, run):
    """[[id: label, crc]] of the script's outputs on a fresh handle for ``run`` (one of RUNS) of the compiled ``model``, in a
    fixed order"""
    from mujoco_robot_environments_amd.model import compile as MC
    cid, n, solver, iterations = run
    if iterations is not None:
        model = dict(model)
        model["opt_iterations"] = np.array([iterations], np.int32)
    blob = MC.to_blob(model)
    h = C.c_void_p()
    assert L.mre_create(blob, len(blob), n, 0, C.byref(h)) == 0, L.mre_last_error()
    r = _Run(L, h, n)
    try:
        r.call("mre_set_solver", solver)
        _script(r)
        r.call("mre_sync")
    finally:
        L.mre_destroy(h)
    assert len({row[0] for row in r.rows}) == len(r.rows)
    return [[f"{cid}: {label}", crc] for label, crc in r.rows]
