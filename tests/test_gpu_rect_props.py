"""Rectangular props on the device: the dynamics, the contact solve and the transport of the three half sizes, held to
the fp64 oracle on the scenes of tests/rect_prop_cases.py (checked on the oracle alone by tests/test_rect_prop_cases.py).

Every other GPU test that steps the physics uses cubes, on which the rotation of the body inertia (com_pos), the
gyroscopic terms of velocity_stage, the index into prop_inertia (smooth_forces, the PGS blocks, the Newton Hessian) and
the per-axis transport of prop_size (step preamble, queue hand-off, save / restore rows, large kernel) cannot be wrong
visibly.  Here every prop's half sizes are a permutation of (1/64, 3/128, 1/32).

  A  free flight, ONE step from a given state (drift-free), Newton and PGS, compact and large kernel: all six velocities
     within 4 float32 ulp at the env's largest speed of the same kind (2^-18 rad/s below 16 rad/s: one rounding of the
     stored velocity, plus h = 1e-3 times an acceleration below 256 rad/s^2 formed in about 30 float32 operations), the
     seven position coordinates within 4 ulp at their own magnitude.  The oracle with the sizes cyclically shifted
     leaves this bound by 372 x or more in every general-position env.
  B  the same envs in free flight over 200 steps: the project's bars (TOL, QVEL_TOL) in every env; worst error within
     8 x the oracle's own float32-state run (1.2e-5 on qpos, 1.1e-5 on qvel); world-frame angular momentum
     R diag(m/3 (b^2 + c^2), ..) w drifts as the oracle's trace does (between half and twice, the first-order integrator's
     drift, up to 5.2e-3 relative); quaternion norms within 1e-5 of 1.
  C  boxes tumbling onto the table and onto each other, robot frozen, 120 steps, Newton / PGS elliptic and Newton
     pyramidal, with the constraint census of tests/test_gpu_newton.py: every env whose constraint set never differed
     holds the bars, nobody leaves without a switch, at most 4 of 32 after one.
  D  a rectangular block 1 mm into a lower finger pad, each half size along the closing direction in turn and one block
     yawed 30 degrees, in prop slot 0 and in slot 2; arm under gravity compensation, gripper closing, 40 steps: the bars
     on all 43 + 39 numbers.
  E  the scenes of C and D in one batch stepped tick by tick, as one queue launch, on the large kernel, in reversed
     batch order and by a handle that forms every Hessian tile: the same bits; and a batch half cubic, half rectangular
     gives every env the bits it has among its own kind.

Device figures (MI355X) against the bounds are printed by every test; measured with this file:
  A  error / bound 0.13 on the velocities (max |dw| 4.8e-7 rad/s against 2^-18 = 3.8e-6), 0.33 on positions and quaternion
     components; the same under Newton and PGS, compact and large kernel.
  B  max |dqpos| 1.1e-6 (float32-state run 1.2e-5, so 9.5e-5 allowed), max |dqvel| 3.2e-5 (float32-state run 1.1e-5, so
     8.6e-5 allowed); momentum drift 0.985 .. 1.065 of the oracle's, quaternion norm error 4.6e-8.
  C  32 of 32 envs never switch their constraint set: max |dqpos| 3.2e-5 / 4.4e-6 / 3.3e-5 (bar 1e-4), max |dqvel|
     2.0e-3 / 1.1e-3 / 2.1e-3 (bar 1e-2) under Newton elliptic / PGS elliptic / Newton pyramidal; nobody leaves the bar.
  D  max |dqpos| 1.2e-7 (bar 1e-4), max |dqvel| 2.1e-5 Newton / 1.4e-5 PGS (bar 1e-2).
  E  identical bits on every path; place_props settles on step 301 in all 16 envs, as the oracle does.
That the tests see what they are for, from a local experiment with two indices of prop_inertia swapped (k - 3 -> 1, 0, 2):
in smooth_forces, A fails under PGS at 9741 x the bound (|dw| 3.7e-2 rad/s), as do B (PGS) and C (PGS; Newton pyramidal);
in the Newton lane's mass diagonal (nw_lane), A, B, C and D fail under Newton.  Every other GPU test stays green with
the first swap in place (the second was run against the Newton and dynamics files only).
"""
import numpy as np
import pytest

from tests import newton_tile_cases as TC
from tests import rect_prop_cases as RC
from tests.test_gpu_newton import M54, QVEL_TOL, TOL, _divergence_report, _qvel_report
from tests.test_gpu_newton_tiles import KEYS, QUEUE_KNOBS, _final, _same

pytestmark = pytest.mark.gpu

F64 = np.float64


def _handle(scene, solver, cone="elliptic"):
    import torch
    from mujoco_robot_environments_amd.physics import BatchedPhysics
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    phys = BatchedPhysics(len(scene), model=RC.model(cone)[0], solver=solver)
    phys.set_props(scene.nprops, scene.sizes)
    phys.reset()
    phys.set_state(scene.qpos, scene.qvel)
    return phys


def _ctrl_seq(phys, scene, ticks):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.broadcast_to(scene.ctrl, (ticks,) + scene.ctrl.shape))).to(phys.device).contiguous()


def _trace(phys, scene, ticks):
    """(qpos [T, N, 43], qvel [T, N, 39], census [T, N]) of the device over ticks * CS steps under the scene's control,
    the census put together as tests/test_gpu_parity.py::_rollout_both does."""
    from mujoco_robot_environments_amd.lib import MRE_TRACE_QVEL
    trace = phys.set_trace(len(scene), ticks * RC.CS)
    phys.rollout(_ctrl_seq(phys, scene, ticks), control_steps=RC.CS, flags=2 if scene.frozen else 0)
    phys.sync()
    tr = trace.cpu().numpy()
    cen = tr[:, :, 43].astype(np.int64) + (tr[:, :, 44].astype(np.int64) << 32) + ((tr[:, :, 45].astype(np.int64) % 509) << 54)
    return tr[:, :, :43].astype(F64), tr[:, :, MRE_TRACE_QVEL:MRE_TRACE_QVEL + 39].astype(F64), cen


# ------------------------------------------------------------------ A
@pytest.mark.parametrize("kernel", ["compact", "large"])
@pytest.mark.parametrize("solver", ["Newton", "PGS"])
def test_family_a_free_flight_one_step(solver, kernel):
    a = RC.family_a()
    q_ref, v_ref = RC.cached(RC.a_reference, solver)
    phys = _handle(a, solver)
    if kernel == "large":
        phys.set_fallback(2)
    phys.set_control(a.ctrl)
    phys.step(1)
    phys.sync()
    q, v = phys.get_state()
    status = phys.status().copy()
    phys.close()
    q, v = q.astype(F64), v.astype(F64)
    bq, bv = RC.a_bounds(a, q_ref, v_ref)
    eq, ev = np.abs(q - q_ref), np.abs(v - v_ref)
    rv, rq = np.where(ev == 0, 0, ev / bv), np.where(eq == 0, 0, eq / bq)
    ratio = RC.a_ratio(a, q, v, q_ref, v_ref)
    w = [15 + 6 * p + k for p in range(4) for k in (3, 4, 5)]
    print(f"A ({solver}, {kernel}): error / bound, worst env: angular velocity {rv[:, w].max():.2f} (max |dw| {np.where(np.isfinite(bv), ev, 0)[:, w].max():.2e} rad/s), "
          f"all velocities {rv.max():.2f}, positions and quaternions {rq.max():.2f}; worst envs {[a.names[i] for i in np.argsort(-ratio)[:3]]}")
    assert (status == 0).all()
    assert ratio.max() <= 1.0, [(a.names[i], float(ratio[i])) for i in np.nonzero(ratio > 1)[0]]


# ------------------------------------------------------------------ B
@pytest.mark.parametrize("solver", ["Newton", "PGS"])
def test_family_b_free_flight_200_steps(solver):
    b = RC.family_b()
    oq, ov, _ = RC.cached(RC.b_reference, solver, False)
    bq, bv, _ = RC.cached(RC.b_reference, solver, True)
    phys = _handle(b, solver)
    gq, gv, _ = _trace(phys, b, RC.B_TICKS)
    status = phys.status().copy()
    phys.close()
    eq, ev = RC.active_error(b, gq, oq, 7), RC.active_error(b, gv, ov, 6)
    emu_q, emu_v = RC.active_error(b, bq, oq, 7).max(), RC.active_error(b, bv, ov, 6).max()
    drift, odrift = RC.momentum_drift(b, gq, gv), RC.momentum_drift(b, oq, ov)
    qn = RC.quat_norm_error(b, gq).max()
    big = odrift > 4 * RC.DRIFT_FLOOR
    print(f"B ({solver}): device vs oracle over {len(gq)} steps max |dqpos| {eq.max():.2e} (props {eq[..., 15:].max():.2e}; float32-state run "
          f"{emu_q:.2e}, x 8 allowed) max |dqvel| {ev.max():.2e} (props {ev[..., 15:].max():.2e}; float32-state run {emu_v:.2e}); angular-momentum "
          f"drift device / oracle {(drift[big] / odrift[big]).min():.4f} .. {(drift[big] / odrift[big]).max():.4f} where the oracle drifts by "
          f"more than {4 * RC.DRIFT_FLOOR:g}, max |difference| {np.abs(drift - odrift).max():.1e}; quaternion norm error {qn:.1e}")
    assert (status == 0).all() and np.isfinite(gq).all() and np.isfinite(gv).all()
    assert eq.max(axis=(0, 2)).max() < TOL and ev.max(axis=(0, 2)).max() < QVEL_TOL
    assert eq.max() <= 8 * emu_q and ev.max() <= 8 * emu_v
    # the drift is the integrator's, not the arithmetic's: within twice the oracle's and never below half of it (beyond
    # the floor two runs of this integrator are told apart by, tests/rect_prop_cases.py: DRIFT_FLOOR)
    assert (drift <= 2 * odrift + RC.DRIFT_FLOOR).all() and (drift >= 0.5 * odrift - RC.DRIFT_FLOOR).all()
    assert qn < 1e-5


# ------------------------------------------------------------------ C
@pytest.mark.parametrize("solver,cone", RC.SOLVER_CONES)
def test_family_c_tumbling_onto_the_table_and_each_other(solver, cone):
    c = RC.family_c()
    oq, ov, ocen = RC.cached(RC.c_reference, solver, cone, False)
    phys = _handle(c, solver, cone)
    gq, gv, gcen = _trace(phys, c, RC.C_TICKS)
    status = phys.status().copy()
    phys.close()
    name = f"C ({solver}, {cone})"
    under, switched, unexplained, cmax = _divergence_report(name, gq, oq, c.nprops, gcen, ocen)
    vmax = _qvel_report(name, gv, ov, c.nprops, under, gcen, ocen)
    clean = [i for i in range(len(c)) if not np.any((gcen[:, i] & M54) != (ocen[:, i] & M54))]
    print(f"{name}: {len(clean)} of {len(c)} envs never switched their constraint set: max |dqpos| {cmax:.2e} (bar {TOL:g}) "
          f"max |dqvel| {vmax:.2e} (bar {QVEL_TOL:g}); {len(switched)} left the bar after a switch (cap 4)")
    assert (status == 0).all() and np.isfinite(gq).all()
    assert not unexplained, unexplained
    assert cmax < TOL and vmax < QVEL_TOL
    assert len(under) + len(switched) == len(c) and len(switched) <= 4


# ------------------------------------------------------------------ D
@pytest.mark.parametrize("solver", ["Newton", "PGS"])
def test_family_d_rectangular_block_between_the_pads(solver):
    d = RC.family_d()
    A = RC.model()[0]
    names = A["_names"]["geoms"]
    oq, ov, _ = RC.cached(RC.d_reference, solver, False)
    bq, bv, _ = RC.cached(RC.d_reference, solver, True)
    phys = _handle(d, solver)
    cnt, con = phys.contacts(full=True, active_only=True)
    for i, name in enumerate(d.names):
        slot = int(name[7])
        assert cnt[i] > 0, (name, int(cnt[i]))
        rows = con[i, :cnt[i]]
        assert TC.contact_sets(rows, np.asarray(A["geom_bodyid"])) == ({slot}, set(), False), name
        pad = [r for r in rows if r[-3] < 0 and f"prop_{slot}" in (names[int(r[-2])], names[int(r[-1])])]
        assert pad and all("pad" in names[int(r[-2])] for r in pad), name
    gq, gv, _ = _trace(phys, d, RC.D_TICKS)
    status = phys.status().copy()
    phys.close()
    eq, ev = np.abs(gq - oq), np.abs(gv - ov)
    print(f"D ({solver}): device vs oracle over {len(gq)} steps, all 43 + 39 numbers: max |dqpos| {eq.max():.2e} (arm {eq[..., :7].max():.2e} "
          f"fingers {eq[..., 7:15].max():.2e} props {eq[..., 15:].max():.2e}; bar {TOL:g}; float32-state run {np.abs(bq - oq).max():.2e}) "
          f"max |dqvel| {ev.max():.2e} (bar {QVEL_TOL:g}; float32-state run {np.abs(bv - ov).max():.2e})")
    assert (status == 0).all()
    assert eq.max() < TOL and ev.max() < QVEL_TOL


# ------------------------------------------------------------------ E
_E = {}


def _run_e(scene, solver, mode, monkeypatch, generic=False):
    """The final words of the batch after C_TICKS ticks: mode "tick" (one launch per tick), "queue" (one queue launch,
    the knobs of tests/test_gpu_newton_tiles.py at 16 waves for 40 envs), "large" (pinned to the large kernel),
    "reversed" (tick by tick in reversed batch order)."""
    for k in QUEUE_KNOBS + ("MRE_NEWTON_GENERIC",):
        monkeypatch.delenv(k, raising=False)
    knobs = {"MRE_QUEUE_WAVES": "16", "MRE_QUEUE_SHARDS": "4", "MRE_QUEUE_MIN_TICKS": "2"} if mode == "queue" else {"MRE_QUEUE": "0"}
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    if generic:
        monkeypatch.setenv("MRE_NEWTON_GENERIC", "1")
    phys = _handle(scene, solver)
    monkeypatch.delenv("MRE_NEWTON_GENERIC", raising=False)
    if mode == "large":
        phys.set_fallback(2)
    if mode == "reversed":
        phys.set_env_order(np.arange(len(scene))[::-1])
    seq = _ctrl_seq(phys, scene, RC.C_TICKS)
    launches = phys.queue_info()["launches"]
    if mode == "queue":
        phys.rollout(seq, control_steps=RC.CS)
    else:
        for t in range(RC.C_TICKS):
            phys.rollout(seq[t:t + 1], control_steps=RC.CS)
    phys.sync()
    launches = phys.queue_info()["launches"] - launches
    assert (launches >= 1) == (mode == "queue"), (mode, launches)
    return _final(phys)


def _e_reference(kind, solver, mode, monkeypatch):
    """Computed once per (sizes, solver, mode), shared, never modified."""
    key = (kind, solver, mode)
    if key not in _E:
        e = RC.family_e()
        scene = {"rect": e, "cubic": e.with_sizes(np.full(e.sizes.shape, RC.CUBE)), "mixed": RC.half_cubic(e)}[kind]
        _E[key] = _run_e(scene, solver, mode, monkeypatch)
        for a in _E[key].values():
            a.setflags(write=False)
    return _E[key]


# (a handle created under MRE_NEWTON_GENERIC=1 forms every Hessian tile: the Newton direction only)
@pytest.mark.parametrize("solver,mode", [("Newton", "queue"), ("Newton", "large"), ("Newton", "reversed"), ("Newton", "generic"),
                                         ("PGS", "queue"), ("PGS", "large"), ("PGS", "reversed")])
def test_family_e_every_path_ends_in_the_same_bits(solver, mode, monkeypatch):
    ref = _e_reference("rect", solver, "tick", monkeypatch)
    e = RC.family_e()
    moved = np.abs(ref["qpos"][:, :43] - e.qpos).max(axis=1)
    assert (moved > 1e-3).all(), moved
    if mode == "generic":
        got = _run_e(e, solver, "tick", monkeypatch, generic=True)
    else:
        got = _e_reference("rect", solver, mode, monkeypatch)
    _same(ref, got, (solver, mode))


@pytest.mark.parametrize("solver", ["Newton", "PGS"])
def test_family_e_no_size_leaks_across_envs_of_a_mixed_batch(solver, monkeypatch):
    """Even envs rectangular, odd envs cubic, one queue launch: every env ends in the bits it has in the batch of its own
    kind -- so no half size reaches another env, or another slot, in the hand-off."""
    rect, cubic = _e_reference("rect", solver, "queue", monkeypatch), _e_reference("cubic", solver, "queue", monkeypatch)
    mixed = _e_reference("mixed", solver, "queue", monkeypatch)
    for k in KEYS:
        assert np.array_equal(mixed[k][0::2], rect[k][0::2]), (solver, k, "rectangular envs", np.argwhere(mixed[k][0::2] != rect[k][0::2])[:4])
        assert np.array_equal(mixed[k][1::2], cubic[k][1::2]), (solver, k, "cubic envs", np.argwhere(mixed[k][1::2] != cubic[k][1::2])[:4])
    # (the two kinds do differ: the comparison above is not between equal batches)
    assert (np.abs(rect["qpos"][1::2] - cubic["qpos"][1::2]).max(axis=1) > 0).all()


# ------------------------------------------------------------------ two small things
def test_arm_dynamics_does_not_see_a_rectangular_block():
    """mre_get_arm_dynamics reads the step preamble's prop sizes and inertias too: its export for an arm state is the
    same bytes with a rectangular block between the pads and rectangular props on the table as with one resting cube."""
    import torch
    d = RC.family_d().take(range(8))
    d.qvel[:, :7] = np.random.RandomState(5).uniform(-1, 1, (len(d), 7)).astype(np.float32)
    plain = d.with_sizes(np.full(d.sizes.shape, RC.CUBE))
    plain.nprops[:] = 1
    plain.qpos[:, 15:] = RC._blank("rearr", 1, plain.sizes[:1])[0, 15:]
    plain.qpos[:, 15:22] = [TC.REST_XY[0][0], TC.REST_XY[0][1], TC.TOP + RC.CUBE, 1, 0, 0, 0]
    plain.qvel[:, 15:] = 0
    out = []
    for sc in (d, plain):
        phys = _handle(sc, "Newton")
        raw = [phys.arm_dynamics(site).raw for site in ("eef", "pinch")]
        torch.cuda.synchronize()
        out.append([t.cpu().numpy().copy() for t in raw])
        phys.close()
    for with_block, without in zip(*out):
        assert with_block.shape == (len(d), 128) and np.isfinite(with_block).all() and np.abs(with_block).max() > 1
        assert np.array_equal(with_block.view(np.uint32), without.view(np.uint32))


def test_place_props_with_rectangular_sizes_follows_the_oracle(compiled_model, oracle_model):
    """tests/test_gpu_env.py::test_place_props_follows_prop_placer_against_the_oracle with rectangular props, 16 envs: the
    accepted poses agree draw for draw (the rejection test reads the box's three half sizes), and the settle ends on the
    same step as the oracle's from the same poses."""
    from mujoco_robot_environments_amd import rng
    from mujoco_robot_environments_amd.physics import BatchedPhysics
    from oracle import oracle as O
    A, _ = compiled_model
    N, off, seed, max_attempts = 16, 512, 6, 1000
    ids = np.arange(off, off + N)
    r = np.random.RandomState(2)
    nprops = (1 + np.arange(N) % 4).astype(np.int32)
    sizes = np.stack([RC._env_sizes(r) for _ in range(N)])
    lo, hi = np.array([0.35, -0.4, 0.44], np.float32), np.array([0.55, 0.4, 0.445], np.float32)
    phys = BatchedPhysics(N, model=A, solver="Newton")
    phys.set_env_id_offset(off)
    phys.set_props(nprops, sizes)
    phys.reset()
    phys.place_props(seed, lo, hi, settle_steps=0)
    q = phys.qpos().copy()
    geom_names = A["_names"]["geoms"]
    table = geom_names.index("table")
    nattempts, envs = [], []
    for i in range(N):
        e = O.Env(oracle_model, int(nprops[i]), sizes[i])
        e.set_solver("Newton")
        e.reset()
        e.arr("qpos")[:7] = A["home_qpos"]
        for p in range(int(nprops[i])):
            gp = geom_names.index(f"prop_{p}")
            for att in range(max_attempts):
                u = rng.uniform(seed, [ids[i]], [p * max_attempts + att], 4)[0, 0]
                pos = (lo.astype(F64) + (hi.astype(F64) - lo.astype(F64)) * u[:3]).astype(np.float32)
                yaw = np.pi * u[3]
                e.arr("qpos")[15 + 7 * p: 22 + 7 * p] = [*pos, np.float32(np.cos(yaw / 2)), 0, 0, np.float32(np.sin(yaw / 2))]
                e.forward()
                if not any((int(c[13]) == gp or int(c[14]) == gp) and table not in (int(c[13]), int(c[14])) for c in e.contacts()):
                    break
            else:
                raise AssertionError("oracle could not place")
            nattempts.append(att + 1)
        n = int(nprops[i])
        assert np.abs(q[i, 15:15 + 7 * n] - e.arr("qpos")[15:15 + 7 * n]).max() < 1e-6, (i, q[i, 15:15 + 7 * n], e.arr("qpos")[15:15 + 7 * n])
        envs.append(e)
    assert max(nattempts) > 1, "the rejection branch must have been exercised"
    # the settle, from the same poses on both sides
    phys.reset()
    phys.place_props(seed, lo, hi, settle_steps=300)
    gsteps = phys.settle_steps().copy()
    gq = phys.qpos()
    osteps, worst = np.zeros(N, int), 0.0
    for i, e in enumerate(envs):
        n = int(nprops[i])
        e.arr("qpos")[:43] = q[i]
        e.arr("qvel")[:] = 0
        e.freeze_robot(True)
        e.forward()
        for k in range(2000):
            e.step(1)
            if np.abs(e.arr("qvel")[15:15 + 6 * n]).max() < 1e-3 and np.abs(e.arr("qacc")[15:15 + 6 * n]).max() < 1e-2 and k + 1 > 300:
                break
        osteps[i] = k + 1
        worst = max(worst, float(np.abs(gq[i, 15:15 + 7 * n] - e.arr("qpos")[15:15 + 7 * n]).max()))
    print(f"place_props, rectangular: attempts per prop mean {np.mean(nattempts):.2f} max {max(nattempts)}; settle steps device "
          f"{gsteps.tolist()} oracle {osteps.tolist()}; settled poses max |dq| {worst:.1e}")
    assert np.array_equal(gsteps, osteps)
    assert worst < TOL and (phys.status() == 0).all()
    phys.close()
