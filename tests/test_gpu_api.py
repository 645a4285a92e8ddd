"""GPU tests of the C-ABI surface itself: state round trips, masks, control modes, trace,
status bits, capacity overflow agreeing with the oracle's capacity emulation."""
import numpy as np
import pytest

from tests.common import HOME, init_oracle_env

pytestmark = pytest.mark.gpu


def _phys(n, model):
    from mujoco_robot_environments_amd.physics import BatchedPhysics
    return BatchedPhysics(n, model=model)


def test_state_roundtrip_reset_and_masks(compiled_model):
    A, _ = compiled_model
    N = 8
    phys = _phys(N, A)
    q, v = phys.get_state()
    assert q.shape == (N, 43) and v.shape == (N, 39)
    assert np.allclose(q[:, :7], A["home_qpos"], atol=1e-7) and (v == 0).all()
    assert np.allclose(q[:, 15:].reshape(N, 4, 7)[:, :, 3], 1.0) and (q[:, 17::7] < -1).all(), "cubes parked"
    rs = np.random.RandomState(0)
    q2 = q + rs.uniform(-0.01, 0.01, q.shape).astype(np.float32)
    v2 = rs.uniform(-0.1, 0.1, v.shape).astype(np.float32)
    phys.set_state(q2, v2)
    q3, v3 = phys.get_state()
    assert np.array_equal(q3, q2) and np.array_equal(v3, v2)
    mask = np.array([1, 0, 1, 0, 0, 0, 0, 1], np.uint8)
    phys.reset(mask)
    q4, v4 = phys.get_state()
    assert np.array_equal(q4[mask == 0], q2[mask == 0]) and np.array_equal(q4[mask == 1], q[mask == 1])
    assert (v4[mask == 1] == 0).all() and np.array_equal(v4[mask == 0], v2[mask == 0])
    phys.close()


def test_step_with_held_control_equals_rollout_and_zero_step_is_identity(compiled_model):
    import torch
    A, _ = compiled_model
    N = 4
    a, b = _phys(N, A), _phys(N, A)
    ctrl = np.tile(np.array([0, -4.5, -0.6, 22.7, 0.6, 2.5, 0, 100.0], np.float32), (N, 1))
    q0, _ = a.get_state()
    a.step(0)
    a.sync()
    assert np.array_equal(a.get_state()[0], q0), "nsubsteps = 0 must not change the state"
    a.set_control(ctrl)
    a.step(10)
    seq = torch.tensor(np.tile(ctrl, (2, 1, 1)), device=b.device)
    b.rollout(seq.contiguous(), control_steps=5)
    qa, va = a.get_state()
    qb, vb = b.get_state()
    assert np.array_equal(qa, qb) and np.array_equal(va, vb), "held control == per-tick sequence of the same control"
    tcp, eef, props = a.sites()
    assert tcp.shape == (N, 3) and eef.shape == (N, 7) and props.shape == (N, 4, 7)
    assert np.allclose(np.linalg.norm(eef[:, 3:], axis=1), 1.0, atol=1e-5)
    assert np.allclose(eef[:, 2] - tcp[:, 2], 0.1558, atol=2e-3), "pinch site sits 0.156 m below the controller site"
    a.close(); b.close()


def test_trace_records_every_step(compiled_model):
    A, _ = compiled_model
    phys = _phys(4, A)
    tr = phys.set_trace(2, 12)
    phys.step(5, flags=1)
    phys.step(7, flags=1)
    phys.sync()
    t = tr.cpu().numpy()
    q, v = phys.get_state()
    assert np.allclose(t[-1, :, :43], q[:2]) and not np.allclose(t[0], t[-1])
    from mujoco_robot_environments_amd.lib import MRE_TRACE_QVEL, MRE_TRACE_W
    assert t.shape[2] == MRE_TRACE_W and np.array_equal(t[-1, :, MRE_TRACE_QVEL:MRE_TRACE_QVEL + 39], v[:2]), "qvel columns of the trace row"
    assert (t[:, :, MRE_TRACE_QVEL + 39:] == 0).all() and np.abs(t[:, :, MRE_TRACE_QVEL:MRE_TRACE_QVEL + 7]).max() > 0
    assert (np.abs(np.diff(t[:, 0, 1])) > 0).all(), "arm sags under gravity at every recorded step"
    phys.close()


def test_capacity_overflow_flag_matches_oracle_emulation(compiled_model, oracle_model):
    """Four cubes interpenetrating in a pile produce more rows than the device keeps; the kernel
    raises MRE_ST_CONTACT_OVERFLOW and the oracle with the same capacities agrees on the rows kept."""
    from oracle import oracle as O
    A, _ = compiled_model
    e = O.Env(oracle_model, 4)
    q = e.arr("qpos")
    q[:7] = HOME
    for p in range(4):  # a 2x2 cluster, overlapping by 2 mm, pressed 2 mm into the table
        q[15 + 7 * p: 22 + 7 * p] = [0.45 + 0.029 * (p % 2), 0.0 + 0.029 * (p // 2), 0.4135, 1, 0, 0, 0]
    e.set_caps(ncon_cap=12, nefc_cap=112, nrrow_cap=62, npp_cap=2)
    e.forward()
    assert e.overflow
    phys = _phys(2, A)
    phys.set_fallback(False)  # pin the envs to the compact kernel: this test is about ITS capacities
    qp = phys.qpos().copy()
    qp[:, :43] = q[:43]
    phys.set_state(qp, np.zeros((2, 39), np.float32))
    phys.step(1)
    st = phys.status()
    # device capacities are larger (32 contacts, 8 cube-cube): re-run the oracle with them
    e.set_caps()
    e.forward()
    stats = phys.solver_stats()
    assert ((st & 4) != 0).all() == e.overflow
    if not e.overflow:
        assert stats[0, 1] == e.nefc
    phys.close()


def test_capacity_fallback_reruns_overflowing_envs_on_the_large_kernel(compiled_model, oracle_model):
    """A stack of three cubes, the middle one yawed by 45 degrees, has 2 x 8 cube-cube contacts: more
    than the compact kernel keeps (8; it lets the top cube sink), within the large one's 16.  With the fallback (default) the env is re-run from its saved
    state on the large kernel: no overflow status, the trajectory follows the oracle with the large
    capacities, and an env that never overflowed is bit-identical to a compact-only run."""
    from oracle import oracle as O
    A, _ = compiled_model
    rows = np.zeros((2, 3, 7))
    c8, s8 = np.cos(np.pi / 8), np.sin(np.pi / 8)
    rows[0] = [[0.45, 0, 0.4154, 1, 0, 0, 0], [0.45, 0, 0.4463, c8, 0, 0, s8], [0.45, 0, 0.4772, 1, 0, 0, 0]]
    for p in range(3):
        rows[1, p] = [0.40 + 0.05 * p, -0.3 + 0.2 * p, 0.4155, 1, 0, 0, 0]      # far apart
    nsteps = 40
    envs = []
    for i in range(2):
        e = O.Env(oracle_model, 3)
        q = e.arr("qpos")
        q[:7] = HOME
        q[15:36] = rows[i].reshape(-1)
        e.set_caps(32, 112, 62, 8)
        e.forward()
        envs.append(e)
    assert envs[0].overflow and not envs[1].overflow
    for e in envs:
        e.set_caps(44, 148, 83, 16)
        e.forward()
        for _ in range(nsteps):
            e.step(1)
            assert not e.overflow
    results = {}
    for fb in (True, False):
        phys = _phys(2, A)
        phys.set_fallback(fb)
        phys.set_props(np.array([3, 3], np.int32), np.full((2, 4, 3), 0.0155, np.float32))
        qp = phys.qpos().copy()
        for i in range(2):
            qp[i, :7] = HOME
            qp[i, 15:36] = rows[i].reshape(-1)
        phys.set_state(qp, np.zeros((2, 39), np.float32))
        phys.step(nsteps)
        results[fb] = (phys.qpos().copy(), phys.status().copy(), phys.fallback_stats())
        phys.close()
    q_fb, st_fb, stats_fb = results[True]
    q_nofb, st_nofb, stats_nofb = results[False]
    assert (st_fb & 4).tolist() == [0, 0]
    assert (st_nofb & 4).tolist() == [4, 0]
    assert stats_fb["promotions"] == 1 and stats_fb["reruns"] == 1 and stats_nofb["promotions"] == 0
    assert np.array_equal(q_fb[1], q_nofb[1])  # untouched env: same kernel, same bits
    err_fb = [np.abs(q_fb[i, :36] - envs[i].arr("qpos")[:36]).max() for i in range(2)]
    assert max(err_fb) < 1e-4, err_fb
    # the compact-only run dropped contacts of env 0 and drifts away from the oracle
    assert np.abs(q_nofb[0, :36] - envs[0].arr("qpos")[:36]).max() > err_fb[0]


def test_nonfinite_state_is_flagged(compiled_model):
    A, _ = compiled_model
    phys = _phys(3, A)
    q, v = phys.get_state()
    q = q.copy()
    q[1, 3] = np.nan
    phys.set_state(q, v)
    phys.step(2, flags=1)
    st = phys.status()
    assert (st[1] & 2) != 0 and (st[0] & 2) == 0 and (st[2] & 2) == 0
    phys.close()


def test_dispatch_order_does_not_change_results(compiled_model):
    """mre_set_env_order only permutes which workgroup advances which env."""
    import torch
    from mujoco_robot_environments_amd import rng
    A, _ = compiled_model
    N = 64
    ids = np.arange(N)
    seq_np = rng.random_actions(4, ids, np.arange(4), scale=0.2).astype(np.float32)
    out = []
    for order in (None, np.random.RandomState(1).permutation(N)):
        phys = _phys(N, A)
        nprops, sizes = rng.prop_params(4, ids)
        phys.set_props(nprops, sizes)
        phys.reset()
        phys.place_props(4, (0.35, -0.4, 0.43), (0.55, 0.4, 0.435), settle_steps=50)
        phys.set_env_order(order)
        phys.rollout(torch.from_numpy(seq_np).to(phys.device).contiguous(), control_steps=5)
        out.append(phys.get_state())
        phys.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("solver,cone", [("PGS", "elliptic"), ("Newton", "elliptic"), ("PGS", "pyramidal"), ("Newton", "pyramidal")])
def test_fallback_reproduces_the_large_kernel_bit_for_bit(compiled_model, solver, cone):
    """Closing the gripper on a cube with the pads pressed onto the table (pick height 1 cm too low:
    pad-table plus pad-cube contacts) overflows the compact capacities.  Running the envs
    compact-first with re-runs (the default) must give exactly the bits of running every env on the
    large kernel from the start: both kernels execute the same arithmetic, and a re-run starts from
    the saved pre-launch rows.  (cone = pyramidal: the same scenario through the pyramidal instantiations of the
    solver phases, compact and large.)"""
    import bench
    from mujoco_robot_environments_amd import demo_logic
    A = dict(compiled_model[0])
    if cone == "pyramidal":
        A["opt_cone"] = np.zeros(1, np.int32)
    N = 64
    out = {}
    for mode in (1, 2):
        phys = _phys(N, A)
        phys.set_solver(solver)
        phys.set_fallback(mode)
        bench.setup_envs(phys, 7, np.arange(N))
        if mode == 2:
            phys.set_fallback(2)   # (reset inside setup keeps the pin, stated again for clarity)
        cube = phys.qpos()[:, 15:22].astype(np.float64)
        yaw = np.abs(demo_logic.quat_to_yaw_deg(cube[:, 3:7]))
        quat = demo_logic.grasp_quat(np.minimum(yaw, yaw - 90.0))
        pick = np.concatenate([cube[:, :2], np.full((N, 1), 0.565)], axis=1)
        pre = pick.copy(); pre[:, 2] = 0.9
        phys.osc_set_target(position=pre, quat=quat, velocity=np.zeros(3), angular_velocity=np.zeros(3))
        phys.gripper_set(np.zeros(N, np.uint8))
        phys.run_controller(400, 5)
        phys.osc_set_target(position=pick)
        phys.run_controller(400, 5)
        phys.gripper_set(np.ones(N, np.uint8))
        for _ in range(4):                      # close in four launches: promotions happen mid-way
            phys.run_controller(50, 5)
        out[mode] = (phys.qpos().copy(), phys.qvel().copy(), phys.status().copy(), phys.fallback_stats())
        phys.close()
    if cone == "elliptic" or solver == "Newton":
        assert out[1][3]["promotions"] > 0, out[1][3]      # the scenario does exercise the fallback
    # (PGS with pyramidal cones: the softer grasp stays below the promotion thresholds; the comparison is then the
    #  compact kernel against the large one on the same envs)
    assert out[2][3]["promotions"] == 0 and out[2][3]["reruns"] == 0
    assert np.array_equal(out[1][0], out[2][0]) and np.array_equal(out[1][1], out[2][1])
    assert np.array_equal(out[1][2], out[2][2])


@pytest.mark.parametrize("solver", ["PGS", "Newton"])
def test_pipelined_env_groups_equal_the_synchronous_path(compiled_model, solver, monkeypatch):
    """The stepping calls cut the batch into env groups on separate streams and return before the launches have
    finished; a group's launch info is read -- and an overflowing env re-run from its saved rows, for that launch and
    for the one enqueued behind it, which skipped the env on the device -- only when the group's next launch but one is
    issued or the state is touched.  Same grasp-on-the-table scenario as above (promotions
    and re-runs mid-phase), then 30 ticks of per-tick control sequences, one call per tick without a sync in
    between: state, status and fallback counters must equal the single-group (synchronous) handle bit for bit."""
    import torch
    import bench
    from mujoco_robot_environments_amd import demo_logic, rng
    A, _ = compiled_model
    N = 64
    out = {}
    # (groups, ring depth, one library call for the 30 ticks): the ring of unprocessed launches is four deep since
    # round 5 -- an env that overflows is skipped by up to three launches behind the one it overflowed in, and re-run
    # for all of them; "one call" = mre_rollout_ticks enqueuing the 30 per-tick launches itself
    for groups, ring, one_call in ((1, 4, False), (3, 4, False), (3, 4, True), (3, 2, False)):
        monkeypatch.setenv("MRE_GROUPS", str(groups))
        monkeypatch.setenv("MRE_RING", str(ring))
        monkeypatch.setenv("MRE_GROUP_MIN", "1")
        phys = _phys(N, A)
        phys.set_solver(solver)
        bench.setup_envs(phys, 7, np.arange(N))
        cube = phys.qpos()[:, 15:22].astype(np.float64)
        yaw = np.abs(demo_logic.quat_to_yaw_deg(cube[:, 3:7]))
        quat = demo_logic.grasp_quat(np.minimum(yaw, yaw - 90.0))
        pick = np.concatenate([cube[:, :2], np.full((N, 1), 0.565)], axis=1)
        pre = pick.copy(); pre[:, 2] = 0.9
        phys.osc_set_target(position=pre, quat=quat, velocity=np.zeros(3), angular_velocity=np.zeros(3))
        phys.gripper_set(np.zeros(N, np.uint8))
        phys.run_controller(400, 5)
        phys.osc_set_target(position=pick)
        phys.run_controller(400, 5)
        phys.gripper_set(np.ones(N, np.uint8))
        phys.run_controller(200, 5)
        seq = torch.from_numpy(rng.random_actions(3, np.arange(N), np.arange(30), scale=0.3).astype(np.float32)).to(phys.device)
        if one_call:
            phys.rollout(seq, control_steps=5, ticks_per_launch=1)
        else:
            for t in range(30):
                phys.rollout(seq[t:t + 1].contiguous(), control_steps=5)   # no sync between the calls
        out[(groups, ring, one_call)] = (phys.qpos().copy(), phys.qvel().copy(), phys.status().copy(), phys.get_warmstart().copy(),
                                         phys.fallback_stats(), phys.solver_stats().copy())
        phys.close()
    ref = out[(1, 4, False)]
    assert ref[4]["promotions"] > 0 and ref[4]["reruns"] > 0, ref[4]
    for key, o in out.items():
        if key[0] == 1:
            continue
        # (the groups read a launch's info late: a promotion takes effect launches later than on the synchronous
        #  handle, so more envs overflow the compact kernel before they are moved -- and are re-run, for every launch
        #  that skipped them)
        assert o[4]["promotions"] > 0 and o[4]["reruns"] >= ref[4]["reruns"], (key, ref[4], o[4])
        for k in (0, 1, 2, 3, 5):
            assert np.array_equal(ref[k], o[k]), (key, k)


def test_run_controller_in_chunks_equals_one_launch(compiled_model, monkeypatch):
    """mre_run_controller cuts a phase into launches of 50 ticks (so that a capacity re-run repeats at
    most one chunk).  State, converged flags and status must be bit-identical to a single launch,
    including a target that is never reached (NOT_CONVERGED judged once, by the last launch) and one
    reached early (flag carried over the cuts)."""
    from mujoco_robot_environments_amd.model.compile import m2q
    A, _ = compiled_model
    N = 4
    out = {}
    for chunk in ("0", "50", "7"):
        monkeypatch.setenv("MRE_RUN_CHUNK", chunk)
        phys = _phys(N, A)
        tcp, eef, _ = phys.sites()
        tgt = eef[:, :3].astype(np.float64).copy()
        tgt[0] += [0.05, 0.05, -0.10]     # reached well within the window
        tgt[1] += [0.0, 0.0, 0.0]         # already there
        tgt[2] += [0.9, 0.0, 0.9]         # out of reach: never converges
        tgt[3] += [-0.02, 0.08, -0.05]
        phys.osc_set_target(position=tgt, quat=eef[:, 3:7], velocity=np.zeros(3), angular_velocity=np.zeros(3))
        phys.gripper_set(np.array([0, 1, 0, 1], np.uint8))
        conv = phys.run_controller(230, 5)
        out[chunk] = (phys.qpos().copy(), phys.qvel().copy(), conv.copy(), phys.status().copy())
        phys.close()
    assert out["0"][2].tolist() == [True, True, False, True]
    assert (out["0"][3] & 1).tolist() == [0, 0, 1, 0]
    for chunk in ("50", "7"):
        for k in range(4):
            assert np.array_equal(out["0"][k], out[chunk][k]), (chunk, k)


def test_reset_with_a_device_mask_and_control_from_a_fresh_torch_tensor(compiled_model, monkeypatch):
    """include/mre.h: masks are `host or device`; controls produced by torch ops on torch's stream a
    moment ago must be ordered before the handle's stream reads them (mre_wait_stream), also when no
    guarded launch host-syncs in between (MRE_NO_FALLBACK=1)."""
    import torch
    from mujoco_robot_environments_amd.physics import BatchedPhysics
    A, _ = compiled_model
    monkeypatch.setenv("MRE_NO_FALLBACK", "1")
    N = 256
    phys = BatchedPhysics(N, model=A)
    phys.reset()
    q0 = phys.qpos().copy()
    big = torch.randn(4096, 4096, device=phys.device)
    for it in range(3):
        # a long matmul keeps torch's stream busy; the control is its by-product
        big = (big @ big).tanh()
        ctrl = (big[:N, :8] * 0 + float(it + 1)).contiguous()
        phys.set_control(ctrl)
        del ctrl                      # the caching allocator may hand the block out again
        _ = torch.full((N, 8), -99.0, device=phys.device)
        phys.step(1)
    phys.sync()
    # the last applied control is what the kernel read
    c = phys.ctrl() if hasattr(phys, "ctrl") else None
    if c is not None:
        assert np.allclose(c[:, :7], 3.0)
    q1 = phys.qpos()
    assert np.isfinite(q1).all() and not np.array_equal(q0, q1)
    # reset through a CUDA uint8 mask: odd envs go back to the start state, even envs stay
    mask = (torch.arange(N, device=phys.device) % 2).to(torch.uint8)
    phys.reset(mask=mask)
    q2 = phys.qpos()
    assert np.array_equal(q2[0::2], q1[0::2])
    assert np.array_equal(q2[1::2][:, :7], q0[1::2][:, :7])
    phys.close() if hasattr(phys, "close") else None


def test_final_state_rows_packed_on_the_device_and_sharded_handles(compiled_model):
    """mre_pack_final_state: the [N, 83] row block a rank hands to the end-of-rollout all_gather is written by a kernel
    (qpos, qvel, status as an exact float) and equals the host-side packing of distributed.pack_final_state; and the
    DEVICE side of the sharding the gloo tests cover on the CPU: two handles that own the global env ids [0, 32) and
    [32, 64) (set_env_id_offset: scenes, placement draws and actions keyed by global id) reproduce, concatenated, the
    one handle that owns all 64 -- rows as all_gather_into_tensor would order them."""
    import torch
    import bench
    from mujoco_robot_environments_amd import distributed as D, rng
    from mujoco_robot_environments_amd.physics import BatchedPhysics
    A, _ = compiled_model

    def run(ids):
        phys = BatchedPhysics(len(ids), model=A, solver="Newton")
        bench.setup_envs(phys, 3, ids)
        acts = torch.from_numpy(rng.random_actions(3, ids, np.arange(10)).astype(np.float32)).to(phys.device)
        phys.rollout(acts.contiguous(), control_steps=5, ticks_per_launch=1)
        rows = phys.pack_final_state()
        qp, qv = phys.get_state()
        host = D.pack_final_state(qp, qv, phys.status())
        assert rows.is_cuda and tuple(rows.shape) == (len(ids), 83)
        assert torch.equal(rows.cpu(), host), "device-packed rows == host-packed rows"
        phys.close()
        return rows.cpu()

    whole = run(np.arange(64))
    parts = torch.cat([run(np.arange(0, 32)), run(np.arange(32, 64))])
    assert torch.equal(whole, parts)
    q, v, st = D.unpack_final_state(whole)
    assert q.shape == (64, 43) and v.shape == (64, 39) and st.dtype == np.uint32 and np.isfinite(q).all()


def test_bench_two_rank_rehearsal_on_one_gpu():
    """`python bench.py --gpus 2` as the driver's launcher would run it, rehearsed on one card: two
    ranks (gloo instead of RCCL, both pinned to device 0) shard 2 x 4096 envs by global env id, time
    the same K steps between barriers, and rank 0 prints the one JSON line with the whole-job rate."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MRE_BENCH_BACKEND="gloo", MRE_BENCH_DEVICE="0")
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1",
                          "--no-cpu-baseline", "--solver", "PGS"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["scaling"] == "weak" and d["value"] > 0
    assert d["config"]["envs_per_gpu"] == 4096
    # value = units all ranks processed / max-over-ranks time
    assert abs(d["value"] - 2 * 4096 * 5 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6


def test_bench_plain_run_dumps_the_window_outputs(tmp_path):
    """`python bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` without --full: exactly K timed ticks of the
    headline solver and nothing else, the contract fields of the line, and the window's final state written as .npy."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 4 and d["warmup"] == 1 and d["unit"] == "env-steps/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["headline_solver"] == "Newton"
    assert abs(d["value"] - 4096 * 5 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    # the other measurements are --full's
    assert d["cpu_baseline"] is None and d["default_regime"] is None and d["per_tick_launches"] is None
    assert "pick_place" not in d and "pgs" not in d and list(d["value_by_solver"]) == ["Newton"]
    q, v, st = (np.load(os.path.join(tmp_path, n + ".npy")) for n in ("qpos", "qvel", "status"))
    assert q.shape == (4096, 43) and v.shape == (4096, 39) and st.shape == (4096,)
    assert q.dtype == np.float64 and v.dtype == np.float64 and st.dtype == np.float32
    assert np.isfinite(q).all() and np.isfinite(v).all() and ((st.astype(np.uint32) & 2) == 0).all()   # no MRE_ST_NAN
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)) <= 64 << 20


def test_placement_failure_is_per_env(compiled_model):
    """PropPlacer raises _REJECTION_SAMPLING_FAILED for ITS env when a prop finds no collision-free pose within
    max_attempts_per_prop (environment/prop_initializer.py:230-233).  Batched: that env gets MRE_ST_PLACEMENT_FAILED
    and keeps its remaining cubes parked; the other envs are placed and settled as usual (round 2 returned an error
    for the whole batch and left it half placed)."""
    from mujoco_robot_environments_amd.physics import BatchedPhysics
    A, _ = compiled_model
    N = 8
    nprops = np.array([1, 3, 1, 2, 1, 4, 1, 1], np.int32)
    phys = BatchedPhysics(N, model=A, solver="Newton")
    phys.set_props(nprops, np.full((N, 4, 3), 0.0155, np.float32))
    phys.reset()
    # a 2 cm square: one cube fits, a second can never keep the 15 cm of detection margin to the first
    phys.place_props(7, np.array([0.45, 0.0, 0.43], np.float32), np.array([0.47, 0.02, 0.435], np.float32),
                     max_attempts=50, settle_steps=300)
    st = phys.status()
    failed = (st & 16) != 0
    assert failed.tolist() == (nprops > 1).tolist()
    assert (st[~failed] == 0).all()                       # placed, settled, nothing else flagged
    q = phys.qpos()
    for i in range(N):
        c0 = q[i, 15:18]
        assert 0.45 - 1e-3 <= c0[0] <= 0.47 + 1e-3 and -1e-3 <= c0[1] <= 0.02 + 1e-3
        if nprops[i] == 1:
            assert abs(c0[2] - 0.4155) < 2e-3            # placed and settled on the table
        if nprops[i] > 1:
            assert 0.43 <= c0[2] <= 0.435                # a failed env is not settled: cube 0 stays where it was drawn
            assert (np.abs(q[i, 22:25] - [2.5, 2.0, -5.0]) < 1e-6).all()                      # cube 1 stayed parked (mre_api.cpp: park_pos)
    steps = np.zeros(N, np.int32)
    from mujoco_robot_environments_amd import lib as _lib
    _lib.check(_lib.lib().mre_get_settle_steps(phys._h, steps.ctypes.data), "settle_steps")
    assert (steps[~failed] >= 300).all() and (steps[~failed] < 2000).all()


def test_state_f64_and_time(compiled_model):
    """physics.data.qpos / .qvel / .time as the reference holds them (float64): every coordinate -- the robot's 15 joints
    and, since round 4, the cubes' poses and velocities -- is a double-float pair on the device, mre_set_state (float
    rows) clears the low-order words, and time counts the physics steps since mre_reset (models/robot_arm.py:68-69)."""
    from mujoco_robot_environments_amd.physics import BatchedPhysics
    A, _ = compiled_model
    N = 8
    phys = BatchedPhysics(N, model=A, solver="Newton")
    phys.set_props(np.full(N, 2, np.int32), np.full((N, 4, 3), 0.0155, np.float32))
    phys.reset()
    assert (phys.time() == 0).all()
    q0, v0 = phys.get_state_f64()
    rs = np.random.RandomState(0)
    q = q0 + 1e-3 * rs.rand(N, 43)
    v = 1e-2 * rs.rand(N, 39)
    phys.set_state_f64(q, v)
    q1, v1 = phys.get_state_f64()
    assert np.abs(q1[:, :15] - q[:, :15]).max() < 1e-14 and np.abs(v1[:, :15] - v[:, :15]).max() < 1e-14   # hi + lo
    n = 15 + 7 * 2                                                                                           # two cubes in use
    assert np.abs(q1[:, 15:n] - q[:, 15:n]).max() < 1e-13 and np.abs(v1[:, 15:27] - v[:, 15:27]).max() < 1e-14
    qf, vf = phys.get_state()
    assert np.array_equal(qf[:, :15], q[:, :15].astype(np.float32))        # the float rows ARE the rounded values
    phys.set_state(qf, vf)                                                 # a float32 state is the value: lo = 0
    q2, _ = phys.get_state_f64()
    assert np.array_equal(q2, qf.astype(np.float64)[:, :43])
    phys.set_state_f64(q0, np.zeros((N, 39)))
    phys.set_control(np.zeros((N, 8), np.float32))
    phys.step(7)
    h = float(np.float32(0.001))
    assert np.allclose(phys.time(), 7 * h, rtol=0, atol=1e-15)
    q3, v3 = phys.get_state_f64()
    lo = q3[:, :15] - q3[:, :15].astype(np.float32)
    assert (lo != 0).any() and np.abs(lo).max() < 3e-7     # the integrator keeps bits below float32's last place
    loc = q3[:, 15:18] - q3[:, 15:18].astype(np.float32)   # ... for the falling cubes too
    assert (loc != 0).any() and np.abs(loc).max() < 3e-7
    phys.reset()
    assert (phys.time() == 0).all()


def test_bench_rccl_path_with_a_world_of_one():
    """The multi-rank branch of bench.py on the one GPU of this box: launched exactly as the driver launches a
    rank (`python -m torch.distributed.run --nproc-per-node 1 ... bench.py --gpus 1`) with MRE_BENCH_FORCE_DIST=1,
    so backend "nccl" (= RCCL) is initialised with `device_id=`, the barriers, the device-tensor
    all_gather_into_tensor of the final state and the MAX all_reduce of the elapsed time all execute.  A fresh
    child process: this one already holds the GPU."""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, MRE_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("MRE_BENCH_BACKEND", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
           "--no-cpu-baseline", "--solver", "Newton"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["distributed"] == {"backend": "nccl", "world": 1, "gathered_rows": 4096}
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["gather_ms"] > 0


def test_launch_info_reports_high_water_marks_and_durations(compiled_model):
    """mre_get_launch_info: the per-env record of the last stepping launch that the capacity fallback and the
    longest-first dispatch read -- overflow flag, high-water marks, the env's own duration."""
    import torch
    from mujoco_robot_environments_amd import rng
    from mujoco_robot_environments_amd.physics import BatchedPhysics
    A, _ = compiled_model
    N = 128
    ids = np.arange(N)
    phys = BatchedPhysics(N, model=A, solver="Newton")
    nprops, sizes = rng.prop_params(3, ids)
    phys.set_props(nprops, sizes)
    phys.reset()
    phys.place_props(3, np.array([0.35, -0.4, 0.43], np.float32), np.array([0.55, 0.4, 0.435], np.float32), settle_steps=300)
    seq = torch.from_numpy(rng.random_actions(3, ids, np.arange(4), scale=0.1).astype(np.float32)).to(phys.device).contiguous()
    for t in range(4):
        phys.rollout(seq[t:t + 1], control_steps=5)
    li = phys.launch_info()
    st = phys.solver_stats()
    assert (li["overflow"] == 0).all() and (li["duration"] > 0).all()
    # resting cubes: 4 table contacts each, 7 equality rows + 3 rows per contact; the marks bound the last step's counts
    assert (li["ncon"] >= st[:, 0]).all() and (li["nefc"] >= st[:, 1]).all()
    assert (li["ncon"] >= 4 * nprops).all() and (li["nefc"] >= 7 + 3 * li["ncon"] - 3).all()
    assert (li["nrrow"] >= 7).all() and (li["npp"] == 0).all()
    phys.close()
