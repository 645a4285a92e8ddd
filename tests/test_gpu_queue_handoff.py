"""The hand-off of an env between the waves of a queue launch (csrc/mre_kernels.hip: queue_take, queue_push): a wave takes
its next item while the current one finishes, the env's rows travel as write-through stores that the wave drains before
it lists the env, and nothing of that may show in a single word of state.  Every test compares a queue launch, forced at a
small batch with the test knob MRE_QUEUE_WAVES, with the launches that hand nothing over (one wave per env and launch),
bit for bit.  The batches are small, so the consumer's compute unit has usually held the env's lines before (an L1-warm
consumer) and the load is uneven from the second tick on (64 waves, 16 shards of 4, envs of different cost)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOBS = ("MRE_QUEUE", "MRE_QUEUE_WAVES", "MRE_QUEUE_SHARDS", "MRE_QUEUE_TICKS", "MRE_QUEUE_MIN_TICKS", "MRE_QUEUE_TEST_SERIAL",
         "MRE_QUEUE_SPARE_LARGE", "MRE_GROUPS")
WORDS = ("qpos", "qvel", "ws", "qfine_q", "qfine_v", "ctrl", "status", "nstep", "stats")


def _knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _words(phys):
    """Every word that travels with an env, as the host reads it after the launch."""
    q, v = phys.get_state()
    q64, v64 = phys.get_state_f64()
    # (float64 = float32 word + low word, exactly: the difference IS the low word of StepArgs::qfine)
    return dict(qpos=q.copy(), qvel=v.copy(), ws=phys.get_warmstart().copy(), qfine_q=q64 - q[:, :43].astype(np.float64),
                qfine_v=v64 - v[:, :39].astype(np.float64), ctrl=phys.ctrl().copy(), status=phys.status().copy(),
                nstep=phys.time().copy(), stats=phys.solver_stats().copy())


def _bench_law(solver, N, T, env, tpl, monkeypatch):
    """T ticks of the benchmark's law (bench.setup_envs, rng.random_actions) in one rollout call."""
    import torch
    import bench
    from mujoco_robot_environments_amd import rng
    from mujoco_robot_environments_amd.physics import BatchedPhysics
    _knobs(monkeypatch, env)
    phys = BatchedPhysics(N, solver=solver)
    bench.setup_envs(phys, 0, np.arange(N))
    seq = torch.from_numpy(rng.random_actions(0, np.arange(N), np.arange(T)).astype(np.float32)).to(phys.device)
    q0 = phys.queue_info()
    phys.rollout(seq, control_steps=5, ticks_per_launch=tpl)
    out = _words(phys)
    q1 = phys.queue_info()
    out["queue"] = {k: q1[k] - q0[k] for k in ("launches", "handovers")}
    phys.close()
    return out


_REF = {}


def _per_tick(solver, N, T, monkeypatch):
    """The reference, once per (solver, batch): one launch per tick and env, nothing handed over.  Never modified."""
    key = (solver, N, T)
    if key not in _REF:
        _REF[key] = _bench_law(solver, N, T, {"MRE_QUEUE": "0"}, 1, monkeypatch)
        assert _REF[key]["queue"]["launches"] == 0
    return _REF[key]


def _same(ref, got, what):
    for k in WORDS:
        assert np.array_equal(ref[k], got[k]), (what, k, int((ref[k] != got[k]).sum()))


@pytest.mark.parametrize("serial", ["0", "1"])
@pytest.mark.parametrize("solver", ["Newton", "PGS"])
def test_192_envs_on_64_waves_equal_per_tick_launches(solver, serial, monkeypatch):
    """192 envs on 64 waves x 12 ticks: three envs per wave, so every wave has taken its next item before it lists the
    current one, and an env changes waves (and compute units, and XCDs) from tick to tick.  qpos, qvel, warm start, every
    low word of qfine, ctrl, status, step count and solver statistics equal those of per-tick launches bit for bit -- with
    the two kernels of the launch side by side and with the large kernel's waiting launch strictly first
    (MRE_QUEUE_TEST_SERIAL=1)."""
    ref = _per_tick(solver, 192, 12, monkeypatch)
    got = _bench_law(solver, 192, 12, {"MRE_QUEUE_WAVES": "64", "MRE_QUEUE_MIN_TICKS": "2", "MRE_QUEUE_TEST_SERIAL": serial}, 0,
                     monkeypatch)
    assert got["queue"]["launches"] == 1, got["queue"]
    _same(ref, got, (solver, serial))


@pytest.mark.parametrize("solver", ["Newton", "PGS"])
def test_65_envs_on_64_waves(solver, monkeypatch):
    """One env more than waves: the wave that finishes first finds the one listed env early, every other wave finds
    nothing early, lists its own env and takes it again (or another wave's) at its late look; at the end of the launch
    the waves leave one by one."""
    ref = _per_tick(solver, 65, 12, monkeypatch)
    got = _bench_law(solver, 65, 12, {"MRE_QUEUE_WAVES": "64", "MRE_QUEUE_MIN_TICKS": "2"}, 0, monkeypatch)
    assert got["queue"]["launches"] == 1, got["queue"]
    _same(ref, got, solver)


@pytest.mark.parametrize("solver", ["Newton", "PGS"])
def test_40_envs_with_64_waves_allowed(solver, monkeypatch):
    """Fewer envs than the waves allowed.  The library starts at most one wave per env and takes queue launches only for
    a batch larger than the wave count (policy::queue_fits), so with 64 waves allowed these 40 envs are stepped by the
    launches without a queue; with 39 allowed they are a queue launch of 39 waves in 16 shards of two or three envs, where
    a wave whose shard is empty looks through the others and the last ticks have more waves than listed envs."""
    ref = _per_tick(solver, 40, 12, monkeypatch)
    got = _bench_law(solver, 40, 12, {"MRE_QUEUE_WAVES": "64", "MRE_QUEUE_MIN_TICKS": "2"}, 0, monkeypatch)
    assert got["queue"]["launches"] == 0, got["queue"]
    _same(ref, got, (solver, "64 waves allowed"))
    got = _bench_law(solver, 40, 12, {"MRE_QUEUE_WAVES": "39", "MRE_QUEUE_MIN_TICKS": "2"}, 0, monkeypatch)
    assert got["queue"]["launches"] == 1, got["queue"]
    _same(ref, got, (solver, "39 waves"))


def _grasp_then_random(solver, env, monkeypatch, N=64, ticks=30):
    """The scene of tests/test_gpu_queue.py whose envs outgrow the compact capacities in the middle of a rollout: a grasp
    on the table (contacts pile up on the pads), then `ticks` ticks of random controls in ONE rollout call."""
    import torch
    import bench
    from mujoco_robot_environments_amd import demo_logic, rng
    from mujoco_robot_environments_amd.physics import BatchedPhysics
    _knobs(monkeypatch, env)
    phys = BatchedPhysics(N, solver=solver)
    bench.setup_envs(phys, 7, np.arange(N))
    cube = phys.qpos()[:, 15:22].astype(np.float64)
    yaw = np.abs(demo_logic.quat_to_yaw_deg(cube[:, 3:7]))
    quat = demo_logic.grasp_quat(np.minimum(yaw, yaw - 90.0))
    pick = np.concatenate([cube[:, :2], np.full((N, 1), 0.565)], axis=1)
    pre = pick.copy()
    pre[:, 2] = 0.9
    phys.osc_set_target(position=pre, quat=quat, velocity=np.zeros(3), angular_velocity=np.zeros(3))
    phys.gripper_set(np.zeros(N, np.uint8))
    phys.run_controller(400, 5)
    phys.osc_set_target(position=pick)
    phys.run_controller(400, 5)
    phys.gripper_set(np.ones(N, np.uint8))
    phys.run_controller(200, 5)
    phys.set_fallback(0)      # every env back on the compact kernel: the rollout has to move the grasping ones itself
    phys.set_fallback(1)
    fb0, q0 = phys.fallback_stats(), phys.queue_info()
    seq = torch.from_numpy(rng.random_actions(3, np.arange(N), np.arange(ticks), scale=0.3).astype(np.float32)).to(phys.device)
    phys.rollout(seq, control_steps=5)
    out = _words(phys)
    fb1, q1 = phys.fallback_stats(), phys.queue_info()
    out["reruns"] = fb1["reruns"] - fb0["reruns"]
    out["queue"] = {k: q1[k] - q0[k] for k in ("launches", "handovers")}
    phys.close()
    return out


def test_abandoned_tick_keeps_the_item_taken_early(monkeypatch):
    """64 grasping envs on 16 waves (Newton: both kernels take early): a tick that overflows the compact capacities is
    abandoned after the wave has taken its next item -- the cubes' low words are put back, the env is listed for the large
    kernel, and the item taken early is stepped next, once.  The hand-over happened, and every word equals the host-side
    fallback's (rows restored, launch re-run on the large kernel)."""
    ref = _grasp_then_random("Newton", {"MRE_QUEUE": "0", "MRE_GROUPS": "1"}, monkeypatch)
    assert ref["queue"]["launches"] == 0 and ref["reruns"] > 0, (ref["queue"], ref["reruns"])
    got = _grasp_then_random("Newton", {"MRE_QUEUE_WAVES": "16", "MRE_QUEUE_SHARDS": "4", "MRE_QUEUE_MIN_TICKS": "2"}, monkeypatch)
    assert got["queue"]["launches"] == 1 and got["queue"]["handovers"] > 0 and got["reruns"] == 0, (got["queue"], got["reruns"])
    _same(ref, got, "hand-over")


@pytest.mark.parametrize("solver", ["Newton", "PGS"])
def test_converged_flag_travels_with_the_env(solver, monkeypatch):
    """64 envs x 20 ticks through mre_run_controller, three phases: targets from 0 to 5 cm above the tool's pose (an env
    converges at a tick of its own, or not at all) and out of reach for every seventh env.  The converged flag is one
    byte that travels with the env from tick to tick: flags of every phase, status and every state word equal the launches
    without a queue."""
    import bench
    from mujoco_robot_environments_amd.physics import BatchedPhysics
    N = 64
    out = {}
    for name, env in (("ref", {"MRE_QUEUE": "0"}),
                      ("queue", {"MRE_QUEUE_WAVES": "16", "MRE_QUEUE_SHARDS": "4", "MRE_QUEUE_MIN_TICKS": "2"})):
        _knobs(monkeypatch, env)
        phys = BatchedPhysics(N, solver=solver)
        bench.setup_envs(phys, 7, np.arange(N))
        tcp = phys.sites()[0].astype(np.float64)
        tgt = tcp.copy()
        tgt[:, 2] += np.arange(N) / N * 0.05
        tgt[::7, 2] = 2.5
        phys.osc_set_target(position=tgt, quat=np.tile(np.array([0.0, 1.0, 0.0, 0.0]), (N, 1)), velocity=np.zeros(3),
                            angular_velocity=np.zeros(3))
        phys.gripper_set(np.zeros(N, np.uint8))
        conv = [phys.run_controller(20, 5).copy() for _ in range(3)]
        o = _words(phys)
        o["conv"] = np.stack(conv)
        o["launches"] = phys.queue_info()["launches"]
        out[name] = o
        phys.close()
    ref, got = out["ref"], out["queue"]
    assert ref["launches"] == 0 and got["launches"] == 3, (ref["launches"], got["launches"])
    assert not ref["conv"][:, ::7].any() and (ref["status"][::7] & 1).all()      # out of reach: NOT_CONVERGED
    assert np.array_equal(ref["conv"], got["conv"]), solver
    _same(ref, got, solver)
