"""mre_get_arm_dynamics / BatchedPhysics.arm_dynamics(): the arm's site Jacobian, mass matrix and bias force exported as
CUDA tensors (csrc/mre_kernels.hip: k_arm_dynamics), the operational-space law in torch over them
(controllers/torch_osc.py) and the hook that runs such a law in RobotArm.run_controller.

References are fp64 and independent of the device code: the Jacobian by central differences of the model's own forward
kinematics (model/compile.py), the mass matrix by its sum_b J_b' I_b J_b formula, bias force / site pose / torques / the
controller loop from the CPU oracle."""
import numpy as np
import pytest

from mujoco_robot_environments_amd.model import compile as MC
from tests.common import HOME, init_oracle_env
from tests.test_torch_osc import GAINS, site_jacobian

pytestmark = pytest.mark.gpu

SITES = {"eef": "eef_site", "pinch": "tcp_site"}
# Worst error of every exported array over the 8 envs and both sites, relative to the array's largest magnitude, as
# measured on the MI355X (float32 rounding of the device's kinematics / CRB / RNE); the bound is 8 x that, rounded up to
# one digit -- the error varies with the pose.
EXPORT_BOUND = {
    "jac": 2e-6,        # measured 1.35e-07
    "mass": 8e-7,       # measured 9.53e-08
    "bias": 1e-6,       # measured 1.23e-07
    "site_pos": 6e-7,   # measured 6.60e-08
    "site_quat": 2e-6,  # measured 1.92e-07 (pinch site; controller site 7.72e-08)
}
CAP = 1e-4   # whatever was measured: a wrong frame, sign, reference point or row order costs 1e-2 or more
TOL, QVEL_TOL = 1e-4, 1e-2   # the project's bars on qpos / qvel against the oracle (tests/test_gpu_newton.py)


class Scene:
    """8 envs, no cubes: arm at HOME +- 0.3 rad with velocities +- 0.5; envs 0..2 with finger joints away from zero and
    finger velocities (reflected gripper inertia, Coriolis terms of the linkage).  The state is float32-rounded: device
    and oracle hold the same numbers."""

    def __init__(self, A, oracle_model):
        from oracle import oracle as O
        self.A, self.N = A, 8
        rs = np.random.RandomState(12)
        self.qpos = np.zeros((self.N, 43), np.float32)
        self.qvel = np.zeros((self.N, 39), np.float32)
        self.envs = []
        for i in range(self.N):
            e = O.Env(oracle_model, nprops=0)
            q = e.arr("qpos")
            q[:7] = np.array(HOME) + rs.uniform(-0.3, 0.3, 7)
            e.arr("qvel")[:7] = rs.uniform(-0.5, 0.5, 7)
            if i < 3:
                q[7:15] = rs.uniform(0.05, 0.3, 8) * [1, -1, 1, -1, 1, -1, 1, -1]
                e.arr("qvel")[7:15] = rs.uniform(-0.5, 0.5, 8)
            q[:43] = q[:43].astype(np.float32)
            e.arr("qvel")[:39] = e.arr("qvel")[:39].astype(np.float32)
            e.forward()
            self.qpos[i], self.qvel[i] = q[:43], e.arr("qvel")[:39]
            self.envs.append(e)
        # targets a few centimetres and 0.2 rad away from where the controller site is
        st = int(A["eef_site"][0])
        self.tgt_pos = np.zeros((self.N, 3), np.float32)
        self.tgt_quat = np.zeros((self.N, 4), np.float32)
        for i, e in enumerate(self.envs):
            self.tgt_pos[i] = e.arr("site_xpos")[3 * st:3 * st + 3] + rs.uniform(-0.05, 0.05, 3)
            ax = rs.randn(3)
            ax /= np.linalg.norm(ax)
            rot = np.concatenate([[np.cos(0.1)], np.sin(0.1) * ax])
            self.tgt_quat[i] = MC.qmul(rot, MC.m2q(e.arr("site_xmat")[9 * st:9 * st + 9].reshape(3, 3)))

    def handle(self, solver):
        from mujoco_robot_environments_amd.physics import BatchedPhysics
        phys = BatchedPhysics(self.N, model=self.A, solver=solver)
        phys.set_props(np.zeros(self.N, np.int32), np.full((self.N, 4, 3), 0.0155))
        phys.reset()
        qp = phys.qpos().copy()
        qp[:, :15] = self.qpos[:, :15]     # (the cube slots stay parked)
        phys.set_state(qp, self.qvel)
        return phys


@pytest.fixture(scope="module")
def scene(compiled_model, oracle_model):
    return Scene(compiled_model[0], oracle_model)


def test_export_against_fp64_references(scene):
    A = scene.A
    pgs, newton = scene.handle("PGS"), scene.handle("Newton")
    worst = {k: 0.0 for k in EXPORT_BOUND}
    for site, key in SITES.items():
        t = pgs.arm_dynamics(site)
        assert t.raw.is_cuda and tuple(t.raw.shape) == (scene.N, 128)
        raw = t.raw.cpu().numpy()
        assert np.array_equal(raw, newton.arm_dynamics(site).raw.cpu().numpy()), "the export depends on the handle's solver"
        assert (raw[:, 119:] == 0).all()
        got = {k: v.cpu().numpy().astype(np.float64) for k, v in t.as_dict().items()}
        assert np.array_equal(got["qpos"], scene.qpos[:, :7]) and np.array_equal(got["qvel"], scene.qvel[:, :7])
        st = int(A[key][0])
        ref = {k: [] for k in EXPORT_BOUND}
        for i, e in enumerate(scene.envs):
            q0 = scene.qpos[i].astype(np.float64)
            _, _, J = site_jacobian(A, q0, st)
            ref["jac"].append(J)
            ref["mass"].append(MC.dense_mass_matrix(A, q0)[:7, :7])
            ref["bias"].append(np.array(e.arr("qfrc_bias")[:7]))
            ref["site_pos"].append(np.array(e.arr("site_xpos")[3 * st:3 * st + 3]))
            q = MC.m2q(e.arr("site_xmat")[9 * st:9 * st + 9].reshape(3, 3))
            ref["site_quat"].append(q if np.dot(q, got["site_quat"][i]) >= 0 else -q)   # (q and -q: one rotation)
        for k in EXPORT_BOUND:
            r = np.array(ref[k])
            err = np.abs(got[k] - r).max() / np.abs(r).max()
            print(f"arm_dynamics({site!r}) {k}: max abs err / max |ref| = {err:.2e} (max |ref| {np.abs(r).max():.3g})")
            worst[k] = max(worst[k], err)
    print("arm_dynamics worst relative errors:", {k: f"{v:.2e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v < CAP, (k, v)
        assert v < EXPORT_BOUND[k], (k, v, EXPORT_BOUND[k])
    pgs.close()
    newton.close()


@pytest.mark.parametrize("pinv_always", [0, 1])
def test_the_law_three_ways(scene, pinv_always):
    """TorchOSC on the exported terms, the in-kernel law (mre_osc_compute) and the oracle's: each device result within
    2e-4 * max(1, |tau|max) of the oracle's."""
    from mujoco_robot_environments_amd.controllers.torch_osc import TorchOSC
    from oracle import oracle as O
    ref = np.zeros((scene.N, 7))
    for i, e in enumerate(scene.envs):
        p = O.make_osc()
        p.target_pos[:] = scene.tgt_pos[i]
        p.target_quat[:] = scene.tgt_quat[i]
        p.pinv_always = pinv_always
        ref[i] = e.osc(p)
    target = dict(eef_target_position=scene.tgt_pos, eef_target_quat=scene.tgt_quat, eef_target_velocity=np.zeros(3),
                  eef_target_angular_velocity=np.zeros(3))
    bound = 2e-4 * np.maximum(1.0, np.abs(ref).max(axis=1))
    for solver in ("PGS", "Newton"):
        phys = scene.handle(solver)
        tau = TorchOSC(gains=GAINS, pinv_always=bool(pinv_always))(phys.arm_dynamics("eef"), target)
        assert tau.is_cuda and tuple(tau.shape) == (scene.N, 7)
        e_torch = np.abs(tau.cpu().numpy() - ref).max(axis=1)
        phys.osc_configure(gains=GAINS, pinv_always=bool(pinv_always))
        phys.osc_set_target(position=scene.tgt_pos, quat=scene.tgt_quat, velocity=np.zeros(3, np.float32),
                            angular_velocity=np.zeros(3, np.float32))
        e_kernel = np.abs(phys.osc_compute()[0].astype(np.float64) - ref).max(axis=1)
        print(f"{solver} handle, pinv_always {pinv_always}: max |tau - oracle| / bound: TorchOSC {(e_torch / bound).max():.3f} "
              f"({e_torch.max():.2e}), in-kernel {(e_kernel / bound).max():.3f} ({e_kernel.max():.2e}); |tau|max {np.abs(ref).max():.1f}")
        assert (e_torch < bound).all(), (e_torch, bound)
        assert (e_kernel < bound).all(), (e_kernel, bound)
        phys.close()


def _snapshot(phys):
    q, v = phys.get_state_f64()
    return dict(qpos=q, qvel=v, ws=phys.get_warmstart().copy(), ctrl=phys.ctrl().copy(), time=phys.time().copy(),
                status=phys.status().copy())


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def _held_controls_run(case, export, monkeypatch):
    """20 control ticks of 5 steps under random held controls; `export`: arm_dynamics() after every tick (queue case:
    between the rollout windows of 4 ticks).  Returns the final snapshot and the number of queue launches."""
    import torch
    import bench
    from mujoco_robot_environments_amd import rng
    from mujoco_robot_environments_amd.physics import BatchedPhysics
    for k in ("MRE_QUEUE", "MRE_QUEUE_WAVES", "MRE_QUEUE_SHARDS", "MRE_QUEUE_TICKS", "MRE_QUEUE_MIN_TICKS", "MRE_GROUPS"):
        monkeypatch.delenv(k, raising=False)
    N = 16
    if case == "queue":
        # (a queue launch needs more envs than waves: the knobs of tests/test_gpu_queue.py at that test's 64 envs)
        N = 64
        for k, v in {"MRE_QUEUE_WAVES": "16", "MRE_QUEUE_SHARDS": "4", "MRE_QUEUE_MIN_TICKS": "2"}.items():
            monkeypatch.setenv(k, v)
    phys = BatchedPhysics(N, solver="Newton")
    ids = np.arange(N)
    if case == "free":
        phys.set_props(np.zeros(N, np.int32), np.full((N, 4, 3), 0.0155))
        phys.reset()
    else:
        bench.setup_envs(phys, 7, ids)     # cubes settled on the table: every env steps with contacts
    T = 20
    acts = rng.random_actions(3, ids, np.arange(T), scale=0.3).astype(np.float32)
    outs = []
    if case == "queue":
        seq = torch.from_numpy(acts).to(phys.device)
        for w in range(0, T, 4):
            phys.rollout(seq[w:w + 4].contiguous(), control_steps=5)
            if export:
                outs.append(phys.arm_dynamics("eef").raw)
    else:
        for t in range(T):
            phys.set_control(acts[t])
            phys.step(5)
            if export:
                outs.append(phys.arm_dynamics("pinch" if t % 2 else "eef").raw)
    snap = _snapshot(phys)
    if case != "free":
        assert (phys.solver_stats()[:, 0] > 0).all(), "the scenario has contacts"
    launches = phys.queue_info()["launches"]
    if export:
        assert all(bool(torch.isfinite(o).all()) for o in outs)
    phys.close()
    return snap, launches


@pytest.mark.parametrize("case", ["free", "contact", "queue"])
def test_exports_between_ticks_leave_the_run_unchanged(case, monkeypatch):
    plain, lp = _held_controls_run(case, False, monkeypatch)
    with_export, le = _held_controls_run(case, True, monkeypatch)
    assert (lp > 0) == (case == "queue") and le == lp, (lp, le)
    assert np.isfinite(plain["qpos"]).all()
    _same(plain, with_export, case)


def test_export_touches_nothing(scene):
    phys = scene.handle("Newton")
    phys.set_control(np.tile(np.array([3, -20, 2, 15, 1, -1, 0.5, 100], np.float32), (scene.N, 1)))
    phys.step(5)      # (a warm start, a clock and controls that are not zero)
    before = _snapshot(phys)
    assert np.abs(before["ws"]).max() > 0 and (before["time"] > 0).all()
    for site in ("eef", "pinch", "eef"):
        phys.arm_dynamics(site)
    phys.sync()
    _same(before, _snapshot(phys), "arm_dynamics")
    phys.close()


def test_torque_law_hook_runs_the_controller_loop(compiled_model, oracle_model):
    """RobotArm(..., torque_law=TorchOSC) against mro_run_controller and against the in-kernel loop of a twin handle: the
    set-up of tests/test_gpu_newton.py::test_newton_run_controller_parity (even envs towards a reachable pre-pick pose,
    odd envs 1.5 m away, Newton) over 200 ticks -- every even env converges within them in the oracle (checked on the
    CPU when the targets were chosen)."""
    from mujoco_robot_environments_amd import rng
    from mujoco_robot_environments_amd.controllers.torch_osc import TorchOSC
    from mujoco_robot_environments_amd.models.robot_arm import RobotArm
    from mujoco_robot_environments_amd.physics import BatchedPhysics
    from mujoco_robot_environments_amd.tasks.rearrangement import home_quat
    from oracle import oracle as O
    A, _ = compiled_model
    N, seed = 16, 9
    ids = np.arange(N)
    nprops, sizes = rng.prop_params(seed, ids)
    u = rng.uniform(seed + 1, ids, [0], 3)[0]
    tgt = (u * [0.2, 0.5, 0.0] + [0.35, -0.25, 0.9])
    tgt[1::2, 0] = 1.5
    tgt = tgt.astype(np.float32)
    quat = home_quat().astype(np.float32)
    grip = ((ids // 2) % 2).astype(np.uint8)
    envs, q0 = [], np.zeros((N, 43))
    for i in range(N):
        e = O.Env(oracle_model, int(nprops[i]), sizes[i])
        e.set_solver("Newton")
        q0[i] = init_oracle_env(e, int(nprops[i]), sizes[i], z_extra=0.0005)
        envs.append(e)

    def handle():
        phys = BatchedPhysics(N, model=A, solver="Newton")
        phys.set_props(nprops, sizes)
        qp = phys.qpos().copy()
        for i in range(N):
            n = int(nprops[i])
            qp[i, :15 + 7 * n] = q0[i, :15 + 7 * n]
        phys.set_state(qp, np.zeros((N, 39), np.float32))
        return phys, qp

    def arm(phys, law):
        robot = RobotArm(phys, torque_law=law)
        robot.arm_controller.set_target(position=tgt, quat=np.tile(quat, (N, 1)), velocity=np.zeros(3),
                                        angular_velocity=np.zeros(3))
        robot.end_effector_controller.status = ["max" if g else "min" for g in grip]
        return robot

    phys, qp = handle()
    robot = arm(phys, TorchOSC(gains=GAINS))
    assert robot.ticks_for(1.0) == 200 and robot.control_steps == 5
    conv = robot.run_controller(1.0)
    phys.sync()
    gq, gv = phys.get_state()
    status = phys.status()
    twin, _ = handle()
    tconv = arm(twin, None).run_controller(1.0)
    oconv = np.zeros(N, bool)
    worst, worst_v = np.zeros(N), np.zeros(N)
    for i, e in enumerate(envs):
        e.arr("qpos")[:43] = qp[i]
        e.forward()
        p = O.make_osc()
        p.target_pos[:] = tgt[i]
        p.target_quat[:] = quat
        oconv[i] = e.run_controller(p, 255.0 if grip[i] else 0.0, 200, 5)
        n = int(nprops[i])
        worst[i] = np.abs(gq[i, :15 + 7 * n] - e.arr("qpos")[:15 + 7 * n]).max()
        worst_v[i] = np.abs(gv[i, :15 + 6 * n] - e.arr("qvel")[:15 + 6 * n]).max()
    print("torque-law hook: max |dqpos| per env", np.round(worst, 7).tolist(), "max |dqvel|", np.round(worst_v, 5).tolist(),
          "converged", conv.tolist())
    assert oconv[0::2].any() and not oconv[1::2].all()     # the reference alone: flags of both kinds occur
    assert (conv == oconv).all(), (conv, oconv)
    assert (tconv == conv).all(), (tconv, conv)
    assert (worst[0::2] < TOL).all() and (worst_v[0::2] < QVEL_TOL).all()
    # the one documented difference: MRE_ST_NOT_CONVERGED is the in-kernel loop's
    assert ((status & 1) == 0).all() and (((twin.status() & 1) != 0) == ~tconv).all()
    phys.close()
    twin.close()


def test_arguments(compiled_model):
    import ctypes as C
    import torch
    from mujoco_robot_environments_amd import lib
    from mujoco_robot_environments_amd.physics import BatchedPhysics
    phys = BatchedPhysics(1, model=compiled_model[0])
    L = lib.lib()
    out = torch.zeros((1, lib.MRE_DYN_W), dtype=torch.float32, device=phys.device)
    assert L.mre_get_arm_dynamics(phys._h, 2, out.data_ptr()) == -1      # MRE_ERR_ARG
    assert L.mre_get_arm_dynamics(phys._h, -1, out.data_ptr()) == -1
    assert L.mre_get_arm_dynamics(phys._h, 0, None) == -1
    assert L.mre_get_arm_dynamics(None, 0, out.data_ptr()) == -1
    phys.sync()
    assert (out == 0).all()
    with pytest.raises(lib.MreError):
        phys.arm_dynamics(2)
    t = phys.arm_dynamics()
    shapes = {k: tuple(v.shape) for k, v in t.as_dict().items()}
    assert shapes == dict(jac=(1, 6, 7), mass=(1, 7, 7), bias=(1, 7), site_pos=(1, 3), site_quat=(1, 4), qpos=(1, 7),
                          qvel=(1, 7))
    assert all(v.is_cuda and v.dtype == torch.float32 for v in t.as_dict().values())
    assert np.allclose(t.qpos.cpu().numpy()[0], HOME) and bool(torch.isfinite(t.raw).all())
    m = t.mass[0].cpu().numpy()
    assert np.array_equal(m, m.T) and np.linalg.eigvalsh(m.astype(np.float64)).min() > 0
    phys.close()
