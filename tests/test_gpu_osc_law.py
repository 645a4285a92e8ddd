"""The operational-space law on the device (csrc/mre_osc.h through mre_osc_compute, mre_osc_configure[_env],
mre_osc_set_target, mre_gripper_set and one tick of mre_run_controller) against the fp64 oracle at the cases of
tests/osc_cases.py: target velocities, the law's own |det| < 1e-2 -> pinv switch, ill-conditioned inverses, the four
branches of mat2q, both sides of the hemisphere sign, per-env gains / null_q / thresholds, the target merge, the
gripper command and the convergence thresholds.  tests/test_osc_cases.py shows on the CPU that the cases are clear of
the law's discontinuities and that a law with one thing wrong misses these comparisons by 10 x the bar or more.

One env per (case, target); every launch is a zero-step launch except the single ticks of the last test.

Bar: the project's, 2e-4 * max(1, |tau|max) against the oracle (tests/osc_cases.py: bar; no case needed the widened
bar of WIDENED_BAR).  Worst |tau - oracle| / bar per class as measured on the MI355X (float32 kinematics / CRB / RNE,
float32 Gauss-Jordan and Jacobi), the same on the PGS and the Newton handle and for a target and its -quat twin:

    class        in-kernel   TorchOSC on the export        in-kernel, per-env configuration
    regular      0.005       0.003                         0.003
    pinv         0.023       0.003                         0.012
    illcond      0.031       0.003                         0.053
    mat2q_t      0.013       0.004                         0.010
    mat2q_m0     0.049       0.003                         0.026
    mat2q_m4     0.119       0.014                         0.072
    mat2q_m8     0.008       0.006                         0.009
    threshold    0.003       0.002                         0.003
    pinv_always = 1:  regular 0.004 / 0.002, illcond 0.002 / 0.000, threshold 0.008 / 0.004  (|tau|max 926 N m)

(|tau|max 746 N m, at an ill-conditioned pose.)  The torque a tick of run_controller applies and the zero-step
evaluation just before it have the same bits, on the compact and on the large kernel (test_one_tick_in_the_loop): the
stages a tick runs between the velocity stage and the law (finger bias, collision, constraint assembly) write nothing
the law reads.
"""
import numpy as np
import pytest

from tests import osc_cases as OC

pytestmark = pytest.mark.gpu


class Rig:
    """The rows (case, target) = envs, one handle per solver kept for the module, and the oracle's torques."""

    def __init__(self, A, oracle_model):
        self.A, self.oracle_model = A, oracle_model
        self.table = OC.cases(A, oracle_model)
        self.rows = [(c, t) for c in self.table for t in c.targets.values()]
        self.N = len(self.rows)
        assert self.N <= 64
        self.cls = np.array([c.cls for c, _ in self.rows])
        self.forced = np.isin(self.cls, OC.FORCED_CLASSES)
        self.qpos = np.stack([c.qpos for c, _ in self.rows])
        self.qvel = np.stack([c.qvel for c, _ in self.rows])
        self.gains = np.stack([c.config.gains for c, _ in self.rows]).astype(np.float32)
        self.null_q = np.stack([c.config.null_q for c, _ in self.rows]).astype(np.float32)
        self.thresholds = np.stack([c.config.thresholds for c, _ in self.rows]).astype(np.float32)
        self._handles, self._refs = {}, {}

    def targets(self, sign=1):
        return [t if sign > 0 else t.negated() for _, t in self.rows]

    @staticmethod
    def arrays(targets):
        return dict(position=np.stack([t.pos for t in targets]), quat=np.stack([t.quat for t in targets]),
                    velocity=np.stack([t.vel for t in targets]), angular_velocity=np.stack([t.angvel for t in targets]))

    def own_config(self, i):
        """Row i's own configuration as the device holds it (float32 numbers)."""
        return OC.Config(self.gains[i], self.null_q[i], self.thresholds[i])

    def reference(self, targets, own=False, pinv_always=0, key=None):
        """The oracle's torque [N, 7] of every row at `targets` (cached under `key`)."""
        k = (key, own, pinv_always)
        if key is None or k not in self._refs:
            ref = np.stack([OC.oracle_law(c.env, t, self.own_config(i) if own else OC.SHARED, pinv_always)
                            for i, ((c, _), t) in enumerate(zip(self.rows, targets))])
            if key is None:
                return ref
            self._refs[k] = ref
        return self._refs[k]

    def bars(self, ref, targets):
        return np.array([OC.bar(r, (c.name, t.name)) for r, (c, _), t in zip(ref, self.rows, targets)])

    def fresh(self, solver, pinv_always=0, sign=1):
        """The handle of `solver` back at the cases' states: shared configuration, the rows' targets, gripper open."""
        from mujoco_robot_environments_amd.physics import BatchedPhysics
        if solver not in self._handles:
            phys = BatchedPhysics(self.N, model=self.A, solver=solver)
            phys.set_props(np.zeros(self.N, np.int32), np.full((self.N, 4, 3), 0.0155))
            self._handles[solver] = phys
        phys = self._handles[solver]
        phys.set_fallback(True)
        phys.reset()
        qp = phys.qpos().copy()
        qp[:, :15] = self.qpos          # (the cube slots stay parked)
        qv = np.zeros((self.N, 39), np.float32)
        qv[:, :15] = self.qvel
        phys.set_state(qp, qv)
        phys.osc_configure(gains=OC.GAINS, null_q=OC.NULL_Q, thresholds=OC.THRESHOLDS, pinv_always=bool(pinv_always))
        phys.osc_set_target(**self.arrays(self.targets(sign)))
        phys.gripper_set(np.zeros(self.N, np.uint8))
        phys.sync()
        return phys

    def close(self):
        for phys in self._handles.values():
            phys.close()

    def per_class(self, ratio, select=None):
        out = {}
        for i, cls in enumerate(self.cls):
            if select is None or select[i]:
                out[str(cls)] = max(out.get(str(cls), 0.0), float(ratio[i]))
        return {k: f"{v:.3f}" for k, v in out.items()}


@pytest.fixture(scope="module")
def rig(compiled_model, oracle_model):
    r = Rig(compiled_model[0], oracle_model)
    yield r
    r.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _torch_target(arrays):
    return dict(eef_target_position=arrays["position"], eef_target_quat=arrays["quat"],
                eef_target_velocity=arrays["velocity"], eef_target_angular_velocity=arrays["angular_velocity"])


@pytest.mark.parametrize("pinv_always", [0, 1])
@pytest.mark.parametrize("solver", ["PGS", "Newton"])
def test_the_law_against_the_oracle(rig, solver, pinv_always):
    """mre_osc_compute and TorchOSC over arm_dynamics("eef") of the same handle, each within the bar of the oracle on
    every row, for the targets and for their -quat twins.  pinv_always = 1 is compared on the regular and the
    ill-conditioned poses (the other poses were not selected clear of the pinv's cutoff)."""
    from mujoco_robot_environments_amd.controllers.torch_osc import TorchOSC
    select = rig.forced if pinv_always else np.ones(rig.N, bool)
    assert select.sum() >= 2 + 3 + 2 + 3
    for sign in (1, -1):
        phys = rig.fresh(solver, pinv_always, sign)
        targets = rig.targets(sign)
        ref = rig.reference(targets, False, pinv_always, key=("rows", sign))
        bars = rig.bars(ref, targets)
        tau = phys.osc_compute()[0]
        assert tau.dtype == np.float32 and tau.shape == (rig.N, 7) and np.isfinite(tau).all()
        e_kernel = np.abs(tau.astype(np.float64) - ref).max(axis=1) / bars
        law = TorchOSC(gains=OC.GAINS, pinv_always=bool(pinv_always))
        t_torch = law(phys.arm_dynamics("eef"), _torch_target(rig.arrays(targets)))
        assert t_torch.is_cuda and tuple(t_torch.shape) == (rig.N, 7)
        e_torch = np.abs(t_torch.cpu().numpy() - ref).max(axis=1) / bars
        print(f"{solver} handle, pinv_always {pinv_always}, quat sign {sign:+d}: worst |tau - oracle| / bar per class: "
              f"in-kernel {rig.per_class(e_kernel, select)}; TorchOSC {rig.per_class(e_torch, select)}; "
              f"|tau|max {np.abs(ref[select]).max():.0f}")
        assert (e_kernel[select] < 1.0).all(), [(rig.rows[i][0].name, rig.rows[i][1].name, e_kernel[i])
                                                for i in np.nonzero(select & (e_kernel >= 1.0))[0]]
        assert (e_torch[select] < 1.0).all(), [(rig.rows[i][0].name, rig.rows[i][1].name, e_torch[i])
                                               for i in np.nonzero(select & (e_torch >= 1.0))[0]]


def _snapshot(phys):
    q, v = phys.get_state_f64()
    return dict(qpos=q, qvel=v, ws=phys.get_warmstart().copy(), time=phys.time().copy(), status=phys.status().copy())


@pytest.mark.parametrize("pinv_always", [0, 1])
def test_exact_properties_of_the_law(rig, pinv_always):
    """Bit for bit: -quat is the same target; zero gains leave the bias force; the solver of the handle does not enter;
    the evaluation repeats and touches nothing of the state."""
    tau = {}
    for solver in ("PGS", "Newton"):
        phys = rig.fresh(solver, pinv_always, 1)
        tau[solver] = phys.osc_compute()[0]
        phys.osc_set_target(quat=rig.arrays(rig.targets(-1))["quat"])
        assert np.array_equal(_bits(phys.osc_compute()[0]), _bits(tau[solver])), (solver, "-quat")
    assert np.array_equal(_bits(tau["PGS"]), _bits(tau["Newton"]))
    # zero gains: F = 0 and tau0 = 0, so that what is left is qfrc_bias -- the bias arm_dynamics exports
    phys.osc_configure(gains=np.zeros(6), pinv_always=bool(pinv_always))
    bias = phys.arm_dynamics("eef").bias.cpu().numpy()
    assert np.abs(bias).max() > 1.0
    assert np.array_equal(phys.osc_compute()[0], bias)
    # a state with a warm start, a clock and a status; two evaluations
    phys = rig.fresh("Newton", pinv_always, 1)
    phys.set_control(np.tile(np.array([3, -20, 2, 15, 1, -1, 0.5, 100], np.float32), (rig.N, 1)))
    phys.step(5)
    phys.sync()
    before = _snapshot(phys)
    assert np.abs(before["ws"]).max() > 0 and (before["time"] > 0).all()
    first, g1 = phys.osc_compute()
    second, g2 = phys.osc_compute()
    assert np.isfinite(first).all() and not np.array_equal(first, tau["Newton"])
    assert np.array_equal(_bits(first), _bits(second)) and np.array_equal(g1, g2)
    after = _snapshot(phys)
    for k in before:
        assert np.array_equal(before[k], after[k]), k


def test_per_env_configuration(rig):
    """mre_osc_configure_env: gains x U(0.5, 1.5), a null_q and thresholds of its own for every env, each env against
    the oracle run with its own set (the thresholds: test_one_tick_in_the_loop); mre_osc_configure returns every env to
    the shared set."""
    targets = rig.targets(1)
    for solver in ("PGS", "Newton"):
        phys = rig.fresh(solver)
        shared = phys.osc_compute()[0]
        phys.osc_configure_env(gains=rig.gains, null_q=rig.null_q, thresholds=rig.thresholds)
        ref = rig.reference(targets, True, 0, key=("rows", 1))
        bars = rig.bars(ref, targets)
        own = phys.osc_compute()[0]
        err = np.abs(own.astype(np.float64) - ref).max(axis=1) / bars
        moved = np.abs(own.astype(np.float64) - shared).max(axis=1) / bars
        print(f"{solver} handle, per-env configuration: worst |tau - oracle| / bar per class {rig.per_class(err)}; the "
              f"configuration moves tau by {moved.min():.0f} .. {moved.max():.0f} bars")
        assert (err < 1.0).all(), err
        assert (moved > 10.0).all(), moved
        # only the nullspace configuration: gains and thresholds keep the shared set's values
        phys.osc_configure_env(null_q=rig.null_q)
        cfgs = [OC.Config(null_q=rig.null_q[i]) for i in range(rig.N)]
        ref_q = np.stack([OC.oracle_law(c.env, t, cfgs[i]) for i, ((c, _), t) in enumerate(zip(rig.rows, targets))])
        err_q = np.abs(phys.osc_compute()[0].astype(np.float64) - ref_q).max(axis=1) / rig.bars(ref_q, targets)
        assert (err_q < 1.0).all(), err_q
        phys.osc_configure(gains=OC.GAINS, null_q=OC.NULL_Q, thresholds=OC.THRESHOLDS)
        assert np.array_equal(_bits(phys.osc_compute()[0]), _bits(shared))


def test_target_merge(rig):
    """mre_osc_set_target keeps what it is not given, broadcasts a 1-D value and honours the per-env mask: after every
    call the torque is the oracle's for the target built on the host, and a masked-out env keeps its bits."""
    from mujoco_robot_environments_amd.model import compile as MC
    rs = np.random.RandomState(31)
    phys = rig.fresh("Newton")
    expect = rig.arrays(rig.targets(1))
    N = rig.N

    def other_quats():
        out = []
        for c, _ in rig.rows:
            ax = rs.randn(3)
            ax /= np.linalg.norm(ax)
            out.append(MC.qmul(np.concatenate([[np.cos(0.1)], np.sin(0.1) * ax]), c.terms.site_quat))
        return np.array(out, np.float32)

    def check(what, before=None, mask=None):
        targets = [OC.Target(t.name, expect["position"][i], expect["quat"][i], expect["velocity"][i],
                             expect["angular_velocity"][i]) for i, (_, t) in enumerate(rig.rows)]
        for (c, _), t in zip(rig.rows, targets):
            assert abs(OC.error_quaternion(c.terms, t)[0]) > OC.QE0_MIN
        ref = rig.reference(targets)
        tau = phys.osc_compute()[0]
        err = np.abs(tau.astype(np.float64) - ref).max(axis=1) / rig.bars(ref, targets)
        print(f"target merge, {what}: worst |tau - oracle| / bar {err.max():.3f}")
        assert (err < 1.0).all(), (what, err)
        if before is not None:
            keep = ~mask.astype(bool)
            assert np.array_equal(_bits(tau[keep]), _bits(before[keep])), what
            assert (np.abs(tau[~keep] - before[~keep]).max(axis=1) > 0).all(), what
        return tau

    tau = check("the full target")
    site = np.stack([c.terms.site_pos for c, _ in rig.rows])
    # 1. position alone: quaternion and velocities stay
    expect["position"] = (site + rs.uniform(-0.05, 0.05, (N, 3))).astype(np.float32)
    phys.osc_set_target(position=expect["position"])
    tau = check("position only")
    # 2. 1-D velocities: one value for every env; position and quaternion stay
    v, w = rs.uniform(-0.2, 0.2, 3).astype(np.float32), rs.uniform(-0.5, 0.5, 3).astype(np.float32)
    expect["velocity"], expect["angular_velocity"] = np.tile(v, (N, 1)), np.tile(w, (N, 1))
    phys.osc_set_target(velocity=v, angular_velocity=w)
    tau = check("1-D velocities")
    # 3. all four arrays under a mask of every third env
    mask = (np.arange(N) % 3 == 0).astype(np.uint8)
    new = dict(position=(site + rs.uniform(-0.05, 0.05, (N, 3))).astype(np.float32), quat=other_quats(),
               velocity=rs.uniform(-0.2, 0.2, (N, 3)).astype(np.float32),
               angular_velocity=rs.uniform(-0.5, 0.5, (N, 3)).astype(np.float32))
    for k in expect:
        expect[k] = np.where(mask[:, None] != 0, new[k], expect[k])
    phys.osc_set_target(mask=mask, **new)
    tau = check("four arrays, every third env", tau, mask)
    # 4. a 1-D quaternion-free call under another mask: angular velocity alone, envs 1, 4, 7, ...
    mask = (np.arange(N) % 3 == 1).astype(np.uint8)
    w = rs.uniform(-0.5, 0.5, 3).astype(np.float32)
    expect["angular_velocity"] = np.where(mask[:, None] != 0, w[None], expect["angular_velocity"])
    phys.osc_set_target(angular_velocity=w, mask=mask)
    tau = check("1-D angular velocity, envs 1, 4, 7, ...", tau, mask)
    # 5. the quaternion alone under the first mask
    mask = (np.arange(N) % 3 == 0).astype(np.uint8)
    q = other_quats()
    expect["quat"] = np.where(mask[:, None] != 0, q, expect["quat"])
    phys.osc_set_target(quat=q, mask=mask)
    check("quaternion only, every third env", tau, mask)


def test_gripper_command(rig):
    lo, hi = (float(x) for x in rig.A["act_ctrlrange"][7])
    assert (lo, hi) == (0.0, 255.0)
    phys = rig.fresh("PGS")
    assert (phys.osc_compute()[1] == lo).all()
    closed = (np.arange(rig.N) % 5 < 2).astype(np.uint8)
    phys.gripper_set(closed)
    tau, grip = phys.osc_compute()
    assert grip.dtype == np.float32 and np.array_equal(grip, np.where(closed != 0, hi, lo).astype(np.float32))
    phys.gripper_set(1 - closed)
    tau2, grip2 = phys.osc_compute()
    assert np.array_equal(grip2, np.where(closed != 0, lo, hi).astype(np.float32))
    assert np.array_equal(_bits(tau), _bits(tau2))      # (the gripper command does not enter the arm's law)


@pytest.mark.parametrize("own", [False, True], ids=["shared", "per_env"])
@pytest.mark.parametrize("solver", ["PGS", "Newton"])
def test_one_tick_in_the_loop(rig, solver, own):
    """run_controller(1, control_steps=1) from the cases' states: the controls it applied are, bit for bit, what the
    zero-step evaluation returned just before (the same function of the same state), on the compact and on the large
    kernel; the converged flags are the oracle's for its replay of the tick, with the envs of class "threshold" given
    targets at 0.98 x / 1.02 x the position threshold and at 2 arcsin(0.98 x / 1.02 x the orientation threshold) of the
    configuration in force."""
    targets = rig.targets(1)
    want = {}
    probes = [i for i in range(rig.N) if rig.cls[i] == "threshold"]
    assert len(probes) == 4
    for k, i in enumerate(probes):
        cfg = rig.own_config(i) if own else OC.SHARED
        name = ("pos0.98", "pos1.02", "ori0.98", "ori1.02")[k]
        targets[i], want[i] = OC.threshold_targets(rig.rows[i][0], cfg.thresholds)[name]
    closed = (np.arange(rig.N) % 2).astype(np.uint8)
    oconv = np.zeros(rig.N, bool)
    for i, ((c, _), t) in enumerate(zip(rig.rows, targets)):
        e = OC.clone_env(c, rig.oracle_model, solver)
        oconv[i] = e.run_controller(OC.osc_params(t, rig.own_config(i) if own else OC.SHARED), 255.0 if closed[i] else 0.0, 1, 1)
    assert all(oconv[i] == w for i, w in want.items()), (oconv[probes], want)   # (the reference alone: both sides occur)
    assert oconv.sum() == 2
    runs = {}
    for mode in (True, 2):      # compact kernel (capacity fallback on, nothing to fall back from); the large kernel
        phys = rig.fresh(solver)
        phys.set_fallback(mode)
        if own:
            phys.osc_configure_env(gains=rig.gains, null_q=rig.null_q, thresholds=rig.thresholds)
        phys.osc_set_target(**rig.arrays(targets))
        phys.gripper_set(closed)
        tau, grip = phys.osc_compute()
        conv = phys.run_controller(1, control_steps=1)
        ctrl = phys.ctrl()
        assert np.array_equal(grip, np.where(closed != 0, 255.0, 0.0).astype(np.float32))
        assert np.array_equal(ctrl[:, 7], grip), mode
        assert np.array_equal(_bits(ctrl[:, :7]), _bits(tau)), (mode, np.abs(ctrl[:, :7] - tau).max())
        assert (conv == oconv).all(), (mode, conv, oconv)
        assert np.allclose(phys.time(), 1e-3) and (((phys.status() & 1) != 0) == ~conv).all()
        q, v = phys.get_state_f64()
        runs[mode] = (ctrl, conv, q, v)
        phys.set_fallback(True)
    for a, b in zip(runs[True], runs[2]):
        assert np.array_equal(a, b)
    if not own:
        ref = rig.reference(targets)
        err = np.abs(runs[True][0][:, :7].astype(np.float64) - ref).max(axis=1) / rig.bars(ref, targets)
        assert (err < 1.0).all(), err
