"""Cases of the operational-space law (csrc/mre_osc.h) shared by tests/test_osc_cases.py, tests/test_gpu_osc_law.py and
the known-answer test of the oracle's law (tests/test_oracle_kat.py): the case table, the law as plain fp64 numpy from
INDEPENDENT ingredients, and that law with one thing wrong each (the mutants).

Ingredients of the independent law: the site Jacobian by central differences of the model's own forward kinematics
(tests/test_torch_osc.py: site_jacobian), the mass matrix by the sum_b J_b' I_b J_b formula (model/compile.py:
dense_mass_matrix), and the oracle's bias force.

A case = a float32-rounded arm state (no cubes), one or more targets and a controller configuration of its own, all
drawn from seeded generators.  Classes (what selects a pose is computed here, in fp64, from L^-1 = J M^-1 J' with
eigenvalues w, and from the rotation matrix R of the controller site):

    regular      HOME +- 0.3 rad, det ~ 1                                                     2 poses
    pinv         |det| < 0.5e-2: the law's own switch to pinv(rcond 1e-2); at least two
                 different numbers of truncated eigenvalues among the poses                    3 poses
    illcond      det >= 2e-2 and w_min / w_max < 5e-4: inv by unpivoted float32 Gauss-Jordan   2 poses
    mat2q_t, mat2q_m0, mat2q_m4, mat2q_m8
                 the four branches of mat2q in osc_errors: trace at least 0.1 from 0 and the
                 winning diagonal entry at least 0.1 ahead of the others                       2 poses each
    threshold    HOME +- 0.3 rad at rest: the poses the convergence thresholds are probed at   4 poses
    forced pinv  = pinv_always on the regular and illcond poses (FORCED_CLASSES)

Eligibility (a case on a discontinuity of the law tests nothing): |det| outside [0.5e-2, 2e-2]; where the pinv is
taken -- the pinv class, and the poses pinv_always is used on -- no w_k / w_max in [0.95e-2, 1.05e-2]; |qe[0]| > 1e-3
for every target.  float32 Jacobi / Gauss-Jordan errors on a 6 x 6 matrix with w_max ~ 20 are about 1e-5 absolute: a
factor 2 on det and 5 % on the ratio are orders above that.

Targets: every pose gets "full" (up to 5 cm away, 0.2 rad about a random axis, velocity U(+-0.2) m/s, angular velocity
U(+-0.5) rad/s); the first pose of a class also gets "lin" (only the linear velocity), "ang" (only the angular velocity)
and "big" (2.5 rad instead of 0.2).  Every target is also used as -quat (the same rotation; qe[0] < 0: the other side
of the hemisphere sign of osc_errors)."""
import numpy as np

from mujoco_robot_environments_amd.model import compile as MC
from tests.common import HOME
from tests.test_torch_osc import GAINS, site_jacobian

NULL_Q = [0.0, -0.785, 0.0, -2.356, 0.0, 1.571, 0.785]   # osc.yaml's nullspace configuration
THRESHOLDS = [5e-3, 68e-3]                               # osc.yaml's convergence thresholds
COUNTS = {"regular": 2, "pinv": 3, "illcond": 2, "mat2q_t": 2, "mat2q_m0": 2, "mat2q_m4": 2, "mat2q_m8": 2,
          "threshold": 4}
LAW_CLASSES = [c for c in COUNTS if c != "threshold"]
FORCED_CLASSES = ("regular", "illcond", "threshold")     # the poses pinv_always = 1 is compared on
FINGER_CLASSES = ("regular", "pinv", "illcond")          # the first pose of each: finger joints and velocities
DET_BAND = (0.5e-2, 2e-2)
RATIO_BAND = (0.95e-2, 1.05e-2)
RCOND = 1e-2
QE0_MIN = 1e-3
MUTANTS = ("swap_velocities", "drop_velocities", "no_sign", "flip_branch", "shared_gains", "default_null_q")

# Section "tolerance" of the test's header: a case whose device result exceeds the project's bar
# 2e-4 * max(1, |tau|max) gets max(that bar, 2 x export_sensitivity()) instead, written here next to its name as
# {(case name, target name): bar in N m}.  (No case needed it: the table is empty.)
WIDENED_BAR = {}


def bar(ref, key=None):
    """The project's bar on a torque against the oracle's `ref` [7]: 2e-4 * max(1, |tau|max)."""
    return max(2e-4 * max(1.0, float(np.abs(ref).max())), WIDENED_BAR.get(key, 0.0))


class Config:
    """Controller parameters of one evaluation: gains [6] (kp, kd of position / orientation / nullspace), null_q [7],
    thresholds [2]."""

    def __init__(self, gains=GAINS, null_q=NULL_Q, thresholds=THRESHOLDS):
        self.gains = np.array(gains, np.float64)
        self.null_q = np.array(null_q, np.float64)
        self.thresholds = np.array(thresholds, np.float64)


SHARED = Config()


class Target:
    """position [3], quaternion [4] (wxyz), linear and angular velocity [3] as the float32 numbers the device is given."""

    def __init__(self, name, pos, quat, vel, angvel, dtype=np.float32):
        self.name = name
        self.pos, self.quat = np.asarray(pos, dtype), np.asarray(quat, dtype)
        self.vel, self.angvel = np.asarray(vel, dtype), np.asarray(angvel, dtype)

    def negated(self):
        return Target(self.name + "_neg", self.pos, -self.quat, self.vel, self.angvel)

    def replaced(self, name, **kw):
        f = dict(pos=self.pos, quat=self.quat, vel=self.vel, angvel=self.angvel)
        f.update(kw)
        return Target(name, **f)


class Terms:
    """The independent ingredients of the law at one state, fp64: jac [6, 7], mass [7, 7], bias [7] (the oracle's),
    site_pos [3], site_mat [3, 3], q [7], qd [7]."""

    def __init__(self, A, env):
        q0 = np.array(env.arr("qpos")[:43])
        self.site_pos, self.site_mat, self.jac = site_jacobian(A, q0, int(A["eef_site"][0]))
        self.mass = MC.dense_mass_matrix(A, q0)[:7, :7]
        self.bias = np.array(env.arr("qfrc_bias")[:7])
        self.q, self.qd = q0[:7].copy(), np.array(env.arr("qvel")[:7])

    @property
    def site_quat(self):
        return MC.m2q(self.site_mat)

    def task_inertia_inverse(self):
        """(L^-1 = J M^-1 J', its determinant, its eigenvalues in ascending order)."""
        Li = self.jac @ np.linalg.solve(self.mass, self.jac.T)
        return Li, float(np.linalg.det(Li)), np.linalg.eigvalsh(0.5 * (Li + Li.T))


def error_quaternion(terms, target):
    qc = terms.site_quat * [1.0, -1.0, -1.0, -1.0]
    return MC.qmul(np.asarray(target.quat, np.float64), qc)


def numpy_law(terms, target, cfg=SHARED, pinv_always=0, mutant=None, shared=SHARED, jac=None, mass=None, bias=None):
    """tau [7] of the law restated at tasks/rearrangement_mjx.py:59-135 in fp64 numpy.  `mutant`: one of MUTANTS, the
    law with that one thing wrong; `shared`: the configuration the two configuration mutants fall back to; jac / mass /
    bias: replacements of the terms' own (export_sensitivity)."""
    assert mutant is None or mutant in MUTANTS, mutant
    J = terms.jac if jac is None else jac
    M = terms.mass if mass is None else mass
    b = terms.bias if bias is None else bias
    g = shared.gains if mutant == "shared_gains" else cfg.gains
    null_q = shared.null_q if mutant == "default_null_q" else cfg.null_q
    Minv = np.linalg.inv(M)
    Li = J @ Minv @ J.T
    use_pinv = bool(pinv_always) or abs(np.linalg.det(Li)) < 1e-2
    if mutant == "flip_branch":
        use_pinv = not use_pinv
    Lam = np.linalg.pinv(Li, rcond=RCOND) if use_pinv else np.linalg.inv(Li)
    qe = error_quaternion(terms, target)
    eo = (1.0 if mutant == "no_sign" else np.sign(qe[0])) * qe[1:]
    v, w = np.asarray(target.vel, np.float64), np.asarray(target.angvel, np.float64)
    if mutant == "swap_velocities":
        v, w = w, v
    if mutant == "drop_velocities":
        v, w = np.zeros(3), np.zeros(3)
    F = np.concatenate([g[0] * (np.asarray(target.pos, np.float64) - terms.site_pos) + g[1] * (v - J[:3] @ terms.qd),
                        g[2] * eo + g[3] * (w - J[3:] @ terms.qd)])
    tn = g[4] * (null_q - terms.q) + g[5] * (0 - terms.qd)
    Jbar = Minv @ J.T @ Lam
    return J.T @ Lam @ F + (np.eye(7) - J.T @ Jbar.T) @ tn + b


def osc_params(target, cfg=SHARED, pinv_always=0):
    """The oracle's parameter block of one evaluation."""
    from oracle import oracle as O
    g = cfg.gains
    p = O.make_osc(dict(kp_pos=g[0], kd_pos=g[1], kp_ori=g[2], kd_ori=g[3], kp_null=g[4], kd_null=g[5],
                        null_q=list(cfg.null_q), pos_thresh=cfg.thresholds[0], ori_thresh=cfg.thresholds[1],
                        pinv_always=pinv_always))
    p.target_pos[:] = np.asarray(target.pos, np.float64)
    p.target_quat[:] = np.asarray(target.quat, np.float64)
    p.target_vel[:] = np.asarray(target.vel, np.float64)
    p.target_angvel[:] = np.asarray(target.angvel, np.float64)
    return p


def oracle_law(env, target, cfg=SHARED, pinv_always=0):
    return env.osc(osc_params(target, cfg, pinv_always))


def export_sensitivity(terms, target, cfg, pinv_always, bounds, samples=64, seed=0):
    """Largest change of tau over `samples` seeded random perturbations of J, M (symmetric) and the bias within the
    relative errors `bounds` (tests/test_gpu_dynamics.py: EXPORT_BOUND, relative to each array's largest magnitude)."""
    rs = np.random.RandomState(seed)
    base = numpy_law(terms, target, cfg, pinv_always)
    worst = 0.0
    for _ in range(samples):
        dJ = rs.uniform(-1, 1, (6, 7)) * bounds["jac"] * np.abs(terms.jac).max()
        dM = rs.uniform(-1, 1, (7, 7)) * bounds["mass"] * np.abs(terms.mass).max()
        db = rs.uniform(-1, 1, 7) * bounds["bias"] * np.abs(terms.bias).max()
        tau = numpy_law(terms, target, cfg, pinv_always, jac=terms.jac + dJ, mass=terms.mass + 0.5 * (dM + dM.T),
                        bias=terms.bias + db)
        worst = max(worst, float(np.abs(tau - base).max()))
    return worst


# ------------------------------------------------------------------------------------------------ the case table
class Case:
    """One pose: name, cls, qpos [15] / qvel [15] (float32: arm and finger joints), the oracle env at that state, the
    independent terms, det / eigenvalues of L^-1, the targets {name: Target} and the case's own Config."""

    def __init__(self, name, cls, env, terms, fingers):
        self.name, self.cls, self.env, self.terms, self.fingers = name, cls, env, terms, fingers
        self.qpos = np.array(env.arr("qpos")[:15], np.float32)
        self.qvel = np.array(env.arr("qvel")[:15], np.float32)
        _, self.det, self.w = terms.task_inertia_inverse()
        self.truncated = int((np.abs(self.w) <= RCOND * np.abs(self.w).max()).sum())
        self.targets, self.config = {}, None

    def all_targets(self):
        """Every target and its -quat twin."""
        out = []
        for t in self.targets.values():
            out += [t, t.negated()]
        return out


def _env_at(oracle_model, q7, qd7, fingers):
    """An oracle env without cubes whose float32-rounded state is (q7, qd7) and, with `fingers` = (q [8], qd [8]),
    finger joints and velocities away from zero."""
    from oracle import oracle as O
    e = O.Env(oracle_model, nprops=0)
    q, v = e.arr("qpos"), e.arr("qvel")
    q[:7], v[:7] = q7, qd7
    if fingers is not None:
        q[7:15], v[7:15] = fingers
    q[:43] = q[:43].astype(np.float32)
    v[:39] = v[:39].astype(np.float32)
    e.forward()
    return e


def clone_env(case, oracle_model, solver=None):
    """A fresh oracle env at the state of `case` (the table's own envs are read only; a replay of a tick moves this
    one)."""
    e = _env_at(oracle_model, case.qpos[:7], case.qvel[:7], (case.qpos[7:15], case.qvel[7:15]))
    if solver is not None:
        e.set_solver(solver)
    assert np.array_equal(e.arr("qpos")[:15], case.qpos) and np.array_equal(e.arr("qvel")[:15], case.qvel)
    return e


def _mat2q_branch(R):
    """The branch of mat2q the rotation matrix takes, or None within the margins of a branch point."""
    t, d = float(np.trace(R)), np.diag(R)
    if abs(t) < 0.1:
        return None
    if t > 0:
        return "mat2q_t"
    k = int(np.argmax(d))
    if d[k] - np.delete(d, k).max() < 0.1:
        return None
    return ("mat2q_m0", "mat2q_m4", "mat2q_m8")[k]


def ratio_clear(w):
    r = np.abs(w) / np.abs(w).max()
    return not ((r >= RATIO_BAND[0]) & (r <= RATIO_BAND[1])).any()


def classify(terms, home=False):
    """The class a pose is eligible for, or None."""
    _, det, w = terms.task_inertia_inverse()
    if DET_BAND[0] <= abs(det) <= DET_BAND[1]:
        return None
    if home:
        return "regular" if det > 0.5 and ratio_clear(w) else None
    if abs(det) < DET_BAND[0]:
        return "pinv" if ratio_clear(w) else None
    if w.min() / w.max() < 5e-4:
        return "illcond" if ratio_clear(w) else None
    return _mat2q_branch(terms.site_mat)


def _targets(case, rs, lead):
    """The targets of one pose: "full", and for the first pose of a class "lin", "ang" and "big"."""
    t = case.terms

    def rotated(angle):
        ax = rs.randn(3)
        ax /= np.linalg.norm(ax)
        return MC.qmul(np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * ax]), t.site_quat)

    full = Target("full", t.site_pos + rs.uniform(-0.05, 0.05, 3), rotated(0.2), rs.uniform(-0.2, 0.2, 3),
                  rs.uniform(-0.5, 0.5, 3))
    out = {"full": full}
    if lead:
        out["lin"] = full.replaced("lin", angvel=np.zeros(3))
        out["ang"] = full.replaced("ang", vel=np.zeros(3))
        out["big"] = full.replaced("big", quat=rotated(2.5))
    return out


def _table(A, oracle_model):
    lo, hi = A["jnt_range"][1:8, 0] + 0.05, A["jnt_range"][1:8, 1] - 0.05
    rs = np.random.RandomState(2024)
    by_cls = {c: [] for c in COUNTS}
    finger_sign = np.array([1, -1, 1, -1, 1, -1, 1, -1])

    def want(cls):
        return cls is not None and len(by_cls[cls]) < COUNTS[cls]

    def candidate(q7, qd7, home, cls_wanted=None):
        fingers = (rs.uniform(0.05, 0.3, 8) * finger_sign, rs.uniform(-0.5, 0.5, 8))
        e = _env_at(oracle_model, q7, qd7, None)
        terms = Terms(A, e)
        cls = classify(terms, home) if cls_wanted is None else cls_wanted
        if cls_wanted is None and not want(cls):
            return
        with_fingers = cls in FINGER_CLASSES and not by_cls[cls]
        if with_fingers:
            e = _env_at(oracle_model, q7, qd7, fingers)
            terms = Terms(A, e)
            if classify(terms, home) != cls:
                return
        if cls == "pinv" and len(by_cls[cls]) == COUNTS[cls] - 1:
            c = Case("", cls, e, terms, with_fingers)
            if {c.truncated} == {k.truncated for k in by_cls[cls]}:
                return     # (the last pose brings a second number of truncated eigenvalues)
        by_cls[cls].append(Case(f"{cls}{len(by_cls[cls])}", cls, e, terms, with_fingers))

    for _ in range(20):
        if len(by_cls["regular"]) < COUNTS["regular"]:
            candidate(np.array(HOME) + rs.uniform(-0.3, 0.3, 7), rs.uniform(-0.5, 0.5, 7), True)
    for _ in range(20):
        if len(by_cls["threshold"]) < COUNTS["threshold"]:
            q7 = np.array(HOME) + rs.uniform(-0.3, 0.3, 7)
            if classify(Terms(A, _env_at(oracle_model, q7, np.zeros(7), None)), True) == "regular":
                candidate(q7, np.zeros(7), True, "threshold")
    for _ in range(400):
        if all(len(by_cls[c]) >= COUNTS[c] for c in COUNTS):
            break
        candidate(rs.uniform(lo, hi), rs.uniform(-0.5, 0.5, 7), False)
    assert {k: len(v) for k, v in by_cls.items()} == COUNTS, "the generators no longer fill every class"
    cases = [c for cls in COUNTS for c in by_cls[cls]]
    for c in cases:
        c.targets = _targets(c, rs, c.name.endswith("0") and c.cls != "threshold")
        c.config = Config(np.array(GAINS) * rs.uniform(0.5, 1.5, 6), np.array(NULL_Q) + rs.uniform(-0.3, 0.3, 7),
                          np.array(THRESHOLDS) * rs.uniform(0.5, 1.5, 2))
    return tuple(cases)


_TABLES = {}


def cases(A, oracle_model):
    """The case table (a tuple of Case; built once per oracle model, read only)."""
    key = id(oracle_model)
    if key not in _TABLES:
        _TABLES[key] = (oracle_model, _table(A, oracle_model))
    return _TABLES[key][1]


def evaluations(table):
    """Every (case, target) the law is evaluated at: each target and its -quat twin."""
    return [(c, t) for c in table for t in c.all_targets()]


def threshold_targets(case, thresholds):
    """Four targets around the convergence thresholds at the pose of `case` (which is at rest):
    {name: (Target, expected converged)} at 0.98 x / 1.02 x the position threshold along a fixed direction, and at a
    rotation of 2 arcsin(0.98 x / 1.02 x the orientation threshold) -- |vector part of the error quaternion| =
    sin(angle / 2)."""
    t = case.terms
    rs = np.random.RandomState(7)
    d = rs.randn(3)
    d /= np.linalg.norm(d)
    ax = rs.randn(3)
    ax /= np.linalg.norm(ax)
    out = {}
    for f, want in ((0.98, True), (1.02, False)):
        out[f"pos{f}"] = (Target(f"pos{f}", t.site_pos + f * thresholds[0] * d, t.site_quat, np.zeros(3), np.zeros(3)),
                          want)
        ang = 2 * np.arcsin(f * thresholds[1])
        rot = np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * ax])
        out[f"ori{f}"] = (Target(f"ori{f}", t.site_pos, MC.qmul(rot, t.site_quat), np.zeros(3), np.zeros(3)), want)
    return out
