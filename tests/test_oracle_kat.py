"""Known-answer tests pinning the CPU oracle (the reference ships no tests and MuJoCo is
absent: SURVEY.md section 8c, 'parity unpinned').  Each test checks one stage of the
restated mj_step pipeline against an analytic result or an independent computation."""
import numpy as np
import pytest

from mujoco_robot_environments_amd.model import compile as MC
from tests.common import HOME, init_oracle_env


def _env(oracle_model, nprops=0, sizes=None):
    from oracle import oracle as O
    e = O.Env(oracle_model, nprops=nprops, prop_size=sizes)
    e.arr("qpos")[:7] = HOME
    return e


def _dense_M(A, e):
    nv = 39
    M = np.zeros((nv, nv))
    qM = e.arr("qM")
    for i in range(nv):
        a, j = int(A["dof_Madr"][i]), i
        while j >= 0:
            M[i, j] = M[j, i] = qM[a]
            a += 1
            j = int(A["dof_parentid"][j])
    return M


def test_free_fall_semi_implicit_euler(compiled_model, oracle_model):
    """z_k = z0 - g h^2 k(k+1)/2 exactly (free joint, no contact, implicitfast == Euler here)."""
    e = _env(oracle_model, 1)
    q = e.arr("qpos")
    q[15:22] = [0.45, 0.0, 1.5, 1, 0, 0, 0]
    e.forward()
    for k in range(1, 201):
        e.step(1)
        assert abs(q[17] - (1.5 - 9.8 * 1e-6 * k * (k + 1) / 2)) < 1e-12
    assert abs(e.arr("qvel")[17] + 9.8 * 0.2) < 1e-12


def test_free_rotation_conserves_angular_momentum(oracle_model):
    sizes = np.tile([0.01, 0.015, 0.02], (4, 1))
    e = _env(oracle_model, 1, sizes)
    q, v = e.arr("qpos"), e.arr("qvel")
    q[15:22] = [0.45, 0.0, 3.0, 1, 0, 0, 0]
    v[18:21] = [3.0, -2.0, 5.0]
    e.forward()
    I = 0.1 / 3 * np.array([0.015**2 + 0.02**2, 0.01**2 + 0.02**2, 0.01**2 + 0.015**2])

    def L():
        return MC.q2m(q[18:22]) @ (I * v[18:21])
    L0 = L()
    for _ in range(300):
        e.step(1)
    assert abs(np.linalg.norm(q[18:22]) - 1) < 1e-12
    assert np.linalg.norm(L() - L0) / np.linalg.norm(L0) < 2e-3  # first-order integrator drift


def test_crb_mass_matrix_matches_jacobian_formula(compiled_model, oracle_model):
    A, _ = compiled_model
    rs = np.random.RandomState(0)
    e = _env(oracle_model, 4)
    for trial in range(3):
        q = e.arr("qpos")
        init_oracle_env(e, 4, yaw=rs.uniform(0, 3, 4))
        q[:7] = HOME + rs.uniform(-0.3, 0.3, 7)
        q[7:15] = rs.uniform(0, 0.3, 8) * [1, -1, 1, -1, 1, -1, 1, -1]
        e.forward()
        M = _dense_M(A, e)
        Md = MC.dense_mass_matrix(A, q[:43].copy())
        # (1e-6: the model constants are float32-rounded, so the constant quaternions are unit only to
        #  6e-8; the oracle renormalises the composed body quaternion like mj_kinematics, the numpy
        #  cross-check does not)
        assert np.abs(M - Md).max() < 1e-6
        assert np.linalg.eigvalsh(M).min() > 0
        # sparse L'DL solve round trip
        y = rs.randn(39)
        x = np.linalg.solve(M, y)
        e.arr("ctrl")[:] = 0
        assert np.abs(M @ x - y).max() < 1e-9


def test_bias_force_is_potential_gradient_at_rest(compiled_model, oracle_model):
    """qvel = 0: qfrc_bias = dV/dq with V = sum m g z_com (finite differences)."""
    A, _ = compiled_model
    e = _env(oracle_model, 0)
    q = e.arr("qpos")
    q[:7] = HOME + 0.2
    e.forward()
    bias = e.arr("qfrc_bias")[:15].copy()

    def V(qq):
        xpos, xquat = MC.forward_kinematics(A, qq)
        z = 0.0
        for b in range(1, 16):
            z += A["body_mass"][b] * 9.8 * (xpos[b] + MC.qrot(xquat[b], A["body_ipos"][b]))[2]
        return z
    q0 = q[:43].copy()
    for d in range(15):
        qp, qm = q0.copy(), q0.copy()
        qp[d] += 1e-6
        qm[d] -= 1e-6
        assert abs((V(qp) - V(qm)) / 2e-6 - bias[d]) < 1e-6


def test_cube_rests_on_table_with_weight_balanced(oracle_model):
    e = _env(oracle_model, 1)
    q = e.arr("qpos")
    q[:7] = HOME                                  # the arm holds still under gravity compensation: PGS ends a sweep
    q[15:22] = [0.45, 0.1, 0.4 + 0.0155 + 0.001, 1, 0, 0, 0]   # loop on the improvement of ALL rows, the robot's included
    e.forward()
    e.arr("ctrl")[:7] = e.arr("qfrc_bias")[:7]
    for _ in range(600):
        e.step(1)
    assert e.ncon >= 4
    n = e.nefc
    f = e.arr("efc_force")[:n]
    normals = f[n - 12::3]
    assert abs(normals.sum() - 0.1 * 9.8) < 6e-4  # PGS stops at 100 sweeps, not at the exact optimum (0.04 % of the weight)
    assert (normals > 0).all() and np.ptp(normals) < 0.02
    assert np.abs(e.arr("qvel")[15:18]).max() < 1e-4
    assert np.abs(e.arr("qvel")[18:21]).max() < 5e-3  # slow PGS friction creep (unconverged sweeps)
    assert -5e-4 < q[17] - 0.4155 < 0  # small steady penetration of the soft contact


def test_boxbox_face_edge_and_margin():
    from oracle import oracle as O
    I = np.eye(3)
    # face-face: unit cube resting 1 mm into a slab -> 4 points at the cube's bottom corners
    n, nrm, pos, dist = O.boxbox([0, 0, 0], I, [1, 1, 0.5], [0, 0, 0.999], I, [0.5, 0.5, 0.5], 0.0)
    assert n == 4 and np.allclose(nrm, [0, 0, 1]) and np.allclose(dist, -0.001)
    assert np.allclose(sorted(map(tuple, np.round(np.abs(pos[:, :2]), 9))), [(0.5, 0.5)] * 4)
    assert np.allclose(pos[:, 2], 0.4995)
    # separated but within margin: reported with positive distance
    n, nrm, pos, dist = O.boxbox([0, 0, 0], I, [1, 1, 0.5], [0, 0, 1.05], I, [0.5, 0.5, 0.5], 0.15)
    assert n == 4 and np.allclose(dist, 0.05)
    n, *_ = O.boxbox([0, 0, 0], I, [1, 1, 0.5], [0, 0, 1.2], I, [0.5, 0.5, 0.5], 0.15)
    assert n == 0
    # edge-edge: two cubes rotated 45 deg about perpendicular axes touching along crossed edges
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    Rx = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    Ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    h = 0.5 * np.sqrt(2)
    n, nrm, pos, dist = O.boxbox([0, 0, 0], Rx, [0.5] * 3, [0, 0, 2 * h - 0.01], Ry, [0.5] * 3, 0.0)
    assert n == 1 and np.allclose(np.abs(nrm), [0, 0, 1], atol=1e-9) and abs(dist[0] + 0.01) < 1e-9
    assert np.allclose(pos[0], [0, 0, h - 0.005], atol=1e-9)


def test_gripper_linkage_closes_symmetrically_with_clamped_force(oracle_model):
    e = _env(oracle_model, 0)
    e.forward()
    e.arr("ctrl")[:7] = e.arr("qfrc_bias")[:7]
    e.arr("ctrl")[7] = 255.0
    for _ in range(400):
        e.arr("ctrl")[:7] = e.arr("qfrc_bias")[:7]
        e.step(1)
        assert abs(e.arr("actuator_force")[7]) <= 1.5 + 1e-12  # forcerange override (robotiq_2f85.py:41-48)
    q = e.arr("qpos")
    assert abs(q[7] - q[11]) < 1e-4, "driver joints are tied by the joint equality"
    assert 0.7 < q[7] <= 0.8 + 2e-3
    n = e.nefc
    assert np.abs(e.arr("efc_pos")[:6]).max() < 5e-4, "connect residuals stay small"


def test_osc_holds_current_pose_and_tracks_a_step(oracle_model):
    from oracle import oracle as O
    e = _env(oracle_model, 0)
    e.forward()
    p = O.make_osc()
    sx = e.arr("site_xpos")[:3].copy()
    p.target_pos[:] = sx
    p.target_quat[:] = MC.m2q(e.arr("site_xmat")[:9].reshape(3, 3))
    tau = e.osc(p)
    assert np.abs(tau - e.arr("qfrc_bias")[:7]).max() < 1e-9  # zero error, q = nullspace config
    assert e.osc_converged(p)
    p.target_pos[:] = sx + [0.05, 0.08, -0.12]
    assert not e.osc_converged(p)
    assert e.run_controller(p, 0.0, 400, 5)  # converges within the 2 s window (rearrangement.py:371)
    assert np.linalg.norm(e.arr("site_xpos")[:3] - np.array(p.target_pos)) < 5e-3


def test_capacity_emulation_cuts_the_contact_list(oracle_model):
    """mro_set_caps reproduces the device capacities: contacts beyond them are dropped in order
    and the overflow flag is raised (device: MRE_ST_CONTACT_OVERFLOW)."""
    e = _env(oracle_model, 4)
    init_oracle_env(e, 4, z_extra=-1e-4)
    e.forward()
    assert e.nefc == 7 + 3 * 16 and not e.overflow
    e.set_caps(ncon_cap=10, nefc_cap=112, nrrow_cap=62, npp_cap=8)
    e.forward()
    assert e.nefc == 7 + 3 * 10 and e.overflow
    e.set_caps(ncon_cap=32, nefc_cap=7 + 3 * 5 + 2, nrrow_cap=62, npp_cap=8)
    e.forward()
    assert e.nefc == 7 + 3 * 5 and e.overflow
    e.set_caps(0, 0, 0, 0)
    e.forward()
    assert e.nefc == 7 + 3 * 16 and not e.overflow


def test_osc_torque_matches_an_independent_numpy_evaluation_of_the_law(compiled_model, oracle_model):
    """The OSC law restated at tasks/rearrangement_mjx.py:59-135 (gains from osc.yaml:5-15),
    evaluated in numpy from INDEPENDENT ingredients: the site Jacobian by central differences of the
    model's own forward kinematics (model/compile.py, not the oracle's), the mass matrix by the
    sum_b J_b' I_b J_b formula, and the oracle's bias force; the oracle's torque must agree.  Covers
    both the regular branch (inverse of J M^-1 J') and pinv(rcond=1e-2), away from the home pose and
    with joint velocities."""
    from oracle import oracle as O
    from tests import osc_cases as OC
    A, _ = compiled_model
    rng = np.random.default_rng(4)
    for trial in range(3):
        e = _env(oracle_model, 0)
        q = e.arr("qpos")
        q[:7] = np.array(HOME) + rng.uniform(-0.3, 0.3, 7)
        e.arr("qvel")[:7] = rng.uniform(-0.5, 0.5, 7)
        e.forward()
        terms = OC.Terms(A, e)       # (the independent ingredients; the law itself: tests/osc_cases.py: numpy_law)
        p = O.make_osc()
        p.target_pos[:] = terms.site_pos + [0.04, -0.03, 0.05]
        yaw = 0.2
        tq = MC.qmul(np.array([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)]), terms.site_quat)
        p.target_quat[:] = tq
        target = OC.Target("kat", np.array(p.target_pos), tq, np.zeros(3), np.zeros(3), dtype=np.float64)
        for pinv_always in (0, 1):
            p.pinv_always = pinv_always
            tau = OC.numpy_law(terms, target, OC.SHARED, pinv_always)
            got = e.osc(p)
            assert np.abs(got - tau).max() < 2e-4 * max(1.0, np.abs(tau).max()), (trial, pinv_always, got, tau)


@pytest.mark.parametrize("gx, slides", [(4.0, False), (14.0, True)])
def test_elliptic_friction_cone_stick_and_slide_under_tilted_gravity(gx, slides):
    """Coulomb friction of the cube-table pair (mu = 1: max of the two geoms' sliding friction at equal
    priority): with gravity tilted to (gx, 0, -9.8) a resting cube must stick while gx < mu g and slide
    beyond, with a friction force that never exceeds the cone (acceleration >= gx - mu g) and reaches
    most of it (PGS stops at its 100-sweep cap short of the cone boundary: measured mu_eff = 0.90).
    The robot is frozen; the soft friction rows allow a small creep in the stick case."""
    from oracle import oracle as O
    from mujoco_robot_environments_amd.model import spec as MS
    A = MC.compile_scene(MS.default_scene(dict(gravity=[gx, 0.0, -9.8])))
    m = O.Model(MC.to_blob(A))
    e = O.Env(m, nprops=1)
    q = e.arr("qpos")
    q[:7] = HOME
    q[15:22] = [0.5, 0.0, 0.4155, 1, 0, 0, 0]
    e.freeze_robot(True)
    e.forward()
    e.step(50)                       # let the normal force build up
    x0, v0 = float(q[15]), float(e.arr("qvel")[15])
    T = 200
    e.step(T)
    x1 = float(q[15])
    t = T * 1e-3
    if not slides:
        assert abs(x1 - x0) < 2e-3, x1 - x0          # sticks (creep of the soft friction rows only)
    else:
        a_measured = 2.0 * (x1 - x0 - v0 * t) / (t * t)
        mu_eff = (gx - a_measured) / 9.8
        assert 0.85 < mu_eff <= 1.0 + 1e-6, (a_measured, mu_eff)
    assert abs(q[17] - 0.4155) < 5e-3                # stays on the table (a sliding cube pitches a little)


def test_boxbox_agrees_with_an_independent_separating_axis_computation():
    """Random box pairs: an independent numpy separating-axis test (15 axes) gives the signed gap along
    the axis of least overlap.  The collider must report contacts exactly when the boxes are closer
    than the margin, its deepest contact distance must match that gap (up to the face-axis preference), every contact must lie within
    the margin of both boxes, and the normal must be a unit vector pointing from box 1 to box 2."""
    from oracle import oracle as O
    rng = np.random.default_rng(12)

    def rot():
        q = rng.standard_normal(4); q /= np.linalg.norm(q)
        return MC.q2m(q)

    def sat_gap(p1, R1, s1, p2, R2, s2):
        axes = [R1[:, i] for i in range(3)] + [R2[:, i] for i in range(3)]
        for i in range(3):
            for j in range(3):
                c = np.cross(R1[:, i], R2[:, j])
                if np.linalg.norm(c) > 1e-8:
                    axes.append(c / np.linalg.norm(c))
        d = p2 - p1
        best = -np.inf
        for a in axes:
            r1 = sum(s1[i] * abs(a @ R1[:, i]) for i in range(3))
            r2 = sum(s2[i] * abs(a @ R2[:, i]) for i in range(3))
            best = max(best, abs(a @ d) - r1 - r2)   # > 0: separated by this much along a
        return best

    def dist_to_box(x, p, R, s):
        loc = R.T @ (x - p)
        return np.linalg.norm(np.maximum(np.abs(loc) - s, 0.0))

    margin = 0.02
    checked = hits = 0
    for _ in range(2000):
        s1, s2 = rng.uniform(0.05, 0.3, 3), rng.uniform(0.05, 0.3, 3)
        R1, R2 = rot(), rot()
        p1 = np.zeros(3)
        p2 = rng.standard_normal(3)
        p2 *= rng.uniform(0.1, 0.6) / np.linalg.norm(p2)
        gap = sat_gap(p1, R1, s1, p2, R2, s2)
        if gap < -0.02 or abs(gap - margin) < 1e-4:
            continue        # deep interpenetration / knife-edge cases are not what the env produces
        n, nrm, pos, dist = O.boxbox(p1, R1, s1, p2, R2, s2, margin)
        checked += 1
        if gap > margin:
            assert n == 0, (gap, n)
            continue
        assert n >= 1, gap
        hits += 1
        assert abs(np.linalg.norm(nrm) - 1) < 1e-9 and nrm @ (p2 - p1) > 0
        # the reported depth is the overlap along the axis the collider settled on: never shallower
        # than the least overlap, and at most a few percent deeper (face axes are preferred over a
        # marginally better edge-edge axis, as in MuJoCo's box-box routine)
        if gap <= 0:
            assert dist.min() <= gap + 2e-6 and dist.min() >= gap - max(0.1 * abs(gap), 1e-4), (dist.min(), gap)
        else:  # separated: the nearest vertex may be clipped away, the kept points are no nearer than the gap
            assert gap - 2e-6 <= dist.min() < margin, (dist.min(), gap)
        for x, dd in zip(pos, dist):
            assert dist_to_box(x, p1, R1, s1) < margin + 1e-6 and dist_to_box(x, p2, R2, s2) < margin + 1e-6
    assert checked > 400 and hits > 100, (checked, hits)


def test_mechanical_energy_balance_of_the_falling_arm(compiled_model, oracle_model):
    """Work-energy theorem over 0.15 s of the arm falling from a bent pose with zero controls (no
    cubes, no joint limit reached): kinetic energy from the oracle's own mass matrix, potential energy
    from an INDEPENDENT forward kinematics (model/compile.py: m g z of every body's centre of mass),
    dissipation = integral of sum_i d_i qdot_i^2 (joint damping) -- the balance closes to about a
    percent of the energy converted (first-order integrator, soft gripper constraints)."""
    A, _ = compiled_model
    e = _env(oracle_model, 0)
    q = e.arr("qpos")
    q[:7] = [0.3, -0.2, 0.4, -1.8, 0.3, 1.9, 0.5]
    e.forward()
    g = 9.8
    damp = np.asarray(A["dof_damping"], float)[:39]

    def energy():
        M = _dense_M(A, e)
        qd = np.array(e.arr("qvel")[:39])
        xpos, xquat = MC.forward_kinematics(A, np.array(q[:43]))
        pe = 0.0
        for b in range(1, 16):  # robot bodies
            com = xpos[b] + MC.qrot(xquat[b], A["body_ipos"][b])
            pe += float(A["body_mass"][b]) * g * com[2]
        return 0.5 * qd @ M @ qd, pe, float(damp @ (qd * qd))

    ke0, pe0, p0 = energy()
    diss, p_prev = 0.0, p0
    h = 1e-3
    for _ in range(150):
        e.step(1)
        _, _, p = energy()
        diss += 0.5 * (p + p_prev) * h
        p_prev = p
        assert np.all(np.abs(q[:7]) < 2.85)   # stays inside the joint ranges used here
    ke1, pe1, _ = energy()
    converted = pe0 - pe1
    assert converted > 0.5, converted         # the arm did fall (J)
    residual = (ke1 + pe1 + diss) - (ke0 + pe0)
    assert abs(residual) < 0.03 * converted, (residual, converted, ke1, diss)


def test_cube_cube_collision_conserves_momentum_in_free_fall(compiled_model, oracle_model):
    """Two cubes collide in mid-air (one thrown down onto the other, off-centre so that they also spin):
    contact forces are internal, so total linear momentum changes by gravity's impulse only and the
    angular momentum about the pair's centre of mass is conserved -- Newton's third law through the
    contact Jacobians (both prop parts of a row), friction cone included."""
    A, _ = compiled_model
    e = _env(oracle_model, 2)
    q, v = e.arr("qpos"), e.arr("qvel")
    s = 0.0155
    q[15:22] = [0.5, 0.0, 0.80, 1, 0, 0, 0]
    q[22:29] = [0.5 + 0.012, 0.006, 0.80 + 2 * s + 0.02, np.cos(0.2), 0, 0, np.sin(0.2)]
    v[15 + 6 + 2] = -1.0   # cube 1 linear z velocity
    e.freeze_robot(True)
    e.forward()
    m = 0.1
    I = m / 3.0 * (s * s + s * s)   # solid cube about its centre: m (2 s)^2 / 6

    def momenta():
        xpos, xquat = MC.forward_kinematics(A, np.array(q[:43]))
        P = np.zeros(3); L = np.zeros(3); com = np.zeros(3)
        bodies = [16, 17]
        for k, b in enumerate(bodies):
            com += xpos[b] / 2
        for k, b in enumerate(bodies):
            lin = np.array(v[15 + 6 * k: 18 + 6 * k])
            w_local = np.array(v[18 + 6 * k: 21 + 6 * k])       # free-joint angular velocity is body-local
            w = MC.q2m(xquat[b]) @ w_local
            P += m * lin
            L += np.cross(xpos[b] - com, m * lin) + I * w
        return P, L

    P0, L0 = momenta()
    hit = False
    for k in range(60):
        e.step(1)
        hit = hit or e.ncon > 0 and (e.contacts()[:, 12] < 0).any()
    P1, L1 = momenta()
    assert hit and q[17] > 0.7 and q[24] > 0.7            # collided, still far above the table
    expected = P0 + np.array([0, 0, -2 * m * 9.8 * 0.060])
    assert np.abs(P1 - expected).max() < 2e-4, (P1, expected)
    assert abs(v[15 + 2] - (-9.8 * 0.06)) > 0.05            # cube 0 was really pushed
    assert np.abs(L1 - L0).max() < 2e-5, (L1, L0)


def test_joint_limit_row_balances_a_torque_pushing_into_the_limit(compiled_model, oracle_model):
    """Joint 6 of the arm (range -0.0175 .. 3.7525) is pushed towards its lower limit by 4 N m on top
    of gravity compensation.  It must come to rest within a few milliradians of the limit (soft
    constraint), with the limit row's force cancelling the push, and no other arm joint moving."""
    e = _env(oracle_model, 0)
    q = e.arr("qpos")
    q[:7] = HOME
    q[5] = 0.05
    e.forward()
    for _ in range(1500):
        ctrl = e.arr("ctrl")
        ctrl[:7] = e.arr("qfrc_bias")[:7]
        ctrl[5] -= 4.0
        e.step(1)
    assert -0.0175 - 6e-3 < q[5] < -0.0175 + 1e-3, q[5]       # resting slightly inside the soft limit
    assert abs(e.arr("qvel")[5]) < 1e-4 and np.abs(e.arr("qvel")[:7]).max() < 5e-3   # (lagged gravity compensation drifts)
    assert abs(e.arr("qfrc_constraint")[5] - 4.0) < 0.05, e.arr("qfrc_constraint")[:7]
    others = [0, 1, 2, 3, 4, 6]
    assert np.abs(np.array(q[:7])[others] - np.array(HOME)[others]).max() < 2e-2


def test_cylinder_box_known_answers():
    """mro_cylbox (the tool cylinder of PushEnv / LasaDrawEnv against boxes; one contact like MuJoCo's convex collider):
    cap flat on a face, generator lying on a face, side against a vertical face, side against a vertical edge, rim
    against a face (tilted), and the detected-but-separated case."""
    from oracle import oracle as O
    I = np.eye(3)
    r, h = 0.015, 0.05
    table = ([0, 0, 0], I, [0.5, 0.5, 0.1])
    # cap flat on the table, 1 mm deep: normal +z, at the cap's centre, half way between the surfaces
    n, nm, pos, d = O.cylbox(*table, [0.1, 0.05, 0.1 + h - 0.001], I, r, h)
    assert n == 1 and np.allclose(nm, [0, 0, 1]) and abs(d + 0.001) < 1e-12 and np.allclose(pos, [0.1, 0.05, 0.0995])
    # lying on its side (axis along x), 2 mm deep: middle of the generator
    Rx = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0.0]])
    n, nm, pos, d = O.cylbox(*table, [0.1, 0.05, 0.1 + r - 0.002], Rx, r, h)
    assert n == 1 and np.allclose(nm, [0, 0, 1]) and abs(d + 0.002) < 1e-12 and np.allclose(pos, [0.1, 0.05, 0.099])
    # upright, pushing a cube's +x face: the generator overlaps the face between z = -0.02 and 0.025
    cube = ([0, 0, 0], I, [0.025] * 3)
    n, nm, pos, d = O.cylbox(*cube, [0.025 + r - 0.001, 0.0, 0.03], I, r, h)
    assert n == 1 and np.allclose(nm, [1, 0, 0]) and abs(d + 0.001) < 1e-12 and np.allclose(pos, [0.0245, 0.0, 0.0025])
    # upright against the cube's vertical edge, along the diagonal: the radial direction, 1 mm deep
    c = 0.025 + (r - 0.001) / np.sqrt(2)
    n, nm, pos, d = O.cylbox(*cube, [c, c, 0.0], I, r, h)
    assert n == 1 and np.allclose(nm, [np.sqrt(0.5), np.sqrt(0.5), 0], atol=1e-6) and abs(d + 0.001) < 1e-6
    assert np.allclose(pos[:2], 0.025 - 0.0005 / np.sqrt(2), atol=1e-6)
    # tilted 30 degrees about y over the table: the rim's lowest point touches first
    th = np.deg2rad(30.0)
    Rt = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    low = h * np.cos(th) + r * np.sin(th)                  # height of the centre when the rim touches z = 0.1
    n, nm, pos, d = O.cylbox(*table, [0.0, 0.0, 0.1 + low - 0.0005], Rt, r, h)
    assert n == 1 and np.allclose(nm, [0, 0, 1]) and abs(d + 0.0005) < 1e-9
    rim = np.array([0.0, 0.0, 0.1 + low - 0.0005]) + Rt @ np.array([r, 0, -h])   # the rim point that is lowest
    assert np.allclose(pos, rim + [0, 0, 0.00025], atol=1e-9)
    # 2 cm apart within a 5 cm margin: detected, positive distance; beyond the margin: nothing
    n, nm, pos, d = O.cylbox(*cube, [0.06, 0.0, 0.0], I, r, h, margin=0.05)
    assert n == 1 and abs(d - 0.02) < 1e-12 and np.allclose(pos, [0.035, 0, 0])
    assert O.cylbox(*cube, [0.06, 0.0, 0.0], I, r, h, margin=0.01)[0] == 0


def test_cylinder_box_distance_is_a_lower_bound_of_the_true_separation():
    """Random separated poses: the reported distance never exceeds the true distance between the two convex bodies
    (a separating-axis search over a finite set of directions underestimates, never overestimates), and equals it to
    1e-6 whenever the closest feature is a face, the axis or the radial direction (sampled surface points)."""
    from oracle import oracle as O
    rng_ = np.random.default_rng(5)
    r, h, s = 0.015, 0.05, np.array([0.025, 0.03, 0.02])
    gaps = []
    for _ in range(300):
        q = rng_.standard_normal(4); q /= np.linalg.norm(q)
        w, x, y, z = q
        Rc = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                       [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                       [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        dirv = rng_.standard_normal(3); dirv /= np.linalg.norm(dirv)
        pc = dirv * rng_.uniform(0.07, 0.12)
        n, nm, pos, d = O.cylbox([0, 0, 0], np.eye(3), s, pc, Rc, r, h, margin=1.0)
        assert n == 1
        # true distance by dense sampling of the cylinder's surface against the box
        tt = np.linspace(-h, h, 41); ph = np.linspace(0, 2 * np.pi, 73)[:-1]
        T, P = np.meshgrid(tt, ph, indexing="ij")
        side = np.stack([r * np.cos(P), r * np.sin(P), T], -1).reshape(-1, 3)
        rr = np.linspace(0, r, 7)
        Rr, P2 = np.meshgrid(rr, ph, indexing="ij")
        caps = np.concatenate([np.stack([Rr * np.cos(P2), Rr * np.sin(P2), np.full_like(Rr, sg * h)], -1).reshape(-1, 3) for sg in (-1, 1)])
        pts = np.concatenate([side, caps]) @ Rc.T + pc
        dd = np.linalg.norm(pts - np.clip(pts, -s, s), axis=1).min()
        if dd < 1e-3:         # (the pose overlaps or touches: the sampled distance says nothing about a penetration depth)
            continue
        assert d <= dd + 1e-9, (d, dd)
        gaps.append(dd - d)
    assert len(gaps) > 150 and max(gaps) < 4e-3 and np.median(gaps) < 2e-4, (len(gaps), max(gaps), np.median(gaps))   # (sampling grid: 2 mm)
