"""The rectangular-prop scenes of tests/rect_prop_cases.py, checked on the CPU oracle alone: that every family is what
its name says, that each bound of tests/test_gpu_rect_props.py leaves room for a float32 implementation (the oracle's own
float32-state run: fp64 arithmetic, qpos / qvel / warm start rounded after every step), and that the tests can SEE an
axis mix-up (the same run with every prop's half sizes cyclically shifted).

Measured here (printed by the tests; the committed generator, both solvers unless stated):
  A  one step: the oracle's result rounded to float32 sits at 0.125 of the bound (a quarter is allowed); a cyclic shift
     of the sizes leaves the bound by 372 x in the least sensitive general-position env (the +1 % intermediate-axis
     one), 2e3 .. 8e5 x in the others -- 100 x is asserted.
  B  200 steps: float32-state run vs the oracle 1.2e-5 on qpos, 1.1e-5 on qvel; angular-momentum drift of the oracle's
     trace up to 5.2e-3 relative (median 1.8e-3), the float32-state run's drift within 8.4e-7 of it.
  C  120 steps: float32-state run 2.0e-6 / 5.4e-6 / 2.6e-6 on qpos and 2.9e-4 / 9.3e-4 / 2.5e-4 on qvel (Newton elliptic,
     PGS elliptic, Newton pyramidal), no constraint-set switch, no env outside the bar.
  D  40 steps: float32-state run 1.1e-6 on qpos, 6.2e-5 (Newton) / 6.7e-5 (PGS) on qvel, no constraint-set switch.
"""
import numpy as np
import pytest

from tests import newton_tile_cases as TC
from tests import rect_prop_cases as RC
from tests.test_gpu_newton import M54, QVEL_TOL, TOL

SOLVERS = ("Newton", "PGS")


def _f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def _check_inputs(sc, n_envs):
    assert len(sc) == n_envs
    assert len(RC.perms_used(sc)) == 6, "all six permutations of the triple occur"
    assert np.array_equal(sc.sizes, _f32(sc.sizes)), "half sizes exact in float32"
    assert sc.qpos.dtype == np.float32 and sc.qvel.dtype == np.float32 and sc.ctrl.dtype == np.float32
    for i in range(len(sc)):
        n = int(sc.nprops[i])
        rect = [p for p in range(n) if len(set(sc.sizes[i, p])) == 3]
        assert rect, sc.names[i]
        assert len({tuple(sc.sizes[i, p]) for p in rect}) == len(rect), "each prop of an env has its own permutation"


def test_prop_slots_and_counts():
    a, c = RC.family_a(), RC.family_c()
    assert sorted(set(a.nprops.tolist())) == [1, 2, 3, 4]
    assert sorted(set(c.nprops.tolist())) == [2, 3, 4]
    for sc, n in ((a, 48), (RC.family_b(), 45), (c, 32), (RC.family_d(), 8), (RC.family_e(), 40)):
        _check_inputs(sc, n)
    one = a.names.index("one_rect")
    assert [len(set(a.sizes[one, p])) for p in range(4)] == [1, 1, 3, 1]


@pytest.mark.parametrize("solver", SOLVERS)
def test_family_a_bound_holds_the_reference_and_sees_an_axis_shift(solver):
    a = RC.family_a()
    q, v = RC.cached(RC.a_reference, solver)
    w = np.abs(a.qvel[:, 15:].reshape(48, 4, 6))
    assert w[:, :, 3:].max() <= 12 and w[:, :, :3].max() <= 1
    # angular speeds below 16 rad/s: the velocity bound is at most 2^-18 rad/s
    _, bv = RC.a_bounds(a, q, v)
    assert bv[np.isfinite(bv)].max() <= 2.0 ** -18
    rounding = RC.a_ratio(a, _f32(q), _f32(v), q, v)
    assert rounding.max() <= 0.25, rounding.max()
    general = RC.general_envs(a)
    worst = np.inf
    for k in (1, 2):
        qs, vs = RC.oracle_step(a, solver, sizes=RC.shifted(a.sizes, k))
        signal = RC.a_ratio(a, qs, vs, q, v)
        worst = min(worst, signal[general].min())
        zero = [a.names.index(nm) for nm in RC.ZERO_TORQUE]
        assert signal[zero].max() <= 0.25, "the zero-torque envs are blind to the sizes, as their name says"
    print(f"A ({solver}): oracle rounded to float32 at {rounding.max():.3f} of the bound; sizes shifted cyclically: "
          f"{worst:.0f} x the bound in the least sensitive general-position env")
    assert worst >= 100


@pytest.mark.parametrize("solver", SOLVERS)
def test_family_b_float32_state_run_and_momentum_drift(solver):
    b = RC.family_b()
    q, v, cen = RC.cached(RC.b_reference, solver, False)
    q32, v32, _ = RC.cached(RC.b_reference, solver, True)
    assert ((cen & 63) == 0).all(), "free flight: no active contact"
    eq, ev = RC.active_error(b, q32, q, 7).max(), RC.active_error(b, v32, v, 6).max()
    drift, drift32 = RC.momentum_drift(b, q, v), RC.momentum_drift(b, q32, v32)
    rect = np.array([[p < b.nprops[i] and len(set(b.sizes[i, p])) == 3 for p in range(4)] for i in range(len(b))])
    noise = np.abs(drift32 - drift).max()
    print(f"B ({solver}): float32-state run vs oracle max |dqpos| {eq:.2e} |dqvel| {ev:.2e}; angular-momentum drift of the oracle "
          f"min {drift[rect].min():.1e} median {np.median(drift[rect]):.1e} max {drift.max():.1e}; float32-state run's drift "
          f"within {noise:.1e} of it; quaternion norm error {RC.quat_norm_error(b, q32).max():.1e}")
    assert eq * 8 < TOL and ev * 8 < QVEL_TOL         # the 8 x rule of the device test is the tighter one
    assert noise <= RC.DRIFT_FLOOR / 8
    assert drift[rect].min() > 4 * RC.DRIFT_FLOOR, "every rectangular prop drifts by more than the floor: the ratio test sees it"
    assert RC.quat_norm_error(b, q32).max() < 1e-5 / 8


@pytest.mark.parametrize("solver,cone", RC.SOLVER_CONES)
def test_family_c_float32_state_run_stays_inside_the_bar(solver, cone):
    c = RC.family_c()
    q, v, cen = RC.cached(RC.c_reference, solver, cone, False)
    q32, v32, cen32 = RC.cached(RC.c_reference, solver, cone, True)
    eq, ev = RC.active_error(c, q32, q, 7).max(), RC.active_error(c, v32, v, 6).max()
    switches = int(((cen & M54) != (cen32 & M54)).any(axis=0).sum())
    print(f"C ({solver}, {cone}): float32-state run vs oracle over {len(q)} steps max |dqpos| {eq:.2e} |dqvel| {ev:.2e}, "
          f"{switches} envs with a constraint-set switch")
    assert switches == 0 and eq < TOL and ev < QVEL_TOL
    w = np.abs(c.qvel[:, 15:].reshape(32, 4, 6))
    assert w[:, :, 3:].max() <= 8 and w[:, :, :3].max() <= 0.3
    kinds, boxbox, moved = RC.c_contact_census(solver, cone)
    assert all(k == {1, 2, 3} for k in kinds), "a vertex, an edge and a face meet the table in every env"
    stacked = np.array([nm.startswith("stack") for nm in c.names])
    assert stacked.sum() == 8 and boxbox[stacked].all() and not boxbox[~stacked].any()
    for i in range(32):
        assert (moved[i, :c.nprops[i]] > 1e-3).all(), (i, moved[i])


def test_family_c_starts_clear_of_the_table():
    c = RC.family_c()
    for i in range(32):
        for p in range(int(c.nprops[i])):
            low = c.qpos[i, 17 + 7 * p] - RC._extent(c.qpos[i, 18 + 7 * p: 22 + 7 * p], c.sizes[i, p], 2) - TC.TOP
            if not (c.names[i].startswith("stack") and p == 1):
                assert 0.005 - 1e-6 <= low <= 0.015 + 1e-6, (i, p, low)
    for e in RC.oracle_envs(c, "Newton"):
        assert not any(r[12] < 0 for r in e.contacts())


@pytest.mark.parametrize("solver", SOLVERS)
def test_family_d_block_on_the_pad(solver):
    d = RC.family_d()
    A = RC.model()[0]
    names = A["_names"]["geoms"]
    along = {0: set(), 2: set()}
    for i, e in enumerate(RC.oracle_envs(d, solver)):
        slot = int(d.names[i][7])
        rows = [r for r in e.contacts() if r[12] < 0]
        assert TC.contact_sets(rows, np.asarray(A["geom_bodyid"])) == ({slot}, set(), False), d.names[i]
        pad = [r for r in rows if f"prop_{slot}" in (names[int(r[13])], names[int(r[14])])]
        assert pad and all("pad" in names[int(r[13])] for r in pad), d.names[i]
        assert all(abs(r[12] + RC.PAD_DEPTH) < 5e-5 for r in pad), [r[12] for r in pad]      # 1 mm into the pad
        if "along" in d.names[i]:
            along[slot].add(float(d.sizes[i, slot, "xyz".index(d.names[i][9])]))
    assert along[0] == along[2] == set(RC.TRIPLE), "each half size lies along the closing direction once per slot"
    assert (d.ctrl[:, 7] == 255).all() and np.abs(d.ctrl[:, :7]).max() > 1
    q, v, cen = RC.cached(RC.d_reference, solver, False)
    q32, v32, cen32 = RC.cached(RC.d_reference, solver, True)
    eq, ev = np.abs(q32 - q).max(), np.abs(v32 - v).max()
    switches = int(((cen & M54) != (cen32 & M54)).any(axis=0).sum())
    print(f"D ({solver}): float32-state run vs oracle over {len(q)} steps, all 43 + 39 numbers: max |dqpos| {eq:.2e} |dqvel| {ev:.2e}, "
          f"{switches} envs with a constraint-set switch")
    assert eq < TOL and ev < QVEL_TOL and switches == 0
    for i in range(8):                                    # the pad pushed the block
        s = 15 + 7 * int(d.names[i][7])
        assert np.abs(q[-1, i, s:s + 3] - d.qpos[i, s:s + 3]).max() > 1e-3
