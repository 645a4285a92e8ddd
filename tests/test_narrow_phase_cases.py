"""The narrow-phase pose families (tests/narrow_phase_cases.py) judged on the CPU, from the oracle's output alone:
each family stays within its cap of ambiguous poses, reaches the branch it was built for, and the stand-alone
oracle.boxbox / oracle.cylbox agree with the rows Env.contacts() lists for the same pair."""
from collections import Counter

import numpy as np
import pytest

from tests import narrow_phase_cases as NC


def _counts(name, active_only=False):
    return Counter(len(v) for p in NC.analysis(name, active_only) for v in p.lists[0].values())


@pytest.mark.parametrize("name", NC.FAMILIES)
def test_ambiguous_share_is_within_the_cap(name):
    for active_only in (False, True):
        amb, exempt, cap = NC.ambiguous_share(name, active_only)
        print(f"{name} {'active' if active_only else 'detected'}: {amb} ambiguous of {NC.N} (cap {cap}), {exempt} exempt")
        assert amb <= cap, (name, active_only, amb, cap)


def _box_pair_results(name):
    """(n contacts, normal, axes of both boxes) of the cube-cube pair of every env, unperturbed pose."""
    names = NC.geom_names("rearr")
    key = (names.index("prop_0"), names.index("prop_1"))
    _, poses = NC.oracle_lists(name)
    out = []
    for p, (gx, gm) in zip(NC.analysis(name, False), poses):
        rows = p.lists[0].get(key, np.zeros((0, 15)))
        if len(rows):
            out.append((len(rows), rows[0, 3:6], np.concatenate([gm[key[0]].T, gm[key[1]].T])))
    return out


def _is_edge(n, normal, axes):
    return n == 1 and np.abs(axes @ normal).max() < 1 - 1e-6     # parallel to no axis of either box


def test_f1_reaches_edge_and_face_results():
    res = _box_pair_results("F1")
    edge = sum(_is_edge(*r) for r in res)
    face = sum(np.abs(r[2] @ r[1]).max() > 1 - 1e-9 for r in res)
    print(f"F1: {edge} edge results, {face} face results of {len(res)} poses with contacts")
    assert edge >= 10 and face >= 10


def test_f2_has_every_polygon_size():
    c = _counts("F2")
    print("F2 contacts per pose:", sorted(c.items()))
    assert all(c[n] >= 1 for n in range(3, 9)), c


def test_f3_is_mostly_edge():
    res = _box_pair_results("F3")
    edge = sum(_is_edge(*r) for r in res)
    print(f"F3: {edge} edge results of {NC.N}")
    assert edge >= 0.8 * NC.N


def test_f4_puts_corners_outside_the_face():
    assert NC.family("F4").meta["outside"].sum() >= 8 and len(_box_pair_results("F4")) >= 0.9 * NC.N


def test_f5_is_exact_and_unambiguous():
    q = NC.family("F5").qpos
    assert np.array_equal(q, q.astype(np.float64).astype(np.float32))
    assert not any(p.ambiguous for a in (False, True) for p in NC.analysis("F5", a))


def test_f6_shows_every_penetration_count_and_the_cut():
    case = NC.family("F6")
    assert {0, 1, 2, 4} <= set(case.meta["npen"].tolist())
    ground = NC.geom_names("rearr").index("ground")
    sg = np.array([[a, b, c] for c in (-1, 1) for b in (-1, 1) for a in (-1, 1)], np.float64)
    pen = Counter()
    for i, p in enumerate(NC.analysis("F6", False)):
        z = case.qpos[i, 17] + (sg * case.sizes[i, 0]) @ NC.q2m(case.qpos[i, 18:22].astype(np.float64))[2]
        assert (z < 0.15).all(), "all eight corners inside the margin"
        assert [k[0] for k in p.lists[0]] == [ground] and len(next(iter(p.lists[0].values()))) == 4, "detected list: cut at four"
        pen[int((z < 0).sum())] += 1
    print("F6 corners below the plane:", sorted(pen.items()))
    assert all(pen[k] >= 8 for k in (0, 1, 2, 4))


def test_f7_has_single_contact_pairs_with_several_active_candidates():
    names = NC.geom_names("rearr")
    A = NC.model("rearr")[0]
    single = {(int(a), int(b)) for (a, b), s in zip(A["pair_geom"], A["pair_single"]) if s}
    hit, deep = Counter(), 0
    for p in NC.analysis("F7", False):
        for k, rows in p.lists[0].items():
            if k in single:
                assert len(rows) == 1
                hit[names[k[0]] + "/" + names[k[1]]] += 1
                deep += rows[0, 12] < 0
    print("F7 single-contact pairs:", dict(hit), "penetrating:", deep)
    assert hit["prop_0/link4_hull"] >= 12 and sum(hit.values()) >= 100 and deep >= 8


def test_f8_has_caps_and_generator_lines():
    case = NC.family("F8")
    names = NC.geom_names("push")
    key = (names.index("prop_0"), names.index("tool_cylinder"))
    found = Counter()
    for i, p in enumerate(NC.analysis("F8", False)):
        found[int(case.meta["pose_kind"][i])] += key in p.lists[0]
    print("F8 poses with a cylinder contact (random, cap, generator):", [found[k] for k in range(3)])
    assert found[0] >= 20 and found[1] == 9 and found[2] == 9      # (the pair's margin is 0: three of twelve are set apart)


def test_f9_exceeds_the_export():
    lists, _ = NC.oracle_lists("F9")
    n = [len(l[0]) for l in lists]
    print("F9 detected contacts per env:", sorted(set(n)))
    assert min(n) > 32


@pytest.mark.parametrize("name", ["F1", "F2", "F3", "F4", "F5", "F8"])
def test_stand_alone_narrow_phase_equals_the_pipeline(name):
    """oracle.boxbox / oracle.cylbox on the geom poses of forward() = that pair's rows of Env.contacts()."""
    from oracle import oracle as O
    case = NC.family(name)
    A = NC.model(case.kind)[0]
    names = NC.geom_names(case.kind)
    g1 = names.index("prop_0")
    g2 = names.index("tool_cylinder" if name == "F8" else "prop_1")
    margin = float(NC.model(case.kind)[0]["pair_margin"][[tuple(p) for p in A["pair_geom"].tolist()].index((g1, g2))])
    lists, poses = NC.oracle_lists(name)
    checked = 0
    for i in range(NC.N):
        gx, gm = poses[i]
        rows = NC.groups(lists[i][0]).get((g1, g2), np.zeros((0, 15)))
        if np.linalg.norm(gx[g2] - gx[g1]) > 0.1 + margin:
            continue        # (past the broad phase's bounding spheres the pipeline does not call the narrow phase)
        if name == "F8":
            n, nm, pos, d = O.cylbox(gx[g1], gm[g1], case.sizes[i, 0], gx[g2], gm[g2], A["geom_size"][g2][0], A["geom_size"][g2][2], margin)
            pos, d = pos[None], np.array([d])
        else:
            n, nm, pos, d = O.boxbox(gx[g1], gm[g1], case.sizes[i, 0], gx[g2], gm[g2], case.sizes[i, 1], margin)
        assert n == len(rows), (i, n, len(rows))
        for k in range(n):
            assert np.array_equal(rows[k, :3], pos[k]) and rows[k, 12] == d[k] and np.array_equal(rows[k, 3:6], nm), (i, k)
        checked += n
    assert checked >= 40


def test_plane_box_lists_the_corners_that_point_down():
    """mjc_PlaneBox picks the bottom corners: with all eight inside the margin the list is the four whose offset from
    the centre points against the plane's normal (not the first four in corner order), each midway between the
    corner and the plane -- so the contacts with dist < margin - gap are exactly the corners that penetrate."""
    case = NC.family("F6")
    sg = np.array([[a, b, c] for c in (-1, 1) for b in (-1, 1) for a in (-1, 1)], np.float64)
    thr = NC.active_threshold("rearr")
    lists, poses = NC.oracle_lists("F6")
    prop = NC.geom_names("rearr").index("prop_0")
    for i in range(NC.N):
        gx, gm = poses[i]
        off = (sg * case.sizes[i, 0]) @ gm[prop].T
        down = off[off[:, 2] <= 0]
        rows = lists[i][0]
        assert len(rows) == len(down) == 4, i
        want = gx[prop] + down
        want[:, 2] *= 0.5
        assert np.abs(rows[:, :3] - want).max() < 1e-12 and np.abs(rows[:, 12] - 2 * want[:, 2]).max() < 1e-12, i
        assert np.array_equal(rows[:, 3:6], np.tile([0.0, 0, 1], (4, 1)))
        assert len(NC.keep_active(rows, thr)) == int(((gx[prop] + off)[:, 2] < 0).sum()) == int(case.meta["npen"][i]), i
