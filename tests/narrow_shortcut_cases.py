"""Pose sets for the narrow phase's register path (csrc/mre_collide.h: a face contact whose incident face lies
wholly inside the reference face is not clipped and its candidates stay in registers).  A plain module, CPU only.

A set is a list of box pairs -- (p1, quat1, half1, p2, quat2, half2, margin), box 1 the one box_box is given first --
with what the register path must do on every pose of it: "hit" (the smaller face lies inside or on the boundary of
the larger one), "miss" (a vertex outside), or None (only equality with the clipped path is asked).  In a "hit" set
box 1 carries the larger face.  Which box owns the reference face is the SAT's decision: where the two faces are
parallel to the last bit (tilt 0) the two face separations differ by rounding only, and at a yaw whose rotation
matrix is not exact either box may win.  A pose where box 2 -- the smaller face -- wins is the reverse case (a large
incident face around a small reference face), which needs the clip and must not take the register path.
tests/test_narrow_shortcut_host.py feeds the pairs to the CPU build of box_box; tests/test_gpu_narrow_shortcut.py
puts the scene sets (`scene_cases`) on the device as qpos rows of the rearrangement scene.

The geometry of an expectation is settled in float64 here with 1 mm to spare (a vertex "outside" is at least 1 mm
outside, one "inside" at least 1 mm inside), except where a set is exact in float32 by construction (dyadic
numbers, rotations by multiples of a quarter turn): those put vertices ON the boundary.
"""
from __future__ import annotations

import numpy as np

from tests.narrow_phase_cases import DY, PERMS, AIR, qaxis, qmul, q2m, qrand, f32

TABLE_P = np.array([0.4, 0.0, 0.2])          # model/spec.py: the table box
TABLE_S = np.array([0.9, 1.0, 0.2])
TOP = 0.4
Q0 = np.array([1.0, 0.0, 0.0, 0.0])
TILTS = (0.0, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2)
YAWS = tuple(np.pi * k / 8 for k in range(16))    # "every yaw": steps of 22.5 degrees round the circle
DEPTH = 5e-4                                     # the lowest corner's penetration


def _h32():
    return float(np.float32(np.sqrt(0.5)))


def _yaw_quat(k):
    """yaw k * 22.5 degrees; the quarter turns as the exact float32 quaternions of narrow_phase_cases.f5_exact_ties"""
    h = _h32()
    exact = {0: [1.0, 0, 0, 0], 4: [h, 0, 0, h], 8: [0.0, 0, 0, 1.0], 12: [h, 0, 0, -h]}
    return np.array(exact[k]) if k in exact else f32(qaxis([0, 0, 1], YAWS[k]))


def _lowest(q, s):
    """-(extent of the box along -z): z of the lowest corner relative to the centre"""
    return -float(np.abs(q2m(q)[2]) @ s)


def _pair(p1, q1, s1, p2, q2, s2, margin=0.0):
    return np.concatenate([p1, q1, s1, p2, q2, s2, [margin, 0, 0, 0]]).astype(np.float32)


def _outside(p_ref, q_ref, s_ref, p, q, s, tol):
    """Corners of box (p, q, s) whose footprint in the frame of the reference box lies more than tol outside its
    x-y rectangle / less than -tol inside, over the four corners of the face turned towards the reference box
    (below: the reference box is underneath)."""
    Rr, R = q2m(q_ref), q2m(q)
    k = int(np.argmax(np.abs(R[2])))                 # the box axis closest to vertical
    sg = -np.sign(R[2, k])                            # its face that looks down
    out = ins = 0
    for a in (-1, 1):
        for b in (-1, 1):
            loc = np.zeros(3)
            loc[k] = sg * s[k]
            loc[(k + 1) % 3] = a * s[(k + 1) % 3]
            loc[(k + 2) % 3] = b * s[(k + 2) % 3]
            w = Rr.T @ (p + R @ loc - p_ref)
            e = np.abs(w[:2]) - s_ref[:2]
            out += bool((e > tol).any())
            ins += bool((e < -tol).all())
    return out, ins


def _cube_on_table(xy, k_yaw, tilt, s, tdir=0.7):
    q = f32(qmul(qaxis([np.cos(tdir), np.sin(tdir), 0], tilt), _yaw_quat(k_yaw))) if tilt else _yaw_quat(k_yaw)
    z = TOP - _lowest(q, s) - DEPTH
    return np.array([xy[0], xy[1], z]), q


# ------------------------------------------------------------------ scene sets (also run on the device)
def resting():
    """One cube flat on the table inside the workspace, every tilt x every yaw; sizes permuted."""
    r = np.random.default_rng(5)
    rows = []
    for tilt in TILTS:
        for k in range(16):
            s = np.array(DY)[list(PERMS[r.integers(6)])]
            xy = (r.uniform(0.35, 0.55), r.uniform(-0.4, 0.4))
            p, q = _cube_on_table(xy, k, tilt, s, tdir=r.uniform(0, 2 * np.pi))
            rows.append((p, q, s))
    return rows


def overhang():
    """The same cube slid over the table's +x or +y edge: 0, 1 or 2 of its bottom corners at least 1 mm outside
    (one corner: the cube turned 45 degrees, its diagonal across the edge), flat and tilted by 1e-3."""
    r = np.random.default_rng(6)
    rows, want = [], []
    edge = {0: TABLE_P[0] + TABLE_S[0], 1: TABLE_S[1]}
    for rep in range(8):
        for nout in (0, 1, 2):
            for axis in (0, 1):
                for tilt in (0.0, 1e-3):
                    s = np.array(DY)[list(PERMS[r.integers(6)])]
                    if nout == 1:
                        k = 2 if rep % 2 else 6                     # 45 / 135 degrees
                        reach = float(np.hypot(s[0], s[1]))       # a footprint corner's distance (flat cube)
                        c = edge[axis] - reach + r.uniform(2e-3, 4e-3)   # that corner 2..4 mm out, the next ones inside
                        if abs(s[0] - s[1]) < 1e-9:
                            continue
                    elif nout == 2:
                        k = 4 * (rep % 4)
                        c = edge[axis] + r.uniform(-2e-3, 2e-3)
                    else:
                        k = rep * 2
                        c = edge[axis] - 0.05 - r.uniform(0, 0.1)
                    other = r.uniform(-0.3, 0.3)
                    xy = (c, other) if axis == 0 else (0.4 + other, c)
                    p, q = _cube_on_table(xy, k, tilt, s, tdir=r.uniform(0, 2 * np.pi))
                    out, ins = _outside(TABLE_P, Q0, TABLE_S, p, q, s, 1e-3)
                    if nout == 0:
                        assert out == 0 and ins == 4, (rep, axis, out, ins)
                    else:
                        assert out == nout, (rep, nout, axis, out)
                    rows.append((p, q, s))
                    want.append("hit" if nout == 0 else "miss")
    return rows, want


def stacked():
    """Two cubes in the air, cube 1 on cube 0, 2^-10 deep, everything exact in float32.  Per pose: (sizes of cube 0 and
    1, pose of both, expectation).  Aligned equal cubes put all four vertices ON the boundary (a hit); a smaller
    cube on top stays inside (hit); equal cubes offset by half a size, and a larger cube on a smaller one -- all
    four vertices outside, the reverse case that needs real clipping -- do not."""
    h = _h32()
    sq = np.array([DY[0], DY[0], DY[1]])                 # square footprint: a quarter turn maps it onto itself
    rows = []
    for s0, s1, yaw, off, want in (
            (np.array(DY), np.array(DY), [1.0, 0, 0, 0], (0, 0), "hit"),
            (np.array(DY), np.array(DY), [0.0, 0, 0, 1.0], (0, 0), "hit"),
            (sq, sq, [h, 0, 0, h], (0, 0), None),         # (h * h is not exactly 1/2: the turned frame is off by an ulp)
            (sq, sq, [1.0, 0, 0, 0], (0, 0), "hit"),
            (np.array(DY), 0.5 * np.array(DY), [1.0, 0, 0, 0], (0, 0), "hit"),
            (np.array(DY), 0.5 * np.array(DY), [1.0, 0, 0, 0], (0.25, 0.25), "hit"),
            (np.array(DY), 0.5 * np.array(DY), [1.0, 0, 0, 0], (0.5, 0.5), "hit"),    # two edges on the boundary
            (np.array(DY), 0.5 * np.array(DY), [h, 0, 0, h], (0.25, -0.25), "hit"),
            (np.array(DY), np.array(DY), [1.0, 0, 0, 0], (0.5, 0), "miss"),
            (np.array(DY), np.array(DY), [1.0, 0, 0, 0], (0, 0.5), "miss"),
            (np.array(DY), np.array(DY), [1.0, 0, 0, 0], (0.5, 0.5), "miss"),
            (np.array(DY), np.array(DY), [0.0, 0, 0, 1.0], (-0.5, 0.25), "miss"),
            (np.array(DY), 2.0 * np.array(DY), [1.0, 0, 0, 0], (0, 0), "miss"),
            (0.5 * np.array(DY), np.array(DY), [1.0, 0, 0, 0], (0.25, 0.25), "miss"),
            (np.array(DY), np.array(DY), [h, 0, 0, h], (0, 0), "miss")):           # DY[0] != DY[1]: the long side sticks out
        p0 = AIR.copy()
        p1 = p0 + [off[0] * s0[0], off[1] * s0[1], s0[2] + s1[2] - 2.0 ** -10]
        rows.append((s0, s1, p0, np.array([1.0, 0, 0, 0]), p1, np.array(yaw, np.float64), want))
    return rows


def scene_cases():
    """{name: (nprops, sizes [N, 4, 3], qpos [N, 43] float32)} of the three scene sets, for the device."""
    from tests.narrow_phase_cases import _blank, _put
    out = {}
    for name, rows in (("resting", resting()), ("overhang", overhang()[0])):
        sizes = np.zeros((len(rows), 4, 3))
        sizes[:] = DY
        for i, (_, _, s) in enumerate(rows):
            sizes[i, 0] = s
        q = _blank("rearr", 1, sizes)
        for i, (p, qq, _) in enumerate(rows):
            _put(q, i, 0, p, qq)
        out[name] = (1, sizes, np.asarray(q, np.float32))
    rows = stacked()
    sizes = np.zeros((len(rows), 4, 3))
    sizes[:] = DY
    for i, row in enumerate(rows):
        sizes[i, 0], sizes[i, 1] = row[0], row[1]
    q = _blank("rearr", 2, sizes)
    for i, (_, _, p0, q0, p1, q1, _) in enumerate(rows):
        _put(q, i, 0, p0, q0)
        _put(q, i, 1, p1, q1)
    out["stacked"] = (2, sizes, np.asarray(q, np.float32))
    return out


# ------------------------------------------------------------------ box pairs for the CPU build of box_box
def host_sets(nrandom=100_000):
    """{name: (pairs [P, 24] float32, expectations: list of "hit" / "miss" / None)}"""
    sets = {}
    rows = resting()
    sets["resting"] = (np.stack([_pair(TABLE_P, Q0, TABLE_S, p, q, s) for p, q, s in rows]), ["hit"] * len(rows))
    rows, want = overhang()
    sets["overhang"] = (np.stack([_pair(TABLE_P, Q0, TABLE_S, p, q, s) for p, q, s in rows]), want)
    # a vertex exactly on the boundary: dyadic reference box at the origin, the cube's +x face flush with its edge
    # (sg * x - lim == 0 for two vertices), then two float32 ulps further out (a miss), one further in (a hit)
    ref_s = np.array([0.5, 0.5, 0.25])
    pairs, want = [], []
    for s in (np.array(DY), np.array(DY)[[1, 0, 2]]):
        for ulps, w in ((0, "hit"), (2, "miss"), (-1, "hit")):   # (one ulp out: centre + half size rounds back to 0.5)
            cx = np.float32(0.5 - s[0])
            for _ in range(abs(ulps)):
                cx = np.nextafter(cx, np.float32(np.inf if ulps > 0 else -np.inf), dtype=np.float32)
            assert ulps != 0 or float(cx) + s[0] == 0.5
            pairs.append(_pair(np.zeros(3), Q0, ref_s, np.array([float(cx), 0.125, 0.25 + s[2] - 2.0 ** -10]), Q0, s))
            want.append(w)
    sets["boundary"] = (np.stack(pairs), want)
    rows = stacked()
    sets["stacked"] = (np.stack([_pair(p0, q0, s0, p1, q1, s1) for s0, s1, p0, q0, p1, q1, _ in rows]), [w for *_, w in rows])
    # a hull-sized box (the stand-ins of the robot's links: single-contact pairs) lying on the table
    r = np.random.default_rng(8)
    pairs = []
    for k in range(16):
        s = np.array([0.045, 0.06, 0.11])[list(PERMS[k % 6])]
        p, q = _cube_on_table((r.uniform(0.2, 0.7), r.uniform(-0.4, 0.4)), k, (0.0, 1e-4, 1e-3)[k % 3], s, tdir=r.uniform(0, 6.28))
        pairs.append(_pair(TABLE_P, Q0, TABLE_S, p, q, s))
    sets["hull"] = (np.stack(pairs), ["hit"] * len(pairs))
    # random pairs as narrow_phase_cases.f1_general draws them (sizes, orientations, direction of the offset), the
    # centre distance uniform over f1's bisection bracket instead of bisected, margins 0 and 2 mm; every fourth
    # pair has box 1 four times as large, so that face contacts inside a larger face occur at random too
    r = np.random.default_rng(9)
    P = np.zeros((nrandom, 24), np.float32)
    for i in range(nrandom):
        s0 = np.array(DY)[list(PERMS[r.integers(6)])] * (4.0 if i % 4 == 3 else 1.0)
        s1 = np.array(DY)[list(PERMS[r.integers(6)])]
        d = r.standard_normal(3)
        d /= np.linalg.norm(d)
        p0 = AIR + r.uniform(-0.01, 0.01, 3)
        t = r.uniform(0.012, 0.08) * (2.5 if i % 4 == 3 else 1.0)
        P[i] = _pair(p0, qrand(r), s0, p0 + t * d, qrand(r), s1, 0.0 if i % 2 else 2e-3)
    sets["random"] = (P, [None] * nrandom)
    return sets
