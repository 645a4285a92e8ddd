"""Hand-placed scenes for the Hessian-tile tests (tests/test_gpu_newton_tiles.py, tests/test_newton_tile_scenes.py).

nw_direction (csrc/mre_newton.h) forms a cross tile of the Hessian only if the step's contact set can fill it: cubes
{0, 1} x robot and cubes {2, 3} x robot take a contact between the robot and a cube of the group, cubes {2, 3} x
cubes {0, 1} one between a cube of each group.  One env per decision, each way:

  name            cubes  what touches                              robot-cube   cube-cube
  stack_0_on_1      4    cube 0 stands on cube 1 (same group)      -            (0, 1)
  stack_2_on_0      4    cube 2 stands on cube 0 (across groups)   -            (0, 2)
  pad_on_0          4    a finger pad presses on cube 0            0            -
  pad_on_2          4    a finger pad presses on cube 2            2            -
  two_cubes         2    cubes rest on the table                   -            -
  four_cubes        4    cubes rest on the table                   -            -
  arm_on_table      4    the hull of arm link 6 lies on the table  -            -
  stack_2_on_1      3    cube 2 stands on cube 1 (across groups)   -            (1, 2)

The cubes not named rest on the table, 0.5 mm deep, out of the arm's way.  expected() states the columns above and
contact_sets() reads them off a contact list, so that a test can hold each scene to its name.
"""
import numpy as np

from tests.narrow_phase_cases import _blank, _put

NAMES = ("stack_0_on_1", "stack_2_on_0", "pad_on_0", "pad_on_2", "two_cubes", "four_cubes", "arm_on_table", "stack_2_on_1")
NPROPS = (4, 4, 4, 4, 2, 4, 4, 3)
HALF = 0.0155                      # the reference's cube
TOP = 0.4                          # table top (model/spec.py)
DEPTH = 5e-4
Q0 = (1.0, 0.0, 0.0, 0.0)
REST_XY = ((0.55, -0.30), (0.55, -0.15), (0.55, 0.15), (0.55, 0.30))
# pads at the home pose (geoms 7 / 8 of the left finger, 10 / 11 of the right): inner faces at x = 0.2643 and 0.3497,
# the lower pad's centre at z = 0.8394; a cube 1 mm into the inner face of the left / right lower pad
PAD_Z = 0.8394
LEFT_PAD_CUBE_X = 0.2603 + 0.004 + HALF - 1e-3
RIGHT_PAD_CUBE_X = 0.3537 - 0.004 - HALF + 1e-3
# found by sampling the joint ranges on the CPU oracle: the hull of link 6 (geom 3) 2.4 mm into the table behind the
# base, no finger and no other link near it
ARM_ON_TABLE = (-2.5535, 0.8391, 0.0747, -2.8748, 1.2913, 0.7483, 2.3287)
TABLE_GEOM, FIRST_CUBE_GEOM, NRB, GRIP_BODY0 = 1, 12, 16, 8


def scenes():
    """(nprops [8] int32, sizes [8, 4, 3], qpos [8, 43] float32)"""
    n = len(NAMES)
    sizes = np.full((n, 4, 3), HALF)
    q = np.zeros((n, 43))
    rest_z = TOP + HALF - DEPTH
    for i, name in enumerate(NAMES):
        q[i] = _blank("rearr", NPROPS[i], sizes[i:i + 1])[0]
        for p in range(NPROPS[i]):
            _put(q, i, p, (REST_XY[p][0], REST_XY[p][1], rest_z), Q0)
        if name.startswith("stack_"):
            up, down = int(name[6]), int(name[-1])
            _put(q, i, up, (REST_XY[down][0], REST_XY[down][1], rest_z + 2 * HALF - DEPTH), Q0)
        elif name == "pad_on_0":
            _put(q, i, 0, (LEFT_PAD_CUBE_X, 0.0, PAD_Z), Q0)
        elif name == "pad_on_2":
            _put(q, i, 2, (RIGHT_PAD_CUBE_X, 0.0, PAD_Z), Q0)
        elif name == "arm_on_table":
            q[i, :7] = ARM_ON_TABLE
    return np.asarray(NPROPS, np.int32), sizes, np.asarray(q, np.float32)


def expected(name):
    """(cubes in contact with the robot, cube pairs in contact, an arm link touches the table)"""
    if name.startswith("stack_"):
        up, down = int(name[6]), int(name[-1])
        return set(), {(min(up, down), max(up, down))}, False
    if name.startswith("pad_on_"):
        return {int(name[-1])}, set(), False
    return set(), set(), name == "arm_on_table"


def contact_sets(rows, geom_body):
    """The same three facts from contact rows (.., dist, geom1, geom2 in the last three columns), penetrating ones only."""
    robot_cube, cube_cube, arm_table = set(), set(), False
    for r in rows:
        if not r[-3] < 0.0:
            continue
        g1, g2 = int(r[-2]), int(r[-1])
        b1, b2 = int(geom_body[g1]), int(geom_body[g2])
        c1, c2 = b1 - NRB, b2 - NRB
        r1, r2 = 0 < b1 < NRB, 0 < b2 < NRB
        if c1 >= 0 and c2 >= 0:
            cube_cube.add((min(c1, c2), max(c1, c2)))
        elif (r1 and c2 >= 0) or (r2 and c1 >= 0):
            robot_cube.add(c2 if r1 else c1)
        elif TABLE_GEOM in (g1, g2) and ((r1 and b1 < GRIP_BODY0) or (r2 and b2 < GRIP_BODY0)):
            arm_table = True
    return robot_cube, cube_cube, arm_table
