"""The narrow phase's register path against its clipped path on the CPU: box_box (csrc/mre_collide.h) is per-lane
code without a device in it, so tests/narrow_phase_host/narrow_host.cpp compiles it with g++ (-O2 -ffp-contract=on,
the contraction rule of the device build) and runs both paths on the same box pairs.  For every pose of
tests/narrow_shortcut_cases.py the number of candidates, the normal and every candidate's position and distance
must be the same bits in the same order; the sets that lie wholly inside the reference face must take the register
path on every pose, and no pose with a vertex outside may take it.

"Inside the reference face" is said of the pose the face branch sees.  At tilt 0 the face separations of the two
boxes tie up to rounding, and at yaws whose rotation matrix is inexact the SAT hands the reference face to the small
box in a few poses (measured: 1 of the 16 tilt-0 poses of `resting`, 1 of the 6 of `hull`, 5 of the 16 untilted inside
poses of `overhang`, 1 of the 7 inside poses of `stacked`; none at any tilt from 1e-6 up).  Those are the reverse
case -- the table's face as the incident one -- which needs the clip; the harness reads the owner of the reference
face off the normal, and a "hit" pose is held to the register path whenever box 1 owns it, every tilted pose of
`resting` unconditionally."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import narrow_shortcut_cases as SC

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "narrow_phase_host", "narrow_host.cpp")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the host harness"
    exe = str(tmp_path_factory.mktemp("narrow_host") / "narrow_host")
    subprocess.check_call([gxx, "-O2", "-ffp-contract=on", "-std=c++17", SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def results(harness, tmp_path_factory):
    d = tmp_path_factory.mktemp("narrow_poses")
    out = {}
    for name, (pairs, want) in SC.host_sets().items():
        fi, fo = str(d / (name + ".f32")), str(d / (name + ".i32"))
        np.ascontiguousarray(pairs, np.float32).tofile(fi)
        p = subprocess.run([harness, fi, fo], capture_output=True, text=True)
        res = np.fromfile(fo, np.int32).reshape(-1, 4)
        assert len(res) == len(pairs) == len(want), name
        print(f"{name}: {p.stdout.strip()}")
        out[name] = (res, want, p)
    return out


@pytest.mark.parametrize("name", ["resting", "overhang", "boundary", "stacked", "hull", "random"])
def test_register_path_returns_the_clipped_path_bits(results, name):
    res, want, p = results[name]
    bad = np.nonzero(res[:, 2])[0]
    assert len(bad) == 0 and p.returncode == 0, (name, p.stdout, bad[:8])
    hit = res[:, 0] != 0
    owner = res[:, 3]
    for i, w in enumerate(want):
        if w == "hit":
            assert owner[i] in (1, 2), (name, i, "a face contact was expected")
            assert hit[i] == (owner[i] == 1), (name, i, owner[i], "a face inside the reference face went through the clip"
                                               if not hit[i] else "the reverse case took the register path")
        elif w == "miss":
            assert not hit[i], (name, i, "a pose with a vertex outside took the register path")
    if name == "resting":     # rows are tilt-major, 16 yaws each: every tilted pose has the table as the reference
        assert (owner[16:] == 1).all() and hit[16:].all() and (res[:, 1] == 4).all(), (name, np.nonzero(~hit)[0])
        assert hit[[0, 4, 8, 12]].all(), "exact quarter turns at tilt 0 tie exactly: box 1 wins"
    print(f"{name}: register path on {int(hit.sum())} of {len(hit)} poses; reference face owned by box 2 on "
          f"{int((owner == 2).sum())}")
    if name == "random":      # the random pairs do exercise both outcomes
        assert hit.any() and (~hit & (res[:, 1] > 1)).any(), (int(hit.sum()), len(res))
