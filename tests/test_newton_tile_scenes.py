"""The hand-placed scenes of tests/newton_tile_cases.py on the CPU oracle: each has the contact it is named for and
none of the others, so the device test that runs them exercises every Hessian-tile decision both ways."""
import numpy as np
import pytest

from tests import newton_tile_cases as TC


@pytest.fixture(scope="module")
def oracle_model():
    from tests.narrow_phase_cases import model
    return model("rearr")


@pytest.mark.parametrize("i", range(len(TC.NAMES)), ids=TC.NAMES)
def test_scene_has_the_contact_it_is_named_for(i, oracle_model):
    from oracle import oracle as O
    A, om = oracle_model
    nprops, sizes, qpos = TC.scenes()
    e = O.Env(om, int(nprops[i]), sizes[i])
    e.reset()
    e.arr("qpos")[:43] = qpos[i]
    e.forward()
    got = TC.contact_sets(e.contacts(), np.asarray(A["geom_bodyid"]))
    assert got == TC.expected(TC.NAMES[i]), (TC.NAMES[i], got)
