"""What the perception entries of the stream-only C ABI answer to bad calls, text and order of the checks included: every
call of tests/refusal_cases.py against the record tests/golden/refusals.json (tests/golden/make_refusals.py, made with the
library of the commit before the checks were last touched).  No GPU: a check refuses every call, or n == 0 returns first."""
import json
import os

import pytest

from tests import refusal_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refusals.json")
ENTRIES = ["mre_heightmap", "mre_heightmap_views", "mre_correlate", "mre_correlate_loss", "mre_correlate_dlogits",
           "mre_correlate_grad_scene", "mre_correlate_grad_kern", "mre_correlate_workspace", "mre_attend", "mre_attend_dlogits",
           "mre_attend_workspace", "mre_correlate_grad_workspace"]


@pytest.fixture(scope="module")
def libmre():
    from mujoco_robot_environments_amd import lib
    lib.build()
    return lib.lib()


def test_refusals_match_the_record(libmre):
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = refusal_cases.answers(libmre)
    assert [g[0] for g in got] == [w[0] for w in want], "the table and the record list different calls"
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, wrong[:5]


def test_the_table_covers_what_it_says():
    with open(GOLDEN) as fh:
        want = json.load(fh)
    for entry in ENTRIES:
        rows = [w for w in want if w[0].startswith(entry + ": ")]
        assert any(w[0].startswith(entry + ": two: ") for w in rows), entry        # wrong in two ways at once
        assert any("n == 0" in w[0] and w[1] == 0 for w in rows), entry            # n == 0 returns MRE_OK
        if not entry.endswith("_workspace"):                                       # (they take no device pointer)
            host = [w for w in rows if w[0].startswith(entry + ": host pointers")]
            assert host and all(w[1] == -1 and w[2].endswith("must be device pointers") for w in host), entry
        assert all(w[1] == 0 or w[2].startswith(entry + ": ") for w in rows), entry
    assert all(w[1] in (0, -1) for w in want)   # MRE_OK or MRE_ERR_ARG: nothing reached a launch (MRE_ERR_HIP is -3)
