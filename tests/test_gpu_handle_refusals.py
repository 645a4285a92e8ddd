"""What the handle entries of the C ABI answer to bad values on a live handle, text and order of the checks included: every
call of tests/handle_refusal_cases.py against the record tests/golden/handle_refusals.json
(tests/golden/make_handle_records.py, made with the library of the commit before the entries' openings were last touched).
The table ends with one step, which must succeed: a refusal leaves the handle usable."""
import json
import os

import pytest

from tests import handle_refusal_cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "handle_refusals.json")
ENTRIES = ["mre_render", "mre_set_fallback", "mre_set_solver", "mre_get_arm_dynamics", "mre_pack_final_state",
           "mre_rollout_ticks", "mre_step", "mre_set_trace", "mre_osc_configure_env", "mre_get_settle_steps", "mre_place_props",
           "mre_prop_place", "mre_sort_colours", "mre_run_controller"]
ONE_CHECK = ["mre_set_fallback", "mre_set_solver", "mre_pack_final_state", "mre_step"]


def test_refusals_on_a_live_handle_match_the_record(compiled_model):
    from mujoco_robot_environments_amd import lib
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = handle_refusal_cases.answers(lib.lib(), compiled_model[1])
    assert [g[0] for g in got] == [w[0] for w in want], "the table and the record list different calls"
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, wrong[:5]


def test_the_record_covers_what_it_says():
    with open(GOLDEN) as fh:
        want = json.load(fh)
    assert want[-1] == ["mre_step: one step after the refusals", 0, ""]
    assert all(w[1] == -1 and w[2] for w in want[:-1])   # MRE_ERR_ARG and a text: nothing reached a launch
    for entry in ENTRIES:
        rows = [w for w in want[:-1] if w[0].startswith(entry + ": ")]
        assert rows, entry
        assert entry in ONE_CHECK or any(w[0].startswith(entry + ": two: ") for w in rows), entry
