"""The output bytes of the handle entries of the C ABI against the record tests/golden/handle_bytes.json
(tests/golden/make_handle_records.py, made with the library of the commit before the host side of those entries was last
touched, and reproduced by a second run of that library): the script of tests/handle_bytes_cases.py on 3 envs and on 1, with
Newton and with PGS.  Every digest is compared for equality."""
import json
import os

import pytest

from tests import handle_bytes_cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "handle_bytes.json")


@pytest.mark.parametrize("run", handle_bytes_cases.RUNS, ids=[r[0] for r in handle_bytes_cases.RUNS])
def test_every_output_byte_of_the_handle_entries_matches_the_record(compiled_model, run):
    from mujoco_robot_environments_amd import lib
    with open(GOLDEN) as fh:
        want = [w for w in json.load(fh) if w[0].startswith(run[0] + ": ")]
    got = handle_bytes_cases.digests(lib.lib(), compiled_model[0], run)
    assert want and [g[0] for g in got] == [w[0] for w in want], "the script and the record list different outputs"
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, (len(wrong), wrong[:5])   # (the first row that differs names the call that went wrong)
