"""What the task envs return through their public API against the record tests/golden/env_record.json
(tests/golden/make_env_record.py, made with the ``tasks`` package of the commit before that package was last regrouped, and
reproduced by a second run of that commit): the script of tests/env_record_cases.py, group by group.  Every digest is
compared for equality."""
import json
import os

import pytest

from tests import env_record_cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "env_record.json")


@pytest.mark.parametrize("group", list(env_record_cases.GROUPS))
def test_every_output_of_the_task_envs_matches_the_record(group):
    with open(GOLDEN) as fh:
        want = json.load(fh)[group]
    got = env_record_cases.digests(group)
    dropped = set(env_record_cases.NOT_DETERMINISTIC.get(group, ()))
    assert want and [c for c in got if c not in dropped] == list(want), "the script and the record list different cases"
    wrong = [c for c in want if got[c] != want[c]]
    assert not wrong, (len(wrong), wrong)   # (the first case that differs names the call that went wrong)
