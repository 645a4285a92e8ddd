"""What the episode-shard path writes and refuses on the host against the record tests/golden/shard_record.json
(tests/golden/make_shard_record.py, made with the package of the commit before dataset.py was split by layer, and reproduced
by a second run of that commit): the host groups of tests/shard_record_cases.py.  Every digest and every message is compared
for equality.  CPU only; the device group is in tests/test_gpu_shard_cases.py."""
import json
import os

import pytest

from mujoco_robot_environments_amd import lib
from tests import shard_record_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shard_record.json")


@pytest.fixture(scope="module", autouse=True)
def _built():
    lib.build()


@pytest.mark.parametrize("group", list(shard_record_cases.GROUPS))
def test_every_file_and_message_matches_the_record(group):
    with open(GOLDEN) as fh:
        want = json.load(fh)[group]
    got = shard_record_cases.digests(group)
    assert want and list(got) == list(want), "the script and the record list different cases"
    wrong = [c for c in want if got[c] != want[c]]
    assert not wrong, (len(wrong), wrong, got[wrong[0]])

