"""Generates tests/golden/shard_record.json: the digests and messages of the script of tests/shard_record_cases.py
(tests/test_shard_record.py, tests/test_gpu_shard_cases.py), as {group: {case: sha256 or message}}.

The record states what the episode-shard path wrote, read and refused BEFORE a regrouping of
mujoco_robot_environments_amd/dataset.py, so it is made with the package of the commit the change starts from (44b1837 for
the split into _tfrecord / _example / _tfds / _shard_io), never with the changed one.  It is only worth keeping if that
commit reproduces it: run this twice, in two fresh processes, the second time with --check, which writes nothing, prints the
cases that differ and fails if there are any.  The host groups need no GPU; the device group is made, and checked, only
where there is one (without a GPU a run keeps the device group the file already has).
Run from the repo root:
    python tests/golden/make_shard_record.py [--out FILE]
    python tests/golden/make_shard_record.py [--out FILE] --check
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import shard_record_cases  # noqa: E402

if __name__ == "__main__":
    import torch
    args = sys.argv[1:]
    path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "tests", "golden", "shard_record.json")
    groups = list(shard_record_cases.GROUPS) + (list(shard_record_cases.GPU_GROUPS) if torch.cuda.is_available() else [])
    record = {group: shard_record_cases.digests(group) for group in groups}
    first = {}
    if os.path.exists(path):
        with open(path) as fh:
            first = json.load(fh)
    if "--check" in args:
        wrong = [(g, c) for g in record for c in record[g] if first.get(g, {}).get(c) != record[g][c]]
        assert {g: list(first.get(g, {})) for g in record} == {g: list(v) for g, v in record.items()}, "the runs list different cases"
        assert not wrong, ("cases that differ between two runs", wrong)
        print(f"{path}: a second run agrees on all {sum(len(v) for v in record.values())} cases of {groups}")
    else:
        with open(path, "w") as fh:
            json.dump({**first, **record}, fh, indent=1)
            fh.write("\n")
        print(f"{path}: {sum(len(v) for v in record.values())} cases of {groups}")
