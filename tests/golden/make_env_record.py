"""Generates tests/golden/env_record.json: the sha256 of every output of the script of tests/env_record_cases.py
(tests/test_gpu_env_record.py), as {group: {case: digest}}.

The record states what the task envs returned BEFORE a regrouping of mujoco_robot_environments_amd/tasks/, so it is made
with the ``tasks`` package of the commit the change starts from (da628a8 for the split into _timestep / _camera / _env /
_transporter), never with the changed one.  It is only worth keeping if that commit reproduces it: run this twice, in two
fresh processes, the second time with --check, which writes nothing, prints the cases that differ and fails if there are any.
A case that differs between two runs of one commit is not deterministic and is taken out of the record by hand.
Run from the repo root, on the GPU:
    python tests/golden/make_env_record.py [--out FILE]
    python tests/golden/make_env_record.py [--out FILE] --check
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import env_record_cases  # noqa: E402

if __name__ == "__main__":
    args = sys.argv[1:]
    path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "tests", "golden", "env_record.json")
    record = {group: env_record_cases.digests(group) for group in env_record_cases.GROUPS}
    if "--check" in args:
        with open(path) as fh:
            first = json.load(fh)
        wrong = [(g, c) for g in record for c in record[g] if first.get(g, {}).get(c) != record[g][c]]
        assert {g: list(v) for g, v in first.items()} == {g: list(v) for g, v in record.items()}, "the runs list different cases"
        assert not wrong, ("cases that differ between two runs", wrong)
        print(f"{path}: a second run agrees on all {sum(len(v) for v in record.values())} cases")
    else:
        with open(path, "w") as fh:
            json.dump(record, fh, indent=1)
            fh.write("\n")
        print(f"{path}: {sum(len(v) for v in record.values())} cases")
