"""Generates the two records of the handle entries that need a GPU:
  tests/golden/handle_refusals.json   code and text of every bad call of tests/handle_refusal_cases.py
                                      (tests/test_gpu_handle_refusals.py)
  tests/golden/handle_bytes.json      CRC-32C of every output of the script of tests/handle_bytes_cases.py
                                      (tests/test_gpu_handle_bytes.py)

The records state what the entries answered and wrote BEFORE a change to them, so they are made with the library of the
commit the change starts from, never with the changed one: build that commit's sources (tools/build_variant.py with
MRE_CSRC) and name the result in MRE_LIB.  The bytes record is only worth keeping if that library reproduces it: run this
twice, in two fresh processes, the second time with --check, which writes nothing and fails unless every row agrees.
Run from the repo root, on the GPU:
    MRE_LIB=/path/to/libmre_of_the_parent.so python tests/golden/make_handle_records.py
    MRE_LIB=/path/to/libmre_of_the_parent.so python tests/golden/make_handle_records.py --check
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from mujoco_robot_environments_amd import lib  # noqa: E402
from mujoco_robot_environments_amd.model import compile as MC  # noqa: E402
from tests import handle_bytes_cases, handle_refusal_cases  # noqa: E402

if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    check = "--check" in sys.argv[1:]
    model = MC.compile_scene()
    L = lib.lib()
    records = {"handle_refusals.json": handle_refusal_cases.answers(L, MC.to_blob(model)),
               "handle_bytes.json": [row for run in handle_bytes_cases.RUNS for row in handle_bytes_cases.digests(L, model, run)]}
    for name, rows in records.items():
        path = os.path.join(here, name)
        if check:
            with open(path) as fh:
                first = json.load(fh)
            wrong = [(a, b) for a, b in zip(first, rows) if a != b]
            assert len(first) == len(rows) and not wrong, (name, len(first), len(rows), wrong[:5])
            print(f"{path}: a second run agrees on all {len(rows)} rows")
        else:
            with open(path, "w") as fh:
                fh.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
            print(f"{path}: {len(rows)} rows")
