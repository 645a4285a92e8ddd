"""Generates tests/golden/handle_null.json: what every handle entry answers to a NULL handle (tests/handle_null_cases.py), the
record tests/test_handle_null.py holds the library to.

The record states what the entries answered BEFORE a change to them, so it is made with the library of the commit the
change starts from, never with the changed one: build that commit's sources (tools/build_variant.py with MRE_CSRC) and name
the result in MRE_LIB.  Run from the repo root, no GPU needed:
    MRE_LIB=/path/to/libmre_of_the_parent.so python tests/golden/make_handle_null.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from mujoco_robot_environments_amd import lib  # noqa: E402
from tests import handle_null_cases  # noqa: E402

if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "handle_null.json")
    rows = handle_null_cases.answers(lib.lib())
    with open(out, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{out}: {len(rows)} calls, {sum(1 for r in rows if r[1])} refused")
