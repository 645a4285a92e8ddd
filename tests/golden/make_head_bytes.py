"""Generates tests/golden/head_bytes.json: the CRC-32C of every input and every output of the calls of
tests/head_bytes_cases.py, the record tests/test_gpu_head_bytes.py holds the two Transporter heads to.

The record states what the kernels wrote BEFORE a change to them, so it is made with the library of the commit the change
starts from, never with the changed one: build that commit's sources (lib.compile_and_link(so, objdir, csrc=<its csrc>)) and
name the result in MRE_LIB.  Run from the repo root, on the GPU:
    MRE_LIB=/path/to/libmre_of_the_parent.so python tests/golden/make_head_bytes.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from mujoco_robot_environments_amd import lib  # noqa: E402
from tests import head_bytes_cases  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "head_bytes.json")
    rows = head_bytes_cases.digests(lib.lib())
    with open(out, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{out}: {len(rows)} calls")
