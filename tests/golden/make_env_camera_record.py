"""Generates tests/golden/env_camera_record.json (tests/test_env_camera.py): inputs and outputs of the pinhole camera maths
of BatchedRearrangementEnv as it stood at da628a8, the commit before that arithmetic moved to tasks/_camera.py.

RUN AT da628a8 ONLY: it calls that commit's unbound methods on a stand-in for ``self`` (no GPU: the table-plane branch of
the unprojection, the corner-projection branch of the boxes), so it states what the env computed BEFORE the regrouping.
Floats are float64 written by ``repr`` (json), which reads back to the same bits.  From the repo root:
    python tests/golden/make_env_camera_record.py
"""
import json
import os
import sys
import types

import numpy as np
from scipy.spatial.transform import Rotation as R

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from mujoco_robot_environments_amd.model import compile as MC  # noqa: E402
from mujoco_robot_environments_amd.tasks.rearrangement import (OVERHEAD, BatchedRearrangementEnv,  # noqa: E402
                                                                colour_separator_task_config)

OBLIQUE = dict(name="oblique", pos=[1.5, -0.9, 1.2], quat=[0.82, 0.41, 0.17, 0.36], fovy=50.0, height=360, width=500)
HALF = (1 / 64, 3 / 128, 1 / 32)


def stand_in():
    B = BatchedRearrangementEnv
    s = types.SimpleNamespace(_cameras={}, num_envs=3, render_observations=False)
    for cam in colour_separator_task_config().arena.cameras:     # (the constructor's loop, rearrangement.py:177-185)
        q = np.asarray(cam.quat, np.float64)
        q = q / np.linalg.norm(q)
        s._cameras[f"{cam.name}/{cam.name}"] = dict(pos=np.asarray(cam.pos, np.float64), mat=MC.q2m(q), fovy=float(cam.fovy),
                                                    height=int(cam.height), width=int(cam.width))
        if cam.name == "overhead_camera":
            s.overhead_camera_height, s.overhead_camera_width = int(cam.height), int(cam.width)
    for name in ("_get_camera_intrinsics", "_get_camera_extrinsics", "get_camera_params", "get_camera_metadata", "world_2_pixel",
                 "pixel_2_world", "pixel_2_world_batch", "add_camera", "props_info_env", "props_info"):
        setattr(s, name, types.MethodType(getattr(B, name), s))
    return s


def lists(x):
    if isinstance(x, dict):
        return {k: lists(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [lists(v) for v in x]
    return x.tolist() if isinstance(x, (np.ndarray, np.generic)) else x


if __name__ == "__main__":
    s = stand_in()
    configured = [dict(name=c.name, pos=list(c.pos), quat=list(c.quat), fovy=c.fovy, height=c.height, width=c.width)
                  for c in colour_separator_task_config().arena.cameras]
    key = s.add_camera(**OBLIQUE)
    h, w = s.overhead_camera_height, s.overhead_camera_width
    rec = {"cameras": configured + [OBLIQUE], "overhead_height": h, "overhead_width": w, "by_camera": {}}
    ov = s._cameras[OVERHEAD]
    # world points: below the overhead camera's centre (projects to (319.5, 239.5): both round at .5), on the table, in the
    # air, and one far off the image
    points = np.array([[ov["pos"][0], ov["pos"][1], 0.4], [0.45, 0.1, 0.4155], [0.62, -0.31, 0.4], [0.3, 0.25, 0.7], [3.0, -2.5, 0.4]])
    # pixels (x, y): the image's corners, its centre, fractional ones (one rounding at .5)
    pixels = np.array([[0.0, 0.0], [w - 1.0, 0.0], [0.0, h - 1.0], [w - 1.0, h - 1.0], [(w - 1) / 2, (h - 1) / 2], [101.25, 77.75],
                       [320.5, 17.5], [511.125, 402.9]])
    rec["points"], rec["pixels"] = lists(points), lists(pixels)
    for name, cam in s._cameras.items():
        K = s._get_camera_intrinsics(name, h, w)
        px5 = s.world_2_pixel(name, points)
        assert px5.dtype == np.int32
        one = [s.pixel_2_world(name, p) for p in pixels]
        batch = [s.pixel_2_world_batch(name, pixels[i:i + 3]) for i in range(len(pixels) - 2)]   # (num_envs = 3 per call)
        rec["by_camera"][name] = lists({
            "mat": cam["mat"], "intrinsics": K, "extrinsics": s._get_camera_extrinsics(name), "params": s.get_camera_params(name),
            "world_2_pixel_one": s.world_2_pixel(name, points[1]), "world_2_pixel_first": s.world_2_pixel(name, points[0]),
            "world_2_pixel": px5, "pixel_2_world": one, "pixel_2_world_batch": batch})
        if name == OVERHEAD:
            E = s._get_camera_extrinsics(name)
            c = (E @ np.append(points[0], 1.0))[:3]
            print("the first point projects to", (K @ c)[:2] / (K @ c)[2], "->", px5[0], "; the last to", px5[-1])
        print(name, "batch rows equal the scalar calls bit for bit:",
              all(np.asarray(batch[i][j]).tobytes() == np.asarray(one[i + j]).tobytes() for i in range(len(batch)) for j in range(3)))
    rec["metadata"] = lists(s.get_camera_metadata())
    # ---- corner-projection boxes: three cube poses (axis-aligned, yawed 30 degrees, tilted) at each of three half sizes;
    # "env" i has the three poses at half size HALF[i]
    quats = [np.array([1.0, 0.0, 0.0, 0.0]), MC.m2q(R.from_euler("z", 30, degrees=True).as_matrix()),
             MC.m2q(R.from_euler("xyz", [25, -40, 10], degrees=True).as_matrix())]
    centres = [[0.45, 0.1, 0.4155], [0.6, -0.2, 0.43], [0.38, 0.33, 0.5]]
    pose = np.zeros((3, 4, 7))
    pose[:, :, 3] = 1.0
    for p in range(3):
        pose[:, p, :3], pose[:, p, 3:] = centres[p], quats[p]
    s.nprops = np.array([3, 3, 3], np.int32)
    s.prop_half_size = np.stack([np.full((4, 3), hs) for hs in HALF])
    s.prop_rgba = np.ones((3, 4, 4))
    s.prop_colours = [["red", "green", "blue"]] * 3
    s._physics = types.SimpleNamespace(sites=lambda: (None, None, pose))
    per_env = [[s.props_info_env(i, pose)[12 + p]["bbox"] for p in range(3)] for i in range(3)]
    assert all(b.dtype == np.int32 for row in per_env for b in row)
    batch = s.props_info()["bbox"]
    assert batch.dtype == np.int64 and np.array_equal(batch[:, :3], np.array(per_env)) and (batch[:, 3] == -1).all()
    rec["boxes"] = lists({"pose": pose[:, :3], "half": list(HALF), "bbox": per_env})
    path = os.path.join(ROOT, "tests", "golden", "env_camera_record.json")
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(path, os.path.getsize(path), "bytes")
