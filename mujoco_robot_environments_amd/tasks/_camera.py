"""The pinhole camera model of the task envs in numpy: no GPU call, no env object.  A camera is the dict ``camera()`` makes
(``pos``, ``mat``, ``fovy``, ``height``, ``width``); the envs keep a table of them and call these functions with it
(the reference's camera maths: tasks/rearrangement.py:480-577).  Pixel arguments are (x, y), one pixel [2] or [N, 2] by the
same lines: the operations and their order are those the envs have always run (tests/test_env_camera.py holds them to a
record bit for bit), so a transpose that does nothing to a vector stays where the batch needs it.
"""
import numpy as np
from scipy.spatial.transform import Rotation as R

from ..model import compile as _compile

TABLE_TOP_Z = 0.4   # the plane a pixel's ray is cut with where there is no depth image
_UNIT_CORNERS = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])


def camera(pos, quat, fovy, height, width) -> dict:
    """A fixed camera at ``pos`` with the orientation ``quat`` (w, x, y, z; normalised here), ``fovy`` in degrees."""
    q = np.asarray(quat, np.float64).reshape(4)
    return dict(pos=np.asarray(pos, np.float64).reshape(3), mat=_compile.q2m(q / np.linalg.norm(q)), fovy=float(fovy),
                height=int(height), width=int(width))


def intrinsics(cam, focal_height, height, width):
    """3 x 3 for an image of ``height`` x ``width`` whose focal length is that of an image ``focal_height`` high."""
    f = (1.0 / np.tan(np.deg2rad(cam["fovy"]) / 2)) * focal_height / 2.0
    return np.array([[-f, 0, (width - 1) / 2], [0, f, (height - 1) / 2], [0, 0, 1]])


def extrinsics(cam):
    """4 x 4, world -> camera."""
    ext = np.eye(4)
    ext[:3, :3] = cam["mat"].T
    ext[:3, 3] = -cam["mat"].T @ cam["pos"]
    return ext


def world_2_pixel(K, E, coords):
    """World points [3] or [N, 3] -> rounded pixels int32 [2] or [N, 2]."""
    c = np.atleast_2d(np.asarray(coords, np.float64))
    cam = (E @ np.concatenate([c, np.ones((len(c), 1))], axis=1).T).T
    cam = cam[:, :3] / cam[:, 3:4]
    img = (K @ cam.T).T
    img = img[:, :2] / img[:, 2:3]
    out = np.round(img).astype(np.int32)
    return out[0] if np.asarray(coords).ndim == 1 else out


def pixel_rays(K, coords):
    """The camera-frame ray of every pixel, [..., 3] with z = 1 (the camera looks along -z)."""
    return (np.linalg.inv(K) @ np.concatenate([coords, np.ones(coords.shape[:-1] + (1,))], axis=-1).T).T


def plane_depth(cam, rays, z=TABLE_TOP_Z):
    """The depth at which every ray of ``pixel_rays`` meets the horizontal plane at height ``z``."""
    d_w = (cam["mat"] @ (-rays).T).T
    return (z - cam["pos"][2]) / d_w[..., 2]


def unproject(E, rays, depth):
    """The world points [..., 3] at ``depth`` [...] along ``rays`` [..., 3]."""
    depth = np.asarray(depth, np.float64)
    camc = np.concatenate([rays * (-depth[..., None]), np.ones(rays.shape[:-1] + (1,))], axis=-1)
    w = (np.linalg.inv(E) @ camc.T).T
    return w[..., :3] / w[..., 3:4]


def corner_box(K, E, pos, mat, half):
    """(xmin, ymin, xmax, ymax), int32, of the eight projected corners of the box at ``pos`` with rotation ``mat`` and
    half sizes ``half``."""
    px = world_2_pixel(K, E, pos + (_UNIT_CORNERS * half) @ mat.T)
    return np.array([px[:, 0].min(), px[:, 1].min(), px[:, 0].max(), px[:, 1].max()])


def metadata(K, E) -> dict:
    """The reference's get_camera_metadata (tasks/rearrangement.py:550-577)."""
    quat = R.from_matrix(E[:3, :3]).as_quat()
    # NB the reference reads the translation from row 3 of the 4x4 (always 0,0,0): kept (:563-565)
    return {"intrinsics": {"fx": K[0, 0], "fy": K[1, 1], "cx": K[0, 2], "cy": K[1, 2]},
            "extrinsics": {"x": E[3, 0], "y": E[3, 1], "z": E[3, 2],
                           "qx": quat[0], "qy": quat[1], "qz": quat[2], "qw": quat[3]}}
