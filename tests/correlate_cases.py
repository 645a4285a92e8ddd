"""Cases of the place head's correlation (mre_correlate, include/mre.h) shared by tests/test_correlate.py and
tests/test_gpu_correlate.py: the shapes, the inputs, the statement as plain numpy loops, and the torch statement
(perception.correlate_reference) computed ONCE per case on the CPU and left unchanged.

Most inputs are integers in -2 .. 2: with K = depth * crop^2 <= 12 288 here every partial sum is an integer of at most
4 K < 2^24, so the float32 result is exact in ANY order of summation and the comparisons are bit for bit.
"""
import functools

import numpy as np
import torch

# n, R, depth, h, w, crop: the smallest shapes at which each mechanism of the kernel can break
SHAPES = [
    (1, 1, 1, 1, 1, 2),        # the smallest call
    (2, 3, 2, 5, 7, 8),        # scene smaller than the crop
    (2, 17, 1, 5, 7, 8),       # a padded second rotation tile
    (3, 36, 3, 24, 40, 6),     # crop not a multiple of 8
    (2, 36, 4, 33, 47, 24),    # partial pixel tiles each way, odd row pitch
    (1, 64, 16, 8, 8, 4),      # the limits of R and depth
    (2, 36, 3, 48, 64, 64),    # the workload's crop and K = 12 288
]
IDS = ["%dx%dx%d_%dx%d_c%d" % s for s in SHAPES]
WORKLOAD = SHAPES[6]


def bf16(a) -> torch.Tensor:
    """A numpy float array as a bfloat16 CPU tensor (nearest even; exact for the integer inputs)."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16)


def integer_inputs(shape, seed=0):
    """scene [n, depth, h, w] and kern [n, R, depth, crop, crop] as float32 arrays of integers in -2 .. 2."""
    n, rot, depth, h, w, crop = shape
    rng = np.random.default_rng(1000 + seed + 7 * sum(shape))
    scene = rng.integers(-2, 3, size=(n, depth, h, w)).astype(np.float32)
    kern = rng.integers(-2, 3, size=(n, rot, depth, crop, crop)).astype(np.float32)
    return scene, kern


def normal_inputs(shape, seed=0):
    """Standard-normal inputs rounded to bfloat16, as float32 arrays of those values."""
    n, rot, depth, h, w, crop = shape
    rng = np.random.default_rng(2000 + seed)
    scene = bf16(rng.standard_normal((n, depth, h, w))).to(torch.float32).numpy()
    kern = bf16(rng.standard_normal((n, rot, depth, crop, crop))).to(torch.float32).numpy()
    return scene, kern


def loops(scene, kern):
    """The formula of include/mre.h as seven plain loops in float64: [n, R, h, w].  For the smallest shapes only."""
    n, depth, h, w = scene.shape
    rot, crop = kern.shape[1], kern.shape[3]
    out = np.zeros((n, rot, h, w), np.float64)
    for e in range(n):
        for r in range(rot):
            for y in range(h):
                for x in range(w):
                    s = 0.0
                    for d in range(depth):
                        for i in range(crop):
                            for j in range(crop):
                                yy, xx = y + i - crop // 2, x + j - crop // 2
                                if 0 <= yy < h and 0 <= xx < w:
                                    s += float(scene[e, d, yy, xx]) * float(kern[e, r, d, i, j])
                    out[e, r, y, x] = s
    return out


def first_argmax(logits):
    """numpy's first-occurrence argmax per env of float32 logits [n, R, h, w]: (index int64 [n], value float32 [n])."""
    flat = np.ascontiguousarray(logits).reshape(logits.shape[0], -1)
    idx = flat.argmax(axis=1).astype(np.int64)
    return idx, flat[np.arange(len(idx)), idx]


@functools.lru_cache(maxsize=None)
def reference(shape, kind="integer", seed=0):
    """(scene, kern) as bfloat16 CPU tensors and the torch statement on them: logits float32 [n, R, h, w] (numpy, read
    only), index int64 [n], value float32 [n].  Computed once per case."""
    from mujoco_robot_environments_amd import perception as P
    scene, kern = (integer_inputs if kind == "integer" else normal_inputs)(shape, seed)
    s, k = bf16(scene), bf16(kern)
    ref = P.correlate_reference(s, k, logits=torch.float32)
    logits = ref.logits.numpy()
    logits.setflags(write=False)
    return s, k, logits, ref.index.numpy(), ref.value.numpy()


def shifted(plane, dy, dx):
    """plane [h, w] moved so that out[y, x] = plane[y + dy, x + dx], zero where that lies outside."""
    h, w = plane.shape
    out = np.zeros_like(plane)
    ys, xs = np.arange(h) + dy, np.arange(w) + dx
    oky, okx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
    out[np.ix_(oky, okx)] = plane[np.ix_(ys[oky], xs[okx])]
    return out
