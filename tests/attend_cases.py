"""Cases of the pick head (mre_attend and mre_attend_dlogits, include/mre.h; csrc/mre_attend.hip) shared by
tests/test_attend.py and tests/test_gpu_attend.py: the shapes, named against the kernel's own constants, the inputs and the
statement as float64 numpy, each computed ONCE per case on the CPU and left unchanged.
"""
import functools

import numpy as np
import torch

# the constants of csrc/mre_attend.h: cells of a lane per chunk (one 16-byte vector of bfloat16, two of float32), cells of a
# workgroup's chunk, and the largest number S of workgroups that share an env
LANE, CHUNK, MAX_SPLIT = 8, 2048, 16


def chunks(cells):
    return (cells + CHUNK - 1) // CHUNK


def split(cells):
    """S of csrc/mre_attend.h: it depends on the number of cells alone"""
    return min(chunks(cells), MAX_SPLIT)


def split_cells(cells):
    """[(first cell, one past the last cell)] of the S splits: contiguous runs of chunks, the first chunks % S one longer"""
    c, s = chunks(cells), split(cells)
    first = lambda k: k * (c // s) + min(k, c % s)
    return [(first(k) * CHUNK, min(first(k + 1) * CHUNK, cells)) for k in range(s)]


# (n, K, h, w)
SHAPES = [
    (1, 1, 1, 1),        # minimal: one cell, one lane, a vector of which one element exists
    (2, 1, 5, 7),        # 35 cells: shorter than CHUNK, no multiple of LANE; env 1 starts off the 16-byte grid
    (3, 1, 33, 47),      # 1551 cells: rows and envs that are not 16-byte aligned
    (2, 2, 16, 24),      # K > 1
    (2, 36, 8, 8),       # many rotations, tiny planes: 2304 cells, S = 2, the second chunk partial
    (1, 1, 70, 130),     # 9100 cells: 5 chunks, S = 5, the last one partial
    (1, 1, 32, 64),      # exactly CHUNK cells: S = 1, every vector whole
    (1, 1, 3, 683),      # CHUNK + 1 cells: S = 2, the second split holds one cell
    (1, 1, 320, 240),    # the workload's env: 37.5 chunks, S = MAX_SPLIT, 6 splits of 3 chunks and 10 of 2, the last partial
]
IDS = ["%dx%dx%dx%d" % s for s in SHAPES]
END_TO_END = (2, 1, 48, 64)
assert [split(k * h * w) for _, k, h, w in SHAPES] == [1, 1, 1, 1, 2, 5, 1, 2, MAX_SPLIT]
assert 32 * 64 == CHUNK and 3 * 683 == CHUNK + 1 and 320 * 240 % CHUNK == CHUNK // 2


def value_range(shape):
    """Integer logits in -4 .. 4, exact in bfloat16 and float32 and full of ties; -1 .. 1 where an env has so few cells
    that e^4 alone could be a quarter of its sum (the loss tests want every probability below 0.25)."""
    n, k, h, w = shape
    return 4 if k * h * w >= 1024 else 1


@functools.lru_cache(maxsize=None)
def integer_logits(shape, masked=False):
    """float32 [n, K, h, w] of integers (read only); `masked`: about a quarter of the cells are -inf"""
    r = value_range(shape)
    rng = np.random.default_rng(5000 + 7 * sum(shape))
    x = rng.integers(-r, r + 1, size=shape).astype(np.float32)
    if masked:
        x[rng.random(shape) < 0.25] = -np.inf
        x.reshape(shape[0], -1)[:, -1] = 0.0   # (every env keeps a finite cell)
    x.setflags(write=False)
    return x


def as_tensor(a, dtype) -> torch.Tensor:
    """A numpy float array as a CPU tensor of `dtype` (exact for the integer inputs and for -inf)"""
    return torch.from_numpy(np.array(a, np.float32)).to(dtype)


def first_argmax(logits):
    """numpy's first-occurrence argmax per env: (index int64 [n], value float32 [n])"""
    flat = np.ascontiguousarray(logits, np.float32).reshape(logits.shape[0], -1)
    idx = flat.argmax(axis=1).astype(np.int64)
    return idx, flat[np.arange(len(idx)), idx]


def softmax64(logits, target, weight=None):
    """From logits [n, K, h, w]: lse [n], loss [n] (NaN for a target outside), g [n, K, h, w] = weight * (softmax - one-hot),
    all float64 numpy.  -inf cells are masked; an env of nothing else has lse -inf, loss NaN and g 0."""
    n = logits.shape[0]
    flat = np.asarray(logits, np.float64).reshape(n, -1)
    lse, loss, g = np.full(n, -np.inf), np.full(n, np.nan), np.zeros_like(flat)
    wgt = np.ones(n) if weight is None else np.asarray(weight, np.float64)
    for e in range(n):
        m = flat[e].max()
        if m == -np.inf:
            continue
        lse[e] = m + np.log(np.exp(flat[e] - m).sum())
        g[e] = np.exp(flat[e] - lse[e])
        t = int(target[e])
        if 0 <= t < flat.shape[1]:
            loss[e] = lse[e] - flat[e, t]
            g[e, t] -= 1.0
        g[e] *= wgt[e]
    return lse, loss, g.reshape(logits.shape)


def loops64(logits, target):
    """The statement as plain Python loops in float64, for the smallest shapes: (index, value, lse, loss) lists"""
    out = []
    for e in range(logits.shape[0]):
        cells = [float(v) for v in np.asarray(logits[e], np.float64).reshape(-1)]
        best, value = 0, cells[0]
        for i, v in enumerate(cells):
            if v > value:
                best, value = i, v
        m = max(cells)
        if m == -np.inf:
            lse = -np.inf
        else:
            total = 0.0
            for v in cells:
                total += np.exp(v - m)
            lse = m + np.log(total)
        t = int(target[e])
        loss = lse - cells[t] if 0 <= t < len(cells) and lse > -np.inf else np.nan
        out.append((best, value, lse, loss))
    return out


def targets(shape):
    """name -> one target per env: the first cell, the last, one in the last (partial) split, one of a rotation >= 1, and
    three outside"""
    n, k, h, w = shape
    cells = k * h * w
    lo, hi = split_cells(cells)[-1]
    kinds = {"first": 0, "last": cells - 1, "last split": lo + (hi - lo) // 2, "below": -1, "above": cells, "far": 2 ** 40}
    if k > 1:
        kinds["rotation"] = ((k - 1) * h + h // 2) * w + w // 3
    return {name: [t] * n for name, t in kinds.items()}


def peak_cells(shape):
    """The cells a unique maximum is placed at in turn: the first and the last cell, the first and the last cell of every
    split, and a cell of rotation K - 1"""
    n, k, h, w = shape
    cells = k * h * w
    at = {0, cells - 1, ((k - 1) * h + h // 2) * w + w // 2}
    for lo, hi in split_cells(cells):
        at.update((lo, hi - 1))
    return sorted(at)
