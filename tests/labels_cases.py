"""The numpy statement of the frame labels (perception.seg_labels, mre_seg_labels) and the synthetic images the CPU and
GPU tests run it on.  The statement is the reference's get_bbox (tasks/rearrangement.py:254-268: np.nonzero of
``seg == id``, min / max of the coordinates) extended with the pixel count, the coordinate sums and the depth minimum."""
import numpy as np


def numpy_labels(seg, depth, id0, nid):
    """(stats int64 [n, nid, 7] = xmin, ymin, xmax, ymax, count, sum_x, sum_y; zmin float32 [n, nid] or None)."""
    n = seg.shape[0]
    stats = np.zeros((n, nid, 7), np.int64)
    stats[..., :4] = -1
    zmin = None if depth is None else np.full((n, nid), np.inf, np.float32)
    for i in range(n):
        for k in range(nid):
            mask = seg[i] == id0 + k
            ys, xs = np.nonzero(mask)
            if len(xs):
                stats[i, k] = [xs.min(), ys.min(), xs.max(), ys.max(), len(xs), xs.sum(), ys.sum()]
                if depth is not None:
                    zmin[i, k] = depth[i][mask].min()
    return stats, zmin


def outside_bytes(id0, nid):
    """The byte values next to the label range and at both ends of a byte that are NOT labels of the call."""
    return [b for b in (id0 - 1, id0 + nid, 0, 1, 254, 255) if 0 <= b <= 255 and not id0 <= b < id0 + nid]


def contents(n, h, w, id0, nid, seed=0):
    """[(name, seg uint8 [n, h, w])]: the content cases, on a background of bytes outside the range."""
    rng = np.random.default_rng(seed + 1000 * n + 10 * h + w + id0)
    out_b = outside_bytes(id0, nid)
    bg = out_b[0]
    lab = lambda k: id0 + k % nid
    cases = []
    s = np.full((n, h, w), bg, np.uint8)
    cases.append(("absent", s.copy()))
    s = np.full((n, h, w), bg, np.uint8)
    for k, (y, x) in enumerate([(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]):
        s[:, y, x] = lab(k)
    cases.append(("corners", s))
    s = np.full((n, h, w), bg, np.uint8)
    s[:, 0, :] = lab(0); s[:, h - 1, :] = lab(1); s[:, :, 0] = lab(2); s[:, :, w - 1] = lab(3)
    cases.append(("edges", s))
    s = np.full((n, h, w), bg, np.uint8)
    s[n - 1, int(rng.integers(h)), int(rng.integers(w))] = lab(nid - 1)
    cases.append(("single pixel", s))
    cases.append(("one label everywhere", np.full((n, h, w), lab(nid - 1), np.uint8)))
    cases.append(("interleaved", (id0 + np.arange(n * h * w) % nid).astype(np.uint8).reshape(n, h, w)))
    s = rng.choice(np.array(out_b, np.uint8), size=(n, h, w))
    hit = rng.random((n, h, w)) < 0.05
    s[hit] = (id0 + rng.integers(0, nid, size=int(hit.sum()))).astype(np.uint8)
    cases.append(("bytes next to the range", s))
    s = np.full((n, h, w), bg, np.uint8)
    s[min(1, n - 1), h // 2:, w // 3:] = lab(1)
    cases.append(("one env only", s))
    s = rng.choice(np.array(out_b, np.uint8), size=(n, h, w))
    for i in range(n):
        for k in range(nid + 2):
            y0, x0 = int(rng.integers(h)), int(rng.integers(w))
            y1, x1 = y0 + 1 + int(rng.integers(max(1, h // 4))), x0 + 1 + int(rng.integers(max(1, w // 4)))
            s[i, y0:y1, x0:x1] = lab(k)
    cases.append(("rectangles", s))
    return cases


def depths(n, h, w, seed=0):
    """[(name, depth float32 [n, h, w])]: random, and strictly decreasing / increasing along the pixels of an image so
    that a label's minimum sits at its last / first pixel.  All finite and positive, exact in float32."""
    rng = np.random.default_rng(seed + 7)
    ramp = (np.arange(h * w, dtype=np.float32) * 0.25 + 0.5).reshape(1, h, w)
    return [("random", (0.3 + rng.random((n, h, w))).astype(np.float32)),
            ("decreasing", np.repeat(ramp[:, ::-1, ::-1], n, axis=0).copy()),
            ("increasing", np.repeat(ramp, n, axis=0).copy())]
