"""The calls whose output BYTES tests/test_gpu_head_bytes.py holds the two Transporter heads to (the place head, mre_correlate*
of include/mre.h, and the pick head, mre_attend*), and ``digests(L)``, which makes them on a loaded library.  The record
tests/golden/head_bytes.json is made by tests/golden/make_head_bytes.py with the library of the commit BEFORE a change to the
heads' kernels: a refactor of them keeps every byte.

A row is [call id, {input name: crc}, {output name: crc}], the crc being CRC-32C (dataset.crc32c) of the bytes as they are
copied to the host.  Every call goes through the C ABI and is made twice: with every tensor's base 16-byte aligned ("a0") and
with every tensor's base one element past a 16-byte boundary ("a1"), so that the vector and the element-wise paths of the
kernels are both in the record (a workspace must be aligned, so it stays).

The place head takes the standard-normal bfloat16 inputs of tests/correlate_cases.py, whose sums round in float32; its loss
takes them a second time with the kernels scaled by a power of two near 1 / sqrt(K) (exact in bfloat16), so that many cells
share in the softmax's sum and not one alone.  mre_correlate_dlogits and mre_attend_dlogits read the lse that the loss call of
the same library wrote, and the two gradients the g that its mre_correlate_dlogits wrote: those rows come after the rows they
depend on, and a difference there shows first as a different output of the earlier row.
"""
import ctypes as C

import numpy as np
import torch

from tests import attend_cases as AC
from tests import correlate_cases as CC
from tests import place_loss_cases as PC

DEV = "cuda"
F32, BF16 = 0, 1
# 98 560 cells: 49 chunks, S = 16, split 0 holds 4 chunks, so k_attend's loop over AT_AHEAD = 3 chunks runs a second time, with
# a partial last chunk; every shape of tests/attend_cases.py has at most 3 chunks per split
ATTEND_SHAPES = AC.SHAPES + [(1, 1, 256, 385)]
assert AC.chunks(256 * 385) == 49 and AC.split_cells(256 * 385)[0] == (0, 4 * AC.CHUNK)


def _raw(a) -> bytes:
    if isinstance(a, torch.Tensor):
        a = a.contiguous().reshape(-1).view(torch.uint8).numpy()
    return np.ascontiguousarray(a).tobytes()


class _Call:
    """The tensors of one call, each `off` elements past a 16-byte boundary of a buffer of its own."""

    def __init__(self, off):
        from mujoco_robot_environments_amd import dataset
        self.off, self.crc, self.ins, self.outs, self.held = off, dataset.crc32c, {}, {}, {}

    def put(self, name, a, item):
        raw = _raw(a)
        buf = torch.zeros(len(raw) + 32, dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 16 == 0
        at = self.off * item
        buf[at:at + len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
        self.ins[name] = self.crc(raw)
        self.held[name] = (buf, at, len(raw))
        return buf.data_ptr() + at

    def out(self, name, nbytes, item):
        buf = torch.full((nbytes + 32,), 0xDE, dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 16 == 0
        self.held[name] = (buf, self.off * item, nbytes)
        self.outs[name] = None
        return buf.data_ptr() + self.off * item

    def work(self, nbytes):
        buf = torch.full((nbytes + 16,), 0xDE, dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 16 == 0
        self.held["workspace"] = (buf, 0, nbytes)
        return buf.data_ptr()

    def read(self, name) -> bytes:
        buf, at, nbytes = self.held[name]
        return buf[at:at + nbytes].cpu().numpy().tobytes()

    def row(self, cid, rc):
        torch.cuda.synchronize()
        assert rc == 0, (cid, rc)
        for name in self.outs:
            self.outs[name] = self.crc(self.read(name))
        return [cid, self.ins, self.outs]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need(fn, *shape):
    need = C.c_size_t(0)
    assert fn(*shape, C.byref(need)) == 0
    return need.value


def _place_inputs(shape, scaled):
    """(scene, kern) as bfloat16 CPU tensors: correlate_cases.normal_inputs, `scaled`: kern times 2^-k ~ 1 / sqrt(K)"""
    n, rot, depth, h, w, crop = shape
    scene, kern = CC.normal_inputs(shape)
    if scaled:
        kern = kern * np.float32(2.0 ** -round(0.5 * np.log2(depth * crop * crop)))
    return CC.bf16(scene), CC.bf16(kern)


def _targets(n, cells, outside):
    t = [(7919 * (e + 1)) % cells for e in range(n)]
    if outside:
        t[-1] = cells
    return np.array(t, np.int64)


def _correlate(L, rows):
    for shape, sid in zip(CC.SHAPES, CC.IDS):
        n, rot, depth, h, w, crop = shape
        scene, kern = _place_inputs(shape, False)
        need = _need(L.mre_correlate_workspace, n, rot, h, w)
        # logits float32, bfloat16 and none, each with best_*; logits alone in both dtypes
        for what, dtype, logits, best in (("f32+best", F32, True, True), ("bf16+best", BF16, True, True), ("best", F32, False, True),
                                          ("f32", F32, True, False), ("bf16", BF16, True, False)):
            for off in (0, 1):
                c = _Call(off)
                s, k = c.put("scene", scene, 2), c.put("kern", kern, 2)
                esize = 2 if dtype == BF16 else 4
                lo = c.out("logits", esize * n * rot * h * w, esize) if logits else None
                bi, bv = (c.out("best_index", 8 * n, 8), c.out("best_value", 4 * n, 4)) if best else (None, None)
                rc = L.mre_correlate(_stream(), s, k, *shape, dtype, lo, bi, bv, c.work(need), need)
                rows.append(c.row(f"mre_correlate {sid} {what} a{off}", rc))


def _place_training(L, rows):
    for shape, sid in zip(PC.SHAPES, PC.IDS):
        n, rot, depth, h, w, crop = shape
        cells = rot * h * w
        need = _need(L.mre_correlate_workspace, n, rot, h, w)
        gneed = _need(L.mre_correlate_grad_workspace, *shape)
        for scaled in (False, True):
            scene, kern = _place_inputs(shape, scaled)
            kind = "scaled" if scaled else "normal"
            for off in (0, 1):
                lse = None
                for outside in (False, True):
                    c = _Call(off)
                    s, k = c.put("scene", scene, 2), c.put("kern", kern, 2)
                    t = c.put("target", _targets(n, cells, outside), 8)
                    rc = L.mre_correlate_loss(_stream(), s, k, *shape, t, c.out("lse", 4 * n, 4), c.out("target_logit", 4 * n, 4),
                                              c.out("loss", 4 * n, 4), c.work(need), need)
                    rows.append(c.row(f"mre_correlate_loss {sid} {kind} {'outside' if outside else 'inside'} a{off}", rc))
                    lse = lse or c.read("lse")
                g = None
                for weighted in (True, False):
                    c = _Call(off)
                    s, k = c.put("scene", scene, 2), c.put("kern", kern, 2)
                    t = c.put("target", _targets(n, cells, False), 8)
                    ls = c.put("lse", np.frombuffer(lse, np.float32), 4)
                    wg = c.put("weight", np.array([1.5, 0.25, 3.0][:n], np.float32), 4) if weighted else None
                    rc = L.mre_correlate_dlogits(_stream(), s, k, *shape, t, ls, wg, c.out("g", 2 * n * cells, 2))
                    rows.append(c.row(f"mre_correlate_dlogits {sid} {kind} {'weight' if weighted else 'no weight'} a{off}", rc))
                    g = g or c.read("g")
                for entry, other, oname, count in (("mre_correlate_grad_scene", kern, "kern", n * depth * h * w),
                                                   ("mre_correlate_grad_kern", scene, "scene", n * rot * depth * crop * crop)):
                    c = _Call(off)
                    gp, op = c.put("g", np.frombuffer(g, np.uint16), 2), c.put(oname, other, 2)
                    rc = getattr(L, entry)(_stream(), gp, op, *shape, c.out("out", 4 * count, 4), c.work(gneed), gneed)
                    rows.append(c.row(f"{entry} {sid} {kind} a{off}", rc))


def attend_logits(shape, normal, masked):
    """float32 [n, K, h, w]: standard-normal values or integers in -4 .. 4; `masked`: about a quarter of the cells are -inf"""
    rng = np.random.default_rng(6000 + 7 * sum(shape) + 2 * normal + masked)
    x = rng.standard_normal(shape).astype(np.float32) if normal else rng.integers(-4, 5, size=shape).astype(np.float32)
    if masked:
        x[rng.random(shape) < 0.25] = -np.inf
        x.reshape(shape[0], -1)[:, -1] = 0.0   # (every env keeps a finite cell)
    return x


def _attend(L, rows):
    for shape in ATTEND_SHAPES:
        n, k, h, w = shape
        cells = k * h * w
        need = _need(L.mre_attend_workspace, *shape)
        target = _targets(n, cells, False)
        for dtype, tdtype, esize in ((F32, torch.float32, 4), (BF16, torch.bfloat16, 2)):
            for normal in (False, True):
                for masked in (False, True):
                    logits = AC.as_tensor(attend_logits(shape, normal, masked), tdtype)
                    kind = "%dx%dx%dx%d %s %s%s" % (*shape, "bf16" if dtype == BF16 else "f32", "normal" if normal else "integer",
                                                    " masked" if masked else "")
                    for off in (0, 1):
                        lse = None
                        for what, best, soft in (("decision", True, False), ("loss", False, True), ("both", True, True)):
                            c = _Call(off)
                            x = c.put("logits", logits, esize)
                            t = c.put("target", target, 8) if soft else None
                            bi, bv = (c.out("best_index", 8 * n, 8), c.out("best_value", 4 * n, 4)) if best else (None, None)
                            so = [c.out(name, 4 * n, 4) for name in ("lse", "target_logit", "loss")] if soft else [None] * 3
                            rc = L.mre_attend(_stream(), x, *shape, dtype, t, bi, bv, *so, c.work(need), need)
                            rows.append(c.row(f"mre_attend {kind} {what} a{off}", rc))
                            if soft:
                                lse = c.read("lse")
                        for weighted in (True, False):
                            c = _Call(off)
                            x, t = c.put("logits", logits, esize), c.put("target", target, 8)
                            ls = c.put("lse", np.frombuffer(lse, np.float32), 4)
                            wg = c.put("weight", np.array([1.5, 0.25, 3.0][:n], np.float32), 4) if weighted else None
                            rc = L.mre_attend_dlogits(_stream(), x, *shape, dtype, t, ls, wg, c.out("g", esize * n * cells, esize))
                            rows.append(c.row(f"mre_attend_dlogits {kind} {'weight' if weighted else 'no weight'} a{off}", rc))


# the record in three parts, in its order: part -> (its calls, the entries whose rows they make)
PARTS = {"place": (_correlate, ("mre_correlate",)),
         "place_training": (_place_training, ("mre_correlate_loss", "mre_correlate_dlogits", "mre_correlate_grad_scene",
                                              "mre_correlate_grad_kern")),
         "pick": (_attend, ("mre_attend", "mre_attend_dlogits"))}


def digests(L, parts=tuple(PARTS)):
    """[[call id, {input: crc}, {output: crc}]] of every call above on the loaded library ``L``, in a fixed order"""
    rows = []
    for part in parts:
        PARTS[part][0](L, rows)
    assert len({r[0] for r in rows}) == len(rows)
    return rows
