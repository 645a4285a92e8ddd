"""Bad calls of the stream-only C ABI's perception entries, for tests/test_refusals.py and tests/golden/make_refusals.py:
what every check of mre_heightmap, mre_heightmap_views, mre_correlate, mre_correlate_loss, mre_correlate_dlogits,
mre_correlate_grad_scene, mre_correlate_grad_kern, mre_correlate_workspace, mre_attend, mre_attend_dlogits, mre_attend_workspace
and mre_correlate_grad_workspace answers, and in which order the checks come.

No case reaches a launch: every pointer is a HOST pointer into one arena, so a call that passes every other check is
refused by the entry's "must be device pointers" check, and a call with n == 0 returns before it.  The shapes are tiny, so
that the byte ranges an entry forms for its overlap check stay inside the slots the pointers come from: what a call
answers does not depend on where the arena lies.
"""
import ctypes as C

import numpy as np

SLOT = 1 << 16   # bytes between two pointers of the arena: far above any byte range of the shapes below
_ARENA = C.create_string_buffer(64 * SLOT + 4096)
_BASE = (C.addressof(_ARENA) + 4095) & ~4095


def slot(k: int) -> int:
    return _BASE + k * SLOT


def _put(k: int, array) -> int:
    a = np.ascontiguousarray(array)
    assert a.nbytes <= SLOT
    C.memmove(slot(k), a.ctypes.data, a.nbytes)
    return slot(k)


INF, NAN = float("inf"), float("nan")
CAM = np.array([0.01, 0, -0.03, 0, -0.01, 0.02, 0, 0, -1, 0.5, 0.0, 1.5], np.float32)
BOUNDS = np.array([0.2, -0.3, 0.0, 0.8, 0.3, 0.3], np.float32)

HEIGHTMAP = ["stream", "depth", "rgb", "seg", "n", "height", "width", "cam", "bounds", "inv_cell", "max_depth", "out_h",
             "out_w", "hmap", "cmap", "smap", "src"]
VIEWS = ["stream", "views", "depth", "rgb", "seg", "n", "height", "width", "cam", "bounds", "inv_cell", "max_depth", "out_h",
         "out_w", "hmap", "cmap", "smap", "src", "view"]
CORRELATE = ["stream", "scene", "kern", "n", "rotations", "depth", "h", "w", "crop", "dtype", "logits", "best_index",
             "best_value", "workspace", "workspace_bytes"]
LOSS = ["stream", "scene", "kern", "n", "rotations", "depth", "h", "w", "crop", "target", "lse", "target_logit", "loss",
        "workspace", "workspace_bytes"]
DLOGITS = ["stream", "scene", "kern", "n", "rotations", "depth", "h", "w", "crop", "target", "lse", "weight", "g"]
GRAD_SCENE = ["stream", "g", "kern", "n", "rotations", "depth", "h", "w", "crop", "out", "workspace", "workspace_bytes"]
GRAD_KERN = ["stream", "g", "scene", "n", "rotations", "depth", "h", "w", "crop", "out", "workspace", "workspace_bytes"]
WORKSPACE = ["n", "rotations", "h", "w", "bytes"]
ATTEND = ["stream", "logits", "n", "rotations", "h", "w", "dtype", "target", "best_index", "best_value", "lse", "target_logit",
          "loss", "workspace", "workspace_bytes"]
ATTEND_DLOGITS = ["stream", "logits", "n", "rotations", "h", "w", "dtype", "target", "lse", "weight", "g"]
ATTEND_WORKSPACE = ["n", "rotations", "h", "w", "bytes"]
GRAD_WORKSPACE = ["n", "rotations", "depth", "h", "w", "crop", "bytes"]


def cases():
    """[(id, entry point, argument tuple)] in a fixed order; the ids are unique."""
    out = []

    def table(entry, names, good, bad):
        for what, kw in bad:
            assert set(kw) <= set(names), (entry, what)
            out.append((f"{entry}: {what}", entry, tuple({**good, **kw}[k] for k in names)))

    # ---- mre_heightmap: 2 frames of 4 x 6 pixels into 5 x 7 cells
    bad_bounds, nan_bounds = BOUNDS.copy(), BOUNDS.copy()
    bad_bounds[1] = BOUNDS[4] + 1
    nan_bounds[5] = NAN
    cam, bounds = _put(0, CAM), _put(1, BOUNDS)
    lo_above_hi, not_finite = _put(2, bad_bounds), _put(3, nan_bounds)
    g = dict(stream=None, depth=slot(4), rgb=slot(5), seg=slot(6), n=2, height=4, width=6, cam=cam, bounds=bounds,
             inv_cell=10.0, max_depth=99.0, out_h=5, out_w=7, hmap=slot(7), cmap=slot(8), smap=slot(9), src=slot(10))
    table("mre_heightmap", HEIGHTMAP, g, [
        ("host pointers", {}), ("host pointers, depth alone", dict(rgb=None, cmap=None, seg=None, smap=None, src=None)),
        ("n == 0", dict(n=0)), ("n < 0", dict(n=-1)), ("height 0", dict(height=0)), ("width 0", dict(width=0)),
        ("2^31 pixels", dict(height=65536, width=32768)), ("out_h 0", dict(out_h=0)), ("out_w 4097", dict(out_w=4097)),
        ("inv_cell 0", dict(inv_cell=0.0)), ("inv_cell inf", dict(inv_cell=INF)), ("max_depth nan", dict(max_depth=NAN)),
        ("max_depth < 0", dict(max_depth=-1.0)), ("null cam", dict(cam=None)), ("null bounds", dict(bounds=None)),
        ("lo above hi", dict(bounds=lo_above_hi)), ("bounds not finite", dict(bounds=not_finite)),
        ("null depth", dict(depth=None)), ("null hmap", dict(hmap=None)), ("rgb without cmap", dict(cmap=None)),
        ("cmap without rgb", dict(rgb=None)), ("seg without smap", dict(smap=None)), ("smap without seg", dict(seg=None)),
        ("depth misaligned", dict(depth=g["depth"] + 2)), ("hmap misaligned", dict(hmap=g["hmap"] + 1)),
        ("src misaligned", dict(src=g["src"] + 2)),
        ("two: n < 0 and out_w 5000", dict(n=-1, out_w=5000)), ("two: out_h 0 and inv_cell 0", dict(out_h=0, inv_cell=0.0)),
        ("two: max_depth 0 and null cam", dict(max_depth=0.0, cam=None)),
        ("two: null cam and null depth", dict(cam=None, depth=None)),
        ("two: lo above hi and rgb without cmap", dict(bounds=lo_above_hi, cmap=None)),
        ("two: null hmap and src misaligned", dict(hmap=None, src=g["src"] + 2)),
        ("two: rgb without cmap and seg without smap", dict(cmap=None, smap=None)),
        ("n == 0 and hmap misaligned", dict(n=0, hmap=g["hmap"] + 2)), ("n == 0 and rgb without cmap", dict(n=0, cmap=None)),
    ])

    # ---- mre_heightmap_views: the same, two views of 4 x 6 and 3 x 5 pixels
    ptrs = lambda *p: np.array(p, np.uint64)
    depth2 = _put(11, ptrs(slot(4), slot(12)))
    rgb2, seg2 = _put(13, ptrs(slot(5), slot(14))), _put(15, ptrs(slot(6), slot(16)))
    heights, widths = _put(17, np.array([4, 3], np.int32)), _put(18, np.array([6, 5], np.int32))
    cams = _put(19, np.concatenate([CAM, CAM]))
    g = dict(stream=None, views=2, depth=depth2, rgb=rgb2, seg=seg2, n=2, height=heights, width=widths, cam=cams,
             bounds=bounds, inv_cell=10.0, max_depth=99.0, out_h=5, out_w=7, hmap=slot(7), cmap=slot(8), smap=slot(9),
             src=slot(10), view=slot(20))
    table("mre_heightmap_views", VIEWS, g, [
        ("host pointers", {}), ("host pointers, depth alone", dict(rgb=None, cmap=None, seg=None, smap=None, src=None, view=None)),
        ("one view, host pointers", dict(views=1)), ("n == 0", dict(n=0)), ("views 0", dict(views=0)), ("views 9", dict(views=9)),
        ("n < 0", dict(n=-1)), ("null height", dict(height=None)), ("null width", dict(width=None)),
        ("height 0 in view 1", dict(height=_put(21, np.array([4, 0], np.int32)))),
        ("2^28 pixels in view 1", dict(height=_put(22, np.array([4, 16384], np.int32)),
                                       width=_put(23, np.array([6, 16384], np.int32)))),
        ("out_h 4097", dict(out_h=4097)), ("out_w 0", dict(out_w=0)), ("inv_cell inf", dict(inv_cell=INF)),
        ("max_depth 0", dict(max_depth=0.0)), ("null cam", dict(cam=None)), ("null bounds", dict(bounds=None)),
        ("lo above hi", dict(bounds=lo_above_hi)), ("bounds not finite", dict(bounds=not_finite)),
        ("null depth", dict(depth=None)), ("null hmap", dict(hmap=None)), ("rgb without cmap", dict(cmap=None)),
        ("cmap without rgb", dict(rgb=None)), ("seg without smap", dict(smap=None)), ("smap without seg", dict(seg=None)),
        ("null depth of view 1", dict(depth=_put(24, ptrs(slot(4), 0)))),
        ("null rgb of view 0", dict(rgb=_put(25, ptrs(0, slot(14))))),
        ("null seg of view 1", dict(seg=_put(26, ptrs(slot(6), 0)))),
        ("depth of view 1 misaligned", dict(depth=_put(27, ptrs(slot(4), slot(12) + 2)))),
        ("hmap misaligned", dict(hmap=g["hmap"] + 2)), ("src misaligned", dict(src=g["src"] + 1)),
        ("two: views 9 and n < 0", dict(views=9, n=-1)), ("two: null height and out_h 0", dict(height=None, out_h=0)),
        ("two: height 0 in view 1 and out_w 0", dict(height=slot(21), out_w=0)),
        ("two: max_depth 0 and null hmap", dict(max_depth=0.0, hmap=None)),
        ("two: null bounds and null depth", dict(bounds=None, depth=None)),
        ("two: seg without smap and null depth of view 1", dict(smap=None, depth=slot(24))),
        ("two: null rgb of view 0 and hmap misaligned", dict(rgb=slot(25), hmap=g["hmap"] + 2)),
        ("n == 0 and null depth of view 1", dict(n=0, depth=slot(24))), ("n == 0 and src misaligned", dict(n=0, src=g["src"] + 2)),
    ])

    # ---- the place head: 2 envs, 2 rotations, depth 2, 8 x 8 cells, crops of 4 x 4
    shape = dict(n=2, rotations=2, depth=2, h=8, w=8, crop=4)
    scene, kern, logits, best_index, best_value, work = (slot(k) for k in range(30, 36))
    g = dict(stream=None, scene=scene, kern=kern, **shape, dtype=0, logits=logits, best_index=best_index,
             best_value=best_value, workspace=work, workspace_bytes=SLOT)
    ranges = [("n < 0", dict(n=-1)), ("rotations 0", dict(rotations=0)), ("rotations 65", dict(rotations=65)),
              ("depth 0", dict(depth=0)), ("depth 17", dict(depth=17)), ("crop odd", dict(crop=3)), ("crop 0", dict(crop=0)),
              ("crop 66", dict(crop=66)), ("h 0", dict(h=0)), ("w 4097", dict(w=4097)),
              ("two: rotations 0 and crop odd", dict(rotations=0, crop=3)), ("two: n < 0 and w 0", dict(n=-1, w=0)),
              ("two: depth 17 and h 4097", dict(depth=17, h=4097))]
    table("mre_correlate", CORRELATE, g, [
        ("host pointers", {}), ("host pointers, no logits", dict(logits=None)),
        ("host pointers, bf16 logits alone", dict(dtype=1, best_index=None, best_value=None)), ("n == 0", dict(n=0)), *ranges,
        ("null scene", dict(scene=None)), ("null kern", dict(kern=None)), ("kern misaligned", dict(kern=kern + 1)),
        ("dtype 2", dict(dtype=2)), ("float32 logits misaligned", dict(logits=logits + 2)),
        ("bf16 logits misaligned", dict(dtype=1, logits=logits + 1)), ("best_index without best_value", dict(best_value=None)),
        ("best_value without best_index", dict(best_index=None)), ("best_index misaligned", dict(best_index=best_index + 4)),
        ("best_value misaligned", dict(best_value=best_value + 2)),
        ("nothing to write", dict(logits=None, best_index=None, best_value=None)), ("null workspace", dict(workspace=None)),
        ("workspace misaligned", dict(workspace=work + 8)), ("workspace too small", dict(workspace_bytes=15)),
        ("logits on scene", dict(logits=scene)), ("workspace inside kern", dict(workspace=kern + 16)),
        ("two: crop odd and null scene", dict(crop=3, scene=None)), ("two: null scene and dtype 7", dict(scene=None, dtype=7)),
        ("two: dtype 2 and nothing to write", dict(dtype=2, logits=None, best_index=None, best_value=None)),
        ("two: best_index misaligned and null workspace", dict(best_index=best_index + 4, workspace=None)),
        ("two: workspace too small and logits on scene", dict(workspace_bytes=0, logits=scene)),
        ("n == 0 and null workspace", dict(n=0, workspace=None)), ("n == 0 and logits on scene", dict(n=0, logits=scene)),
        ("n == 0 and dtype 2", dict(n=0, dtype=2)),
    ])

    target, lse, target_logit, loss, weight, grad = (slot(k) for k in range(36, 42))
    g = dict(stream=None, scene=scene, kern=kern, **shape, target=target, lse=lse, target_logit=target_logit, loss=loss,
             workspace=work, workspace_bytes=SLOT)
    table("mre_correlate_loss", LOSS, g, [
        ("host pointers", {}), ("n == 0", dict(n=0)), *ranges,
        ("null kern", dict(kern=None)), ("null target", dict(target=None)), ("scene misaligned", dict(scene=scene + 1)),
        ("target misaligned", dict(target=target + 4)), ("null lse", dict(lse=None)), ("null loss", dict(loss=None)),
        ("target_logit misaligned", dict(target_logit=target_logit + 2)), ("null workspace", dict(workspace=None)),
        ("workspace too small", dict(workspace_bytes=8)), ("lse on target", dict(lse=target)), ("workspace on scene", dict(workspace=scene)),
        ("two: crop odd and null target", dict(crop=3, target=None)), ("two: h 0 and null workspace", dict(h=0, workspace=None)),
        ("two: target misaligned and null lse", dict(target=target + 4, lse=None)),
        ("two: loss misaligned and workspace too small", dict(loss=loss + 1, workspace_bytes=0)),
        ("n == 0 and null loss", dict(n=0, loss=None)), ("n == 0 and lse on target", dict(n=0, lse=target)),
    ])

    g = dict(stream=None, scene=scene, kern=kern, **shape, target=target, lse=lse, weight=weight, g=grad)
    table("mre_correlate_dlogits", DLOGITS, g, [
        ("host pointers", {}), ("host pointers, no weight", dict(weight=None)), ("n == 0", dict(n=0)), *ranges,
        ("null scene", dict(scene=None)), ("null lse", dict(lse=None)), ("kern misaligned", dict(kern=kern + 1)),
        ("target misaligned", dict(target=target + 2)), ("lse misaligned", dict(lse=lse + 2)),
        ("weight misaligned", dict(weight=weight + 1)), ("null g", dict(g=None)), ("g misaligned", dict(g=grad + 1)),
        ("g on kern", dict(g=kern)), ("g on weight", dict(g=weight)),
        ("two: n < 0 and null g", dict(n=-1, g=None)), ("two: null lse and target misaligned", dict(lse=None, target=target + 2)),
        ("two: weight misaligned and g on kern", dict(weight=weight + 1, g=kern)),
        ("n == 0 and null g", dict(n=0, g=None)), ("n == 0 and g on kern", dict(n=0, g=kern)),
    ])

    for entry, names, other in (("mre_correlate_grad_scene", GRAD_SCENE, "kern"), ("mre_correlate_grad_kern", GRAD_KERN, "scene")):
        o = dict(kern=kern, scene=scene)[other]
        g = dict(stream=None, g=grad, **{other: o}, **shape, out=logits, workspace=work, workspace_bytes=SLOT)
        table(entry, names, g, [
            ("host pointers", {}), ("n == 0", dict(n=0)), *ranges,
            ("null g", dict(g=None)), (f"null {other}", {other: None}), ("g misaligned", dict(g=grad + 1)),
            (f"{other} misaligned", {other: o + 1}), ("null out", dict(out=None)), ("out misaligned", dict(out=logits + 2)),
            ("null workspace", dict(workspace=None)), ("workspace misaligned", dict(workspace=work + 4)),
            ("workspace too small", dict(workspace_bytes=15)), ("out on g", dict(out=grad)), (f"workspace on {other}", dict(workspace=o)),
            (f"two: crop 66 and null {other}", {"crop": 66, other: None}), ("two: null g and null out", dict(g=None, out=None)),
            ("two: out misaligned and null workspace", dict(out=logits + 2, workspace=None)),
            ("two: workspace too small and out on g", dict(workspace_bytes=0, out=grad)),
            ("n == 0 and null out", dict(n=0, out=None)), ("n == 0 and out on g", dict(n=0, out=grad)),
            ("n < 0 and null g", dict(n=-1, g=None)),
        ])

    nbytes = C.cast(slot(42), C.POINTER(C.c_size_t))
    table("mre_correlate_workspace", WORKSPACE, dict(n=2, rotations=2, h=8, w=8, bytes=nbytes), [
        ("good", {}), ("n == 0", dict(n=0)), ("null bytes", dict(bytes=None)), ("n < 0", dict(n=-1)),
        ("rotations 0", dict(rotations=0)), ("rotations 65", dict(rotations=65)), ("h 0", dict(h=0)), ("w 4097", dict(w=4097)),
        ("two: null bytes and n < 0", dict(bytes=None, n=-1)), ("two: rotations 65 and h 0", dict(rotations=65, h=0)),
    ])
    # ---- the pick head: 2 envs, 2 rotations, 8 x 8 cells
    shape = dict(n=2, rotations=2, h=8, w=8)
    alogits, agrad = slot(43), slot(44)
    aranges = [("n < 0", dict(n=-1)), ("rotations 0", dict(rotations=0)), ("rotations 65", dict(rotations=65)), ("h 0", dict(h=0)),
               ("w 4097", dict(w=4097)), ("dtype 2", dict(dtype=2)), ("two: rotations 0 and h 0", dict(rotations=0, h=0)),
               ("two: n < 0 and w 0", dict(n=-1, w=0)), ("two: h 4097 and dtype 7", dict(h=4097, dtype=7))]
    g = dict(stream=None, logits=alogits, **shape, dtype=0, target=target, best_index=best_index, best_value=best_value, lse=lse,
             target_logit=target_logit, loss=loss, workspace=work, workspace_bytes=SLOT)
    no_best, no_loss = dict(best_index=None, best_value=None), dict(target=None, lse=None, target_logit=None, loss=None)
    table("mre_attend", ATTEND, g, [
        ("host pointers", {}), ("host pointers, the decision alone", no_loss), ("host pointers, the loss alone", no_best),
        ("host pointers, bf16", dict(dtype=1)), ("n == 0", dict(n=0)), *aranges,
        ("null logits", dict(logits=None)), ("float32 logits misaligned", dict(logits=alogits + 2)),
        ("bf16 logits misaligned", dict(dtype=1, logits=alogits + 1)), ("best_index without best_value", dict(best_value=None)),
        ("best_value without best_index", dict(best_index=None)), ("best_index misaligned", dict(best_index=best_index + 4)),
        ("best_value misaligned", dict(best_value=best_value + 2)), ("target without lse", dict(lse=None)),
        ("target without target_logit", dict(target_logit=None)), ("target without loss", dict(loss=None)),
        ("lse without target", dict(target=None)), ("loss alone", dict(target=None, lse=None, target_logit=None)),
        ("target misaligned", dict(target=target + 4)), ("lse misaligned", dict(lse=lse + 2)),
        ("target_logit misaligned", dict(target_logit=target_logit + 1)), ("loss misaligned", dict(loss=loss + 2)),
        ("nothing to write", {**no_best, **no_loss}), ("null workspace", dict(workspace=None)),
        ("workspace misaligned", dict(workspace=work + 8)), ("workspace too small", dict(workspace_bytes=31)),
        ("lse on target", dict(lse=target)), ("best_value on logits", dict(best_value=alogits)),
        ("workspace inside logits", dict(workspace=alogits + 16)),
        ("two: dtype 2 and null logits", dict(dtype=2, logits=None)),
        ("two: null logits and best_index without best_value", dict(logits=None, best_value=None)),
        ("two: best_index misaligned and target without lse", dict(best_index=best_index + 4, lse=None)),
        ("two: target without loss and target misaligned", dict(loss=None, target=target + 4)),
        ("two: target misaligned and lse misaligned", dict(target=target + 4, lse=lse + 2)),
        ("two: loss misaligned and nothing to write", {**no_best, **no_loss, "loss": loss + 2}),
        ("two: nothing to write and null workspace", {**no_best, **no_loss, "workspace": None}),
        ("two: workspace too small and lse on target", dict(workspace_bytes=0, lse=target)),
        ("n == 0 and null workspace", dict(n=0, workspace=None)), ("n == 0 and lse on target", dict(n=0, lse=target)),
        ("n == 0 and dtype 2", dict(n=0, dtype=2)),
    ])

    g = dict(stream=None, logits=alogits, **shape, dtype=0, target=target, lse=lse, weight=weight, g=agrad)
    table("mre_attend_dlogits", ATTEND_DLOGITS, g, [
        ("host pointers", {}), ("host pointers, no weight", dict(weight=None)), ("host pointers, bf16", dict(dtype=1)),
        ("n == 0", dict(n=0)), *aranges,
        ("null logits", dict(logits=None)), ("null target", dict(target=None)), ("null lse", dict(lse=None)),
        ("float32 logits misaligned", dict(logits=alogits + 2)), ("bf16 logits misaligned", dict(dtype=1, logits=alogits + 1)),
        ("target misaligned", dict(target=target + 2)), ("lse misaligned", dict(lse=lse + 2)),
        ("weight misaligned", dict(weight=weight + 1)), ("null g", dict(g=None)), ("float32 g misaligned", dict(g=agrad + 2)),
        ("bf16 g misaligned", dict(dtype=1, g=agrad + 1)), ("g on logits", dict(g=alogits)), ("g on weight", dict(g=weight)),
        ("two: dtype 2 and null lse", dict(dtype=2, lse=None)), ("two: null target and logits misaligned", dict(target=None, logits=alogits + 2)),
        ("two: logits misaligned and target misaligned", dict(logits=alogits + 2, target=target + 2)),
        ("two: target misaligned and weight misaligned", dict(target=target + 2, weight=weight + 1)),
        ("two: lse misaligned and null g", dict(lse=lse + 2, g=None)), ("two: g misaligned and g on logits", dict(g=alogits + 2)),
        ("n == 0 and null g", dict(n=0, g=None)), ("n == 0 and g on logits", dict(n=0, g=alogits)),
    ])

    nbytes = C.cast(slot(45), C.POINTER(C.c_size_t))
    table("mre_attend_workspace", ATTEND_WORKSPACE, dict(**shape, bytes=nbytes), [
        ("good", {}), ("n == 0", dict(n=0)), ("null bytes", dict(bytes=None)), ("n < 0", dict(n=-1)),
        ("rotations 0", dict(rotations=0)), ("rotations 65", dict(rotations=65)), ("h 0", dict(h=0)), ("w 4097", dict(w=4097)),
        ("two: null bytes and n < 0", dict(bytes=None, n=-1)), ("two: rotations 65 and h 0", dict(rotations=65, h=0)),
    ])
    table("mre_correlate_grad_workspace", GRAD_WORKSPACE, dict(n=2, rotations=2, depth=2, h=8, w=8, crop=4, bytes=nbytes), [
        ("good", {}), ("n == 0", dict(n=0)), ("null bytes", dict(bytes=None)), *ranges,
        ("two: null bytes and crop odd", dict(bytes=None, crop=3)), ("n == 0 and depth 0", dict(n=0, depth=0)),
    ])
    assert len({c[0] for c in out}) == len(out)
    return out


def answers(L):
    """[[id, return code, message]] of ``cases()`` on the loaded library ``L``.  A call that returns 0 sets no message
    (mre_last_error keeps that of an earlier refusal), so its message is recorded as empty."""
    res = []
    for what, entry, args in cases():
        rc = int(getattr(L, entry)(*args))
        res.append([what, rc, L.mre_last_error().decode() if rc else ""])
    return res
