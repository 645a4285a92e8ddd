"""GPU tests of mre_correlate (csrc/mre_correlate.hip) against the torch statement perception.correlate_reference, which
tests/test_correlate.py checks against plain loops.  The shapes (n, R, depth, h x w, crop) are those of
tests/correlate_cases.py, the smallest at which each mechanism of the kernel can break.

Most inputs are integers in -2 .. 2: every partial sum is an integer below 2^24, the float32 result is exact in any order,
and the comparison is EXACT: every bit of every logit, no tolerance, no cell left out.  One test compares standard-normal
inputs with the float64 correlation under the derived bound  |error| <= K * 2^-23 * sum |scene| |kern|  over the cell's own
terms (2^-23, not 2^-24: the rounding of the matrix core's internal additions is not documented as nearest).

Every call of the C ABI here reads its inputs from between NaN guards (a guard that reached a sum would show) at element
offset 0 (the 16-byte loads of the kernel rows) and 1 (the element-wise ones), writes the logits into a sentinel-filled
buffer at element offsets 0 (the vector stores where the width allows) to 3, and has best_* and the workspace in
sentinel-filled buffers; no sentinel outside the outputs may change, and the workspace's sentinel, larger than any sum,
never comes back as a best value.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import correlate_cases as CC
from tests import warp_input_cases as IC

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD16 = 0x7FC0                        # a bfloat16 NaN
SENT32, SENT16 = -0x21524111, -0x2153   # the bits 0xDEADBEEF and 0xDEAD
SENT64 = -0x2152411021524111            # 0xDEADBEEFDEADBEEF
WORK32 = 0x7F000000                     # 1.7e38 as a float, and no index of any call: a slot read before it is written wins
F32, BF16 = torch.float32, torch.bfloat16
PAD = 64                                # elements of guard before the data: 128 bytes, so offset 0 is 16-byte aligned


def _lib():
    from mujoco_robot_environments_amd import lib as L
    return L.lib()


def _guarded(t, off):
    """A bfloat16 CPU tensor on the device between NaN guards, `off` elements past a 16-byte boundary: (buffer, start)."""
    flat = t.contiguous().view(torch.int16).reshape(-1)
    buf = torch.full((flat.numel() + 2 * PAD + 1,), GUARD16, dtype=torch.int16, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[PAD + off: PAD + off + flat.numel()] = flat.to(DEV)
    return buf, PAD + off


def _workspace_bytes(n, rot, h, w):
    need = C.c_size_t(0)
    assert _lib().mre_correlate_workspace(n, rot, h, w, C.byref(need)) == 0
    return need.value


def _raw(a):
    """mre_correlate on torch's current stream with the arguments of dict a (pointers as ints or None); the status."""
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib().mre_correlate(stream, a["scene"], a["kern"], a["n"], a["rotations"], a["depth"], a["h"], a["w"], a["crop"],
                              a["dtype"], a["logits"], a["best_index"], a["best_value"], a["workspace"], a["workspace_bytes"])
    torch.cuda.synchronize()
    return rc


def _call(scene, kern, dtype=F32, off=0, in_off=0, best=True):
    """One call of the C ABI on bfloat16 CPU tensors.  Asserts the status, the sentinels and the guards; returns (logits as
    float32 values or bfloat16 bits, or None; index int64 [n] or None; value float32 [n] or None) as numpy."""
    n, depth, h, w = scene.shape
    rot, crop = kern.shape[1], kern.shape[3]
    what = (tuple(scene.shape), tuple(kern.shape), dtype, off, in_off, best)
    sbuf, s0 = _guarded(scene, in_off)
    kbuf, k0 = _guarded(kern, in_off)
    total = n * rot * h * w
    bf = dtype == BF16
    lbuf = None if dtype is None else torch.full((total + 8,), SENT16 if bf else SENT32,
                                                 dtype=torch.int16 if bf else torch.int32, device=DEV)
    ibuf = torch.full((n + 2,), SENT64, dtype=torch.int64, device=DEV)
    vbuf = torch.full((n + 2,), SENT32, dtype=torch.int32, device=DEV)
    need = _workspace_bytes(n, rot, h, w)
    wbuf = torch.full((need // 4 + 8,), WORK32, dtype=torch.int32, device=DEV)
    assert wbuf.data_ptr() % 16 == 0 and (lbuf is None or lbuf.data_ptr() % 16 == 0)
    rc = _raw(dict(scene=sbuf[s0:].data_ptr(), kern=kbuf[k0:].data_ptr(), n=n, rotations=rot, depth=depth, h=h, w=w, crop=crop,
                   dtype=int(bf), logits=None if lbuf is None else lbuf[off:].data_ptr(),
                   best_index=ibuf[1:].data_ptr() if best else None, best_value=vbuf[1:].data_ptr() if best else None,
                   workspace=wbuf.data_ptr(), workspace_bytes=need))
    assert rc == 0, what + (rc, _lib().mre_last_error())
    logits = index = value = None
    if lbuf is not None:
        got = lbuf.cpu().numpy().view(np.uint16 if bf else np.uint32)
        rest = np.concatenate([got[:off], got[off + total:]])
        assert (rest == (0xDEAD if bf else 0xDEADBEEF)).all(), what
        logits = got[off:off + total].reshape(n, rot, h, w)
        logits = logits if bf else logits.view(np.float32)
    i_all, v_all = ibuf.cpu().numpy(), vbuf.cpu().numpy()
    if best:
        assert i_all[0] == SENT64 and i_all[-1] == SENT64 and v_all[0] == SENT32 and v_all[-1] == SENT32, what
        index, value = i_all[1:-1].copy(), v_all[1:-1].copy().view(np.float32)
        assert not (v_all[1:-1] == WORK32).any() and not (v_all[1:-1] == SENT32).any(), what
        assert ((index >= 0) & (index < rot * h * w)).all(), what
    else:
        assert (i_all == SENT64).all() and (v_all == SENT32).all(), what
    assert bool((wbuf[need // 4:] == WORK32).all()), what
    for buf, start, t in ((sbuf, s0, scene), (kbuf, k0, kern)):
        assert bool((buf[:start] == GUARD16).all()) and bool((buf[start + t.numel():] == GUARD16).all()), what
        assert torch.equal(buf[start:start + t.numel()].cpu(), t.contiguous().view(torch.int16).reshape(-1)), what
    return logits, index, value


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    same = got.view(np.uint32 if got.dtype == np.float32 else got.dtype) == want.view(np.uint32 if want.dtype == np.float32 else want.dtype)
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:4].tolist())


@pytest.mark.parametrize("shape", CC.SHAPES, ids=CC.IDS)
def test_random_integer_inputs_match_the_statement_exactly(shape):
    from mujoco_robot_environments_amd import perception as P
    scene, kern, logits, index, value = CC.reference(shape)
    assert np.abs(logits).max() < 2 ** 24
    want16 = IC.bf16_bits(logits).reshape(logits.shape)
    for in_off in (0, 1):
        for dtype in (F32, BF16):
            for off in (0, 1, 2, 3):
                got, gi, gv = _call(scene, kern, dtype, off, in_off)
                what = (shape, dtype, off, in_off)
                _same(got, want16 if dtype == BF16 else logits, what)
                assert np.array_equal(gi, index) and np.array_equal(gv.view(np.uint32), value.view(np.uint32)), what
                if dtype == F32:   # and numpy's first-occurrence argmax of the logits the kernel wrote
                    ni, nv = CC.first_argmax(got)
                    assert np.array_equal(gi, ni) and np.array_equal(gv.view(np.uint32), nv.view(np.uint32)), what
        _, gi, gv = _call(scene, kern, None, 0, in_off)
        assert np.array_equal(gi, index) and np.array_equal(gv.view(np.uint32), value.view(np.uint32)), (shape, in_off)
        got, gi, gv = _call(scene, kern, F32, in_off, in_off, best=False)
        _same(got, logits, (shape, "logits alone"))
        assert gi is None and gv is None
    # through the wrapper, on torch's stream; a second call gives the same bytes
    s, k = scene.to(DEV), kern.to(DEV)
    for dtype in (None, F32, BF16):
        a, b = P.correlate(s, k, logits=dtype), P.correlate(s, k, logits=dtype)
        assert a.index.is_cuda and a.index.dtype == torch.int64 and a.value.dtype == torch.float32
        assert np.array_equal(a.index.cpu().numpy(), index) and np.array_equal(a.value.cpu().numpy().view(np.uint32), value.view(np.uint32))
        assert torch.equal(a.index, b.index) and torch.equal(a.value.view(torch.int32), b.value.view(torch.int32))
        if dtype is None:
            assert a.logits is None
        else:
            assert a.logits.dtype == dtype and a.logits.shape == logits.shape and a.logits.is_contiguous()
            bits = a.logits.view(torch.int16 if dtype == BF16 else torch.int32)
            assert torch.equal(bits, b.logits.view(bits.dtype))
            _same(bits.cpu().numpy().view(np.uint16) if dtype == BF16 else a.logits.cpu().numpy(), want16 if dtype == BF16 else logits,
                  (shape, dtype, "wrapper"))


def _one_hot(shape, taps):
    """For every (r, d, i, j) of taps: the logits of r are the scene's channel d shifted by (i - crop/2, j - crop/2) and
    zero-filled, every other rotation is all zeros."""
    from mujoco_robot_environments_amd import perception as P
    n, rot, depth, h, w, crop = shape
    scene = CC.integer_inputs(shape, seed=1)[0]
    scene[scene == 0] = 1.0   # no zero in the scene: a cell that should be zero-filled cannot be right by accident
    s = CC.bf16(scene).to(DEV)
    for r, d, i, j in taps:
        kern = np.zeros((n, rot, depth, crop, crop), np.float32)
        kern[:, r, d, i, j] = 1.0
        want = np.zeros((n, rot, h, w), np.float32)
        for e in range(n):
            want[e, r] = CC.shifted(scene[e, d], i - crop // 2, j - crop // 2)
        got = P.correlate(s, CC.bf16(kern).to(DEV), logits=F32)
        _same(got.logits.cpu().numpy(), want, (shape, r, d, i, j))
        wi, wv = CC.first_argmax(want)
        assert np.array_equal(got.index.cpu().numpy(), wi) and np.array_equal(got.value.cpu().numpy(), wv), (shape, r, d, i, j)


def test_one_hot_kernels_shift_the_scene_at_every_tap_of_crop_8():
    shape = CC.SHAPES[1]
    n, rot, depth, h, w, crop = shape
    _one_hot(shape, [((i * crop + j) % rot, (i + j) % depth, i, j) for i in range(crop) for j in range(crop)])
    shape = CC.SHAPES[2]   # and into the padded rotation tile
    _one_hot(shape, [(16, 0, 0, 0), (16, 0, 7, 7), (15, 0, 4, 4), (0, 0, 3, 5)])


def test_one_hot_kernels_at_the_corners_and_the_pivot_of_crop_64():
    _one_hot(CC.WORKLOAD, [(0, 0, 0, 0), (17, 1, 0, 63), (35, 2, 63, 0), (16, 0, 63, 63), (31, 1, 32, 32)])


def test_ties_go_to_the_lowest_flat_index():
    from mujoco_robot_environments_amd import perception as P
    n, rot, depth, h, w, crop = CC.SHAPES[4]
    zero = P.correlate(torch.zeros((n, depth, h, w), dtype=BF16, device=DEV), torch.zeros((n, rot, depth, crop, crop), dtype=BF16, device=DEV))
    assert zero.index.tolist() == [0] * n and zero.value.tolist() == [0.0] * n
    # two identical blobs, in different workgroups' tiles: two equal peaks, and the lower row wins although its column is
    # the higher; rotations 1 and 2 hold the blob, 0 holds nothing: rotation 1 wins
    rng = np.random.default_rng(5)
    crop = 8
    blob = rng.integers(1, 3, size=(crop, crop)).astype(np.float32)
    scene = np.zeros((1, 1, h, w), np.float32)
    for row, col in ((5, 40), (20, 10)):
        scene[0, 0, row - 4: row + 4, col - 4: col + 4] = blob
    kern = np.zeros((1, 3, 1, crop, crop), np.float32)
    kern[0, 1:] = blob
    peak = float((blob * blob).sum())
    got = P.correlate(CC.bf16(scene).to(DEV), CC.bf16(kern).to(DEV), logits=F32)
    lg = got.logits.cpu().numpy()
    assert lg[0, 1, 5, 40] == peak and lg[0, 1, 20, 10] == peak and lg[0, 2, 5, 40] == peak and (lg == peak).sum() == 4 and lg.max() == peak
    assert got.index.tolist() == [(1 * h + 5) * w + 40] and got.value.tolist() == [peak]
    ref = P.correlate_reference(CC.bf16(scene), CC.bf16(kern))
    assert ref.index.tolist() == got.index.tolist()
    # two equal peaks in one lane's own columns (row 3, columns 3 and 6 of the first wave), crop 2
    scene = np.zeros((1, 1, 8, 16), np.float32)
    scene[0, 0, 2:4, 2:4] = 1.0
    scene[0, 0, 2:4, 5:7] = 1.0
    got = P.correlate(CC.bf16(scene).to(DEV), torch.ones((1, 1, 1, 2, 2), dtype=BF16, device=DEV), logits=F32)
    lg = got.logits.cpu().numpy()
    assert lg[0, 0, 3, 3] == 4.0 and lg[0, 0, 3, 6] == 4.0 and (lg == 4.0).sum() == 2 and lg.max() == 4.0
    assert got.index.tolist() == [3 * 16 + 3] and got.value.tolist() == [4.0]


def test_a_padded_rotation_never_wins():
    """R = 17: the second rotation tile holds one rotation and 15 padded rows.  With everything but rotation 16 zeroed the
    best cell lies in rotation 16 -- not beyond it -- and is the statement's."""
    from mujoco_robot_environments_amd import perception as P
    shape = CC.SHAPES[2]
    scene, kern = CC.integer_inputs(shape, seed=2)
    kern[:, :16] = 0.0
    ref = P.correlate_reference(CC.bf16(scene), CC.bf16(kern))
    assert (ref.value > 0).all() and (ref.index >= 16 * 5 * 7).all()
    for in_off in (0, 1):
        _, gi, gv = _call(CC.bf16(scene), CC.bf16(kern), None, 0, in_off)
        assert np.array_equal(gi, ref.index.numpy()) and np.array_equal(gv, ref.value.numpy())


@pytest.mark.parametrize("shape", [CC.SHAPES[4], CC.WORKLOAD], ids=[CC.IDS[4], CC.IDS[6]])
def test_best_is_the_same_bits_whether_or_not_the_logits_are_written(shape):
    scene, kern = (CC.bf16(x) for x in CC.normal_inputs(shape, seed=3))
    l32, i32, v32 = _call(scene, kern, F32)
    l16, i16, v16 = _call(scene, kern, BF16)
    _, i0, v0 = _call(scene, kern, None)
    for gi, gv in ((i16, v16), (i0, v0)):
        assert np.array_equal(gi, i32) and np.array_equal(gv.view(np.uint32), v32.view(np.uint32))
    _same(l16, IC.bf16_bits(l32).reshape(l32.shape), (shape, "bfloat16 logits are wi_bf16 of the float32 ones"))
    ni, nv = CC.first_argmax(l32)
    assert np.array_equal(i32, ni) and np.array_equal(v32.view(np.uint32), nv.view(np.uint32))
    again = _call(scene, kern, F32, 1, 1)   # other offsets, other load and store paths: the same bytes
    _same(again[0], l32, (shape, "a second call"))
    assert np.array_equal(again[1], i32) and np.array_equal(again[2].view(np.uint32), v32.view(np.uint32))


def test_normal_inputs_stay_inside_the_derived_bound():
    """Standard-normal inputs rounded to bfloat16 at the workload's crop, against the float64 correlation of the same
    bfloat16 values: |error| <= K * 2^-23 * sum |scene| |kern| over the cell's own terms."""
    from mujoco_robot_environments_amd import perception as P
    shape = CC.WORKLOAD
    n, rot, depth, h, w, crop = shape
    scene, kern = CC.normal_inputs(shape, seed=4)

    def conv64(a, b):
        x = torch.from_numpy(a).to(torch.float64).reshape(1, n * depth, h, w)
        k = torch.from_numpy(b).to(torch.float64).reshape(n * rot, depth, crop, crop)
        return torch.nn.functional.conv2d(x, k, padding=crop // 2, groups=n)[..., :h, :w].reshape(n, rot, h, w).numpy()

    exact, mass = conv64(scene, kern), conv64(np.abs(scene), np.abs(kern))
    bound = depth * crop * crop * 2.0 ** -23 * mass
    assert (bound > 0).all()
    got = P.correlate(CC.bf16(scene).to(DEV), CC.bf16(kern).to(DEV), logits=F32)
    err = np.abs(got.logits.cpu().numpy().astype(np.float64) - exact)
    ratio = float((err / bound).max())
    print("worst |error| / bound = %.3g, worst |error| = %.3g, largest |logit| = %.3g" % (ratio, err.max(), np.abs(exact).max()))
    assert ratio <= 1.0
    wi, _ = CC.first_argmax(got.logits.cpu().numpy())
    assert np.array_equal(got.index.cpu().numpy(), wi)


def test_empty_calls_and_refused_arguments_write_nothing():
    n, rot, depth, h, w, crop = shape = CC.SHAPES[1]
    scene, kern, logits, index, value = CC.reference(shape)
    ns, nk, total = scene.numel(), kern.numel(), n * rot * h * w
    need = _workspace_bytes(n, rot, h, w)
    # one allocation, so that overlapping ranges can be built from it: [scene | kern | gap | logits | index | value | work]
    o_kern, o_log = 2 * ns, 2 * (ns + nk) + 64
    o_idx = o_log + 4 * total + 8
    o_idx += -o_idx % 8
    o_val = o_idx + 8 * n + 8
    o_work = o_val + 4 * n + 16
    o_work += -o_work % 16
    buf = torch.full((o_work + need + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    buf[:o_kern] = scene.view(torch.uint8).reshape(-1).to(DEV)
    buf[o_kern:o_kern + 2 * nk] = kern.view(torch.uint8).reshape(-1).to(DEV)
    snapshot = buf.clone()
    b0 = buf.data_ptr()
    assert b0 % 16 == 0
    good = dict(scene=b0, kern=b0 + o_kern, n=n, rotations=rot, depth=depth, h=h, w=w, crop=crop, dtype=0, logits=b0 + o_log,
                best_index=b0 + o_idx, best_value=b0 + o_val, workspace=b0 + o_work, workspace_bytes=need)
    host = np.zeros(4096, np.uint8)
    bad = [dict(n=-1), dict(rotations=0), dict(rotations=65), dict(depth=0), dict(depth=17), dict(crop=0), dict(crop=7), dict(crop=66),
           dict(h=0), dict(w=0), dict(h=4097), dict(w=4097), dict(scene=None), dict(kern=None), dict(scene=b0 + 1), dict(kern=b0 + o_kern + 1),
           dict(scene=host.ctypes.data), dict(kern=host.ctypes.data), dict(logits=host.ctypes.data), dict(workspace=host.ctypes.data - host.ctypes.data % 16 + 16),
           dict(dtype=2), dict(dtype=-1), dict(logits=b0 + o_log + 2), dict(dtype=1, logits=b0 + o_log + 1),
           dict(best_index=None), dict(best_value=None), dict(best_index=b0 + o_idx + 4), dict(best_value=b0 + o_val + 2),
           dict(logits=None, best_index=None, best_value=None),
           dict(workspace=None), dict(workspace=b0 + o_work + 8), dict(workspace_bytes=need - 1),
           dict(logits=b0), dict(logits=b0 + o_kern - 4), dict(logits=b0 + o_kern + 2 * nk - 4), dict(dtype=1, logits=b0 + o_kern + 2 * nk - 2),
           dict(best_index=b0 + 8), dict(best_value=b0 + o_kern + 2 * nk - 4), dict(workspace=b0 + 16),
           dict(workspace=b0 + 16 * ((o_kern + 2 * nk - 1) // 16)), dict(kern=b0 + o_log + 4 * total - 2), dict(scene=b0 + o_work + need - 2)]
    for kw in bad:
        rc = _raw({**good, **kw})
        assert rc == -1, (kw, rc)   # MRE_ERR_ARG
        assert _lib().mre_last_error().startswith(b"mre_correlate"), kw
        assert torch.equal(buf, snapshot), kw
    for kw in (dict(n=0), dict(n=0, logits=None), dict(n=0, best_index=None, best_value=None)):   # MRE_OK, nothing launched
        assert _raw({**good, **kw}) == 0, kw
        assert torch.equal(buf, snapshot), kw
    assert _raw(good) == 0       # and the good call writes every element it owns, and outside the workspace no other
    got = buf.cpu()
    _same(got[o_log:o_log + 4 * total].numpy().view(np.float32).reshape(logits.shape), logits, "the good call")
    assert np.array_equal(got[o_idx:o_idx + 8 * n].numpy().view(np.int64), index)
    assert np.array_equal(got[o_val:o_val + 4 * n].numpy().view(np.float32), value)
    keep = torch.ones(buf.numel(), dtype=torch.bool)
    for start, size in ((o_log, 4 * total), (o_idx, 8 * n), (o_val, 4 * n), (o_work, need)):
        keep[start:start + size] = False
    assert torch.equal(got[keep], snapshot.cpu()[keep])


def test_a_strided_view_float32_and_cpu_tensors_go_through_the_fallback():
    from mujoco_robot_environments_amd import perception as P
    shape = CC.SHAPES[3]
    scene, kern, logits, index, value = CC.reference(shape)
    wide = torch.zeros(tuple(scene.shape[:3]) + (2 * scene.shape[3],), dtype=BF16, device=DEV)
    wide[..., ::2] = scene.to(DEV)
    view = wide[..., ::2]
    assert not view.is_contiguous()
    for s, k, cuda in ((view, kern.to(DEV), True), (scene.to(DEV).float(), kern.to(DEV).float(), True),
                       (scene.to(DEV), kern.to(DEV).float(), True), (scene, kern, False)):
        got = P.correlate(s, k, logits=F32)
        assert got.logits.is_cuda == cuda and got.index.is_cuda == cuda and got.logits.dtype == F32 and got.index.dtype == torch.int64
        _same(got.logits.cpu().numpy(), logits, "fallback")
        assert np.array_equal(got.index.cpu().numpy(), index) and np.array_equal(got.value.cpu().numpy(), value)
    with pytest.raises(ValueError):
        P.correlate(scene.to(DEV), kern)   # one on the device, one not


def test_env_transporter_place_of_16_envs_after_reset():
    """One-hot scene features at the cell of each env's scripted place position and one-hot crop features at the pivot of
    rotation e % 36: transporter_place returns that cell, that rotation, and a world xy within half a cell of the place.
    The scripted place positions reach past the default map's last row (the target zone straddles y = 0.4, the map's
    edge), where no feature can be one-hot; the feature maps here are therefore the default grid continued by whole tiles
    of rows -- the same origin and the same cell -- so that every one of the 16 envs is checked."""
    from mujoco_robot_environments_amd import perception as P
    from mujoco_robot_environments_amd.tasks.rearrangement import (HEIGHTMAP_BOUNDS, BatchedRearrangementEnv,
                                                                   colour_separator_task_config)
    N, rows, cols, rot, crop, cell = 16, 320, 240, 36, 64, 0.0025
    env = BatchedRearrangementEnv(cfg=colour_separator_task_config(), num_envs=N, render=True)
    try:
        env.reset()
        place = np.asarray(env.sort_colours(peek=True)[2][:, :3], np.float64)
        cells = P.world_2_cell(place, HEIGHTMAP_BOUNDS, cell)
        rows = max(rows, 16 * (int(cells[:, 1].max()) // 16 + 1))
        assert ((cells >= 0) & (cells < [cols, rows])).all() and rows <= 400, (cells, rows)
        scene = torch.zeros((N, 1, rows, cols), dtype=BF16, device=DEV)
        crops = torch.zeros((N, rot, 1, crop, crop), dtype=BF16, device=DEV)
        e = torch.arange(N, device=DEV)
        scene[e, 0, torch.from_numpy(cells[:, 1]).to(DEV), torch.from_numpy(cells[:, 0]).to(DEV)] = 1.0
        crops[e, e % rot, 0, crop // 2, crop // 2] = 1.0
        got = env.transporter_place(scene, crops, cell=cell)
        assert got.cells.is_cuda and got.cells.dtype == torch.int64 and got.xy.dtype == torch.float64
        assert np.array_equal(got.cells.cpu().numpy(), cells)
        assert got.rotation.tolist() == [i % rot for i in range(N)]
        assert np.allclose(got.angle.cpu().numpy(), 2 * np.pi * (np.arange(N) % rot) / rot, atol=1e-12)
        assert got.value.tolist() == [1.0] * N
        assert np.abs(got.xy.cpu().numpy() - place[:, :2]).max() <= cell / 2
    finally:
        env.close()
