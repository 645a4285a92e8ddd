"""GPU tests of the pick head (csrc/mre_attend.hip; include/mre.h, mre_attend and mre_attend_dlogits) against the statements
of tests/attend_cases.py, which tests/test_attend.py checks against plain loops.  The shapes (n, K, h, w) are those of
tests/attend_cases.py, named there against the kernel's lane vector, chunk and largest split; both dtypes.

The decision takes integer logits in -4 .. 4 (-1 .. 1 for the smallest envs), exact in both dtypes and full of ties, and is
compared with numpy's first-occurrence argmax EXACTLY.  The loss and g take the same logits, so the float64 softmax is exact
in its inputs, and are held to
    |lse - lse64| <= 2^-15 + 2^-22 |lse64|        (the same for loss; mre_correlate_loss's bound for the same accumulator)
    |g - g64|     <= 2^-8  |g64| + 2^-22 |weight|   bfloat16 (mre_correlate_dlogits' bound)
    |g - g64|     <= 2^-13 |g64| + 2^-22 |weight|   float32: lse's bound enters g as a relative error of at most
                     2^-15 + 2^-22 * 15.3 ~ 2^-14.8 at these inputs; the 3.5 x left over covers the rounding of l - lse and
                     of exp2.
The worst fraction of each bound that the kernel reaches over the cases here is printed by the tests and recorded in
DESIGN.md 8f.10.

Every call of the C ABI here reads its logits from between NaN guards at element offsets 0 and 1 and writes into
sentinel-filled buffers, the workspace too; no sentinel outside an output may change.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import attend_cases as AC

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT32 = -0x21524111   # the bits 0xDEADBEEF
PAD = 64               # elements of guard before the data: a multiple of 16 bytes, so offset 0 is 16-byte aligned
DTYPES = [torch.bfloat16, torch.float32]
CODE = {torch.float32: 0, torch.bfloat16: 1}
BITS = {torch.float32: (torch.int32, 0x7FC00000, SENT32), torch.bfloat16: (torch.int16, 0x7FC0, -0x2153)}   # view, NaN guard, sentinel
SHAPES, IDS = AC.SHAPES, AC.IDS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from mujoco_robot_environments_amd import lib as L
    return L.lib()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(t, off):
    """A CPU tensor on the device between NaN guards, `off` elements past a 16-byte boundary: (buffer, start)."""
    view, guard, _ = BITS[t.dtype]
    flat = t.contiguous().view(view).reshape(-1)
    buf = torch.full((flat.numel() + 2 * PAD + 1,), guard, dtype=view, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[PAD + off: PAD + off + flat.numel()] = flat.to(DEV)
    return buf, PAD + off


def _guards_intact(pair, t, what):
    buf, start = pair
    view, guard, _ = BITS[t.dtype]
    assert bool((buf[:start] == guard).all()) and bool((buf[start + t.numel():] == guard).all()), what
    assert torch.equal(buf[start:start + t.numel()].cpu(), t.contiguous().view(view).reshape(-1)), what


def _attend(logits, target=None, best=True, in_off=0):
    """mre_attend on a CPU tensor [n, K, h, w]: dict of numpy arrays index, value, lse, target_logit, loss (those asked for)."""
    n, k, h, w = logits.shape
    what = (tuple(logits.shape), logits.dtype, in_off, best, None if target is None else list(target)[:3])
    need = C.c_size_t(0)
    assert _lib().mre_attend_workspace(n, k, h, w, C.byref(need)) == 0
    assert need.value == n * AC.split(k * h * w) * 16
    x = _guarded(logits, in_off)
    t = None if target is None else torch.tensor(list(target), dtype=torch.int64, device=DEV)
    ibuf = torch.full((n + 2,), SENT32, dtype=torch.int64, device=DEV)
    obuf = torch.full((4, n + 2), SENT32, dtype=torch.int32, device=DEV)
    wbuf = torch.full((need.value // 4 + 8,), SENT32, dtype=torch.int32, device=DEV)
    assert wbuf.data_ptr() % 16 == 0
    on = lambda k_, yes: obuf[k_, 1:].data_ptr() if yes else None
    rc = _lib().mre_attend(_stream(), x[0][x[1]:].data_ptr(), n, k, h, w, CODE[logits.dtype], None if t is None else t.data_ptr(),
                           ibuf[1:].data_ptr() if best else None, on(0, best), on(1, t is not None), on(2, t is not None),
                           on(3, t is not None), wbuf.data_ptr(), need.value)
    torch.cuda.synchronize()
    assert rc == 0, what + (rc, _lib().mre_last_error())
    got, idx = obuf.cpu().numpy(), ibuf.cpu().numpy()
    assert (got[:, 0] == SENT32).all() and (got[:, -1] == SENT32).all() and idx[0] == SENT32 and idx[-1] == SENT32, what
    written = [best, t is not None, t is not None, t is not None]
    for row, yes in enumerate(written):   # no element of what was asked for keeps the sentinel; what was not is untouched
        assert ((got[row, 1:-1] == SENT32).all() if not yes else not (got[row, 1:-1] == SENT32).any()), what + (row,)
    assert ((idx[1:-1] == SENT32).all() if not best else not (idx[1:-1] == SENT32).any()), what
    assert bool((wbuf[need.value // 4:] == SENT32).all()), what
    _guards_intact(x, logits, what)
    if t is not None:
        assert t.cpu().tolist() == [int(v) for v in target]
    names = ("value", "lse", "target_logit", "loss")
    out = {name: got[row, 1:-1].copy().view(np.float32) for row, name in enumerate(names) if written[row]}
    if best:
        out["index"] = idx[1:-1].copy()
    return out


def _dlogits(logits, target, lse, weight, in_off=0, out_off=0):
    """mre_attend_dlogits on a CPU tensor: g as float64 numpy [n, K, h, w] (the stored values, exactly)."""
    n, k, h, w = logits.shape
    what = (tuple(logits.shape), logits.dtype, in_off, out_off, list(target)[:3])
    view, _, sent = BITS[logits.dtype]
    x = _guarded(logits, in_off)
    t = torch.tensor(list(target), dtype=torch.int64, device=DEV)
    ls = torch.from_numpy(np.asarray(lse, np.float32)).to(DEV)
    wg = None if weight is None else torch.from_numpy(np.asarray(weight, np.float32)).to(DEV)
    total = logits.numel()
    gbuf = torch.full((total + 16,), sent, dtype=view, device=DEV)
    assert gbuf.data_ptr() % 16 == 0
    rc = _lib().mre_attend_dlogits(_stream(), x[0][x[1]:].data_ptr(), n, k, h, w, CODE[logits.dtype], t.data_ptr(), ls.data_ptr(),
                                   None if wg is None else wg.data_ptr(), gbuf[out_off:].data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, what + (rc, _lib().mre_last_error())
    rest = torch.cat([gbuf[:out_off], gbuf[out_off + total:]])
    assert bool((rest == sent).all()), what
    _guards_intact(x, logits, what)
    return gbuf[out_off:out_off + total].view(logits.dtype).to(torch.float64).cpu().numpy().reshape(n, k, h, w)


# ------------------------------------------------------------------------------------------------ the decision
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_decision_is_the_first_occurrence_of_the_maximum(shape, dtype):
    n, k, h, w = shape
    cells = k * h * w
    logits = AC.integer_logits(shape)
    want_i, want_v = AC.first_argmax(logits)
    for in_off in (0, 1):
        got = _attend(AC.as_tensor(logits, dtype), None, True, in_off)
        assert np.array_equal(got["index"], want_i) and np.array_equal(got["value"], want_v), (shape, in_off)
    # a unique maximum at every cell where a lane, a wave or a split begins or ends: one env per cell
    at = AC.peak_cells(shape)
    peaks = np.repeat(logits[:1], len(at), axis=0).reshape(len(at), cells).copy()
    peaks[np.arange(len(at)), at] = 5.0
    for in_off in (0, 1):
        got = _attend(AC.as_tensor(peaks.reshape((len(at), k, h, w)), dtype), None, True, in_off)
        assert got["index"].tolist() == at and (got["value"] == 5.0).all(), (shape, in_off)
    # -inf everywhere but one cell: that cell, wherever it is
    alone = np.full((len(at), cells), -np.inf, np.float32)
    alone[np.arange(len(at)), at] = -3.0
    got = _attend(AC.as_tensor(alone.reshape((len(at), k, h, w)), dtype), [0] * len(at))
    assert got["index"].tolist() == at and (got["value"] == -3.0).all() and (got["lse"] == -3.0).all(), shape
    assert np.array_equal(got["loss"] == 0.0, np.array(at) == 0) and np.array_equal(got["loss"] == np.inf, np.array(at) != 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_an_all_masked_env_leaves_its_neighbours_untouched(dtype):
    shape = SHAPES[2]
    logits = AC.integer_logits(shape).copy()
    target = [5, 6, 7]
    weight = np.array([1.5, 2.0, 0.5], np.float32)
    before = _attend(AC.as_tensor(logits, dtype), target)
    g_before = _dlogits(AC.as_tensor(logits, dtype), target, before["lse"], weight)
    logits[1] = -np.inf
    got = _attend(AC.as_tensor(logits, dtype), target)
    assert got["index"][1] == 0 and got["value"][1] == -np.inf and got["lse"][1] == -np.inf and np.isnan(got["loss"][1])
    for name in before:
        assert np.array_equal(got[name][[0, 2]].view(np.uint32 if name != "index" else np.int64),
                              before[name][[0, 2]].view(np.uint32 if name != "index" else np.int64)), name
    g = _dlogits(AC.as_tensor(logits, dtype), target, got["lse"], weight)
    assert not g[1].any() and np.array_equal(g[[0, 2]], g_before[[0, 2]])


# ------------------------------------------------------------------------------------------------ loss and g
WORST = {}


def _bounds(dtype, lse64, g64, weight, n):
    wabs = np.ones(n) if weight is None else np.abs(weight.astype(np.float64))
    rel = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -13
    return 2.0 ** -15 + 2.0 ** -22 * np.abs(lse64), rel * np.abs(g64) + 2.0 ** -22 * wabs[:, None, None, None]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("shape", SHAPES[1:], ids=IDS[1:])
def test_the_loss_and_its_gradient_against_the_float64_softmax(shape, masked, dtype):
    n, k, h, w = shape
    cells = k * h * w
    logits = AC.integer_logits(shape, masked)
    x = AC.as_tensor(logits, dtype)
    worst = WORST.setdefault(dtype, {"lse": 0.0, "loss": 0.0, "g": 0.0})
    for name, target in AC.targets(shape).items():
        inside = 0 <= target[0] < cells
        weight = None if name == "first" else np.array([1.5, 0.25, 3.0][:n], np.float32)
        lse64, loss64, g64 = AC.softmax64(logits, target, weight)
        # (on the reference alone) no probability is so large that its error would hide in the bound's first term
        assert np.exp(logits.reshape(n, -1).astype(np.float64) - lse64[:, None]).max() < 0.25, shape
        for in_off in (0, 1):
            got = _attend(x, target, False, in_off)
            what = (shape, masked, name, in_off)
            bound, _ = _bounds(dtype, lse64, g64, weight, n)
            worst["lse"] = max(worst["lse"], (np.abs(got["lse"] - lse64) / bound).max())
            assert (np.abs(got["lse"] - lse64) <= bound).all(), what + (got["lse"], lse64)
            if inside:
                assert np.array_equal(got["target_logit"], logits.reshape(n, -1)[np.arange(n), target]), what   # exact
                finite = np.isfinite(loss64)   # (a masked target cell: the loss is +inf, exactly)
                assert np.array_equal(got["loss"][~finite], loss64[~finite].astype(np.float32)), what
                err = np.abs(got["loss"][finite] - loss64[finite])
                worst["loss"] = max([worst["loss"]] + (err / bound[finite]).tolist())
                assert (err <= bound[finite]).all(), what + (got["loss"], loss64)
            else:
                assert np.isnan(got["target_logit"]).all() and np.isnan(got["loss"]).all(), what
            for out_off in ((0, 1, 3) if in_off == 0 else (0,)):
                g = _dlogits(x, target, got["lse"], weight, in_off, out_off)
                _, gbound = _bounds(dtype, lse64, g64, weight, n)
                worst["g"] = max(worst["g"], (np.abs(g - g64) / gbound).max())
                assert (np.abs(g - g64) <= gbound).all(), what + (out_off, float((np.abs(g - g64) / gbound).max()))
                masked_cells = np.isinf(logits).reshape(n, -1).copy()   # a masked cell gets exactly 0 (the target apart)
                if inside:
                    masked_cells[np.arange(n), target] = False
                assert not g.reshape(n, -1)[masked_cells].any(), what
                if not inside:   # the weighted softmax alone: nothing is subtracted anywhere
                    assert (g[np.isfinite(logits)] > 0).all(), what
    print(shape, masked, dtype, "worst error / bound so far", worst)
    # weight 0: g is all zeros
    target = AC.targets(shape)["last"]
    lse = _attend(x, target, False)["lse"]
    assert not _dlogits(x, target, lse, np.zeros(n, np.float32)).any(), shape


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_one_cell_has_no_loss_and_no_gradient(dtype):
    x = AC.as_tensor(np.array([[[[3.0]]]], np.float32), dtype)
    for in_off in (0, 1):
        got = _attend(x, [0], True, in_off)
        assert got["index"].tolist() == [0] and got["value"].tolist() == [3.0] and got["lse"].tolist() == [3.0]
        assert got["target_logit"].tolist() == [3.0] and got["loss"].tolist() == [0.0]
        assert _dlogits(x, [0], got["lse"], None, in_off, in_off).tolist() == [[[[0.0]]]]
    got = _attend(x, [1])
    assert np.isnan(got["loss"]).all() and _dlogits(x, [1], got["lse"], np.array([2.0], np.float32)).tolist() == [[[[2.0]]]]


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[5], SHAPES[8]], ids=[IDS[2], IDS[5], IDS[8]])
def test_the_bytes_repeat_and_do_not_depend_on_the_batch_or_on_what_else_is_asked(shape, dtype):
    from mujoco_robot_environments_amd import perception as P
    n, k, h, w = shape
    rng = np.random.default_rng(9)
    x = torch.from_numpy(rng.standard_normal((3, k, h, w)).astype(np.float32)).to(dtype).to(DEV)
    target = torch.tensor([1, k * h * w - 1, 17 % (k * h * w)], device=DEV)
    bits = lambda t: t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16 if t.dtype == torch.bfloat16 else t.dtype)
    a, b = P.attend(x, target), P.attend(x, target)
    for u, v in zip(a, b):   # a second call gives the same bytes
        assert u.is_cuda and torch.equal(bits(u), bits(v))
    ga, gb = P.attend_dlogits(x, target, a.lse), P.attend_dlogits(x, target, a.lse)
    assert ga.dtype == dtype and ga.shape == x.shape and torch.equal(bits(ga), bits(gb))
    # the decision alone, the loss alone and both together agree on what they share
    only_best, only_loss = P.attend(x), P.attend(x, target, best=False)
    assert only_best.lse is None and only_loss.index is None and only_loss.value is None
    assert torch.equal(only_best.index, a.index) and torch.equal(bits(only_best.value), bits(a.value))
    for name in ("lse", "target_logit", "loss"):
        assert torch.equal(bits(getattr(only_loss, name)), bits(getattr(a, name))), name
    # env 0 alone and env 0 as the last of three give the same bytes (its address and alignment differ too where the
    # env's byte length is no multiple of 16)
    three_x, three_t = torch.cat([x[-1:], x[-1:], x[:1]]).contiguous(), torch.cat([target[-1:], target[-1:], target[:1]])
    alone, last = P.attend(x[:1].contiguous(), target[:1]), P.attend(three_x, three_t)
    for u, v in zip(alone, last):
        assert torch.equal(bits(u[0]), bits(v[2]))
    g1 = P.attend_dlogits(x[:1].contiguous(), target[:1], alone.lse)
    g3 = P.attend_dlogits(three_x, three_t, last.lse)
    assert torch.equal(bits(g1[0]), bits(g3[2]))


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_pick_loss_backward_against_the_float64_statement(dtype):
    from mujoco_robot_environments_amd import perception as P
    n, k, h, w = AC.END_TO_END
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((n, k, h, w)).astype(np.float32)).to(dtype)
    target = np.array([5 * w + 9, (h - 2) * w + w - 3], np.int64)
    weight = np.array([1.0, 2.5], np.float32)
    lse64, loss64, g64 = AC.softmax64(x.to(torch.float64).numpy(), target, weight)
    xd = x.to(DEV).requires_grad_(True)
    loss = P.pick_loss(xd, torch.from_numpy(target).to(DEV), torch.from_numpy(weight).to(DEV))
    assert loss.is_cuda and loss.dtype == torch.float32 and loss.shape == (n,)
    bound, gbound = _bounds(dtype, lse64, g64, weight, n)
    assert (np.abs(loss.detach().cpu().numpy() - weight * loss64) <= weight * bound).all()
    loss.sum().backward()
    assert xd.grad.dtype == dtype and xd.grad.shape == xd.shape
    ratio = np.abs(xd.grad.to(torch.float64).cpu().numpy() - g64) / gbound
    print(dtype, "worst error / bound of the gradient", ratio.max())
    assert (ratio <= 1.0).all(), float(ratio.max())
    # an incoming gradient scales the weight
    xd.grad = None
    (3.0 * P.pick_loss(xd, torch.from_numpy(target).to(DEV), torch.from_numpy(weight).to(DEV))).sum().backward()
    ratio = np.abs(xd.grad.to(torch.float64).cpu().numpy() - 3.0 * g64) / (3.0 * gbound)
    assert (ratio <= 1.0).all(), float(ratio.max())


def test_crops_at_device_cells_equal_crops_at_host_cells():
    from mujoco_robot_environments_amd import perception as P
    rng = np.random.default_rng(3)
    cells = np.concatenate([[[0, 0], [239, 0], [0, 319], [239, 319], [-5, 7], [250, 400]],
                            rng.integers(-64, 400, size=(26, 2))]).astype(np.int64)
    for rot, crop in ((36, 64), (8, 10)):
        want_m, want_i = P.crop_matrices(cells, rot, crop)
        mats, index = P.crop_matrices_device(torch.from_numpy(cells).to(DEV), rot, crop)
        assert mats.is_cuda and mats.dtype == torch.float32 and index.dtype == torch.int32
        assert np.array_equal(mats.cpu().numpy().view(np.uint32), want_m.view(np.uint32))
        assert np.array_equal(index.cpu().numpy(), want_i)


def test_cpu_strided_and_other_dtypes_take_the_reference_path():
    from mujoco_robot_environments_amd import perception as P
    shape = SHAPES[3]
    n, k, h, w = shape
    logits = AC.integer_logits(shape)
    target = torch.tensor([3, 40])
    x = AC.as_tensor(logits, torch.float32)
    want = P.attend_reference(x, target)
    cpu = P.attend(x, target)
    assert not cpu.index.is_cuda and torch.equal(cpu.index, want.index) and torch.equal(cpu.loss, want.loss)
    dev = P.attend(x.to(DEV), target.to(DEV))   # the kernel agrees: integers
    assert torch.equal(dev.index.cpu(), want.index) and torch.allclose(dev.loss.cpu(), want.loss, rtol=0, atol=2.0 ** -14)
    strided = x.to(DEV).transpose(2, 3).contiguous().transpose(2, 3)
    assert not strided.is_contiguous()
    for other in (strided, x.to(DEV).to(torch.float64), x.to(DEV).to(torch.float16)):
        got = P.attend(other, target.to(DEV))
        assert got.index.is_cuda and torch.equal(got.index.cpu(), want.index)
        assert torch.allclose(got.loss.cpu(), want.loss, rtol=1e-5, atol=1e-5)
        leaf = other.detach().requires_grad_(True)   # differentiable by torch itself
        P.pick_loss(leaf, target.to(DEV)).sum().backward()
        assert leaf.grad is not None and leaf.grad.shape == leaf.shape and bool(leaf.grad.abs().sum() > 0)


# ------------------------------------------------------------------------------------------------ the env
@pytest.fixture(scope="module")
def env():
    from mujoco_robot_environments_amd.tasks.rearrangement import BatchedRearrangementEnv, colour_separator_task_config
    e = BatchedRearrangementEnv(cfg=colour_separator_task_config(), num_envs=16, render=True)
    try:
        e.reset()
        yield e
    finally:
        e.close()


def _demo_cells(env, P, cell=0.0025):
    from mujoco_robot_environments_amd.tasks.rearrangement import HEIGHTMAP_BOUNDS
    _, pick, place = env.sort_colours(peek=True)
    return P.world_2_cell(pick[:, :3], HEIGHTMAP_BOUNDS, cell), pick


def _one_hot(cells, rows, cols, dtype=torch.bfloat16):
    n = len(cells)
    assert (cells >= 0).all() and (cells[:, 0] < cols).all() and (cells[:, 1] < rows).all(), cells
    x = torch.zeros((n, 1, rows, cols), dtype=dtype, device=DEV)
    x[torch.arange(n), 0, torch.as_tensor(cells[:, 1]), torch.as_tensor(cells[:, 0])] = 1.0
    return x


def test_transporter_pick_and_its_loss_of_an_env_batch(env):
    from mujoco_robot_environments_amd import perception as P
    from mujoco_robot_environments_amd.tasks.rearrangement import HEIGHTMAP_BOUNDS, PickDecision
    batch = env.transporter_batch(seed=11, n_rotations=4, crop=8)
    n, rows, cols = 16, int(batch.scene.shape[2]), int(batch.scene.shape[3])
    inside = lambda c: (c[:, 0] >= 0) & (c[:, 0] < cols) & (c[:, 1] >= 0) & (c[:, 1] < rows)
    pick = np.asarray(batch.pick).copy()
    pick[0], pick[5] = (-1, 3), (2, rows)   # two envs without a label, whatever the motion did: a pick cell outside the map
    batch = batch._replace(pick=pick)
    ok = inside(pick)
    assert ok.any() and not ok[0] and not ok[5]
    at = pick.copy()
    at[~ok] = 0
    decision = env.transporter_pick(_one_hot(at, rows, cols))
    assert isinstance(decision, PickDecision) and all(t.is_cuda for t in decision)
    assert np.array_equal(decision.cells.cpu().numpy(), at) and not decision.bins.any() and not decision.angles.any()
    assert np.array_equal(decision.xy.cpu().numpy(), P.cell_2_world(at, HEIGHTMAP_BOUNDS, 0.0025))
    assert (decision.value == 1.0).all()
    # the loss: log(E - 1 + e) - 1 for a one-hot at the target, less than for a one-hot elsewhere, NaN without a label
    logits = _one_hot(at, rows, cols).requires_grad_(True)
    loss = env.transporter_pick_loss(logits, batch)
    okt = torch.from_numpy(ok)
    assert loss.shape == (n,) and loss.dtype == torch.float32 and bool(torch.isnan(loss[~okt]).all())
    cells = rows * cols
    assert torch.allclose(loss[okt].detach().cpu(), torch.full((int(ok.sum()),), float(np.log(cells - 1 + np.e) - 1.0)), rtol=0, atol=2.0 ** -14)
    other = at.copy()
    other[:, 0] = (other[:, 0] + 5) % cols
    elsewhere = env.transporter_pick_loss(_one_hot(other, rows, cols), batch)
    assert bool((loss[okt] < elsewhere[okt]).all())
    # an env without a label: alone its gradient is the softmax (nothing subtracted); the caller's weight 0 makes it zero
    bare = _one_hot(at, rows, cols).requires_grad_(True)
    env.transporter_pick_loss(bare, batch).backward(torch.from_numpy((~ok).astype(np.float32)).to(DEV))   # (no sum: the losses are NaN)
    gb = bare.grad.to(torch.float32).cpu().numpy()
    assert (gb[~ok] > 0).all() and np.allclose(gb[~ok].sum(axis=(1, 2, 3)), 1.0, atol=2.0 ** -6) and not gb[ok].any()
    weight = torch.from_numpy(ok.astype(np.float32)).to(DEV)
    env.transporter_pick_loss(logits, batch, weight).backward(torch.ones(n, device=DEV))
    g = logits.grad.to(torch.float32).cpu().numpy()
    assert np.isfinite(g).all() and not g[~ok].any() and (np.abs(g[ok]).sum(axis=(1, 2, 3)) > 0).all()
    for e in np.flatnonzero(ok):
        assert g[e, 0].argmin() == at[e, 1] * cols + at[e, 0] and g[e, 0].min() < -0.9


def test_transporter_act_with_stand_in_networks(env):
    from mujoco_robot_environments_amd import perception as P
    from mujoco_robot_environments_amd.tasks.rearrangement import home_quat
    rot, crop = 4, 16
    cells, pick_world = _demo_cells(env, P)
    seen = {}

    def attention(scene):
        seen["scene"] = scene
        return _one_hot(cells, int(scene.shape[2]), int(scene.shape[3]))

    def query(crops):
        seen["crops"] = crops
        return crops[:, 3:4].contiguous()

    channels = P.CHANNELS_RGBH
    rgb, depth, seg = env.render()
    pick_pose, place_pose, pick, place = env.transporter_act(attention, query, lambda scene: scene[:, 3:4].contiguous(), channels=channels,
                                                             dtype=torch.bfloat16, n_rotations=rot, crop=crop, depth=depth,
                                                             rgb=rgb, seg=seg)
    n = env.num_envs
    assert pick_pose.shape == place_pose.shape == (n, 7) and pick_pose.dtype == np.float64
    assert np.array_equal(pick.cells.cpu().numpy(), cells)
    # the demonstrator's pick position, to the cell: the centre of the cell it lies in
    assert np.abs(pick_pose[:, :2] - pick_world[:, :2]).max() <= 0.0025 / 2 + 1e-6
    assert np.array_equal(pick_pose[:, 3:], np.tile(home_quat(), (n, 1)))
    assert np.allclose(np.linalg.norm(place_pose[:, 3:], axis=1), 1.0) and all(t.is_cuda for t in place)
    # the crops are those of transporter_batch's lines on unperturbed maps: crop_matrices on the host, bit for bit
    maps = env.heightmap(depth, rgb, seg)
    identity = np.tile(np.array([1, 0, 0, 0, 1, 0], np.float32), (n, 1))
    warped = P.warp_maps(maps.height, maps.colour, mats=identity, with_source=False)
    mats, index = P.crop_matrices(cells, rot, crop)
    want = P.warp_inputs(warped.height, warped.colour, mats=mats, index=index, out_shape=(crop, crop), channels=channels,
                         dtype=torch.bfloat16)
    assert seen["crops"].shape == (n * rot, 4, crop, crop) and torch.equal(seen["crops"].view(torch.int16), want.view(torch.int16))
    assert torch.equal(seen["scene"].view(torch.int16),
                       P.warp_inputs(maps.height, maps.colour, mats=identity, channels=channels, dtype=torch.bfloat16).view(torch.int16))
    # the place decision is transporter_place's on the same features, and its position is what place_pose carries
    rows, cols = int(seen["scene"].shape[2]), int(seen["scene"].shape[3])
    again = env.transporter_place(seen["scene"][:, 3:4].contiguous(), seen["crops"][:, 3:4].reshape(n, rot, 1, crop, crop).contiguous())
    assert torch.equal(again.cells, place.cells) and torch.equal(again.rotation, place.rotation)
    assert np.array_equal(place_pose[:, :2], place.xy.cpu().numpy())
    # step() takes the poses, twice
    env.step({"pose": pick_pose})
    env.step({"pose": place_pose})
    assert env.mode == "pick"


def test_the_rollout_example_runs_at_16_envs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "transporter_rollout.py"), "--num-envs", "16"],
                         cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "converged" in out.stdout, out.stdout
