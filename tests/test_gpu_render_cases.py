"""GPU tests of the batched camera (csrc/mre_render.hip, mre_render) over the cases of tests/render_cases.py: every
image shape, camera and scene against the numpy oracle under the rule stated there, then the promises of the header
that the oracle has no say in -- NULL outputs, masks, guard rows, the background cache of a live handle, the two
environment knobs and the refused arguments.  Nothing here steps the physics: every state is written with set_state."""
import functools

import numpy as np
import pytest

from tests import render_cases as RC

pytestmark = pytest.mark.gpu

SENT_F, SENT_B = -7.0, 0xA5


def _handle(c):
    from mujoco_robot_environments_amd.physics import BatchedPhysics
    phys = BatchedPhysics(c.N, model=RC.model())
    phys.set_props(c.nprops, c.sizes.astype(np.float32))
    phys.reset()
    phys.set_state(c.qpos, np.zeros((c.N, 39), np.float32))
    phys.set_render_colours(c.prop_rgb, c.geom_rgb)
    return phys


def _render(phys, c, **kw):
    out = phys.render(c.cam_pos, c.cam_mat, c.fovy, c.height, c.width, **kw)
    return tuple(None if t is None else t.cpu().numpy() for t in out)


@functools.lru_cache(maxsize=None)
def _device(name):
    """(rgb, depth, seg) of a fresh handle, all outputs, no mask."""
    c = RC.case(name)
    phys = _handle(c)
    out = _render(phys, c)
    phys.close()
    return out


def _against_oracle(name, images, envs=None):
    c = RC.case(name)
    rgb, depth, seg = images
    problems, worst_d, worst_c, n, above = [], 0.0, 0, 0, 0
    for i in (range(c.N) if envs is None else envs):
        pr, st = RC.compare(name, i, rgb[i], depth[i], seg[i])
        problems += [f"env {i}: {p}" for p in pr]
        worst_d, worst_c, n, above = max(worst_d, st["depth"]), max(worst_c, st["rgb"]), n + st["n"], above + st["above1"]
    for env, v, u, g in c.probes:
        if (envs is None or env in envs) and seg[env, v, u] != g:
            problems.append(f"env {env}: probe at row {v}, column {u} shows geom {seg[env, v, u]}, not {g}")
    return problems, worst_d, worst_c, n, above


@pytest.mark.parametrize("name", RC.NAMES)
def test_device_matches_the_oracle(name):
    problems, worst_d, worst_c, n, above = _against_oracle(name, _device(name))
    print(f"{name}: worst depth error {worst_d:.2e} x max(1, d), worst rgb error {worst_c}, above 1 on {above} of {n} pixels "
          f"({100.0 * above / max(n, 1):.4f} %)")
    assert not problems, "\n".join(problems)


def test_rgb_is_within_one_on_all_but_a_ten_thousandth_of_the_pixels():
    n = above = 0
    for name in RC.NAMES:
        _, _, _, k, a = _against_oracle(name, _device(name))
        n, above = n + k, above + a
    print(f"pooled over {len(RC.NAMES)} cases: rgb error above 1 on {above} of {n} pixels ({100.0 * above / n:.5f} %)")
    assert 1.0 - above / n >= RC.RGB_POOLED_SHARE


# ------------------------------------------------------------------ outputs, guards, masks (the C ABI, raw pointers)
class _Guarded:
    """The three image buffers of a case with two guard rows before and after each, everything filled with a sentinel."""

    def __init__(self, phys, c):
        import torch
        self.c, n, H, W = c, c.N, c.height, c.width
        self.g = 2 * W                              # guard: two rows (a multiple of 4 pixels, so alignment is kept)
        px = n * H * W
        self.depth = torch.full((px + 2 * self.g,), SENT_F, dtype=torch.float32, device=phys.device)
        self.rgb = torch.full(((px + 2 * self.g) * 3,), SENT_B, dtype=torch.uint8, device=phys.device)
        self.seg = torch.full((px + 2 * self.g,), SENT_B, dtype=torch.uint8, device=phys.device)

    def ptrs(self, rgb=True, depth=True, seg=True):
        return (self.rgb.data_ptr() + 3 * self.g if rgb else None, self.depth.data_ptr() + 4 * self.g if depth else None,
                self.seg.data_ptr() + self.g if seg else None)

    def read(self):
        """-> (rgb, depth, seg) images, and whether every guard element still holds the sentinel."""
        c, g = self.c, self.g
        r, d, s = self.rgb.cpu().numpy(), self.depth.cpu().numpy(), self.seg.cpu().numpy()
        intact = ((r[:3 * g] == SENT_B).all() and (r[-3 * g:] == SENT_B).all() and (d[:g] == SENT_F).all() and (d[-g:] == SENT_F).all()
                  and (s[:g] == SENT_B).all() and (s[-g:] == SENT_B).all())
        return (r[3 * g:-3 * g].reshape(c.N, c.height, c.width, 3), d[g:-g].reshape(c.N, c.height, c.width),
                s[g:-g].reshape(c.N, c.height, c.width)), bool(intact)

    def untouched(self):
        return bool((self.rgb == SENT_B).all() and (self.depth == SENT_F).all() and (self.seg == SENT_B).all())


def _raw(phys, c, ptrs, mask=None, fovy=None, height=None, width=None):
    from mujoco_robot_environments_amd import lib as L
    from mujoco_robot_environments_amd.physics import _ptr
    cp = np.ascontiguousarray(c.cam_pos, np.float32)
    cm = np.ascontiguousarray(c.cam_mat, np.float32).reshape(9)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    rc = L.lib().mre_render(phys._h, _ptr(cp), _ptr(cm), c.fovy if fovy is None else fovy, c.height if height is None else height,
                            c.width if width is None else width, ptrs[0], ptrs[1], ptrs[2], _ptr(m))
    phys.sync()
    return rc


@pytest.mark.parametrize("name", ["A-4x5-cubes", "A-776x4-cubes", "A-64x21-cubes", "C-tumbling-side"])
def test_single_outputs_guards_and_masks(name):
    c = RC.case(name)
    phys = _handle(c)
    full = _Guarded(phys, c)
    assert _raw(phys, c, full.ptrs()) == 0
    ref, intact = full.read()
    assert intact, "a guard row was written by the three-output call"
    for k, want in enumerate(_device(name)):
        assert np.array_equal(ref[k], want)
    for k, only in enumerate(("rgb", "depth", "seg")):
        buf = _Guarded(phys, c)
        assert _raw(phys, c, buf.ptrs(**{o: o == only for o in ("rgb", "depth", "seg")})) == 0
        got, intact = buf.read()
        assert intact, f"a guard row was written by the {only}-only call"
        assert np.array_equal(got[k], ref[k]), f"{only}-only differs from the three-output call"
        for j in range(3):
            if j != k:
                assert (got[j] == (SENT_F if j == 1 else SENT_B)).all(), f"{only}-only wrote another output"
    mask = np.zeros(c.N, np.uint8)
    mask[c.N - 1] = 1                                  # only the last env is drawn
    buf = _Guarded(phys, c)
    assert _raw(phys, c, buf.ptrs(), mask=mask) == 0
    got, intact = buf.read()
    assert intact
    for k in range(3):
        assert np.array_equal(got[k][c.N - 1], ref[k][c.N - 1])
        assert (got[k][:c.N - 1] == (SENT_F if k == 1 else SENT_B)).all(), "a masked-out env's image was written"
    phys.close()


# ------------------------------------------------------------------ background cache of one live handle
def test_background_cache_follows_camera_shape_and_colours():
    """One handle renders D_STEPS in turn (camera A, B, A again, another fovy, another H x W, other geom colours): every
    result equals a fresh handle's bit for bit, which test_device_matches_the_oracle holds against the oracle."""
    first = RC.case("D-cache-top")
    phys = _handle(first)
    for step in RC.D_STEPS:
        c = RC.case(f"D-cache-{step}")
        assert np.array_equal(c.qpos, first.qpos) and np.array_equal(c.prop_rgb, first.prop_rgb)
        if step == "recoloured":
            phys.set_render_colours(geom_rgb=c.geom_rgb)
        got = _render(phys, c)
        for k, want in enumerate(_device(c.name)):
            assert np.array_equal(got[k], want), (step, ("rgb", "depth", "seg")[k])
        problems = _against_oracle(c.name, got)[0]
        assert not problems, "\n".join(problems)
    phys.close()


@pytest.mark.parametrize("name", ["D-cache-side", "A-776x4-cubes"])
def test_first_render_with_env_0_masked_out(name):
    """The background is cast from env 0's geoms: a handle whose FIRST render masks env 0 out must export them all the same."""
    c = RC.case(name)
    phys = _handle(c)
    mask = np.ones(c.N, np.uint8)
    mask[0] = 0
    buf = _Guarded(phys, c)
    assert _raw(phys, c, buf.ptrs(), mask=mask) == 0
    got, intact = buf.read()
    assert intact
    for k, want in enumerate(_device(name)):
        assert np.array_equal(got[k][1:], want[1:]), ("rgb", "depth", "seg")[k]
        assert (got[k][0] == (SENT_F if k == 1 else SENT_B)).all()
    problems = _against_oracle(name, got, envs=range(1, c.N))[0]
    assert not problems, "\n".join(problems)
    phys.close()


# ------------------------------------------------------------------ knobs
KNOBS = [("MRE_RENDER_NO_BACKGROUND", "1"), ("MRE_RENDER_ROW_GROUPS", "1"), ("MRE_RENDER_ROW_GROUPS", "3"), ("MRE_RENDER_ROW_GROUPS", "64")]


@pytest.mark.parametrize("var,value", KNOBS)
def test_knobs_do_not_change_a_bit(var, value, monkeypatch):
    """mre_render reads both variables at every call.  Compositing over the cached background visits the geoms in the
    same order with the same arithmetic as casting them all, and the row groups only split the rows between workgroups."""
    for name in ("A-32x41-cubes", "A-800x8-hull", "B-side-120x160", "B-near-48x64", "C-tumbling-top"):
        want = _device(name)             # rendered before the variable is set
        c = RC.case(name)
        phys = _handle(c)
        monkeypatch.setenv(var, value)
        got = _render(phys, c)
        monkeypatch.delenv(var)
        phys.close()
        for k in range(3):
            assert np.array_equal(got[k], want[k]), (name, var, value, ("rgb", "depth", "seg")[k])


# ------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_and_nothing_is_written():
    from mujoco_robot_environments_amd import lib as L
    c = RC.case("C-tumbling-top")
    phys = _handle(c)
    buf = _Guarded(phys, c)
    ok = buf.ptrs()
    host = np.full(c.N * c.height * c.width * 3, SENT_B, np.uint8)
    ERR = -1                                                         # MRE_ERR_ARG (include/mre.h)
    refused = {
        "width 6": dict(ptrs=ok, width=6), "width 1284": dict(ptrs=ok, width=1284), "width 0": dict(ptrs=ok, width=0),
        "height 0": dict(ptrs=ok, height=0), "fovy 0": dict(ptrs=ok, fovy=0.0), "fovy 180": dict(ptrs=ok, fovy=180.0),
        "host rgb": dict(ptrs=(host.ctypes.data, ok[1], ok[2])),
        "depth + 4 bytes": dict(ptrs=(ok[0], ok[1] + 4, ok[2])),
        "rgb + 1 byte": dict(ptrs=(ok[0] + 1, ok[1], ok[2])),
    }
    for what, kw in refused.items():
        assert _raw(phys, c, **kw) == ERR, what
        assert L.lib().mre_last_error()
        assert buf.untouched() and (host == SENT_B).all(), what
    assert _raw(phys, c, ok) == 0                                    # the handle still renders
    got, intact = buf.read()
    assert intact and all(np.array_equal(got[k], _device(c.name)[k]) for k in range(3))
    phys.close()
