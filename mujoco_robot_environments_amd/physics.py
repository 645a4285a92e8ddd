"""BatchedPhysics: host-side mirror of the ``dm_control.mjcf.Physics`` members the
reference's hot path touches, batched over ``num_envs``
environments and backed by the HIP kernels through the C ABI (include/mre.h).

reference member                       -> this class
  physics.step() (robot_arm.py:79)     -> step(nsubsteps)
  physics.set_control(u) (:78)         -> set_control(u[N,8])
  physics.reset() (rearrangement.py:302) + arm.set_joint_angles(home) -> reset(mask)
  physics.bind(joints).qpos/.qvel      -> qpos() / qvel() / set_state()
  physics.data.site_xpos[pinch]        -> sites()
PyTorch is used only to own device memory handed across the boundary.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as _lib
from .lib import MRE_NQ, MRE_NQ_PAD, MRE_NU, MRE_NV, MRE_NV_PAD, MRE_MAX_PROPS, MRE_TRACE_W, check
from .model import compile as _compile

FLAG_NO_CONSTRAINTS = 1
FLAG_FREEZE_ROBOT = 2


def _ptr(t) -> Optional[int]:
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        assert t.is_contiguous()
        return t.data_ptr()
    if isinstance(t, np.ndarray):
        assert t.flags["C_CONTIGUOUS"]
        return t.ctypes.data
    raise TypeError(type(t))


class BatchedPhysics:
    SOLVERS = {"PGS": 0, "Newton": 2}  # mjtSolver values (include/mre.h)

    def __init__(self, num_envs: int, scene: Optional[dict] = None, device: int = 0,
                 model: Optional[dict] = None, solver: Optional[str] = None):
        self.model = model if model is not None else _compile.compile_scene(scene)
        if solver is not None:  # override the model's opt_solver ("PGS" / "Newton")
            self.model = dict(self.model)
            self.model["opt_solver"] = np.array([self.SOLVERS[solver]], np.int32)
        self.blob = _compile.to_blob(self.model)
        self.num_envs = int(num_envs)
        self.device_id = int(device)
        self.device = torch.device("cuda", self.device_id)
        self._h = C.c_void_p()
        L = _lib.lib()
        check(L.mre_create(self.blob, len(self.blob), self.num_envs, self.device_id,
                           C.byref(self._h)), "mre_create")
        self.timestep = float(self.model["opt_timestep"][0])
        self._trace = None

    # ------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _lib.lib().mre_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(_lib.lib().mre_sync(self._h), "mre_sync")
        self._keepalive = []

    def _after_torch(self, *tensors) -> None:
        """Order the handle's stream after torch's current stream (the tensors about to be handed over
        may still be in flight there) and keep them alive until the next sync()."""
        st = torch.cuda.current_stream(self.device).cuda_stream
        check(_lib.lib().mre_wait_stream(self._h, C.c_void_p(st)), "mre_wait_stream")
        if not hasattr(self, "_keepalive"):
            self._keepalive = []
        # A rollout's control rows are copied on the handle's stream by the pipelined and the guarded launches, but an
        # unguarded launch (no-constraints flag, fallback off) hands the caller's pointer straight to a kernel that runs
        # later: nothing is dropped before the handle's stream has been waited for.  A loop that never calls sync()
        # syncs here every 64 hand-overs instead of holding every tensor it ever passed -- BEFORE the new tensors are
        # registered (sync() empties the list; the tensors of THIS call are read by the library call that follows it).
        if len(self._keepalive) + len(tensors) > 64:
            self.sync()
        self._keepalive.extend(tensors)

    def set_solver(self, solver: str) -> None:
        """mjOption.solver of a live handle: "PGS" or "Newton" (state and warm start carry over)."""
        check(_lib.lib().mre_set_solver(self._h, self.SOLVERS[solver]), "mre_set_solver")

    @property
    def solver(self) -> str:
        code = _lib.lib().mre_get_solver(self._h)
        return {v: k for k, v in self.SOLVERS.items()}[code]

    @property
    def stream_ptr(self) -> int:
        return _lib.lib().mre_stream(self._h)

    # --------------------------------------------------------------- scene
    def set_props(self, nprops: Sequence[int], half_size) -> None:
        n = np.ascontiguousarray(nprops, np.int32).reshape(self.num_envs)
        s = np.ascontiguousarray(half_size, np.float32).reshape(self.num_envs, MRE_MAX_PROPS, 3)
        check(_lib.lib().mre_set_props(self._h, _ptr(n), _ptr(s)), "mre_set_props")
        self.sync()

    def _mask(self, mask):
        """uint8 [N] mask as numpy (host) or a CUDA torch tensor (device pointer handed over as is)."""
        if mask is None:
            return None
        if isinstance(mask, torch.Tensor):
            m = mask.to(torch.uint8).contiguous()
            assert tuple(m.shape) == (self.num_envs,)
            if m.is_cuda:
                self._after_torch(m)
                return m
            return m.numpy()
        return np.ascontiguousarray(mask, np.uint8)

    def reset(self, mask=None) -> None:
        m = self._mask(mask)
        check(_lib.lib().mre_reset(self._h, _ptr(m)), "mre_reset")
        self.sync()

    def set_env_order(self, order=None) -> None:
        """Heavy-first dispatch: workgroup b advances env order[b] (None = identity)."""
        if order is None:
            check(_lib.lib().mre_set_env_order(self._h, None), "mre_set_env_order")
            return
        o = np.ascontiguousarray(order, np.int32)
        assert sorted(o.tolist()) == list(range(self.num_envs)), "order must be a permutation"
        check(_lib.lib().mre_set_env_order(self._h, _ptr(o)), "mre_set_env_order")

    def set_env_ids(self, ids) -> None:
        """Explicit global env ids (RNG keys of prop placement); envs may share an id = a scene."""
        a = np.ascontiguousarray(ids, np.int64).reshape(self.num_envs)
        check(_lib.lib().mre_set_env_ids(self._h, a.ctypes.data_as(C.POINTER(C.c_longlong))), "mre_set_env_ids")

    def set_env_id_offset(self, offset: int) -> None:
        check(_lib.lib().mre_set_env_id_offset(self._h, int(offset)), "mre_set_env_id_offset")

    def place_props(self, seed: int, ws_min, ws_max, mask=None, max_attempts: int = 1000,
                    settle_steps: int = 300) -> None:
        m = self._mask(mask)
        lo = np.ascontiguousarray(ws_min, np.float32)
        hi = np.ascontiguousarray(ws_max, np.float32)
        check(_lib.lib().mre_place_props(self._h, _ptr(m), int(seed), _ptr(lo), _ptr(hi),
                                         int(max_attempts), int(settle_steps)), "mre_place_props")
        self.sync()

    # --------------------------------------------------------------- state
    def set_state(self, qpos=None, qvel=None) -> None:
        def prep(x, w, wp):
            if x is None:
                return None
            if isinstance(x, torch.Tensor):
                x = x.detach().to(torch.float32)
                if x.shape[-1] == w:
                    x = torch.nn.functional.pad(x, (0, wp - w))
                return x.contiguous()
            x = np.asarray(x, np.float32)
            if x.shape[-1] == w:
                x = np.concatenate([x, np.zeros((x.shape[0], wp - w), np.float32)], axis=1)
            return np.ascontiguousarray(x)
        qp, qv = prep(qpos, MRE_NQ, MRE_NQ_PAD), prep(qvel, MRE_NV, MRE_NV_PAD)
        check(_lib.lib().mre_set_state(self._h, _ptr(qp), _ptr(qv)), "mre_set_state")
        self.sync()

    def get_state(self) -> Tuple[np.ndarray, np.ndarray]:
        qp = np.empty((self.num_envs, MRE_NQ_PAD), np.float32)
        qv = np.empty((self.num_envs, MRE_NV_PAD), np.float32)
        check(_lib.lib().mre_get_state(self._h, _ptr(qp), _ptr(qv)), "mre_get_state")
        return qp[:, :MRE_NQ], qv[:, :MRE_NV]

    def qpos(self) -> np.ndarray:
        return self.get_state()[0]

    def pack_final_state(self) -> torch.Tensor:
        """[N, 83] float32 CUDA tensor: qpos[43], qvel[39], status of every env, packed by a kernel on the handle's
        stream (mre_pack_final_state) -- the block this rank contributes to the end-of-rollout all_gather; complete
        when this returns."""
        out = torch.empty((self.num_envs, _lib.MRE_FINAL_W), dtype=torch.float32, device=self.device)
        self._after_torch(out)
        check(_lib.lib().mre_pack_final_state(self._h, out.data_ptr()), "mre_pack_final_state")
        self.sync()
        return out

    def get_state_f64(self):
        """physics.data.qpos / .qvel as float64 [N, 43] / [N, 39]: float32 word + the low-order word the device carries
        for every coordinate (robot joints and cube poses / velocities are double-float pairs; mre_get_state_f64)."""
        q = np.empty((self.num_envs, MRE_NQ), np.float64)
        v = np.empty((self.num_envs, MRE_NV), np.float64)
        check(_lib.lib().mre_get_state_f64(self._h, _ptr(q), _ptr(v)), "mre_get_state_f64")
        return q, v

    def set_state_f64(self, qpos=None, qvel=None) -> None:
        q = None if qpos is None else np.ascontiguousarray(np.asarray(qpos, np.float64)[:, :MRE_NQ])
        v = None if qvel is None else np.ascontiguousarray(np.asarray(qvel, np.float64)[:, :MRE_NV])
        check(_lib.lib().mre_set_state_f64(self._h, _ptr(q) if q is not None else None,
                                           _ptr(v) if v is not None else None), "mre_set_state_f64")

    def time(self) -> np.ndarray:
        """physics.data.time per env [N] (seconds of physics since the last reset)."""
        t = np.empty(self.num_envs, np.float64)
        check(_lib.lib().mre_get_time(self._h, _ptr(t)), "mre_get_time")
        return t

    def qvel(self) -> np.ndarray:
        return self.get_state()[1]

    def get_warmstart(self) -> np.ndarray:
        w = np.empty((self.num_envs, MRE_NV_PAD), np.float32)
        check(_lib.lib().mre_get_warmstart(self._h, _ptr(w)), "mre_get_warmstart")
        return w[:, :MRE_NV]

    def set_warmstart(self, w) -> None:
        w = np.asarray(w, np.float32)
        if w.shape[-1] == MRE_NV:
            w = np.concatenate([w, np.zeros((w.shape[0], 1), np.float32)], axis=1)
        w = np.ascontiguousarray(w)
        check(_lib.lib().mre_set_warmstart(self._h, _ptr(w)), "mre_set_warmstart")
        self.sync()

    def set_control(self, ctrl) -> None:
        if isinstance(ctrl, torch.Tensor):
            c = ctrl.detach().to(torch.float32).contiguous()
        else:
            c = np.ascontiguousarray(ctrl, np.float32)
        assert tuple(c.shape) == (self.num_envs, MRE_NU)
        if isinstance(c, torch.Tensor) and c.is_cuda:
            self._after_torch(c)
        check(_lib.lib().mre_set_ctrl(self._h, _ptr(c)), "mre_set_ctrl")
        if not isinstance(ctrl, torch.Tensor):
            self.sync()

    def ctrl(self) -> np.ndarray:
        """physics.data.ctrl [N, 8]: the controls last applied (after run_controller: its last tick's)."""
        c = np.empty((self.num_envs, MRE_NU), np.float32)
        check(_lib.lib().mre_get_ctrl(self._h, _ptr(c)), "mre_get_ctrl")
        return c

    # ---------------------------------------------------------------- step
    def step(self, nsubsteps: int = 1, flags: int = 0) -> None:
        check(_lib.lib().mre_step(self._h, int(nsubsteps), int(flags)), "mre_step")

    def rollout(self, ctrl_seq: torch.Tensor, control_steps: int = 5, flags: int = 0, ticks_per_launch: int = 0) -> None:
        """ctrl_seq: cuda float32 [T, N, 8]; one launch for T*control_steps steps, or -- ticks_per_launch > 0 -- the T
        ticks as launches of that many ticks each, all enqueued by this one call (mre_rollout_ticks)."""
        assert ctrl_seq.is_cuda and ctrl_seq.dtype == torch.float32 and ctrl_seq.is_contiguous()
        assert ctrl_seq.shape[1:] == (self.num_envs, MRE_NU)
        self._after_torch(ctrl_seq)
        check(_lib.lib().mre_rollout_ticks(self._h, ctrl_seq.data_ptr(), int(ctrl_seq.shape[0]),
                                           int(control_steps), int(flags), int(ticks_per_launch)), "mre_rollout")

    def set_trace(self, nenv: int, max_steps: int) -> Optional[torch.Tensor]:
        """Capture qpos of the first ``nenv`` envs after every step (parity tests)."""
        if nenv <= 0:
            self._trace = None
            check(_lib.lib().mre_set_trace(self._h, None, 0, 0), "mre_set_trace")
            return None
        self._trace = torch.zeros((max_steps, nenv, MRE_TRACE_W), dtype=torch.float32,
                                  device=self.device)
        self._after_torch()  # the zero fill runs on torch's stream
        check(_lib.lib().mre_set_trace(self._h, self._trace.data_ptr(), nenv, max_steps),
              "mre_set_trace")
        return self._trace

    # ----------------------------------------------------------- controller
    def osc_configure(self, gains=None, null_q=None, thresholds=None, pinv_always: bool = False):
        g = None if gains is None else np.ascontiguousarray(gains, np.float32)
        q = None if null_q is None else np.ascontiguousarray(null_q, np.float32)
        t = None if thresholds is None else np.ascontiguousarray(thresholds, np.float32)
        check(_lib.lib().mre_osc_configure(self._h, _ptr(g), _ptr(q), _ptr(t), int(pinv_always)),
              "mre_osc_configure")

    def osc_configure_env(self, gains=None, null_q=None, thresholds=None) -> None:
        """One controller parameter set per env: gains [N, 6] (kp, kd of position / orientation /
        nullspace), null_q [N, 7], thresholds [N, 2]; None keeps the shared set's values."""
        def prep(x, w):
            if x is None:
                return None
            x = np.ascontiguousarray(x, np.float32)
            assert x.shape == (self.num_envs, w), (x.shape, w)
            return x
        g, q, t = prep(gains, 6), prep(null_q, 7), prep(thresholds, 2)
        check(_lib.lib().mre_osc_configure_env(self._h, _ptr(g), _ptr(q), _ptr(t)), "mre_osc_configure_env")

    def osc_set_target(self, position=None, quat=None, velocity=None, angular_velocity=None,
                       mask=None) -> None:
        def prep(x, w):
            if x is None:
                return None
            x = np.asarray(x, np.float32)
            if x.ndim == 1:
                x = np.tile(x, (self.num_envs, 1))
            assert x.shape == (self.num_envs, w)
            return np.ascontiguousarray(x)
        p, q = prep(position, 3), prep(quat, 4)
        v, w = prep(velocity, 3), prep(angular_velocity, 3)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        check(_lib.lib().mre_osc_set_target(self._h, _ptr(p), _ptr(q), _ptr(v), _ptr(w), _ptr(m)),
              "mre_osc_set_target")

    def osc_compute(self):
        """(tau [N, 7], gripper command [N]) of the controllers on the current state, no stepping:
        OSC.compute_control_output() / MinMax.compute_control_output() (models/robot_arm.py:71,73)."""
        tau = np.empty((self.num_envs, 7), np.float32)
        grip = np.empty(self.num_envs, np.float32)
        check(_lib.lib().mre_osc_compute(self._h, _ptr(tau), _ptr(grip)), "mre_osc_compute")
        return tau, grip

    SITES = {"eef": 0, "pinch": 1}   # controller (attachment) site, gripper pinch site (include/mre.h)

    def arm_dynamics(self, site="eef"):
        """mj_jacSite / mj_fullM / qfrc_bias of the arm on the current state, no stepping (mre_get_arm_dynamics): an
        ``ArmTerms`` (controllers/torch_osc.py) of CUDA float32 views into one [N, 128] tensor -- jac [N, 6, 7] of
        ``site`` ("eef": the controller site, "pinch"; or 0 / 1), mass [N, 7, 7], bias [N, 7], site_pos [N, 3],
        site_quat [N, 4], qpos [N, 7], qvel [N, 7].  The kernel runs on the handle's stream and torch's current stream is
        ordered after it on the device: nothing waits on the host, and nothing of the handle's state is written."""
        from .controllers.torch_osc import ArmTerms
        out = torch.empty((self.num_envs, _lib.MRE_DYN_W), dtype=torch.float32, device=self.device)
        self._after_torch()   # the block may have been another tensor's on torch's stream a moment ago
        check(_lib.lib().mre_get_arm_dynamics(self._h, int(self.SITES.get(site, site)), out.data_ptr()),
              "mre_get_arm_dynamics")
        if getattr(self, "_ext_stream", None) is None:
            self._ext_stream = torch.cuda.ExternalStream(self.stream_ptr, device=self.device)
        torch.cuda.current_stream(self.device).wait_stream(self._ext_stream)
        return ArmTerms.from_packed(out)

    def gripper_set(self, closed) -> None:
        c = np.ascontiguousarray(np.broadcast_to(np.asarray(closed, np.uint8), (self.num_envs,)))
        check(_lib.lib().mre_gripper_set(self._h, _ptr(c)), "mre_gripper_set")
        self.sync()

    def run_controller(self, nticks: int, control_steps: int = 5) -> np.ndarray:
        conv = np.zeros(self.num_envs, np.uint8)
        check(_lib.lib().mre_run_controller(self._h, int(nticks), int(control_steps), _ptr(conv)),
              "mre_run_controller")
        return conv.astype(bool)

    # -------------------------------------------------------------- queries
    def sites(self):
        tcp = np.empty((self.num_envs, 3), np.float32)
        eef = np.empty((self.num_envs, 7), np.float32)
        props = np.empty((self.num_envs, MRE_MAX_PROPS, 7), np.float32)
        check(_lib.lib().mre_get_sites(self._h, _ptr(tcp), _ptr(eef), _ptr(props)), "mre_get_sites")
        return tcp, eef, props

    def contacts(self, full: bool = False, active_only: bool = False):
        """physics.data.contact of every env on the current poses: (count [N] (negative: list cut),
        contacts [N, 32, 3] = geom1, geom2, dist) -- every DETECTED contact (dist < margin).
        full: contacts [N, 32, 15] = pos[3], frame[9], dist, geom1, geom2 instead (mre_get_contacts_full);
        active_only (with full): the contacts the next solve would be given (dist < margin - gap)."""
        cnt = np.empty(self.num_envs, np.int32)
        if full:
            con = np.empty((self.num_envs, 32, 15), np.float32)
            check(_lib.lib().mre_get_contacts_full(self._h, int(active_only), _ptr(cnt), _ptr(con)), "mre_get_contacts_full")
            return cnt, con
        assert not active_only, "active_only needs full=True"
        con = np.empty((self.num_envs, 32, 3), np.float32)
        check(_lib.lib().mre_get_contacts(self._h, _ptr(cnt), _ptr(con)), "mre_get_contacts")
        return cnt, con

    def prop_place(self, seed: int, prop, bounds, tick, max_attempts: int = 10000, max_dist: float = 0.05):
        """prop_place (tasks/rearrangement.py:597-665) for every env on the device (mre_prop_place):
        prop [N] cube index (< 0: skip), bounds [N, 6] lo / hi, tick [N] first RNG tick ->
        (pose [N, 7] fp64, attempts [N])."""
        n = self.num_envs
        pr = np.ascontiguousarray(prop, np.int32)
        bd = np.ascontiguousarray(bounds, np.float64)
        tk = np.ascontiguousarray(tick, np.int32)
        assert pr.shape == (n,) and bd.shape == (n, 6) and tk.shape == (n,)
        pose = np.empty((n, 7), np.float64)
        att = np.empty(n, np.int32)
        check(_lib.lib().mre_prop_place(self._h, int(seed), _ptr(pr), _ptr(bd), _ptr(tk), int(max_attempts),
                                        float(max_dist), _ptr(pose), _ptr(att)), "mre_prop_place")
        return pose, att

    def sort_colours(self, seed: int, call_counts, zones, max_attempts: int = 10000, max_dist: float = 0.05):
        """sort_colours (tasks/rearrangement.py:700-751) for every env on the device (mre_sort_colours):
        zones [N, 4, 4] = lo x, lo y, hi x, hi y of every cube's colour zone ->
        (which [N], pick [N, 7], place [N, 7], attempts [N])."""
        n = self.num_envs
        cc = np.ascontiguousarray(call_counts, np.int32)
        zn = np.ascontiguousarray(zones, np.float64)
        assert cc.shape == (n,) and zn.shape == (n, 4, 4)
        which = np.empty(n, np.int32)
        pick = np.empty((n, 7), np.float64)
        place = np.empty((n, 7), np.float64)
        att = np.empty(n, np.int32)
        check(_lib.lib().mre_sort_colours(self._h, int(seed), _ptr(cc), _ptr(zn), int(max_attempts), float(max_dist),
                                          _ptr(which), _ptr(pick), _ptr(place), _ptr(att)), "mre_sort_colours")
        return which, pick, place, att

    def launch_info(self) -> dict:
        """Per-env record of the last stepping launch (mre_get_launch_info): overflow flag, high-water marks
        and the env's own duration (clock ticks >> 10, the key of the longest-first dispatch)."""
        li = np.empty((self.num_envs, 4), np.int32)
        check(_lib.lib().mre_get_launch_info(self._h, _ptr(li)), "mre_get_launch_info")
        return dict(overflow=li[:, 0], ncon=li[:, 1] & 0xFFFF, duration=li[:, 1] >> 16, nefc=li[:, 2],
                    nrrow=li[:, 3] & 0xFFFF, npp=li[:, 3] >> 16)

    def settle_steps(self) -> np.ndarray:
        """Physics steps every env took in the last place_props() settle (negative: not settled in 2 s)."""
        st = np.empty(self.num_envs, np.int32)
        check(_lib.lib().mre_get_settle_steps(self._h, _ptr(st)), "mre_get_settle_steps")
        return st

    def status(self) -> np.ndarray:
        st = np.empty(self.num_envs, np.uint32)
        check(_lib.lib().mre_get_status(self._h, _ptr(st)), "mre_get_status")
        return st

    def solver_stats(self) -> np.ndarray:
        st = np.empty((self.num_envs, 4), np.int32)
        check(_lib.lib().mre_get_solver_stats(self._h, _ptr(st)), "mre_get_solver_stats")
        # column 2 = solver iterations of the last step | Hessian factorisations << 8 (Newton only)
        self.last_factorizations = st[:, 2] >> 8
        st[:, 2] &= 0xFF
        return st

    # ---------------------------------------------------------- measurement
    # ------------------------------------------------------------------ camera
    def set_render_colours(self, prop_rgb=None, geom_rgb=None) -> None:
        """prop_rgb [N, 4, 3] uint8 cube albedo; geom_rgb [ngeom, 3] float albedo of the other geoms."""
        p = None if prop_rgb is None else np.ascontiguousarray(prop_rgb, np.uint8).reshape(self.num_envs, MRE_MAX_PROPS, 3)
        g = None if geom_rgb is None else np.ascontiguousarray(geom_rgb, np.float32).reshape(int(self.model["ngeom"][0]), 3)
        check(_lib.lib().mre_set_render_colours(self._h, _ptr(p), _ptr(g)), "mre_set_render_colours")

    def render(self, cam_pos, cam_mat, fovy: float, height: int, width: int, rgb: bool = True, depth: bool = True,
               seg: bool = True, mask=None):
        """Overhead camera images of the current state of every env (mre_render) as CUDA tensors:
        rgb uint8 [N, H, W, 3], depth float32 [N, H, W], seg uint8 [N, H, W] (255 = background);
        entries not asked for are None."""
        n = self.num_envs
        t_rgb = torch.empty((n, height, width, 3), dtype=torch.uint8, device=self.device) if rgb else None
        t_depth = torch.empty((n, height, width), dtype=torch.float32, device=self.device) if depth else None
        t_seg = torch.empty((n, height, width), dtype=torch.uint8, device=self.device) if seg else None
        cp = np.ascontiguousarray(cam_pos, np.float32).reshape(3)
        cm = np.ascontiguousarray(cam_mat, np.float32).reshape(9)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        check(_lib.lib().mre_render(self._h, _ptr(cp), _ptr(cm), float(fovy), int(height), int(width),
                                    _ptr(t_rgb), _ptr(t_depth), _ptr(t_seg), _ptr(m)), "mre_render")
        self.sync()
        return t_rgb, t_depth, t_seg

    def set_fallback(self, mode=True) -> None:
        """Capacity fallback (include/mre.h): True / 1 = on (default), False / 0 = compact kernel only,
        2 = large kernel only."""
        check(_lib.lib().mre_set_fallback(self._h, int(mode)), "mre_set_fallback")

    def fallback_stats(self) -> dict:
        out = (C.c_longlong * 4)()
        check(_lib.lib().mre_get_fallback_stats(self._h, out), "mre_get_fallback_stats")
        return {"large_envs": int(out[0]), "reruns": int(out[1]), "promotions": int(out[2]), "demotions": int(out[3])}

    def queue_info(self) -> dict:
        """Queue launches (include/mre.h: mre_get_queue_info): how many so far, their waves, the library's ticks per launch."""
        out = (C.c_longlong * 5)()
        check(_lib.lib().mre_get_queue_info(self._h, out), "mre_get_queue_info")
        return {"launches": int(out[0]), "waves": int(out[1]), "ticks_per_launch": int(out[2]), "enabled": bool(out[3]),
                "handovers": int(out[4])}

    def profile_enable(self, on: bool = True) -> None:
        check(_lib.lib().mre_profile_enable(self._h, int(on)), "mre_profile_enable")

    def profile_read(self):
        """(summed kernel ms, launches) measured with HIP events on the handle's stream."""
        ms, n = C.c_float(0), C.c_int(0)
        check(_lib.lib().mre_profile_read(self._h, C.byref(ms), C.byref(n)), "mre_profile_read")
        return float(ms.value), int(n.value)
