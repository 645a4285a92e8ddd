"""Torque laws in torch over the arm's exported dynamics terms.

``BatchedPhysics.arm_dynamics()`` hands out what every MuJoCo controller reads -- ``mj_jacSite``, ``mj_fullM``,
``qfrc_bias`` -- as CUDA tensors (include/mre.h: mre_get_arm_dynamics).  A torque law is a plain callable

    law(terms, target) -> tau [N, 7]

``terms``: an ``ArmTerms``; ``target``: anything that carries ``OSC``'s ``eef_target_position`` [N, 3],
``eef_target_quat`` [N, 4] (wxyz), ``eef_target_velocity`` [N, 3] and ``eef_target_angular_velocity`` [N, 3] -- the
``OSC`` object itself, a mapping with those keys, or ``target_tensors()`` of either (tensors, converted once).
``RobotArm(..., torque_law=law)`` runs such a law tick by tick in place of the in-kernel one.

``TorchOSC`` is the law of csrc/mre_osc.h (the reference restates it at tasks/rearrangement_mjx.py:59-135) in batched
torch: a candidate law is a subclass or a ten-line function beside it (examples/controller_laws.py)."""
from __future__ import annotations

import numpy as np
import torch

# slices of one packed row (include/mre.h: MRE_DYN_W)
_JAC, _MASS, _BIAS, _POS, _QUAT, _QPOS, _QVEL = (0, 42), (42, 91), (91, 98), (98, 101), (101, 105), (105, 112), (112, 119)
TARGET_FIELDS = ("eef_target_position", "eef_target_quat", "eef_target_velocity", "eef_target_angular_velocity")


class ArmTerms:
    """Views into one [N, 128] tensor (``raw``): jac [N, 6, 7] (rows 0-2 jacp, 3-5 jacr), mass [N, 7, 7], bias [N, 7],
    site_pos [N, 3], site_quat [N, 4] (wxyz), qpos [N, 7], qvel [N, 7].  Built from arrays of those shapes as well
    (CPU tensors included): a law does not care where its terms come from."""
    __slots__ = ("raw", "jac", "mass", "bias", "site_pos", "site_quat", "qpos", "qvel")

    def __init__(self, jac, mass, bias, site_pos, site_quat, qpos, qvel, raw=None):
        self.raw = raw
        self.jac, self.mass, self.bias = torch.as_tensor(jac), torch.as_tensor(mass), torch.as_tensor(bias)
        self.site_pos, self.site_quat = torch.as_tensor(site_pos), torch.as_tensor(site_quat)
        self.qpos, self.qvel = torch.as_tensor(qpos), torch.as_tensor(qvel)
        n = self.jac.shape[0]
        assert self.jac.shape == (n, 6, 7) and self.mass.shape == (n, 7, 7) and self.bias.shape == (n, 7)
        assert self.site_pos.shape == (n, 3) and self.site_quat.shape == (n, 4)
        assert self.qpos.shape == (n, 7) and self.qvel.shape == (n, 7)

    @classmethod
    def from_packed(cls, raw: torch.Tensor) -> "ArmTerms":
        n = raw.shape[0]
        assert raw.shape == (n, 128)
        cut = lambda s: raw[:, s[0]:s[1]]  # noqa: E731
        return cls(cut(_JAC).view(n, 6, 7), cut(_MASS).view(n, 7, 7), cut(_BIAS), cut(_POS), cut(_QUAT), cut(_QPOS),
                   cut(_QVEL), raw=raw)

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k in self.__slots__[1:]}


def target_tensors(target, device, dtype=torch.float64) -> dict:
    """The four ``eef_target_*`` arrays of ``target`` as [N, w] or [w] tensors on ``device``: convert once per phase, not
    once per tick."""
    out = {}
    for k in TARGET_FIELDS:
        v = target[k] if isinstance(target, dict) else getattr(target, k)
        out[k] = torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).to(device=device, dtype=dtype)
    return out


def _qmul(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


class TorchOSC:
    """tau = J' L F + (I - J' Jbar') tau0 + qfrc_bias with L = inv(J M^-1 J') -- or pinv(rcond = 1e-2) of it where
    |det| < 1e-2 or ``pinv_always`` --, F = [kp_p e_p + kd_p (v* - J_p qd); kp_o e_o + kd_o (w* - J_r qd)],
    tau0 = kp_n (q0 - q) + kd_n (0 - qd), Jbar = M^-1 J' L.

    gains: [6] or [N, 6] = kp, kd of position / orientation / nullspace (osc.yaml: 350 20 500 100 200 30);
    thresholds: (position, orientation) of ``converged`` (osc.yaml: 5e-3, 68e-3).  The terms are float32 numbers; the law
    is evaluated in ``dtype`` (float64) on the device the terms live on.  On CUDA both inverses are evaluated and
    selected per env on the device, so that no tick waits for the host; on the CPU the pseudo-inverse is computed
    only where the rule asks for it."""

    def __init__(self, gains=(350.0, 20.0, 500.0, 100.0, 200.0, 30.0),
                 null_q=(0.0, -0.785, 0.0, -2.356, 0.0, 1.571, 0.785), thresholds=(5e-3, 68e-3),
                 pinv_always: bool = False, dtype=torch.float64):
        self.gains = torch.as_tensor(np.asarray(gains, np.float64))
        assert self.gains.shape[-1] == 6 and self.gains.dim() in (1, 2)
        self.null_q = torch.as_tensor(np.asarray(null_q, np.float64))
        self.position_threshold, self.orientation_threshold = float(thresholds[0]), float(thresholds[1])
        self.pinv_always = bool(pinv_always)
        self.dtype = dtype

    @classmethod
    def from_osc(cls, osc, **kw) -> "TorchOSC":
        """The gains, nullspace configuration and thresholds an ``OSC`` parameter holder carries."""
        g = osc.controller_gains
        return cls(gains=[g["position"]["kp"], g["position"]["kd"], g["orientation"]["kp"], g["orientation"]["kd"],
                          g["nullspace"]["kp"], g["nullspace"]["kd"]], null_q=osc.nullspace_config,
                   thresholds=(osc.position_threshold, osc.orientation_threshold), **kw)

    # ------------------------------------------------------------------ pieces a candidate law reuses
    def _target(self, terms: ArmTerms, target) -> dict:
        if isinstance(target, dict) and all(isinstance(target.get(k), torch.Tensor) for k in TARGET_FIELDS):
            return target
        return target_tensors(target, terms.jac.device, self.dtype)

    def _gain(self, k: int, terms: ArmTerms):
        g = self.gains.to(device=terms.jac.device, dtype=self.dtype)
        return g[..., k:k + 1]   # [1] or [N, 1]: broadcasts over the components

    def errors(self, terms: ArmTerms, target):
        """(e_p [N, 3], e_o [N, 3]): target - site position; vector part of target * conj(site quaternion), signed by
        its scalar part (mre_osc.h: osc_errors)."""
        t = self._target(terms, target)
        ep = t["eef_target_position"].to(self.dtype) - terms.site_pos.to(self.dtype)
        qc = terms.site_quat.to(self.dtype) * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=self.dtype, device=terms.jac.device)
        tq = t["eef_target_quat"].to(self.dtype).expand_as(qc)
        qe = _qmul(tq, qc)
        return ep, torch.sign(qe[:, :1]) * qe[:, 1:]

    def converged(self, terms: ArmTerms, target) -> torch.Tensor:
        ep, eo = self.errors(terms, target)
        return (ep.norm(dim=1) < self.position_threshold) & (eo.norm(dim=1) < self.orientation_threshold)

    def task_inertia(self, terms: ArmTerms):
        """(L [N, 6, 6], M^-1 J' [N, 7, 6]) by the kernel's inverse rule."""
        J, M = terms.jac.to(self.dtype), terms.mass.to(self.dtype)
        MiJt = torch.linalg.solve(M, J.transpose(1, 2))
        Li = J @ MiJt
        use_pinv = ~(torch.linalg.det(Li).abs() >= 1e-2)
        if self.pinv_always:
            use_pinv = torch.ones_like(use_pinv)
        Lam = torch.linalg.inv_ex(Li).inverse   # (no error check: a singular env takes the other branch)
        if self.pinv_always or Li.is_cuda or bool(use_pinv.any()):
            Lp = torch.linalg.pinv(0.5 * (Li + Li.transpose(1, 2)), rtol=1e-2, hermitian=True)
            Lam = torch.where(use_pinv[:, None, None], Lp, Lam)
        return Lam, MiJt

    def nullspace_torque(self, terms: ArmTerms):
        q, qd = terms.qpos.to(self.dtype), terms.qvel.to(self.dtype)
        q0 = self.null_q.to(device=q.device, dtype=self.dtype)
        return self._gain(4, terms) * (q0 - q) + self._gain(5, terms) * (0.0 - qd)

    def task_force(self, terms: ArmTerms, target):
        t = self._target(terms, target)
        ep, eo = self.errors(terms, t)
        xd = (terms.jac.to(self.dtype) @ terms.qvel.to(self.dtype)[:, :, None])[:, :, 0]
        v, w = t["eef_target_velocity"].to(self.dtype), t["eef_target_angular_velocity"].to(self.dtype)
        return torch.cat([self._gain(0, terms) * ep + self._gain(1, terms) * (v - xd[:, :3]),
                          self._gain(2, terms) * eo + self._gain(3, terms) * (w - xd[:, 3:])], dim=1)

    def project(self, terms: ArmTerms, F, tau0, Lam=None, MiJt=None):
        """J' L F + (I - J' Jbar') tau0 + qfrc_bias."""
        if Lam is None:
            Lam, MiJt = self.task_inertia(terms)
        Jt = terms.jac.to(self.dtype).transpose(1, 2)
        Jbar = MiJt @ Lam
        task = (Jt @ (Lam @ F[:, :, None]))[:, :, 0]
        null = tau0 - (Jt @ (Jbar.transpose(1, 2) @ tau0[:, :, None]))[:, :, 0]
        return task + null + terms.bias.to(self.dtype)

    # ------------------------------------------------------------------ the law
    def __call__(self, terms: ArmTerms, target) -> torch.Tensor:
        t = self._target(terms, target)
        return self.project(terms, self.task_force(terms, t), self.nullspace_torque(terms))


__all__ = ["ArmTerms", "TorchOSC", "target_tensors", "TARGET_FIELDS"]
