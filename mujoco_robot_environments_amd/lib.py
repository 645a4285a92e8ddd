"""ctypes binding of the C-ABI library ``libmre.so`` (include/mre.h), and the one recipe that builds it.

The HIP path has no CPU fallback: a missing library or a missing GPU raises.
"""
from __future__ import annotations

import ctypes as C
import glob
import os
import shutil
import subprocess
from typing import Optional

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
_SO = os.path.join(_CSRC, "libmre.so")
# What source_hash() names: the step and camera sources.  Every other unit stays outside, because the committed counter
# passes (profiles/*pmc_summary*.json) name that hash: a unit added beside the step must not orphan them.
_HASHED = ["mre_kernels.hip", "mre_render.hip", "mre_dev.h", "mre_math.h", "mre_collide.h", "mre_solver.h", "mre_newton.h",
           "mre_osc.h"]
_LIB: Optional[C.CDLL] = None

# -ffp-contract=on: a * b + c is fused where the SOURCE expression says so, not wherever the optimiser
# finds one after unrolling -- the compact and the large instantiation of the step kernel must round
# identically (the capacity fallback re-runs an env on the other one and promises the same bits)
# -fno-hip-fp32-correctly-rounded-divide-sqrt: fp32 a / b and sqrtf as v_rcp_f32 / v_sqrt_f32 (about 1 ulp)
# instead of the ten-instruction correctly rounded sequences; the fp64 finger-frame code is not affected,
# and the parity tests against the fp64 oracle see no difference (+2 % on the Newton bench)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-ffp-contract=on",
         "-fno-hip-fp32-correctly-rounded-divide-sqrt"]
# (object name, source, defines).  The step kernel is instantiated four times: {compact, large constraint capacities
# (mre_dev.h)} x {PGS, Newton (mre_newton.h)}
STEP_SOURCE = "mre_kernels.hip"
UNITS = [("kernels", STEP_SOURCE, []), ("kernels_large", STEP_SOURCE, ["-DMRE_LARGE_CAPS"]),
         ("kernels_newton", STEP_SOURCE, ["-DMRE_NEWTON"]),
         ("kernels_large_newton", STEP_SOURCE, ["-DMRE_LARGE_CAPS", "-DMRE_NEWTON"]),
         ("render", "mre_render.hip", []), ("records", "mre_records.hip", []),
         ("labels", "mre_labels.hip", []), ("heightmap", "mre_heightmap.hip", []),
         ("heightmap_views", "mre_heightmap_views.hip", []),
         ("warp", "mre_warp.hip", []), ("warp_inputs", "mre_warp_inputs.hip", []),
         ("correlate", "mre_correlate.hip", []), ("correlate_grad", "mre_correlate_grad.hip", []),
         ("attend", "mre_attend.hip", []), ("api", "mre_api.cpp", []), ("stream_api", "mre_stream_api.cpp", []),
         ("sched", "mre_sched.cpp", []), ("model", "mre_model.cpp", [])]

MRE_NQ, MRE_NV, MRE_NU, MRE_NQ_PAD, MRE_NV_PAD, MRE_MAX_PROPS = 43, 39, 8, 44, 40, 4
MRE_TRACE_W = 88   # row of the parity trace (mre_set_trace): qpos, census columns, then qvel from MRE_TRACE_QVEL on
MRE_TRACE_QVEL = 48
MRE_FINAL_W = 83    # row of mre_pack_final_state: qpos[43], qvel[39], status
MRE_DYN_W = 128     # row of mre_get_arm_dynamics: jac[6][7], mass[7][7], bias[7], site pos[3] quat[4], qpos[7], qvel[7], pad

# Every export of include/mre.h, once: name -> argtypes, or (restype, argtypes) where the result is not an int.
vp, ci, cu, fp, sz, u64, u32 = C.c_void_p, C.c_int, C.c_uint, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint32
_SIGNATURES = {
    "mre_create": [C.c_char_p, sz, ci, ci, C.POINTER(vp)], "mre_destroy": [vp],
    "mre_last_error": (C.c_char_p, None), "mre_num_envs": [vp], "mre_stream": (vp, [vp]), "mre_sync": [vp],
    "mre_set_props": [vp, fp, fp], "mre_reset": [vp, fp], "mre_place_props": [vp, fp, u64, fp, fp, ci, ci],
    "mre_set_state": [vp, fp, fp], "mre_get_state": [vp, fp, fp], "mre_get_ctrl": [vp, fp],
    "mre_set_warmstart": [vp, fp], "mre_get_warmstart": [vp, fp], "mre_set_ctrl": [vp, fp], "mre_step": [vp, ci, cu],
    "mre_rollout": [vp, fp, ci, ci, cu], "mre_rollout_ticks": [vp, fp, ci, ci, cu, ci],
    "mre_set_trace": [vp, fp, ci, ci], "mre_osc_set_target": [vp, fp, fp, fp, fp, fp],
    "mre_osc_configure": [vp, fp, fp, fp, ci], "mre_gripper_set": [vp, fp],
    "mre_run_controller": [vp, ci, ci, fp], "mre_get_sites": [vp, fp, fp, fp], "mre_get_status": [vp, fp],
    "mre_get_solver_stats": [vp, fp],
    "mre_profile_enable": [vp, ci], "mre_profile_read": [vp, C.POINTER(C.c_float), C.POINTER(ci)],
    "mre_set_env_id_offset": [vp, C.c_longlong], "mre_set_env_order": [vp, fp],
    "mre_set_fallback": [vp, ci], "mre_get_fallback_stats": [vp, C.POINTER(C.c_longlong)],
    "mre_get_queue_info": [vp, C.POINTER(C.c_longlong)], "mre_set_solver": [vp, ci], "mre_get_solver": [vp],
    "mre_wait_stream": [vp, vp], "mre_osc_compute": [vp, fp, fp], "mre_get_contacts": [vp, fp, fp],
    "mre_get_contacts_full": [vp, ci, fp, fp], "mre_get_settle_steps": [vp, fp], "mre_get_launch_info": [vp, fp],
    "mre_prop_place": [vp, u64, fp, fp, fp, ci, C.c_float, fp, fp],
    "mre_sort_colours": [vp, u64, fp, fp, ci, C.c_float, fp, fp, fp, fp],
    "mre_crc32c": (u32, [C.c_char_p, sz]), "mre_osc_configure_env": [vp, fp, fp, fp],
    "mre_set_env_ids": [vp, C.POINTER(C.c_longlong)], "mre_set_render_colours": [vp, fp, fp],
    "mre_render": [vp, fp, fp, C.c_float, ci, ci, fp, fp, fp, fp],
    "mre_get_state_f64": [vp, fp, fp], "mre_set_state_f64": [vp, fp, fp], "mre_get_time": [vp, fp],
    "mre_pack_final_state": [vp, fp],
    "mre_records_workspace_bytes": (sz, [ci, sz]),
    "mre_varint_pack_rows": [vp, fp, sz, sz, fp, ci, ci, fp, sz, fp, fp, fp, fp, sz],
    "mre_crc32c_rows": [vp, fp, sz, sz, fp, ci, ci, fp, fp, sz], "mre_crc32c_combine": (u32, [u32, u32, sz]),
    "mre_varint_unpack_workspace_bytes": (sz, [ci, sz]),
    "mre_varint_unpack_rows": [vp, fp, sz, fp, fp, fp, fp, ci, sz, fp, sz, fp, fp, sz],
    "mre_get_arm_dynamics": [vp, ci, fp], "mre_seg_labels": [vp, fp, fp, ci, ci, ci, ci, ci, fp, fp],
    "mre_heightmap": [vp, fp, fp, fp, ci, ci, ci, fp, fp, C.c_float, C.c_float, ci, ci, fp, fp, fp, fp],
    "mre_heightmap_views": [vp, ci, fp, fp, fp, ci, fp, fp, fp, fp, C.c_float, C.c_float, ci, ci, fp, fp, fp, fp, fp],
    "mre_warp_maps": [vp, fp, fp, fp, ci, ci, ci, fp, fp, ci, ci, ci, fp, fp, fp, fp],
    "mre_warp_inputs": [vp, fp, fp, ci, ci, ci, fp, fp, ci, ci, ci, ci, fp, fp, fp, ci, fp],
    "mre_correlate_workspace": [ci, ci, ci, ci, C.POINTER(sz)],
    "mre_correlate": [vp, fp, fp, ci, ci, ci, ci, ci, ci, ci, fp, fp, fp, fp, sz],
    "mre_correlate_loss": [vp, fp, fp, ci, ci, ci, ci, ci, ci, fp, fp, fp, fp, fp, sz],
    "mre_correlate_dlogits": [vp, fp, fp, ci, ci, ci, ci, ci, ci, fp, fp, fp, fp],
    "mre_correlate_grad_workspace": [ci, ci, ci, ci, ci, ci, C.POINTER(sz)],
    "mre_correlate_grad_scene": [vp, fp, fp, ci, ci, ci, ci, ci, ci, fp, fp, sz],
    "mre_correlate_grad_kern": [vp, fp, fp, ci, ci, ci, ci, ci, ci, fp, fp, sz],
    "mre_attend_workspace": [ci, ci, ci, ci, C.POINTER(sz)],
    "mre_attend": [vp, fp, ci, ci, ci, ci, ci, fp, fp, fp, fp, fp, fp, fp, sz],
    "mre_attend_dlogits": [vp, fp, ci, ci, ci, ci, ci, fp, fp, fp, fp],
}
EXPORTS = list(_SIGNATURES)
# status bits of mre_varint_unpack_rows (include/mre.h)
MRE_UNPACK_LONG, MRE_UNPACK_OVERFLOW, MRE_UNPACK_TRUNCATED, MRE_UNPACK_COUNT, MRE_UNPACK_DESC = 1, 2, 4, 8, 16


class MreError(RuntimeError):
    pass


def source_hash() -> str:
    """sha256 (16 hex digits) over the DEVICE sources of the step and the camera (the two .hip files and their headers;
    not the host side of the C ABI, which decides how launches are issued but not what a launch executes): what a
    profile summary must have been taken on for its per-launch counters to describe the build being run (bench.py,
    tools/summarize_profiles.py)."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(_HASHED):
        with open(os.path.join(_CSRC, f), "rb") as fh:
            h.update(f.encode() + b"\0" + fh.read())
    return h.hexdigest()[:16]


def needs_build() -> bool:
    """libmre.so is missing, or older than a source or header directly under csrc/ or than include/mre.h"""
    if not os.path.exists(_SO):
        return True
    t = os.path.getmtime(_SO)
    watched = [p for ext in ("*.hip", "*.cpp", "*.h") for p in glob.glob(os.path.join(_CSRC, ext))]
    watched.append(os.path.join(_CSRC, "..", "..", "include", "mre.h"))
    return any(os.path.getmtime(p) > t for p in watched)


def compile_and_link(so: str, objdir: str, suffix: str = "", csrc: Optional[str] = None, extra=(), step_extra=(),
                     verbose: bool = False) -> str:
    """Compile UNITS for gfx950, all at once (16 compilers: the 16 CPUs a build may count on), and link them to `so`.
    Objects go to objdir as NAME + suffix + .o; `extra` flags go to every unit, `step_extra` to the instantiations of
    the step kernel only.  csrc may be another checkout's sources: units that checkout lacks are skipped."""
    csrc = csrc or _CSRC
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    base = [hipcc] + (["-Rpass-analysis=kernel-resource-usage"] if verbose else []) + FLAGS + list(extra)
    os.makedirs(objdir, exist_ok=True)
    procs = []
    for name, src, defines in UNITS:
        if csrc != _CSRC and not os.path.exists(os.path.join(csrc, src)):
            continue
        obj = os.path.join(objdir, name + suffix + ".o")
        cmd = base + defines + (list(step_extra) if src == STEP_SOURCE else []) + ["-c", os.path.join(csrc, src), "-o", obj]
        procs.append((name, obj, subprocess.Popen(cmd)))
    failed = [name for name, _, pr in procs if pr.wait() != 0]   # (every compiler is waited for)
    if failed:
        raise MreError(f"hipcc failed on translation unit {failed[0]}")
    subprocess.check_call([hipcc, FLAGS[0], "-shared", "-fPIC", "-o", so] + [obj for _, obj, _ in procs])
    return so


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP kernels + C-ABI host code for gfx950 in-tree."""
    if not force and not needs_build():
        return _SO
    return compile_and_link(_SO, os.path.join(_CSRC, "_build"), verbose=verbose)


def lib() -> C.CDLL:
    """Load libmre.so (never builds implicitly on a GPU box: the .so travels in-tree)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # torch first: its wheel bundles a HIP runtime of the same soname, and a process must hold ONE
    # runtime (libmre.so loaded first would bind /opt/rocm's copy and see no device once torch has
    # initialised its own)
    import torch  # noqa: F401
    so = os.environ.get("MRE_LIB", _SO)  # diagnostic builds (tools/build_variant.py, tools/phase_stamps.py) only
    if not os.path.exists(so):
        raise MreError(f"{so} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(the HIP extension is the only implementation of the step)")
    L = C.CDLL(so)
    for name, sig in _SIGNATURES.items():
        restype, argtypes = sig if isinstance(sig, tuple) else (ci, sig)
        fn = getattr(L, name)
        fn.restype = restype
        if argtypes is not None:
            fn.argtypes = argtypes
    _LIB = L
    return L


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().mre_last_error()
        raise MreError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
