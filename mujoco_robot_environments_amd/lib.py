"""ctypes binding of the C-ABI library ``libmre.so`` (include/mre.h).

The HIP path has no CPU fallback: a missing library or a missing GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
from typing import Optional

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
_SO = os.path.join(_CSRC, "libmre.so")
_SOURCES = ["mre_kernels.hip", "mre_render.hip", "mre_api.cpp"]
_HEADERS = ["mre_dev.h", "mre_math.h", "mre_collide.h", "mre_solver.h", "mre_newton.h", "mre_osc.h",
            os.path.join("..", "..", "include", "mre.h")]
# Built and watched by needs_build(), but NOT hashed by source_hash(): the record kernels (varint packing, CRC-32C of
# episode shards) launch nothing that bench.py times, and the hash names the step / camera sources that the committed
# counter passes (profiles/*pmc_summary*.json) were taken on -- adding a unit beside them must not orphan those.
# The model builder and the launch scheduler are host code like mre_api.cpp: they decide what is uploaded and how
# launches are issued, not what a launch executes.  The frame-label kernel (mre_labels.hip) reads rendered images and is
# launched by neither the step nor the camera, and so are the heightmap kernel (mre_heightmap.hip), the map warp
# (mre_warp.hip) and the network inputs (mre_warp_inputs.hip) with the gather they share (mre_warp_gather.h), and the
# place head's correlation (mre_correlate.hip).
_UNHASHED_SOURCES = ["mre_records.hip", "mre_records.h", "mre_labels.hip", "mre_labels.h", "mre_heightmap.hip", "mre_heightmap.h",
                     "mre_heightmap_point.h", "mre_warp.hip", "mre_warp.h", "mre_warp_point.h", "mre_warp_gather.h", "mre_warp_inputs.hip", "mre_warp_inputs.h",
                     "mre_warp_input_point.h", "mre_correlate.hip", "mre_correlate.h", "mre_model.cpp", "mre_model.h", "mre_sched.cpp", "mre_env.h",
                     "mre_policy.h", "mre_launch.h"]
_LIB: Optional[C.CDLL] = None

MRE_NQ, MRE_NV, MRE_NU, MRE_NQ_PAD, MRE_NV_PAD, MRE_MAX_PROPS = 43, 39, 8, 44, 40, 4
MRE_TRACE_W = 88   # row of the parity trace (mre_set_trace): qpos, census columns, then qvel from MRE_TRACE_QVEL on
MRE_TRACE_QVEL = 48
MRE_FINAL_W = 83    # row of mre_pack_final_state: qpos[43], qvel[39], status
MRE_DYN_W = 128     # row of mre_get_arm_dynamics: jac[6][7], mass[7][7], bias[7], site pos[3] quat[4], qpos[7], qvel[7], pad

EXPORTS = [
    "mre_create", "mre_destroy", "mre_last_error", "mre_num_envs", "mre_stream", "mre_sync",
    "mre_set_props", "mre_reset", "mre_place_props", "mre_set_state", "mre_get_state", "mre_get_ctrl",
    "mre_set_warmstart", "mre_get_warmstart", "mre_set_ctrl", "mre_step", "mre_rollout", "mre_rollout_ticks",
    "mre_set_trace", "mre_osc_set_target", "mre_osc_configure", "mre_gripper_set",
    "mre_run_controller", "mre_get_sites", "mre_get_status", "mre_get_solver_stats",
    "mre_profile_enable", "mre_profile_read", "mre_set_env_id_offset", "mre_set_env_order",
    "mre_set_fallback", "mre_get_fallback_stats", "mre_get_queue_info", "mre_set_solver", "mre_get_solver", "mre_wait_stream", "mre_osc_compute", "mre_get_contacts", "mre_get_contacts_full", "mre_get_settle_steps", "mre_get_launch_info", "mre_prop_place", "mre_sort_colours", "mre_crc32c", "mre_osc_configure_env", "mre_set_env_ids", "mre_set_render_colours", "mre_render",
    "mre_get_state_f64", "mre_set_state_f64", "mre_get_time", "mre_pack_final_state",
    "mre_records_workspace_bytes", "mre_varint_pack_rows", "mre_crc32c_rows", "mre_crc32c_combine",
    "mre_varint_unpack_workspace_bytes", "mre_varint_unpack_rows", "mre_get_arm_dynamics", "mre_seg_labels",
    "mre_heightmap", "mre_warp_maps", "mre_warp_inputs", "mre_correlate_workspace", "mre_correlate",
]
# status bits of mre_varint_unpack_rows (include/mre.h)
MRE_UNPACK_LONG, MRE_UNPACK_OVERFLOW, MRE_UNPACK_TRUNCATED, MRE_UNPACK_COUNT, MRE_UNPACK_DESC = 1, 2, 4, 8, 16


class MreError(RuntimeError):
    pass


def source_hash() -> str:
    """sha256 (16 hex digits) over the DEVICE sources of libmre.so (the .hip files and their headers; not the host
    side of the C ABI, which decides how launches are issued but not what a launch executes): what a profile summary
    must have been taken on for its per-launch counters to describe the build being run (bench.py,
    tools/summarize_profiles.py)."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(f for f in _SOURCES + _HEADERS if not f.endswith(("mre_api.cpp", "mre.h"))):
        with open(os.path.join(_CSRC, f), "rb") as fh:
            h.update(f.encode() + b"\0" + fh.read())
    return h.hexdigest()[:16]


def needs_build() -> bool:
    if not os.path.exists(_SO):
        return True
    t = os.path.getmtime(_SO)
    for f in _SOURCES + _HEADERS + _UNHASHED_SOURCES:
        p = os.path.join(_CSRC, f)
        if os.path.exists(p) and os.path.getmtime(p) > t:
            return True
    return False


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP kernels + C-ABI host code for gfx950 in-tree."""
    if not force and not needs_build():
        return _SO
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    # -ffp-contract=on: a * b + c is fused where the SOURCE expression says so, not wherever the optimiser
    # finds one after unrolling -- the compact and the large instantiation of the step kernel must round
    # identically (the capacity fallback re-runs an env on the other one and promises the same bits)
    # -fno-hip-fp32-correctly-rounded-divide-sqrt: fp32 a / b and sqrtf as v_rcp_f32 / v_sqrt_f32 (about 1 ulp)
    # instead of the ten-instruction correctly rounded sequences; the fp64 finger-frame code is not affected,
    # and the parity tests against the fp64 oracle see no difference (+2 % on the Newton bench)
    base = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-ffp-contract=on",
            "-fno-hip-fp32-correctly-rounded-divide-sqrt"]
    if verbose:
        base.insert(1, "-Rpass-analysis=kernel-resource-usage")
    bdir = os.path.join(_CSRC, "_build")
    os.makedirs(bdir, exist_ok=True)
    # the step kernel is instantiated four times: {compact, large constraint capacities (mre_dev.h)}
    # x {PGS, Newton (mre_newton.h)}
    units = [("kernels", "mre_kernels.hip", []), ("kernels_large", "mre_kernels.hip", ["-DMRE_LARGE_CAPS"]),
             ("kernels_newton", "mre_kernels.hip", ["-DMRE_NEWTON"]),
             ("kernels_large_newton", "mre_kernels.hip", ["-DMRE_LARGE_CAPS", "-DMRE_NEWTON"]),
             ("render", "mre_render.hip", []), ("records", "mre_records.hip", []),
             ("labels", "mre_labels.hip", []), ("heightmap", "mre_heightmap.hip", []),
             ("warp", "mre_warp.hip", []), ("warp_inputs", "mre_warp_inputs.hip", []),
             ("correlate", "mre_correlate.hip", []), ("api", "mre_api.cpp", []),
             ("sched", "mre_sched.cpp", []), ("model", "mre_model.cpp", [])]
    procs = [(name, subprocess.Popen(base + flags + ["-c", os.path.join(_CSRC, src), "-o",
                                                     os.path.join(bdir, name + ".o")]))
             for name, src, flags in units]
    for name, pr in procs:
        if pr.wait() != 0:
            raise MreError(f"hipcc failed on translation unit {name}")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", _SO] +
                          [os.path.join(bdir, name + ".o") for name, _, _ in units])
    return _SO


def lib() -> C.CDLL:
    """Load libmre.so (never builds implicitly on a GPU box: the .so travels in-tree)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # torch first: its wheel bundles a HIP runtime of the same soname, and a process must hold ONE
    # runtime (libmre.so loaded first would bind /opt/rocm's copy and see no device once torch has
    # initialised its own)
    import torch  # noqa: F401
    so = os.environ.get("MRE_LIB", _SO)  # diagnostic builds (tools/phase_stamps.py) only
    if not os.path.exists(so):
        raise MreError(f"{so} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(the HIP extension is the only implementation of the step)")
    L = C.CDLL(so)
    vp, ci, cu, fp = C.c_void_p, C.c_int, C.c_uint, C.c_void_p
    L.mre_create.argtypes = [C.c_char_p, C.c_size_t, ci, ci, C.POINTER(vp)]
    L.mre_destroy.argtypes = [vp]
    L.mre_last_error.restype = C.c_char_p
    L.mre_num_envs.argtypes = [vp]
    L.mre_stream.restype = vp
    L.mre_stream.argtypes = [vp]
    L.mre_sync.argtypes = [vp]
    L.mre_set_props.argtypes = [vp, fp, fp]
    L.mre_reset.argtypes = [vp, fp]
    L.mre_place_props.argtypes = [vp, fp, C.c_uint64, fp, fp, ci, ci]
    L.mre_set_state.argtypes = [vp, fp, fp]
    L.mre_get_state.argtypes = [vp, fp, fp]
    L.mre_get_state_f64.argtypes = [vp, fp, fp]
    L.mre_set_state_f64.argtypes = [vp, fp, fp]
    L.mre_get_time.argtypes = [vp, fp]
    L.mre_get_ctrl.argtypes = [vp, fp]
    L.mre_set_warmstart.argtypes = [vp, fp]
    L.mre_get_warmstart.argtypes = [vp, fp]
    L.mre_set_ctrl.argtypes = [vp, fp]
    L.mre_step.argtypes = [vp, ci, cu]
    L.mre_rollout.argtypes = [vp, fp, ci, ci, cu]
    L.mre_rollout_ticks.argtypes = [vp, fp, ci, ci, cu, ci]
    L.mre_pack_final_state.argtypes = [vp, fp]
    L.mre_set_trace.argtypes = [vp, fp, ci, ci]
    L.mre_osc_set_target.argtypes = [vp, fp, fp, fp, fp, fp]
    L.mre_osc_configure.argtypes = [vp, fp, fp, fp, ci]
    L.mre_gripper_set.argtypes = [vp, fp]
    L.mre_run_controller.argtypes = [vp, ci, ci, fp]
    L.mre_get_sites.argtypes = [vp, fp, fp, fp]
    L.mre_get_status.argtypes = [vp, fp]
    L.mre_get_solver_stats.argtypes = [vp, fp]
    L.mre_set_env_id_offset.argtypes = [vp, C.c_longlong]
    L.mre_set_env_ids.argtypes = [vp, C.POINTER(C.c_longlong)]
    L.mre_set_env_order.argtypes = [vp, fp]
    L.mre_profile_enable.argtypes = [vp, ci]
    L.mre_profile_read.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(ci)]
    L.mre_set_fallback.argtypes = [vp, ci]
    L.mre_set_solver.argtypes = [vp, ci]
    L.mre_get_solver.argtypes = [vp]
    L.mre_wait_stream.argtypes = [vp, vp]
    L.mre_osc_compute.argtypes = [vp, fp, fp]
    L.mre_get_arm_dynamics.argtypes = [vp, ci, fp]
    L.mre_get_contacts.argtypes = [vp, fp, fp]
    L.mre_get_contacts_full.argtypes = [vp, ci, fp, fp]
    L.mre_get_settle_steps.argtypes = [vp, fp]
    L.mre_get_launch_info.argtypes = [vp, fp]
    L.mre_prop_place.argtypes = [vp, C.c_uint64, fp, fp, fp, ci, C.c_float, fp, fp]
    L.mre_sort_colours.argtypes = [vp, C.c_uint64, fp, fp, ci, C.c_float, fp, fp, fp, fp]
    L.mre_set_render_colours.argtypes = [vp, fp, fp]
    L.mre_render.argtypes = [vp, fp, fp, C.c_float, ci, ci, fp, fp, fp, fp]
    L.mre_osc_configure_env.argtypes = [vp, fp, fp, fp]
    L.mre_get_fallback_stats.argtypes = [vp, C.POINTER(C.c_longlong)]
    L.mre_get_queue_info.argtypes = [vp, C.POINTER(C.c_longlong)]
    sz = C.c_size_t
    L.mre_crc32c.restype = C.c_uint32
    L.mre_crc32c.argtypes = [C.c_char_p, sz]
    L.mre_crc32c_combine.restype = C.c_uint32
    L.mre_crc32c_combine.argtypes = [C.c_uint32, C.c_uint32, sz]
    L.mre_records_workspace_bytes.restype = sz
    L.mre_records_workspace_bytes.argtypes = [ci, sz]
    L.mre_varint_pack_rows.argtypes = [vp, fp, sz, sz, fp, ci, ci, fp, sz, fp, fp, fp, fp, sz]
    L.mre_crc32c_rows.argtypes = [vp, fp, sz, sz, fp, ci, ci, fp, fp, sz]
    L.mre_varint_unpack_workspace_bytes.restype = sz
    L.mre_varint_unpack_workspace_bytes.argtypes = [ci, sz]
    L.mre_varint_unpack_rows.argtypes = [vp, fp, sz, fp, fp, fp, fp, ci, sz, fp, sz, fp, fp, sz]
    L.mre_seg_labels.argtypes = [vp, fp, fp, ci, ci, ci, ci, ci, fp, fp]
    L.mre_heightmap.argtypes = [vp, fp, fp, fp, ci, ci, ci, fp, fp, C.c_float, C.c_float, ci, ci, fp, fp, fp, fp]
    L.mre_warp_maps.argtypes = [vp, fp, fp, fp, ci, ci, ci, fp, fp, ci, ci, ci, fp, fp, fp, fp]
    L.mre_warp_inputs.argtypes = [vp, fp, fp, ci, ci, ci, fp, fp, ci, ci, ci, ci, fp, fp, fp, ci, fp]
    L.mre_correlate_workspace.argtypes = [ci, ci, ci, ci, C.POINTER(sz)]
    L.mre_correlate.argtypes = [vp, fp, fp, ci, ci, ci, ci, ci, ci, ci, fp, fp, fp, fp, sz]
    for name in EXPORTS:
        if name not in ("mre_last_error", "mre_stream", "mre_crc32c", "mre_crc32c_combine",
                        "mre_records_workspace_bytes", "mre_varint_unpack_workspace_bytes"):
            getattr(L, name).restype = ci
    _LIB = L
    return L


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().mre_last_error()
        raise MreError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
