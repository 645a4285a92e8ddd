"""Every entry of include/mre.h that works on an mre_env handle, called with a NULL handle, for tests/test_handle_null.py and
tests/golden/make_handle_null.py: what the entry returns and what mre_last_error() then says.

Each entry is called once with a NULL handle and otherwise plausible arguments, and -- where it has a pointer it requires --
once more with that pointer NULL as well.  An entry looks at its handle before it makes any HIP call, so no call here needs
a GPU, and none gets as far as reading the host pointer it is given.  Four entries do not refuse a NULL handle with
MRE_ERR_ARG and a text of their own: mre_num_envs (0), mre_stream (NULL), mre_destroy (MRE_OK) and mre_get_solver, whose
return value is the solver and which answers MRE_ERR_ARG all the same.
"""
import ctypes as C

_ARENA = C.create_string_buffer(1 << 12)
P = C.addressof(_ARENA)                       # a host pointer
LL = C.cast(P, C.POINTER(C.c_longlong))
PF = C.cast(P, C.POINTER(C.c_float))
PI = C.cast(P, C.POINTER(C.c_int))

# (entry, arguments after the handle, index of a required pointer among them or None)
TABLE = [
    ("mre_destroy", (), None), ("mre_num_envs", (), None), ("mre_stream", (), None), ("mre_sync", (), None),
    ("mre_set_props", (P, P), 0), ("mre_reset", (P,), None),
    ("mre_place_props", (P, 7, P, P, 100, 150), 2), ("mre_get_settle_steps", (P,), 0), ("mre_get_launch_info", (P,), 0),
    ("mre_prop_place", (7, P, P, P, 10, 0.05, P, P), 2), ("mre_sort_colours", (7, P, P, 10, 0.05, P, P, P, P), 2),
    ("mre_get_contacts", (P, P), 0), ("mre_get_contacts_full", (0, P, P), 2),
    ("mre_set_env_id_offset", (5,), None), ("mre_set_env_ids", (LL,), None),
    ("mre_set_state", (P, P), None), ("mre_get_state", (P, P), None), ("mre_pack_final_state", (P,), 0),
    ("mre_get_state_f64", (P, P), None), ("mre_set_state_f64", (P, P), None), ("mre_get_time", (P,), 0),
    ("mre_set_warmstart", (P,), 0), ("mre_get_warmstart", (P,), 0), ("mre_set_ctrl", (P,), 0), ("mre_get_ctrl", (P,), 0),
    ("mre_step", (1, 0), None), ("mre_rollout", (P, 4, 5, 0), 0), ("mre_rollout_ticks", (P, 4, 5, 0, 2), 0),
    ("mre_set_trace", (P, 1, 10), None), ("mre_osc_set_target", (P, P, P, P, P), None),
    ("mre_osc_configure", (P, P, P, 0), None), ("mre_osc_configure_env", (P, P, P), None), ("mre_gripper_set", (P,), 0),
    ("mre_run_controller", (6, 5, P), None), ("mre_osc_compute", (P, P), None), ("mre_get_arm_dynamics", (0, P), 1),
    ("mre_get_sites", (P, P, P), None), ("mre_get_status", (P,), 0), ("mre_get_solver_stats", (P,), 0),
    ("mre_set_env_order", (P,), None), ("mre_set_render_colours", (P, P), None),
    ("mre_render", (P, P, 45.0, 4, 8, P, P, P, P), 1), ("mre_set_fallback", (1,), None), ("mre_wait_stream", (None,), None),
    ("mre_set_solver", (2,), None), ("mre_get_solver", (), None), ("mre_get_fallback_stats", (LL,), 0),
    ("mre_get_queue_info", (LL,), 0), ("mre_profile_enable", (1,), None), ("mre_profile_read", (PF, PI), 1),
]


def cases():
    """[(id, entry point, argument tuple)] in a fixed order; the ids are unique."""
    out = []
    for entry, args, required in TABLE:
        out.append((f"{entry}: null handle", entry, (None,) + args))
        if required is not None:
            twice = list(args)
            twice[required] = None
            out.append((f"{entry}: null handle and null argument {required + 1}", entry, (None,) + tuple(twice)))
    assert len({c[0] for c in out}) == len(out)
    return out


def answers(L):
    """[[id, return value, message]] of ``cases()`` on the loaded library ``L``.  mre_stream's NULL is recorded as 0; a call
    that returns 0 sets no message, so its message is recorded as empty."""
    res = []
    for what, entry, args in cases():
        rc = getattr(L, entry)(*args)
        rc = 0 if rc is None else int(rc)
        res.append([what, rc, L.mre_last_error().decode() if rc else ""])
    return res
