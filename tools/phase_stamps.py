"""Per-phase share of a control tick, from diagnostic builds with s_memtime stamps.

  python tools/phase_stamps.py build      # here (no GPU): tools/_diag/libmre_stamps{0,1}.so
  python tools/phase_stamps.py run [N]    # on the GPU box; MRE_LIB selects the diagnostic library
The product library never carries the stamps (MRE_PHASE_STAMPS is undefined in lib.build()).
"""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = os.path.join(ROOT, "tools", "_diag")
NAMES = ["position+crb+factor", "velocity", "collide", "assemble", "control", "smooth", "solve", "integrate+io",
         "newton: setup", "newton: direction (H, factor, solves)", "newton: direction (factor re-used)", "newton: line search + move + update",
         "  position: kinematics + comPos", "  position: (gripper_pose: merged into kinematics, round 5)", "  position: gripper_local + connect rows (fp64)", "  position: crb + factor",
         "  direction: M rows", "  direction: J'DJ on the matrix cores", "  direction: tiles to rows", "  direction: elimination, both solves, decrement",
         "  position_stage: kinematics", "  position_stage: comPos", "  (unused)", "  (unused)",
         "  collide: broad phase", "  collide: geom frames", "  collide: box-box / plane-box", "  collide: filter, prefix, write-out",
         "  search: M v, J v", "  search: line search", "  search: move, update, J'f, gradient", "  (unused)",
         # set 8 counts, it does not time: lanes per env and tick (5 steps) that took box_box's face-contact branch, those
         # whose candidates stayed in registers (mre_collide.h), and the same two over the pairs with the table
         "  collide: face contacts", "  collide: face contacts kept in registers", "  collide: table face contacts",
         "  collide: table face contacts kept in registers",
         # set 9 counts too: nw_direction calls per env and tick, and those that formed no c10 / c20 / c21 tile (cubes 0-1 x
         # robot, cubes 2-3 x robot, cubes 2-3 x cubes 0-1; an env of at most two cubes has no second group and always
         # counts under the last two)
         "  direction: calls", "  direction: calls without tile c10", "  direction: calls without tile c20",
         "  direction: calls without tile c21",
         "  setup: dense robot M", "  setup: M a, J a, J a_smooth", "  setup: constraint updates, choice of the start",
         "  setup: J'f, gradient",
         # set 11 counts: set-up calls per env and tick, and those in which qacc_smooth beat the warm start
         "  setup: calls", "  setup: calls won by qacc_smooth", "  (unused)", "  (unused)"]

if sys.argv[1] == "build":
    sys.path.insert(0, ROOT)
    from mujoco_robot_environments_amd import lib
    for k in ([int(x) for x in sys.argv[2:]] or (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)):   # the flags and units of lib.build()
        lib.compile_and_link(os.path.join(DIAG, f"libmre_stamps{k}.so"), DIAG, suffix=str(k),
                             step_extra=[f"-DMRE_PHASE_STAMPS={k}"])
elif sys.argv[1] == "run":
    if "MRE_LIB" not in os.environ:
        solver = sys.argv[3] if len(sys.argv) > 3 else "PGS"
        tot = []
        for k in ([int(x) for x in os.environ["MRE_STAMP_SETS"].split(",")] if "MRE_STAMP_SETS" in os.environ else ((0, 1, 2, 3, 4, 5) if solver == "Newton" else (0, 1, 3))):
            env = dict(os.environ, MRE_LIB=os.path.join(DIAG, f"libmre_stamps{k}.so"))
            out = subprocess.check_output([sys.executable, __file__, "run"] + sys.argv[2:], env=env, text=True)
            tot += [float(x) for x in out.split()[-4:]]
        if "MRE_STAMP_SETS" in os.environ:   # selected sets only: raw numbers
            sets = [int(x) for x in os.environ["MRE_STAMP_SETS"].split(",")]
            for q, k in enumerate(sets):
                for n, v in zip(NAMES[4 * k:4 * k + 4], tot[4 * q:4 * q + 4]):
                    print(f"{n:48s} {v:12.0f}")
            sys.exit(0)
        s = sum(tot[:12]) if solver == "Newton" else sum(tot[:8])   # (the sub-buckets repeat their parents)
        print(f"solver {solver}: cycles / 16 per env and tick (5 steps), share of the tick")
        names = NAMES if solver == "Newton" else NAMES[:8] + NAMES[12:]
        for n, v in zip(names, tot):
            print(f"{n:48s} {v:12.0f}  {100 * v / s:5.1f} %")
    else:
        sys.path.insert(0, ROOT)
        import numpy as np, torch
        import bench
        from mujoco_robot_environments_amd import rng
        from mujoco_robot_environments_amd.physics import BatchedPhysics
        N = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
        solver = sys.argv[3] if len(sys.argv) > 3 else "PGS"
        nticks = int(sys.argv[4]) if len(sys.argv) > 4 else 20
        phys = BatchedPhysics(N, solver=solver); ids = np.arange(N)
        bench.setup_envs(phys, 0, ids)
        seq = torch.from_numpy(rng.random_actions(0, ids, np.arange(nticks)).astype(np.float32)).to(phys.device).contiguous()
        acc = np.zeros(4)
        for t in range(nticks):
            phys.rollout(seq[t:t + 1], control_steps=5)
            st = np.empty((N, 4), np.int32)
            from mujoco_robot_environments_amd import lib as _lib
            _lib.check(_lib.lib().mre_get_solver_stats(phys._h, st.ctypes.data), "stats")
            acc += st.astype(np.float64).mean(axis=0)
        print(*(acc / nticks))
