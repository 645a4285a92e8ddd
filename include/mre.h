/* mre.h -- C ABI of the MI355X batched RearrangementEnv physics step.
 *
 * The reference exposes no FFI for this path; its hot loop sits behind two
 * Python object protocols:
 *   - dm_control ``mjcf.Physics``: .step() / .forward() / .reset() /
 *     .set_control(u) / .data.{qpos,qvel,time,site_xpos,contact}
 *     (reference: mujoco_robot_environments/models/robot_arm.py:78-79,
 *      environment/prop_initializer.py:190,221,250, tasks/rearrangement.py:302)
 *   - mujoco_controllers ``OSC`` / ``MinMax``: set_target / compute_control_output /
 *     is_converged / .status (models/robot_arm.py:71,73,83;
 *     tasks/rearrangement.py:365-370,380,422)
 * Each entry point below names the member it replaces, batched over
 * ``num_envs`` independent environments (one 64-lane wavefront per env).
 *
 * Conventions
 *   - return 0 on success, negative mre_status on error; message via
 *     mre_last_error().  No exceptions cross the boundary.
 *   - array arguments are BORROWED for the duration of the call; they may be
 *     device pointers (e.g. torch.Tensor.data_ptr()) or host pointers
 *     (copied with hipMemcpyDefault on the handle's stream).
 *   - batched arrays are env-major rows: x[env][k] (one wavefront reads one
 *     row with a single coalesced access).  fp32 on device.
 *   - one handle <-> one host thread / HIP stream; calls are asynchronous on
 *     that stream, mre_sync() / mre_get_* synchronise.
 *   - the stepping calls (mre_step, mre_rollout, mre_run_controller) cut the batch into env groups on
 *     streams of their own and return before the launches have finished; every other entry point
 *     first completes what is pending.  Results do not depend on the grouping (MRE_GROUPS=1 in the
 *     environment: a stepping call completes before it returns).  ctrl_seq of mre_rollout is copied
 *     at the call; it need not outlive it.
 */
#ifndef MRE_H
#define MRE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MRE_NQ 43      /* 7 arm + 8 gripper + 4 x 7 free-joint coordinates */
#define MRE_NV 39
#define MRE_NU 8       /* 7 arm motors + fingers_actuator */
#define MRE_NQ_PAD 44  /* row stride of qpos arrays */
#define MRE_TRACE_W 88 /* row of the parity trace (mre_set_trace) */
#define MRE_TRACE_QVEL 48 /* first qvel column of a trace row */
#define MRE_NV_PAD 40  /* row stride of qvel / qacc arrays */
#define MRE_MAX_PROPS 4

typedef enum {
  MRE_OK = 0,
  MRE_ERR_ARG = -1,
  MRE_ERR_MODEL = -2,   /* blob malformed or topology differs from the compiled kernels */
  MRE_ERR_HIP = -3,
  MRE_ERR_NOGPU = -4
} mre_status;

/* per-env status bits (mre_get_status); the reference raises exceptions instead
 * (tasks/rearrangement.py:371-440, dm_control PhysicsError) */
#define MRE_ST_NOT_CONVERGED 1u   /* arm outside OSC thresholds after run_controller */
#define MRE_ST_NAN 2u             /* non-finite state detected */
#define MRE_ST_CONTACT_OVERFLOW 4u /* contact / constraint-row capacity exceeded */
#define MRE_ST_NOT_SETTLED 8u     /* PropPlacer: cubes still moving after max_settle_physics_time (2 s) in each of the
                                   * max_settle_physics_attempts (10) placements (prop_initializer.py:240-283) */
#define MRE_ST_PLACEMENT_FAILED 16u /* PropPlacer: no collision-free pose for one of the env's cubes within
                                   * max_attempts_per_prop (_REJECTION_SAMPLING_FAILED, prop_initializer.py:230-233) */

typedef struct mre_env mre_env;

/* mjcf.Physics.from_mjcf_model (tasks/rearrangement.py:181): model_blob is the
 * output of mujoco_robot_environments_amd.model.compile.to_blob(). */
int mre_create(const void* model_blob, size_t nbytes, int num_envs, int device_id, mre_env** out);
int mre_destroy(mre_env*);
const char* mre_last_error(void);
int mre_num_envs(const mre_env*);
/* raw HIP stream of the handle (hipStream_t as void*) for event timing */
void* mre_stream(mre_env*);
int mre_sync(mre_env*);

/* per-env scene parameters: number of cubes (2..4, environment/props.py:604-607)
 * and half sizes [N][4][3] (colour_splitter.yaml:3-4) */
int mre_set_props(mre_env*, const int32_t* nprops, const float* prop_half_size);

/* Physics.reset() + arm.set_joint_angles(home) (tasks/rearrangement.py:302-306):
 * qpos = qpos0 with arm at home, qvel = 0, warm start = 0, time = 0.
 * mask [N] (host or device, may be NULL = all). Props are parked; use
 * mre_place_props() for PropPlacer. */
int mre_reset(mre_env*, const uint8_t* mask);
/* PropPlacer.__call__ (environment/prop_initializer.py:164-283).  Props are placed one index at a
 * time over the batch: pose ~ U(workspace), yaw = pi U(0,1), rejected while the prop has ANY detected
 * contact (physics.data.contact: dist < margin) with a geom other than the table -- placed props
 * and robot geoms alike (:121-140), at most max_attempts draws per prop (beyond: the reference raises
 * for its one env; here THAT env gets MRE_ST_PLACEMENT_FAILED and the others carry on).  Then the
 * physics settles with the robot frozen; every env stops by itself once max|qvel| < 1e-3 and
 * max|qacc| < 1e-2 after at least settle_steps steps (:240-258: 0.3 s), at most 2 s; an env still moving
 * then is placed again from fresh draws, up to 10 times (max_settle_physics_attempts), then flagged
 * MRE_ST_NOT_SETTLED.  mre_get_settle_steps: steps each env took in its last settle (negative: not settled). */
int mre_place_props(mre_env*, const uint8_t* mask, uint64_t seed, const float* ws_min,
                    const float* ws_max, int max_attempts, int settle_steps);
int mre_get_settle_steps(mre_env*, int32_t* steps);
/* Per-env record of the last stepping launch, info [N][4] int32: {1: overflowed the compact capacities (the library
 * has re-run the env on the large kernel by the time this returns), 2: overflowed the large ones (MRE_ST_OVERFLOW),
 * 0: neither, -1: the env was not part of the launch, max contacts | the env's own duration << 16 (clock ticks >> 10; the key of
 * the longest-first dispatch of the next launch), max constraint rows, max robot rows | max cube-cube
 * contacts << 16} over the launch's steps.  Diagnostics; nothing in the reference corresponds to it. */
int mre_get_launch_info(mre_env*, int32_t* info);

/* prop_place (tasks/rearrangement.py:597-665), batched and on the device (one wave per env runs its
 * own attempt loop; the physics state is left alone, the reference works on a deepcopy).  Env i looks
 * for a pose of cube prop[i] (< 0: nothing asked) in [bounds[i][0:3], bounds[i][3:6]] (min_pose /
 * max_pose) with orientation mju_mat2Quat(Ry(180 deg)); draw t is keyed by (seed, global env id,
 * tick[i] + t); a pose is rejected while a detected contact (dist < margin) of the cube with a geom
 * other than the table has dist <= max_dist (:623: 0.05).  pose [N][7] (xyz, quat wxyz, fp64),
 * attempts [N]: draws used, 0 = nothing asked, < 0 = none accepted within max_attempts (the
 * reference raises "Failed to find collision free place pose.").  All arrays host or device. */
int mre_prop_place(mre_env*, uint64_t seed, const int32_t* prop, const double* bounds, const int32_t* tick,
                   int max_attempts, float max_dist, double* pose, int32_t* attempts);
/* sort_colours (tasks/rearrangement.py:700-751) for every env, on the device: the first cube (prop
 * order) outside its colour's zone (zones [N][4][4]: lo x, lo y, hi x, hi y per cube), prop_pick for
 * it (:579-595) and prop_place inside the zone at z = 0.4 (keys: seed + 1, ticks call_counts[i] * 10000
 * + t).  which [N]: the selected cube or -1 (all sorted: pick / place rows unspecified); pick, place
 * [N][7] fp64; attempts as in mre_prop_place. */
int mre_sort_colours(mre_env*, uint64_t seed, const int32_t* call_counts, const double* zones, int max_attempts,
                     float max_dist, int32_t* which, double* pick, double* place, int32_t* attempts);
/* physics.forward() + physics.data.contact (prop_initializer.py:123-139, tasks/rearrangement.py:
 * 612-627): every contact the narrow phase DETECTS on the current poses (dist < margin; the solver
 * only uses those with dist < margin - gap).  count[N] (negative: list cut at -count),
 * contacts[N][MRE_MAX_CONTACTS][3] = (geom1, geom2, dist), host or device pointers. */
#define MRE_MAX_CONTACTS 32
int mre_get_contacts(mre_env*, int32_t* count, float* contacts);
/* The whole contact record (physics.data.contact[i].pos / .frame / .dist / .geom1 / .geom2) of the same launch:
 * contacts[N][MRE_MAX_CONTACTS][15] = pos[3], frame[9] (normal from geom1 to geom2, then the two tangents), dist,
 * geom1, geom2; rows past the count are zero.  active_only = 0: every detected contact (dist < margin), the list of
 * mre_get_contacts.  active_only = 1: the list the next step's solve would be given (dist < margin - gap; the narrow
 * phase runs with that threshold, as it does inside a step).  count[N]: rows filled; negative: the list was cut
 * (more than MRE_MAX_CONTACTS contacts, or the kernel's contact capacity exceeded) and holds the first -count. */
int mre_get_contacts_full(mre_env*, int active_only, int32_t* count, float* contacts);
/* global id of env 0 of this handle (rank r of a sharded batch: r * num_envs); random
 * draws are keyed by global id so results do not depend on the sharding */
int mre_set_env_id_offset(mre_env*, long long offset);
/* explicit global ids [N] instead of offset + index (NULL = back to the offset form): lets several
 * envs share one id, i.e. one scene -- a population of controllers on the same scene replicates */
int mre_set_env_ids(mre_env*, const long long* ids);

/* physics.bind(joints).qpos / .qvel access: rows [N][MRE_NQ_PAD] / [N][MRE_NV_PAD] */
int mre_set_state(mre_env*, const float* qpos, const float* qvel);
int mre_get_state(mre_env*, float* qpos, float* qvel);
/* the same state as ONE packed row per env, written on the device: out[N][MRE_FINAL_W] (device pointer) = qpos[43],
 * qvel[39], status (exact in a float).  north_star's "end-of-rollout gather": the block a rank hands to
 * all_gather_into_tensor without a host round trip (mujoco_robot_environments_amd/distributed.py).  Enqueued on the
 * handle's stream; order other streams with mre_sync / stream events. */
#define MRE_FINAL_W 83
int mre_pack_final_state(mre_env*, float* out);
/* the same state as the reference holds it (physics.data.qpos / .qvel are float64): rows [N][MRE_NQ] /
 * [N][MRE_NV] of doubles, HOST pointers.  On the device every coordinate is a double-float pair (the float32 row
 * entry + a low-order word): the robot's 15 joints because the soft closures of the 2F-85 four-bars amplify a float32
 * rounding of the state past the 1e-4 parity bar within 1000 steps, the cubes' poses and velocities (round 4) because
 * the envs whose reference trajectory amplifies a difference a hundredfold do the same to a float32 random walk of a
 * cube.  mre_set_state (float rows) clears the low-order words. */
int mre_get_state_f64(mre_env*, double* qpos, double* qvel);
int mre_set_state_f64(mre_env*, const double* qpos, const double* qvel);
/* physics.data.time (models/robot_arm.py:68-69): seconds of physics since the last mre_reset, per env, host [N] */
int mre_get_time(mre_env*, double* time);
int mre_set_warmstart(mre_env*, const float* qacc_warmstart);
int mre_get_warmstart(mre_env*, float* qacc_warmstart);
/* Physics.set_control(u) (models/robot_arm.py:78): rows [N][MRE_NU] */
int mre_set_ctrl(mre_env*, const float* ctrl);
/* physics.bind(arm_actuators).ctrl (tasks/lasa_draw.py:349): the controls last applied, rows [N][MRE_NU]
 * (after mre_run_controller: the OSC torques and gripper command of its last tick) */
int mre_get_ctrl(mre_env*, float* ctrl);
/* Physics.step() x nsubsteps with ctrl held (models/robot_arm.py:77-81);
 * dm_control legacy order step2->step1 is preserved (results identical to
 * nsubsteps reference steps).  flags: bit0 = disable constraints (test only),
 * bit1 = freeze robot joints (JointStaticIsolator, prop_initializer.py:246). */
int mre_step(mre_env*, int nsubsteps, unsigned flags);
/* fused rollout: T control ticks, ctrl_seq[T][N][MRE_NU] resampled per tick,
 * control_steps physics steps per tick (BASELINE config 2: random actions). */
int mre_rollout(mre_env*, const float* ctrl_seq, int nticks, int control_steps, unsigned flags);
/* the same T ticks cut into launches of `ticks_per_launch` ticks (<= 0: the library's cut = mre_rollout: one launch, or --
 * when the batch exceeds the GPU's wave slots -- queue launches of <= 200 ticks / per-tick launches for a short window:
 * mre_get_queue_info), all enqueued by this
 * one call: the reference's loop `for tick: set_control; 5 x step` (models/robot_arm.py:69-81) with the host out of it.
 * Results do not depend on the cut (tests/test_gpu_properties.py). */
int mre_rollout_ticks(mre_env*, const float* ctrl_seq, int nticks, int control_steps, unsigned flags,
                      int ticks_per_launch);
/* optional trajectory capture for parity tests: qpos AND qvel (physics.bind(joints).qpos / .qvel,
 * models/robot_arm.py:40,48; environment/prop_initializer.py:247-252) of the first `nenv` envs
 * after every physics step -> out[step][nenv][MRE_TRACE_W] (device): columns 0..42 qpos, 43 the constraint census
 * the step's solve saw (active contacts + 64 * bit mask of the joints at a limit), 44 a 22-bit hash of the geom pairs
 * those contacts belong to (a contact that opens while another closes leaves the count unchanged), 45 a hash of the
 * solution's per-row state, 46..47 zero, MRE_TRACE_QVEL..MRE_TRACE_QVEL + 38 qvel, the last column zero.
 * Pass NULL to disable. Applies to subsequent mre_step / mre_rollout / mre_run_controller. */
int mre_set_trace(mre_env*, float* out, int nenv, int max_steps);

/* OSC.set_target(position=, velocity=, quat=, angular_velocity=) -- any NULL keeps
 * the previous value (tasks/rearrangement.py:365-375); rows [N][3|4]; mask [N] or NULL */
int mre_osc_set_target(mre_env*, const float* pos, const float* quat, const float* vel,
                       const float* angvel, const uint8_t* mask);
/* OSC gains/thresholds (config/robots/arm/controller_config/osc.yaml:5-22):
 * gains[6] = kp_pos,kd_pos,kp_ori,kd_ori,kp_null,kd_null; null_q[7]; thresholds[2] */
int mre_osc_configure(mre_env*, const float* gains, const float* null_q, const float* thresholds,
                      int pinv_always);
/* one parameter set PER ENV (gains [N][6] = kp/kd position, orientation, nullspace; null_q [N][7];
 * thr [N][2]; NULL = the shared set's values): a population of controllers evaluated as one batch,
 * the batched form of automated_controller_tuning/rearrangement_controller_tuning.py:144-197
 * (`controller_gains = {...}` per candidate).  mre_osc_configure returns to one shared set. */
int mre_osc_configure_env(mre_env*, const float* gains, const float* null_q, const float* thr);
/* MinMax.status = "max"/"min" (tasks/rearrangement.py:380,422): closed[N] 1 -> 255, 0 -> 0 */
int mre_gripper_set(mre_env*, const uint8_t* closed);
/* RobotArm.run_controller(duration) (models/robot_arm.py:61-94): nticks control
 * ticks of (OSC + MinMax command, control_steps physics steps); converged_out[N]
 * (uint8, device or host, may be NULL) = arm_converged flag.  A phase is cut into launches of 100 ticks (queue launches:
 * mre_get_queue_info) or 50 ticks (env groups); the converged flag carries over, results do not depend on the cut. */
int mre_run_controller(mre_env*, int nticks, int control_steps, uint8_t* converged_out);

/* OSC.compute_control_output() and MinMax.compute_control_output() (models/robot_arm.py:71,73)
 * on the CURRENT state, without stepping: tau[N][7] arm torques (host or device, may be NULL),
 * grip[N] gripper command (may be NULL).  The commands are also left in the ctrl rows. */
int mre_osc_compute(mre_env*, float* tau, float* grip);

/* physics.data.site_xpos[pinch] (models/robot_arm.py:55-58), controller site pose,
 * prop poses (props_info, tasks/rearrangement.py:245-246): rows [N][3], [N][7], [N][4][7] */
#define MRE_DYN_W 128
/* mj_jacSite / mj_fullM / qfrc_bias of the arm on the CURRENT state, no stepping: out = device pointer
 * [N][MRE_DYN_W]; site 0 = controller (attachment) site, 1 = pinch site.  Enqueued on the handle's stream
 * after outstanding launches are drained; no host synchronisation.  Row of one env, float32 -- the very
 * numbers the in-kernel law (csrc/mre_osc.h) works with:
 *   [0:42)    jac[6][7] of the site over the 7 arm dofs, rows 0-2 jacp, rows 3-5 jacr
 *   [42:91)   mass[7][7], the arm block of the full mass matrix (reflected gripper inertia included), dense
 *   [91:98)   qfrc_bias of the arm dofs
 *   [98:101)  site_xpos            [101:105) site quaternion, wxyz
 *   [105:112) arm qpos             [112:119) arm qvel            [119:128) zero
 * Nothing but out is written: state, warm start, ctrl, status and time are as before the call, and the rows
 * are the same whichever solver the handle runs.  MRE_ERR_ARG: null handle, null / host / misaligned (8 bytes)
 * out, another site value. */
int mre_get_arm_dynamics(mre_env*, int site, float* out);
int mre_get_sites(mre_env*, float* tcp_pos, float* eef_pose, float* prop_pose);
int mre_get_status(mre_env*, uint32_t* status);
/* telemetry: per-env [active contacts, constraint rows, solver iterations (PGS sweeps / Newton
 * iterations in the low byte, Newton: Hessian factorisations << 8), active limit rows] of the last step */
int mre_get_solver_stats(mre_env*, int32_t* stats);

/* dispatch order: workgroup b of the step kernel advances env order[b] (a permutation of
 * 0..N-1, host or device pointer; NULL = identity).  Lock-step batches end with their slowest
 * env, so callers may put envs with many constraint rows first (see mre_get_solver_stats). */
int mre_set_env_order(mre_env*, const int32_t* order);

/* Batched overhead camera (replaces the mujoco.Renderer passes of
 * tasks/rearrangement.py:254-280, 460-478, 500-530): one ray per pixel against the scene's ground
 * plane, table, cubes and robot box hulls, for the CURRENT state of every env (mask: NULL = all).
 *   cam_pos[3], cam_mat[9]  camera frame -> world (row-major; MuJoCo cameras look along -z, y up)
 *   rgb   device u8  [N][H][W][3] or NULL     (flat-shaded approximation of MuJoCo's lighting)
 *   depth device f32 [N][H][W]    or NULL     (distance along the optical axis [m]; 100 = nothing hit)
 *   seg   device u8  [N][H][W]    or NULL     (geom index: 0 ground, 1 table, 2..11 robot hulls,
 *                                              12 + p cube p; 255 = nothing hit)
 * width must be a multiple of 4 and at most 1280, height at least 1, 0 < fovy_deg < 180; depth must be 16-byte
 * aligned, rgb and seg 4-byte aligned (MRE_ERR_ARG otherwise, nothing is written).  Enqueued on the handle's stream.
 * Colours: cube albedo per env [N][4][3] u8 and the other geoms' albedo [20][3] floats, one row per geom (NULL keeps
 * the current / default grey). */
int mre_set_render_colours(mre_env*, const uint8_t* prop_rgb, const float* geom_rgb);
int mre_render(mre_env*, const float* cam_pos, const float* cam_mat, float fovy_deg, int height, int width,
               uint8_t* rgb, float* depth, uint8_t* seg, const uint8_t* mask);

/* Constraint capacities.  The library holds the step kernel in two capacity sets
 * (csrc/mre_dev.h): compact (32 contacts / 112 rows / 62 robot rows / 8 cube-cube contacts, 8
 * workgroups per CU) and large (44 / 148 / 83 / 16, 6 per CU).  By default every launch runs each
 * env on the compact kernel, re-runs from the saved pre-launch state on the large kernel the envs
 * that overflowed it, and keeps them there until their contact set has shrunk again -- results
 * never depend on the compact capacities, and MRE_ST_CONTACT_OVERFLOW reports an overflow of the
 * LARGE ones only.  mre_set_fallback(mode): 1 = the above (default); 0 pins all envs to the compact
 * kernel (status then reports compact overflows; profiling and capacity tests); 2 pins all envs to
 * the large kernel (the run the fallback must reproduce bit for bit).  Stats: out4 = {envs currently on the large
 * kernel, env launches re-run so far, promotions, demotions}. */
int mre_set_fallback(mre_env*, int mode);

/* Constraint solver (mjOption.solver; MuJoCo's enum values).  The model blob's `opt_solver`
 * selects it at mre_create; the reference leaves MuJoCo's default, Newton
 * (tasks/rearrangement.py:77-80 sets timestep / gravity / nconmax / njmax only), BASELINE.json's
 * north_star prescribes PGS.  Both are built; mre_set_solver switches a live handle (the state,
 * warm start included, carries over). mre_get_solver returns the current value.
 *
 * Friction cone (mjOption.cone): the blob's `opt_cone`, 0 = pyramidal (MuJoCo's default: the reference's PushEnv /
 * LasaDrawEnv models, which set neither cone nor impratio), 1 = elliptic (the rearrangement and base scenes inherit it
 * from the 2F-85's model).  Blobs without the entry are elliptic.  Both cones are built into both solvers. */
/* Stream ordering with the caller's own stream: device buffers handed to the library (controls,
 * control sequences, trace buffers) are consumed on the handle's stream (mre_stream); when another
 * stream produced them, mre_wait_stream(h, that_stream) makes every later launch of the handle wait
 * for the work already enqueued there (hipEventRecord + hipStreamWaitEvent; stream = hipStream_t,
 * NULL = the legacy default stream).  The caller keeps the buffers alive until mre_sync. */
int mre_wait_stream(mre_env*, void* stream);

/* CRC-32C (Castagnoli) of a host buffer -- TFRecord framing of the episode shards
 * (transporter_network_data_generation.py:103-111; mujoco_robot_environments_amd/dataset.py) */
uint32_t mre_crc32c(const void* data, size_t nbytes);

/* Episode records on the device (csrc/mre_records.hip): the two per-byte stages of the shard writer
 * (dataset.py), for frames that are already in device memory.  Both calls read `rows` rows of row_bytes bytes (1 ..
 * 2^30) from src [src_rows][row_stride]: row r is source row rows_idx[r] (device int32 [rows]; an index outside
 * 0 .. src_rows - 1 is clamped, never followed) or source row r when rows_idx is NULL.  Everything is enqueued on
 * `stream` (hipStream_t, NULL = the legacy default stream) of the current device; nothing synchronises.  All pointers
 * but the stream are device pointers; workspace holds mre_records_workspace_bytes(rows, row_bytes) bytes (0 = bad
 * arguments) and may be reused by the next call on the same stream.
 *
 * mre_varint_pack_rows: every byte as a protobuf varint (v < 128: one byte v; otherwise (v & 0x7f) | 0x80, then
 * v >> 7) -- the packed int64_list TFDS stores a uint8 tensor as.
 *   out   the packed rows, contiguous, in row order; out_capacity must cover the worst case 2 * rows * row_bytes
 *         (MRE_ERR_ARG otherwise, nothing is launched).  NULL = sizing pass: only off and len are written.
 *   off   int64 [rows] offset of each row in out (one call over 8192 frames of 480 x 640 x 3 emits up to 15 GB)
 *   len   uint32 [rows] packed length of each row
 *   crc   uint32 [rows] CRC-32C of each row's packed bytes, in the form mre_crc32c returns
 * mre_crc32c_rows: crc [rows] = CRC-32C of each row's bytes as they are (a float32 frame is a packed float_list). */
size_t mre_records_workspace_bytes(int rows, size_t row_bytes);
int mre_varint_pack_rows(void* stream, const uint8_t* src, size_t row_stride, size_t row_bytes,
                         const int32_t* rows_idx, int src_rows, int rows, uint8_t* out, size_t out_capacity,
                         int64_t* off, uint32_t* len, uint32_t* crc, void* workspace, size_t workspace_bytes);
int mre_crc32c_rows(void* stream, const uint8_t* src, size_t row_stride, size_t row_bytes,
                    const int32_t* rows_idx, int src_rows, int rows, uint32_t* crc, void* workspace,
                    size_t workspace_bytes);
/* The reader's side: mre_varint_unpack_rows is the inverse of mre_varint_pack_rows for rows as a shard holds them.  A
 * record stores a step field as ONE list over all steps, so row r is a whole list: the packed bytes
 * src[src_off[r] .. + src_len[r]) of one device buffer of src_bytes bytes (the file), nvalues[r] values expected, written
 * as uint8 to out[out_off[r] .. + nvalues[r]).  The four descriptors are device int64 [rows]; rows may differ in length
 * and sit at any byte offset; their out ranges must not overlap (not checked).  max_src_len is the host's bound on
 * src_len[] (1 .. 2^31): it sizes the grid and the workspace, mre_varint_unpack_workspace_bytes(rows, max_src_len)
 * bytes (0 = bad arguments).  Enqueued on `stream` like the calls above; nothing synchronises; MRE_ERR_ARG with nothing
 * launched when an argument the host can check is bad.
 *
 * The bytes and the descriptors are outside input and are never followed: status[r] (device uint32 [rows]) is 0 for a
 * row decoded in full, otherwise a set of the MRE_UNPACK_* bits, and the call still returns MRE_OK -- the data is bad,
 * not the arguments.  Whatever they hold, no byte outside src[0 .. src_bytes) is read, no byte outside a row's own out
 * range is written (a row with more values than nvalues[r] is clipped), and the other rows are decoded correctly.
 * Only what TFDS and this library's writer emit for a uint8 tensor is decoded: one or two bytes per value, the second
 * 0 or 1.  Legal protobuf that neither emits -- a varint of three bytes or more, a non-canonical zero such as 80 80 00
 * among them -- is flagged, not decoded (80 00 decodes to 0 unflagged); such lists stay with the host reader. */
#define MRE_UNPACK_LONG 1        /* two consecutive bytes with the high bit set: a varint longer than two bytes */
#define MRE_UNPACK_OVERFLOW 2    /* a second byte above 1: the value does not fit a byte */
#define MRE_UNPACK_TRUNCATED 4   /* the row ends in a byte with the high bit set */
#define MRE_UNPACK_COUNT 8       /* the row holds a number of values other than nvalues[r] */
#define MRE_UNPACK_DESC 16       /* the descriptor points outside src or out, or src_len[r] > max_src_len: nothing of
                                  * the row is read or written */
size_t mre_varint_unpack_workspace_bytes(int rows, size_t max_src_len);
int mre_varint_unpack_rows(void* stream, const uint8_t* src, size_t src_bytes, const int64_t* src_off,
                           const int64_t* src_len, const int64_t* nvalues, const int64_t* out_off, int rows,
                           size_t max_src_len, uint8_t* out, size_t out_capacity, uint32_t* status, void* workspace,
                           size_t workspace_bytes);
/* CRC-32C of A || B from the CRCs of A and B and the length of B (host arithmetic, no data is read):
 * crc_a * x^(8 len_b) mod P xor crc_b over the reflected Castagnoli polynomial. */
uint32_t mre_crc32c_combine(uint32_t crc_a, uint32_t crc_b, size_t len_b);

/* Frame labels on the device (csrc/mre_labels.hip): what props_info takes from a segmentation image
 * (get_bbox, tasks/rearrangement.py:254-268), for every env and every label id0 .. id0 + nid - 1 in one pass.
 *   seg    device u8  [n][height][width], contiguous, at any byte alignment (what mre_render writes, or a view of it)
 *   depth  device f32 [n][height][width] or NULL, 4-byte aligned; finite and non-negative, which is what mre_render
 *          writes -- negative, infinite or NaN depths are not supported (zmin is then unspecified)
 *   stats  device int64 [n][nid][7]: {xmin, ymin, xmax, ymax, count, sum_x, sum_y} over the pixels of env e whose seg byte
 *          is id0 + k (x = column, y = row): the PASCAL-VOC box, the visible pixel count, and the centroid's numerators
 *   zmin   device f32 [n][nid]: the smallest depth among those pixels; NULL if and only if depth is NULL
 * A label with no pixel gives {-1, -1, -1, -1, 0, 0, 0} and zmin = +inf.  Every output element is written by the call;
 * the caller initialises nothing.  All arithmetic is integer (zmin: a minimum), so the outputs are the same bits on
 * every run.  Enqueued on `stream` (hipStream_t, NULL = the legacy default stream) of the current device; nothing
 * synchronises; no byte outside seg[0 .. n * height * width) and depth[0 .. n * height * width) is read.
 * MRE_ERR_ARG, with nothing launched, unless n >= 0 (0: MRE_OK, nothing launched), height and width >= 1,
 * height * width < 2^31, 1 <= nid <= 8, id0 >= 0, id0 + nid <= 256, seg and stats non-NULL device pointers (stats 8-byte
 * aligned), depth and zmin both NULL or both 4-byte aligned device pointers. */
int mre_seg_labels(void* stream, const uint8_t* seg, const float* depth, int n, int height, int width, int id0, int nid,
                   int64_t* stats, float* zmin);

/* Orthographic heightmaps on the device (csrc/mre_heightmap.hip): the top-down height, colour and label
 * maps a Transporter network is trained on, from the frames of mre_render (or any frames of that layout).
 *   depth  device f32 [n][height][width], 4-byte aligned      rgb  device u8 [n][height][width][3] or NULL
 *   seg    device u8  [n][height][width] or NULL
 *   cam    HOST f32 [12]: A row-major, then the camera position pos; A = -R K^-1 (pixel_2_world,
 *          tasks/rearrangement.py:505-531), formed in float64 and rounded once
 *   bounds HOST f32 [6]: lo[3], hi[3] of the box the map covers; cells are 1 / inv_cell wide
 * For env e and pixel (u, v) with depth d, in float32 with every operation rounded on its own (no fused multiply-add):
 *   t0 = A[k][0]*u;  t1 = A[k][1]*v;  s = t0 + t1;  s = s + A[k][2];  m = d*s;  P[k] = pos[k] + m      (k = 0, 1, 2)
 *   cx = floorf((P[0] - lo[0]) * inv_cell)      cy = floorf((P[1] - lo[1]) * inv_cell)      hz = P[2] - lo[2]
 *   valid  <=>  d > 0  &&  d < max_depth  &&  0 <= cx < out_w  &&  0 <= cy < out_h  &&  lo[2] <= P[2] <= hi[2]
 * (NaN and infinite depths are not valid).  Cell (row cy, column cx) takes the valid pixel with the largest hz, among
 * equal hz the smallest index v * width + u:
 *   hmap  device f32 [n][out_h][out_w]     hz                  0.0f where no pixel landed
 *   cmap  device u8  [n][out_h][out_w][3]  the pixel's rgb     0, 0, 0        NULL if and only if rgb is NULL
 *   smap  device u8  [n][out_h][out_w]     the pixel's seg     255            NULL if and only if seg is NULL
 *   src   device i32 [n][out_h][out_w]     the pixel's index   -1             or NULL
 * A filled cell may hold hz = 0.0: src tells filled from empty.  Every element of every non-NULL output is written by
 * the call and nothing else is; no byte outside the n images is read; the outputs are the same bits on every run.
 * Enqueued on `stream` (hipStream_t, NULL = the legacy default stream) of the current device; nothing synchronises.
 * MRE_ERR_ARG, with nothing launched, unless n >= 0 (0: MRE_OK, nothing launched), height and width >= 1,
 * height * width < 2^31, 1 <= out_h, out_w <= 4096, inv_cell > 0 and max_depth > 0 (finite), cam and bounds non-NULL,
 * lo <= hi (finite), depth and hmap non-NULL 4-byte-aligned device pointers, cmap NULL exactly when rgb is, smap NULL
 * exactly when seg is, src NULL or a 4-byte-aligned device pointer. */
int mre_heightmap(void* stream, const float* depth, const uint8_t* rgb, const uint8_t* seg, int n, int height, int width,
                  const float* cam, const float* bounds, float inv_cell, float max_depth, int out_h, int out_w,
                  float* hmap, uint8_t* cmap, uint8_t* smap, int32_t* src);

/* The same maps from several cameras in one pass (csrc/mre_heightmap_views.hip): the pixels of `views`
 * views compete for the cells of one set of maps, so that what one camera cannot see another fills in.
 *   depth, rgb, seg  HOST arrays of `views` device pointers, view i holding n frames [n][height[i]][width[i]] with the
 *                    layouts and alignments of mre_heightmap; rgb and seg may be NULL, and when one is given every one
 *                    of its `views` entries is non-NULL
 *   height, width    HOST i32 [views]: the views may differ in size
 *   cam              HOST f32 [views][12]: cam of mre_heightmap for every view
 *   bounds, inv_cell, max_depth, out_h, out_w: those of mre_heightmap, shared by all views
 * Per pixel of every view the statement of mre_heightmap holds word for word.  Cell (row cy, column cx) of env e takes
 * the valid pixel with the largest hz over all views, among equal hz the one of the smallest view index i, inside that
 * view the smallest index v * width[i] + u.  Equivalently: the result is the merge of the `views` single-view maps of
 * mre_heightmap -- per cell the largest hz among the views that filled it, the lowest view among equal hz.
 *   hmap, cmap, smap, src  as mre_heightmap's, with the same values for an empty cell; src is the index inside the
 *                    winning view's image; cmap NULL if and only if rgb is NULL, smap NULL if and only if seg is NULL
 *   view   device u8 [n][out_h][out_w]     the winning view    255            or NULL
 * With views == 1 every output it shares with mre_heightmap equals that call's bit for bit.  Every element of every
 * non-NULL output is written exactly once by the call and nothing else is; no byte outside the views' images is read; the
 * outputs are the same bits on every run; no global atomics, no init pass, no workspace.  Enqueued on `stream` of the
 * current device; nothing synchronises.
 * MRE_ERR_ARG, with nothing launched, unless 1 <= views <= MRE_HM_MAX_VIEWS, the conditions of mre_heightmap hold for
 * every view and for the shared arguments, every height[i] * width[i] < 2^28 (view and index then fit the low word of
 * one 64-bit key, and no key is 0), and view is NULL or a device pointer.  n == 0: MRE_OK, nothing launched. */
#define MRE_HM_MAX_VIEWS 8
int mre_heightmap_views(void* stream, int views, const float* const* depth, const uint8_t* const* rgb,
                        const uint8_t* const* seg, int n, const int32_t* height, const int32_t* width, const float* cam,
                        const float* bounds, float inv_cell, float max_depth, int out_h, int out_w, float* hmap,
                        uint8_t* cmap, uint8_t* smap, int32_t* src, uint8_t* view);

/* Warped and cropped maps on the device (csrc/mre_warp.hip): a nearest-neighbour affine gather of the
 * maps of mre_heightmap (or any maps of that layout) -- the SE(2) perturbation and the rotated pick crops of a Transporter
 * training sample are both calls of it.
 *   hmap   device f32 [n][in_h][in_w], 4-byte aligned          cmap  device u8 [n][in_h][in_w][3] or NULL
 *   smap   device u8  [n][in_h][in_w] or NULL
 *   index  device i32 [samples]: the source map of sample s; NULL = s itself (then samples <= n)
 *   mats   device f32 [samples][6]: M row-major (2 x 3), OUTPUT cell (column, row, 1) -> SOURCE cell (column, row)
 * For sample s, output row r and column c, in float32 with every operation rounded on its own (no fused multiply-add):
 *   a = M[0]*c;  b = M[1]*r;  x = a + b;  x = x + M[2];  x = x + 0.5f;  fx = floorf(x)
 *   a = M[3]*c;  b = M[4]*r;  y = a + b;  y = y + M[5];  y = y + 0.5f;  fy = floorf(y)
 *   valid  <=>  0 <= e < n  &&  fx >= 0  &&  fx < in_w  &&  fy >= 0  &&  fy < in_h      (e = index[s], or s)
 * (fx, fy compared as floats, before any conversion: NaN, infinite or huge matrix entries are not valid; an index
 * outside [0, n) makes the whole sample invalid).  A valid cell copies source cell (row (int)fy, column (int)fx) of map e:
 *   out_h_  device f32 [samples][out_h][out_w]     its height            0.0f where not valid
 *   out_c   device u8  [samples][out_h][out_w][3]  its colour            0, 0, 0       NULL if and only if cmap is NULL
 *   out_s   device u8  [samples][out_h][out_w]     its label             255           NULL if and only if smap is NULL
 *   from    device i32 [samples][out_h][out_w]     (int)fy * in_w + (int)fx   -1       or NULL
 * Every element of every non-NULL output is written exactly once by the call and nothing else is; no byte outside the n
 * maps, index and mats is read; the outputs are the same bits on every run.  A row of 4 cells is stored at once when
 * out_w is a multiple of 4, out_h_ and from are 16-byte aligned and out_c and out_s 4-byte aligned; any other width or
 * byte offset is stored element by element, with the same result.  Enqueued on `stream` (hipStream_t, NULL = the legacy
 * default stream) of the current device; nothing synchronises.
 * MRE_ERR_ARG, with nothing launched, unless n >= 0 and samples >= 0 (either 0: MRE_OK, nothing launched),
 * 1 <= in_h, in_w, out_h, out_w <= 4096, hmap, mats and out_h_ non-NULL 4-byte-aligned device pointers, out_c NULL exactly
 * when cmap is, out_s NULL exactly when smap is, index and from NULL or 4-byte-aligned device pointers, samples <= n when
 * index is NULL, and no output byte range overlaps an input byte range (the maps, index, mats). */
int mre_warp_maps(void* stream, const float* hmap, const uint8_t* cmap, const uint8_t* smap, int n, int in_h, int in_w,
                  const int32_t* index, const float* mats, int samples, int out_h, int out_w,
                  float* out_h_, uint8_t* out_c, uint8_t* out_s, int32_t* from);

/* Network-ready inputs on the device (csrc/mre_warp_inputs.hip): the gather of mre_warp_maps written as
 * the tensor a convolution consumes -- planar, normalised per channel, float32 or bfloat16 -- in one launch.
 * hmap, cmap (may be NULL), n, in_h, in_w, index, mats, samples, out_h, out_w are those of mre_warp_maps: the same device
 * pointers and alignment, the same source cell (fx, fy) and the same `valid`, NaN or huge matrix entries and an index
 * outside [0, n) included.
 *   channels    1 .. 8 channels of the output
 *   chan_src    HOST i32 [channels]: what channel k holds, MRE_SRC_RED / _GREEN / _BLUE / _HEIGHT; sources may repeat and
 *               come in any order (a colour source needs cmap)
 *   chan_scale, chan_bias   HOST f32 [channels], finite
 *   dtype       MRE_F32 or MRE_BF16
 *   out         device [samples][channels][out_h][out_w] of that type, aligned to its element size
 * The raw value v of a valid cell is the source cell's colour byte converted to float (exact) or its height; of any other
 * cell 0.0f, in every channel -- the values mre_warp_maps writes.  Channel k of the cell is, in float32 with both
 * operations rounded on their own (no fused multiply-add):
 *   t = v * chan_scale[k];   t = t + chan_bias[k]
 * MRE_F32 stores t.  MRE_BF16 stores t rounded to bfloat16, nearest and ties to even, on the bits: for a non-NaN t with
 * bits b the upper half of  b + 0x7FFF + ((b >> 16) & 1)  (an overflow rounds to +-inf); a NaN t (from a NaN or infinite
 * height only) stores some bfloat16 NaN.
 * Every element of out is written exactly once by the call and nothing else is; no byte outside the n maps, index and mats
 * is read; out is the same bits on every run.  A lane's 4 cells of a channel are stored at once (16 B, or 8 B of bfloat16)
 * when out_w is a multiple of 4 and out is aligned to that; any other width or offset is stored element by element, with
 * the same result.  Enqueued on `stream` of the current device; nothing synchronises.
 * MRE_ERR_ARG, with nothing launched, unless the conditions of mre_warp_maps on the shared arguments hold (n == 0 or
 * samples == 0: MRE_OK, nothing launched), 1 <= channels <= 8, the three channel arrays are non-NULL, every chan_src is one
 * of the four codes, cmap is non-NULL when a colour source is named, every chan_scale and chan_bias is finite (0 * inf
 * would make the sign and payload of a NaN part of the statement), dtype is one of the two codes, out is a non-NULL device
 * pointer aligned to its element size and its byte range overlaps no input byte range (the maps, index, mats). */
#define MRE_SRC_RED 0
#define MRE_SRC_GREEN 1
#define MRE_SRC_BLUE 2
#define MRE_SRC_HEIGHT 3
#define MRE_F32 0
#define MRE_BF16 1
int mre_warp_inputs(void* stream, const float* hmap, const uint8_t* cmap, int n, int in_h, int in_w,
                    const int32_t* index, const float* mats, int samples, int out_h, int out_w,
                    int channels, const int32_t* chan_src, const float* chan_scale, const float* chan_bias,
                    int dtype, void* out);

/* The Transporter place head on the device (csrc/mre_correlate.hip): every env's scene feature map
 * cross-correlated with that env's own rotated crop feature maps, and the best (rotation, row, column) per env.
 *   scene   device bfloat16 [n][depth][h][w]
 *   kern    device bfloat16 [n][rotations][depth][crop][crop], crop even
 * For env e, rotation r, row y and column x:
 *   logit[e][r][y][x] = sum_d sum_{i<crop} sum_{j<crop} scene[e][d][y + i - crop/2][x + j - crop/2] * kern[e][r][d][i][j]
 * A scene cell outside [0, h) x [0, w) counts as 0.  Crop index crop/2 is the pivot -- where crop_matrices puts the pick
 * cell at rotation 0 -- so a scene patch that equals the crop peaks at the cell where its pivot lies.
 * Every product is exact in float32 because both factors are bfloat16.  The sum is accumulated in float32 on the matrix
 * cores; its order is the kernel's own, fixed, and the same on every run; it is not part of the statement.
 *   logits      NULL, or device [n][rotations][h][w] of `dtype`: the float32 sums (MRE_F32), or those sums rounded to
 *               bfloat16 as mre_warp_inputs rounds (MRE_BF16)
 *   best_index  device i64 [n], best_value device f32 [n] (NULL together): the largest float32 sum of env e, taken before
 *               any bfloat16 rounding, and its flat index (r * h + y) * w + x.  The first cell is the initial candidate and
 *               a later cell replaces it only when it is strictly greater: ties go to the lowest flat index, and a NaN
 *               never wins.  The same bits whether or not logits is written.
 *   workspace   device, 16-byte aligned, at least the bytes mre_correlate_workspace answers for (n, rotations, h, w);
 *               its contents before and after the call mean nothing
 * All inputs are assumed finite; non-finite inputs do not fault, and beyond that the results are unspecified.
 * Every element of logits and best_* is written exactly once and nothing else but the workspace is; no atomics; the same
 * bytes on every run.  Logits are stored 8 columns at a time where w is a multiple of 8 and logits is 16-byte aligned, else
 * element by element at any element offset, with the same bits.  Enqueued on `stream` of the current device (two launches
 * with best_*, one without); nothing synchronises.
 * MRE_ERR_ARG, with nothing launched, unless n >= 0 (0: MRE_OK, nothing launched), 1 <= rotations <= 64,
 * 1 <= depth <= 16, crop even and 2 <= crop <= 64, 1 <= h, w <= 4096, rotations * h * w < 2^31, scene and kern are non-NULL
 * device pointers aligned to 2 bytes, dtype is MRE_F32 or MRE_BF16, logits is NULL or aligned to its element size,
 * best_index and best_value are NULL together or aligned (8 and 4 bytes), logits and best_* are not all NULL, workspace
 * is non-NULL, 16-byte aligned and large enough, and no output or workspace byte range overlaps an input.
 * mre_correlate_workspace: MRE_ERR_ARG unless bytes is non-NULL and n, rotations, h, w are in those ranges; at least 16. */
int mre_correlate_workspace(int n, int rotations, int h, int w, size_t* bytes);
int mre_correlate(void* stream, const uint16_t* scene, const uint16_t* kern, int n, int rotations, int depth,
                  int h, int w, int crop, int dtype, void* logits, int64_t* best_index, float* best_value,
                  void* workspace, size_t workspace_bytes);

/* Training the place head on the device (csrc/mre_correlate_grad.hip): the softmax cross-entropy of every
 * env's logits against a target cell, its gradient with respect to the logits, and the gradients of any g with respect to
 * the scene and the kernels.  scene, kern, n, rotations (R), depth, h, w, crop and logit[e] = l are those of mre_correlate;
 * no logit is ever stored.  With t = target[e], a flat index (r * h + y) * w + x, and the sums over all R * h * w cells:
 *   lse[e]  = log sum_cells exp(l)          target_logit[e] = l[t]          loss[e] = lse[e] - l[t]
 *   g[e][cell] = weight[e] * (exp(l[cell] - lse[e]) - [cell == t])      rounded to bfloat16 as mre_warp_inputs rounds
 *   grad_kern[e][r][d][i][j] = sum_y sum_x g[e][r][y][x] * scene[e][d][y + i - crop/2][x + j - crop/2]
 *   grad_scene[e][d][v][u]   = sum_r sum_i sum_j g[e][r][v - i + crop/2][u - j + crop/2] * kern[e][r][d][i][j]
 * where a scene cell or a g cell outside [0, h) x [0, w) counts as 0: the two gradients of sum_cells g * l.
 * A t outside [0, R * h * w) gives target_logit[e] = loss[e] = NaN, lse[e] as ever, and a g that is the weighted softmax
 * alone.  The host never reads target.
 *   target        device i64 [n], 8-byte aligned
 *   lse, target_logit, loss   device f32 [n]; lse is an output of mre_correlate_loss and an input of mre_correlate_dlogits
 *   weight        NULL (1 for every env) or device f32 [n]
 *   g             device bfloat16 [n][R][h][w]: the output of mre_correlate_dlogits, and an INPUT of the two gradient entries,
 *                 which therefore serve any loss
 *   grad_scene    device f32 [n][depth][h][w];  grad_kern  device f32 [n][R][depth][crop][crop]
 *   workspace     device, 16-byte aligned: for mre_correlate_loss at least what mre_correlate_workspace answers, for the two
 *                 gradient entries at least what mre_correlate_grad_workspace answers (the larger of the flipped kernels,
 *                 2 B, and min(ceil(h / 64), 4) partial grad_kern per env, 4 B, the latter only when h > 64: 7 MB per env at
 *                 36 x 3 x 64 x 64 and h = 320 -- split a large batch); its contents before and after mean nothing
 * lse is accumulated as an online (max, sum of exp2) in float32: within 2^-15 + 2^-22 |lse| of the exact value of the
 * float32 logits.  The sums of the gradients are accumulated in float32 on the matrix cores in the kernels' own fixed order.
 * Every output element is written exactly once and nothing else but the workspace is; no atomics; the same bytes on every
 * run, and an env's bytes depend neither on n nor on its place in the batch.  g is stored 8 columns at a time where w is a
 * multiple of 8 and g is 16-byte aligned, else element by element, with the same bits.  Enqueued on `stream` of the current
 * device (loss: 2 launches, dlogits: 1, grad_scene: 2, grad_kern: 1, or 2 when h > 64); nothing synchronises.
 * MRE_ERR_ARG, with nothing launched and no byte touched, unless the shape is in mre_correlate's ranges (n == 0: MRE_OK,
 * nothing launched), the bfloat16 pointers are non-NULL and 2-byte aligned, target is non-NULL and 8-byte aligned, the
 * float32 pointers are 4-byte aligned and (weight apart) non-NULL, workspace is non-NULL, 16-byte aligned and large enough,
 * every pointer is a device pointer, and no output or workspace byte range overlaps an input. */
int mre_correlate_loss(void* stream, const uint16_t* scene, const uint16_t* kern, int n, int rotations, int depth,
                       int h, int w, int crop, const int64_t* target, float* lse, float* target_logit, float* loss,
                       void* workspace, size_t workspace_bytes);
int mre_correlate_dlogits(void* stream, const uint16_t* scene, const uint16_t* kern, int n, int rotations, int depth,
                          int h, int w, int crop, const int64_t* target, const float* lse, const float* weight, uint16_t* g);
int mre_correlate_grad_workspace(int n, int rotations, int depth, int h, int w, int crop, size_t* bytes);
int mre_correlate_grad_scene(void* stream, const uint16_t* g, const uint16_t* kern, int n, int rotations, int depth,
                             int h, int w, int crop, float* grad_scene, void* workspace, size_t workspace_bytes);
int mre_correlate_grad_kern(void* stream, const uint16_t* g, const uint16_t* scene, int n, int rotations, int depth,
                            int h, int w, int crop, float* grad_kern, void* workspace, size_t workspace_bytes);

/* The Transporter pick head on the device (csrc/mre_attend.hip): what turns an attention network's
 * per-cell logits into a pick cell, and what trains that network.
 *   logits   device [n][rotations][h][w] of `dtype` (MRE_F32 or MRE_BF16), aligned to its element size; rotations (K) is
 *            the number of pick rotations, 1 for a classic Transporter.  The flat index of a cell is (k * h + y) * w + x, as
 *            in mre_correlate; l is the env's K * h * w logits as float32 (a bfloat16 widened exactly).
 * mre_attend, in one pass over the logits, per env e:
 *   best_index  device i64 [n], best_value device f32 [n] (NULL together): the largest logit and its flat index, by
 *               mre_correlate's rule: the first cell is the initial candidate and a later cell replaces it only when it is
 *               strictly greater: ties go to the lowest flat index, and a NaN never wins.
 *   target      device i64 [n], 8-byte aligned, or NULL; with it, and NULL together with it,
 *   lse, target_logit, loss   device f32 [n]:  lse[e] = log sum_cells exp(l),  target_logit[e] = l[t],  loss[e] = lse[e] - l[t]
 *               with t = target[e].  A t outside [0, K * h * w) gives target_logit[e] = loss[e] = NaN and lse[e] as ever.
 *               The host never reads target.
 *   workspace   device, 16-byte aligned, at least the bytes mre_attend_workspace answers for (n, rotations, h, w): 16 bytes
 *               for each of the S = min(ceil(K h w / 2048), 16) workgroups of an env; its contents mean nothing
 * target and best_* may not all be NULL.  What the decision and the loss share is the same bits whether they are asked for
 * together or alone.
 * mre_attend_dlogits, in one read and one write:
 *   g[e][cell] = weight[e] * (exp(l[cell] - lse[e]) - [cell == t])     device [n][rotations][h][w] of `dtype`
 * float32, or rounded to bfloat16 as mre_warp_inputs rounds.  lse is what mre_attend wrote; weight is NULL (1 for every env)
 * or device f32 [n]; a t outside gives the weighted softmax alone.
 * -inf is a valid logit: a masked cell.  It never is the best cell while the env has a finite one, it adds 0 to the sum and
 * its g is 0.  An env whose cells are all -inf has lse = -inf, loss = NaN, best_index = 0, best_value = -inf and g = 0 in
 * every cell; it puts no NaN into another env, and no -inf cell puts one into its own.  +inf and NaN logits do not fault,
 * and beyond that their results are unspecified.
 * lse is accumulated as an online (max, sum of exp2) in float32: within 2^-15 + 2^-22 |lse| of the exact value, as
 * mre_correlate_loss has it.  Every output element is written exactly once and nothing else but the workspace is; no
 * atomics; the same bytes on every run; an env's bytes depend neither on n nor on its place in the batch nor on the
 * alignment of its first byte.  Logits are read, and g is written, 16 bytes at a time where the env's first byte is 16-byte
 * aligned, except for a last partial vector; any other env element by element, with the same bits.  Enqueued on `stream`
 * of the current device (mre_attend: 2 launches, mre_attend_dlogits: 1); nothing synchronises.
 * MRE_ERR_ARG, with nothing launched and no byte touched, unless n >= 0 (0: MRE_OK, nothing launched),
 * 1 <= rotations <= 64, 1 <= h, w <= 4096, rotations * h * w < 2^31, dtype is one of the two codes, logits (and g) are
 * non-NULL and aligned to the element size, the i64 pointers are 8-byte and the f32 pointers 4-byte aligned, the NULL rules
 * above hold (mre_attend_dlogits: target and lse non-NULL), workspace is non-NULL, 16-byte aligned and large enough, every
 * pointer is a device pointer, and no output or workspace byte range overlaps an input.
 * mre_attend_workspace: MRE_ERR_ARG unless bytes is non-NULL and n, rotations, h, w are in those ranges; at least 16. */
int mre_attend_workspace(int n, int rotations, int h, int w, size_t* bytes);
int mre_attend(void* stream, const void* logits, int n, int rotations, int h, int w, int dtype, const int64_t* target,
               int64_t* best_index, float* best_value, float* lse, float* target_logit, float* loss,
               void* workspace, size_t workspace_bytes);
int mre_attend_dlogits(void* stream, const void* logits, int n, int rotations, int h, int w, int dtype,
                       const int64_t* target, const float* lse, const float* weight, void* g);

#define MRE_SOLVER_PGS 0
#define MRE_SOLVER_NEWTON 2
int mre_set_solver(mre_env*, int solver);
int mre_get_solver(mre_env*);
int mre_get_fallback_stats(mre_env*, long long* out4);
/* Queue launches: a rollout of several control ticks over more envs than the GPU holds waves (mre_rollout /
 * mre_rollout_ticks with ticks_per_launch <= 0 or >= 2) runs as launches of persistent waves that take the env furthest
 * behind, one control tick at a time, instead of one wave per env per launch; results are bit-identical to the per-tick
 * launches (tests/test_gpu_properties.py).  An env that outgrows the compact kernel's capacities in such a launch is handed
 * to the large kernel's waves of the same launch, for the same tick (no re-run).  out5 = {queue launches so far, waves of a
 * queue launch, control ticks per queue launch at most when the cut is the library's (MRE_QUEUE_TICKS, default 200), 1 if enabled
 * (MRE_QUEUE=0 disables), envs handed over inside a launch so far}. */
int mre_get_queue_info(mre_env*, long long* out5);

/* measurement support for bench.py: when enabled every step-kernel launch is
 * bracketed by hipEvents on its stream; mre_profile_read synchronises and returns the SUM of the
 * bracketed durations [ms] and the launch count since enable (and resets).  The env-group launches of a
 * stepping call overlap on the GPU, so the sum can exceed the wall time: it is a per-launch figure
 * (total / launches), not a tick time. */
int mre_profile_enable(mre_env*, int on);
int mre_profile_read(mre_env*, float* total_ms, int* launches);

#ifdef __cplusplus
}
#endif
#endif
