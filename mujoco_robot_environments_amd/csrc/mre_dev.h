// mre_dev.h -- device-side model constants and compile-time dimensions of the
// RearrangementEnv scene (fp32).  Filled on the host by mre_model.cpp from the
// model blob (mujoco_robot_environments_amd/model/compile.py) and uploaded once.
#pragma once
#include <stdint.h>

namespace mre {

// Scene topology the kernels are specialised for (verified against the blob
// in mre_create; mismatch -> MRE_ERR_MODEL).
constexpr int NB = 20;     // bodies incl. world: 7 arm + 8 gripper + 4 cubes
constexpr int NRB = 16;    // world + robot bodies (ids 0..15)
constexpr int GRIP_BODY0 = 8;  // first finger body (8..15: two four-bar fingers below arm link 7)
constexpr int NV = 39;
constexpr int NRV = 15;    // robot dofs (ids 0..14), cube p owns dofs 15+6p..
constexpr int NQ = 43;
constexpr int NQP = 44;    // padded qpos row
constexpr int TRACE_W = 88; // row of the parity trace: qpos[43], constraint census, contact-set hash, solution-state hash, pad to 48, then qvel[39] + pad (MRE_TRACE_W)
constexpr int TRACE_QVEL = 48;  // first qvel column of a trace row (MRE_TRACE_QVEL)
constexpr int NVP = 40;    // padded qvel row
constexpr int NU = 8;
constexpr int QFINE = 32;  // low-order state words of the robot kept in LDS: joint angles [0:15], velocities [16:31]
// row of StepArgs::qfine in HBM: the robot's words, then the cubes' -- pose (position + quaternion) of cube p at
// [QFINE_CUBE_Q + 7 p, +7), velocity at [QFINE_CUBE_V + 6 p, +6).  The cubes' words never enter LDS: the integrator
// reads and writes them in place once per step (round 4: the cubes' state is a double-float pair like the robot's).
constexpr int QFINE_ROW = 96;
constexpr int QFINE_CUBE_Q = 32;
constexpr int QFINE_CUBE_V = 60;
static_assert(QFINE_CUBE_Q + 7 * 4 == QFINE_CUBE_V && QFINE_CUBE_V + 6 * 4 <= QFINE_ROW, "qfine row layout");
constexpr int NPROP = 4;
constexpr int NG = 20;     // geoms: ground, table, robot hulls + pads, 4 cubes, then the hulls of arm links 1..4
constexpr int PROP_GEOM0 = 12;  // geom id of cube 0 (cubes 12..15; checked against the blob in mre_create)
constexpr int NPAIR = 128; // static collision pair table: one lane per pair, two passes (84 pairs in use)
constexpr int NMR = 96;    // entries of the robot block of the sparse mass matrix
constexpr int NSITE = 2;
constexpr int NEQ = 3;
constexpr int CONTACT_EXPORT = 32;  // contacts per env exported by a detect launch (mre_get_contacts)
constexpr int MAXCHAIN = 9;   // longest dof chain root->leaf (7 arm + 2 finger)
// dof tree of the robot block (arm chain 0..6, four two-dof finger branches off dof 6); the
// register-resident L'DL solve is unrolled over it at compile time, mre_create checks the blob
constexpr int ROBOT_DOF_PARENT[NRV] = {-1, 0, 1, 2, 3, 4, 5, 6, 7, 6, 9, 6, 11, 6, 13};
constexpr int robot_dof_depth(int i) { return ROBOT_DOF_PARENT[i] < 0 ? 0 : 1 + robot_dof_depth(ROBOT_DOF_PARENT[i]); }
constexpr int robot_dof_madr(int i) { return i == 0 ? 0 : robot_dof_madr(i - 1) + robot_dof_depth(i - 1) + 1; }
constexpr int robot_dof_anc(int i, int k) {  // k-th ancestor (0 = parent), -1 past the root
  int j = ROBOT_DOF_PARENT[i];
  for (int t = 0; t < k && j >= 0; t++) j = ROBOT_DOF_PARENT[j];
  return j;
}
static_assert(robot_dof_madr(NRV) == NMR, "robot mass-matrix size");

// Per-env constraint capacities (LDS is sized for them).  The library carries the step kernel in
// two capacity sets: the compact one keeps a workgroup at 20 KB of LDS (8 workgroups per CU) and
// covers cubes resting / sliding on the table; the large one (6 per CU) covers grasps and piles.
// mre_api.cpp runs every env on the compact kernel and re-runs, from the saved pre-launch state, the
// envs that report an overflow on the large kernel, so results never depend on the compact caps.
#if defined(MRE_LARGE_CAPS) && defined(MRE_NEWTON)
// the Newton kernels carry no M^-1 J' pool and no block records: the same LDS (6 workgroups per CU)
// holds more rows
constexpr int NCON_MAX = 48;
constexpr int NEFC_MAX = 160;
constexpr int NRROW_MAX = 100;
constexpr int NPP_MAX = 16;
constexpr int MAXBLK = 58;
#elif defined(MRE_LARGE_CAPS)
constexpr int NCON_MAX = 44;   // active contacts kept per env
constexpr int NEFC_MAX = 148;  // constraint rows per env (7 equality + limits + 3 per contact)
constexpr int NRROW_MAX = 83;  // rows with a robot part (7 equality + limits + 3 per robot contact)
constexpr int NPP_MAX = 16;    // cube-cube contacts (rows with two prop parts)
constexpr int MAXBLK = 52;     // <= 8 scalar-row triples + NCON_MAX contact blocks (also bounds the schedule length)
#elif defined(MRE_NEWTON)
// compact Newton: the LDS the PGS builds spend on the stored factor of M holds seven more robot rows (round 5)
constexpr int NCON_MAX = 32;
constexpr int NEFC_MAX = 112;
constexpr int NRROW_MAX = 69;
constexpr int NPP_MAX = 8;
constexpr int MAXBLK = 40;
#else
constexpr int NCON_MAX = 32;
constexpr int NEFC_MAX = 112;
constexpr int NRROW_MAX = 62;
constexpr int NPP_MAX = 8;
constexpr int MAXBLK = 40;
#endif
// the compact capacities as the host needs them (it is compiled once, without MRE_NEWTON / MRE_LARGE_CAPS, and picks
// the robot-row capacity by the handle's solver)
constexpr int NRROW_MAX_COMPACT_PGS = 62, NRROW_MAX_COMPACT_NEWTON = 69;
#if !defined(MRE_LARGE_CAPS)
static_assert(NRROW_MAX ==
#ifdef MRE_NEWTON
              NRROW_MAX_COMPACT_NEWTON,
#else
              NRROW_MAX_COMPACT_PGS,
#endif
              "host-side copy of the compact robot-row capacity");
#endif
static_assert(NEFC_MAX <= 256 && NRROW_MAX < 127 && NPP_MAX <= 16 && MAXBLK >= 8 + NCON_MAX,
              "capacities must fit the block descriptor fields (mre_solver.h)");

// Everything the collision stages need to know about one entry of the static pair table, in one 128-byte record:
// the broad phase reads it with independent 16-byte loads (one trip to memory) where the separate tables cost a chain
// of dependent loads -- pair -> geom -> body -> prop id, then the geoms' local frames -- per pass and lane
// (round 3's phase stamps: broad phase 1.5 k of a Newton tick's 46.7 k units, geom frames 0.5 k).
struct alignas(16) PairRec {
  int g1, g2, b1, b2;              // geoms (g1 < 0: unused entry) and their bodies
  int pid1, pid2, type1, single;   // cube slot of each geom (-1: none), type of geom 1 (0 = plane), one-contact pair | type of geom 2 << 8
  float pos1[3], rb1;              // geom 1 in its body's frame; bounding radius (a cube's comes from its per-env size)
  float pos2[3], rb2;
  float quat1[4], quat2[4];
  float size1[3], margin;          // half sizes (a cube's come from its per-env size); pair margin
  float size2[3], gap;
};
static_assert(sizeof(PairRec) == 128, "PairRec is eight 16-byte words");

// The same treatment for the rest of the step (round 6).  A phase used to fetch its model constants where it used
// them: one dword, waited for at once, and often the index of the next one (dof -> body -> prop id; matrix entry -> dof
// -> damping -> actuator bias) -- some 95 separate trips to memory per step outside the solver, at two waves per SIMD.
// The records below hold, per lane, what a phase reads for its own body / dof / matrix entry / constraint row, so that
// it costs ONE group of independent 16-byte loads issued at the phase's entry.  They carry the very float32 / int
// values of the host's model tables (ModelTables, mre_model.h: mre_model.cpp fills them from the tables and compares
// every field afterwards), and the kernels apply the same operations in the same order.  Of the tables themselves the
// device keeps only the few that DevModel lists below.
struct alignas(16) BodyRec {   // lane = body
  float quat[4];
  float pos[3], mass;
  float jnt_pos[3], qpos0;          // qpos0[qposadr]
  float jnt_axis[3]; int qposadr;
  float ipos[3]; int propid;
  float iquat[4];
  float inertia[3]; int dofadr;
  float jnt_range[2], invweight0[2];
  float jnt_stiffness, jnt_springref; int parent, jnt_limited;
};
static_assert(sizeof(BodyRec) == 144, "BodyRec is nine 16-byte words");
struct alignas(16) DofRec {    // lane = dof
  int body, propid, dofadr, ten;    // the dof's body, that body's prop id and first dof; tendon slot of this dof (-1: none)
  float armature, damping, invweight0, ten_coef;   // ten_coef[ten] (0 where none)
  float jnt_stiffness, jnt_springref, act_gain, act_bias0;   // of the dof's body; of the arm actuator on this dof (0 where none)
  float act_bias1, act_bias2, act_ctrl_lo, act_ctrl_hi;
  float act_force_lo, act_force_hi; int act_forcelimited, pad;
};
static_assert(sizeof(DofRec) == 80, "DofRec is five 16-byte words");
struct alignas(16) MEntryRec {  // lane = entry of the robot block of the sparse mass matrix
  int i, j; float armature, damping;     // M(i, j); dof_armature[i], dof_damping[i]
  float act_bias2, ten_coef; int ten, pad;   // act_bias[i][2] (0 past the arm), ten_coef[ten] of dof i (ten = -1: none)
};
static_assert(sizeof(MEntryRec) == 32, "MEntryRec is two 16-byte words");
// parameters of one constraint row by its source: equality e -> row_rec[e], limit of the joint of body b ->
// row_rec[ROWREC_JNT + b], contact of pair pr -> row_rec[ROWREC_PAIR + pr]
struct alignas(16) RowRec {
  float solref[2], margin, gap;     // (margin, gap: pairs only)
  float solimp[5], friction;        // (friction: pairs only, pair_friction[pr][0])
  float invw1, invw2;               // connect: body_invweight0[b][0] of its two bodies; joint equality / limit:
                                    //  dof_invweight0 of its dof(s); pair: body_invweight0[b][0] of each ROBOT body (cubes: per env)
};
static_assert(sizeof(RowRec) == 48, "RowRec is three 16-byte words");
constexpr int ROWREC_JNT = NEQ, ROWREC_PAIR = NEQ + NB, NROWREC = NEQ + NB + NPAIR;
struct alignas(16) EqRec {     // equality constraint e
  int type, b1, b2, pb1;            // eq_type, eq_obj, body_parent of both bodies
  int pb2, root, pad0, pad1;        // first body at or above b1 that is no finger body (the arm link the linkage hangs off)
  float data[8];
  float qpos0_1, qpos0_2; int pad2, root_chain_len;   // qpos0 of the dofs of b1 / b2 (joint equality); chain_len[root]
  int root_chain[12];               // chain_dof[root][0 .. MAXCHAIN), padded
};
static_assert(sizeof(EqRec) == 128 && MAXCHAIN <= 12, "EqRec is eight 16-byte words");
struct alignas(16) SiteRec {   // lane = site
  float pos[3]; int body;
  float quat[4];
};
static_assert(sizeof(SiteRec) == 32, "SiteRec is two 16-byte words");
// wave-uniform options, tendon and gripper-actuator scalars in one block
struct alignas(16) OptRec {
  float timestep, impratio, tolerance; int iterations;
  float gravity[3]; int cone;                    // mjtCone: 0 = pyramidal, 1 = elliptic (mre_solver.h: assemble_constraints)
  float ten_coef[2]; int ten_dof[2];
  float grip_gainprm, grip_biasprm[3];
  float grip_forcerange[2], grip_ctrlrange[2];   // act_ctrlrange[NU - 1]
  float robot_mass, M0_diag_robot_sum; int tcp_site, eef_site;   // sum_i M0(i,i) over robot dofs (meaninertia)
  float tcp_pos[3]; int pad;                     // site_pos[tcp_site]
};
static_assert(sizeof(OptRec) == 112, "OptRec is seven 16-byte words");

// What device code reads of the model, and nothing else: the per-lane records above and the few tables that are
// still indexed directly (collision, controller, reset, exports).  Everything the records are packed from is host-only
// (ModelTables, mre_model.h).  A member that no kernel reads does not belong here.
struct DevModel {
  // ---- bodies (index = body id)
  int body_propid[NB];
  int chain_len[NB];             // dofs root->body (robot bodies; cubes: 0, handled apart)
  int chain_dof[NB][MAXCHAIN];
  float body_mass[NB];
  // ---- dofs / robot mass-matrix structure
  int dof_Madr[NV + 1];
  float qpos0[NQP];
  int M_i[NMR], M_j[NMR];        // entry e = M(i, j), j ancestor-or-self of i
  // ---- geoms / pairs
  int geom_type[NG], geom_body[NG], geom_propid[NG];
  float geom_size[NG][3], geom_pos[NG][3], geom_quat[NG][4], geom_rbound[NG];
  int pair_g1[NPAIR], pair_g2[NPAIR];
  float pair_margin[NPAIR];
  PairRec pair_rec[NPAIR];       // the pair table packed per pair for the collision stages
  // ---- actuation / reset (the options and the site ids are in opt_rec)
  float act_ctrlrange[NU][2];
  float home_qpos[7];
  float park_pos[NPROP][3];      // where inactive cube slots are parked
  // ---- the host's tables packed per lane for the step's phases (filled and verified by mre_model.cpp)
  BodyRec body_rec[NB];
  DofRec dof_rec[NV];
  MEntryRec m_rec[NMR];
  RowRec row_rec[NROWREC];
  EqRec eq_rec[NEQ];
  SiteRec site_rec[NSITE];
  OptRec opt_rec;
};

// OSC controller parameters (config/robots/arm/controller_config/osc.yaml:5-22)
struct OscConfig {
  float kp_pos, kd_pos, kp_ori, kd_ori, kp_null, kd_null;
  float null_q[7];
  float pos_thresh, ori_thresh;
  int pinv_always;
};

// F_CONV_CONTINUE: this launch continues a run_controller call cut into several launches (the
// converged flag carries over); F_CONV_OPEN: more launches follow (NOT_CONVERGED is not judged yet)
// F_OSC_EVAL (zero-step launch): evaluate the controller on the current state and store the command
// (OSC.compute_control_output + MinMax.compute_control_output) in ctrl without stepping
enum StepFlags : unsigned { F_NO_CONSTRAINTS = 1u, F_FREEZE_ROBOT = 2u, F_CONV_CONTINUE = 4u, F_CONV_OPEN = 8u,
                            F_OSC_EVAL = 16u, F_DETECT = 32u, F_SETTLE_EXIT = 64u, F_DETECT_ACTIVE = 128u,
                            F_CLIP_ALWAYS = 256u, F_NW_ALL_TILES = 512u };
// F_DETECT (zero-step launch): narrow phase on the current poses, every detected contact (dist < margin)
//   exported to `contacts` -- physics.forward() + physics.data.contact of the reference's PropPlacer
// F_DETECT_ACTIVE (with F_DETECT): the list the next solve would get instead (dist < margin - gap: collide(.., detect = false))
// F_CLIP_ALWAYS: the narrow phase clips every face contact through its LDS buffers, also where nothing is clipped
//   (set for every launch of a handle created under MRE_NARROW_GENERIC=1: the two paths compared inside one process)
// F_NW_ALL_TILES: nw_direction forms and moves all six Hessian tiles, also the cross tiles the step's contact set leaves
//   zero (set for every launch of a handle created under MRE_NEWTON_GENERIC=1; mre_newton.h)
// F_SETTLE_EXIT: an env leaves the step loop once its cubes have settled (max |qvel| < 1e-3, max |qacc| <
//   1e-2, time > min_settle_steps * dt: environment/prop_initializer.py:240-258); steps taken -> settle_steps
enum CtrlMode : int { CTRL_HELD = 0, CTRL_SEQ = 1, CTRL_OSC = 2 };

struct StepArgs {
  const DevModel* M;
  int N;
  float* qpos;            // [N][NQP]
  float* qvel;            // [N][NVP]
  float* qacc_ws;         // [N][NVP]
  float* qfine;           // [N][QFINE_ROW] or null: low-order words of the robot's state -- its 15 joint angles
                          //  [0:15] and their velocities [16:31] are carried as unevaluated sums hi + lo of two
                          //  floats (hi = the qpos / qvel row entry, i.e. the value rounded to float32)
  float* ctrl;            // [N][NU]  (held control / last applied control)
  const float* ctrl_seq;  // [T][seq_stride][NU] or null
  int seq_stride;         // envs per tick of ctrl_seq (the handle's env count; N may be a group of them)
  const int* nprops;      // [N]
  const float* prop_size; // [N][NPROP][3]
  int nsteps, control_steps, mode;
  unsigned flags;
  // OSC
  const OscConfig* osc;      // device copy of the controller parameters: one, or one per env
  int osc_stride;            // 0 = shared by all envs, 1 = osc[env]
  const float* osc_target;   // [N][16]: pos3 quat4 vel3 angvel3 pad3
  const uint8_t* grip_closed;  // [N]
  uint8_t* converged;        // [N] or null
  // outputs
  float* sites;              // [N][16]: tcp_pos3, eef_pos3, eef_quat4, pad
  uint32_t* status;          // [N]
  int* nstep;                // [N] or null: physics steps taken since the last reset (physics.data.time / timestep)
  int* stats;                // [N][4]
  float* trace;              // [max_steps][trace_nenv][TRACE_W] or null
  int trace_nenv, trace_max, trace_base;
  const uint8_t* env_mask;   // [N] or null: envs with 0 are skipped by this launch
  const int* env_order;      // [N] or null: workgroup b steps env env_order[b] (heavy-first dispatch)
  float* geoms;              // [N][NG][16] or null: world pose of every geom for the renderer
                             //  (pos3, rotation 9 row-major geom->world, half sizes 3, type)
  float* contacts;           // [N][1 + 3 * CONTACT_EXPORT] or null (F_DETECT): count, then (geom1, geom2, dist) each
  float* contacts_full;      // [N][CONTACT_EXPORT][12] or null (F_DETECT): pos[3], frame[9] of the same contacts (mre_get_contacts_full)
  int* settle_steps;         // [N] or null (F_SETTLE_EXIT): physics steps the env took in this launch
  int min_settle_steps;
  // capacity fallback (mre_api.cpp: launch_step): the launch is split between the compact and the large kernel by
  // the per-env flag `large` (an env takes part in the kernel whose `want_large` equals its flag; null: every
  // unmasked env takes part), and an env copies its state rows aside before it steps (sv_qpos != null), so that
  // an env that overflows the compact capacities can be put back and re-run on the large kernel
  const uint8_t* large;      // [N] or null
  int want_large;
  float *sv_qpos, *sv_qvel, *sv_qacc_ws, *sv_qfine, *sv_ctrl;
  int* sv_nstep;
  uint32_t* sv_status;
  uint8_t* sv_converged;
  int* launch_info;          // [N][4] or null: {overflow in this launch: 1 on the compact kernel (the host re-runs the
                             //  env), 2 on the large one; -1: not part of the launch; -2: skipped, see `pending`,
                             //  max ncon | the env's own duration in this launch (s_memtime ticks >> 10) << 16,
                             //  max nefc, max robot rows | max cube-cube contacts << 16} over the launch's steps
  // The host reads a launch's info one launch late (the next launch of the group is already enqueued by then).  An env
  // that overflows the compact kernel raises its `pending` byte; the launches that follow leave such an env alone
  // (state rows and save area untouched) until the host has put it back and re-run every launch it missed on the
  // large kernel (k_restore_rows clears the byte).  null: no such protocol (synchronous launches, re-runs).
  uint8_t* pending;          // [N] or null
  // Queue launches (k_step_queue, k_step_queue_large; mre_api.cpp: launch_group_enqueue).  A launch of q_nticks control
  // ticks whose waves are not bound to an env: a wave takes the ready env that is furthest behind, steps it ONE tick,
  // stores its rows, makes it ready for the next tick and takes another, until nothing is ready.  Compact waves and
  // envs are dealt to q_shards shards (wave w: w % q_shards; entry i of env_order: i % q_shards), each with its own
  // lists; shards q_shards .. q_shards + q_lshards - 1 are the large kernel's (env e: q_shards + e % q_lshards).  Bucket t of shard s lists the envs ready for tick t in the order
  // they became so: q_buf[t][s][0 .. q_tail[s][t]) (entry = env + 1; 0 = counted by a push, not written yet), of which
  // q_head[s][t] are taken -- except bucket 0 of a compact shard, which is the shard's entries of env_order (all there
  // from the start; the envs flagged large among them are skipped: the host lists those in bucket 0 of the large shard).
  // q_acc[env] carries the env's launch info (high-water marks, summed duration, "handed over") from tick to tick;
  // q_done counts the envs that are through.  The host zeroes all of it before every launch.  q_head null: one env per
  // workgroup for the whole launch.
  int* q_head;               // [q_shards + q_lshards][QUEUE_TICKS_MAX]
  int* q_tail;               // [q_shards + q_lshards][QUEUE_TICKS_MAX]
  int* q_buf;                // [q_nticks][q_stride]: q_shards compact shards of q_cap entries, then q_lshards large ones of q_capl
  int* q_acc;                // [N][4]
  int* q_done;               // one word
  int* q_started;            // one word: compact waves that have started
  const int* q_gen;          // one word, outside the block the host zeroes: the number of the launch whose lists are set up
  int q_gen_expect;
  int q_wait;                // large kernel: 1 = wait for hand-overs until every env is through; 0 = take what is listed and leave
  int* q_err;                // one word (mapped host memory): set when something that must arrive did not (a bug; the host fails the handle)
  int q_nticks, q_shards, q_cap, q_stride;   // q_cap = ceil(N / q_shards), q_stride = q_shards * q_cap + q_lshards * q_capl
  int q_lshards, q_capl;                     // the large kernel's shards and their capacity, ceil(N / q_lshards)
};
constexpr int QUEUE_TICKS_MAX = 256;  // control ticks of a queue launch at most (a wave's search for work: one lane per bucket, four rounds)
constexpr int QUEUE_SHARDS_MAX = 32;
constexpr int QUEUE_LSHARDS_MAX = 16;

// Rejection sampling of a cube pose (k_pose_search): PropPlacer.__call__'s per-prop loop
// (environment/prop_initializer.py:164-232) and prop_place (tasks/rearrangement.py:597-665).  One wave
// per env; attempt t draws u = U01(seed, global env id, tick_base + t, channel 0..3), the pose
// lo + (hi - lo) u[0:3] (fp64, rounded to fp32 for the test), moves the cube there IN LDS ONLY, runs the
// narrow phase of every pair of the cube with a geom other than the table, and rejects the pose while a
// detected contact (dist < margin) has dist <= max_dist.
struct SearchArgs {
  const DevModel* M;
  int N;
  float* qpos;               // [N][NQP]; written only when commit != 0
  const int* nprops;         // [N]
  const float* prop_size;    // [N][NPROP][3]
  const uint8_t* env_mask;   // [N] or null
  const long long* env_ids;  // [N] global env ids or null (then env_id_offset + env)
  long long env_id_offset;
  unsigned long long seed;
  const int* prop;           // [N] cube index to move (< 0: nothing to do for this env) or null
  int fixed_prop;            //   (prop == null: this cube in every env that has it)
  const double* bounds;      // [N][6] lo xyz, hi xyz or null
  double shared_bounds[6];   //   (bounds == null)
  const int* tick_base;      // [N] or null
  long long tick0;           //   (tick_base == null)
  int max_attempts;
  int yaw_mode;              // 1: quat = (cos(pi u3 / 2), 0, 0, sin(pi u3 / 2)); 0: quat = fixed_quat
  double fixed_quat[4];
  float max_dist;            // +inf: any detected contact rejects (PropPlacer); 0.05: prop_place
  int commit;                // 1: the accepted pose is written to qpos (PropPlacer); 0: state untouched
  float* qfine;              // [N][QFINE_ROW] or null: with commit, the low-order words of the accepted fp64 pose
  double* pose;              // [N][7] accepted pose (xyz fp64, quat) or null
  int* attempts;             // [N]: attempts used (>= 1); -max_attempts: none accepted; 0: env skipped
  unsigned flags;            // F_CLIP_ALWAYS or 0
};

// Export of the arm's dynamics terms on the current state (k_arm_dynamics; mre_get_arm_dynamics): what a torque law
// reads -- mj_jacSite, mj_fullM, qfrc_bias -- as the float32 values the in-kernel law (mre_osc.h) consumes.  One wave per
// env; nothing but `out` is written.  Row layout (DYN_W floats): jac[6][7] (jacp; jacr) | mass[7][7] | qfrc_bias[7] |
// site_xpos[3] | site quaternion wxyz | arm qpos[7] | arm qvel[7] | zeros.
constexpr int DYN_W = 128;   // MRE_DYN_W
constexpr int DYN_JAC = 0, DYN_MASS = 42, DYN_BIAS = 91, DYN_POS = 98, DYN_QUAT = 101, DYN_QPOS = 105, DYN_QVEL = 112,
              DYN_PAD = 119;
struct DynArgs {
  const DevModel* M;
  int N;
  const float* qpos;         // [N][NQP]
  const float* qvel;         // [N][NVP]
  const float* qfine;        // [N][QFINE_ROW] or null
  const int* nprops;         // [N]
  const float* prop_size;    // [N][NPROP][3]
  int site;                  // 0: the controller (attachment) site, 1: the pinch site
  float* out;                // [N][DYN_W]
};

// sort_colours' selection + prop_pick (k_sort_select; tasks/rearrangement.py:700-751, :579-595), one thread per env
struct SortArgs {
  const DevModel* M;
  int N;
  const float* qpos;         // [N][NQP]
  const int* nprops;         // [N]
  const double* zones;       // [N][NPROP][4]: lo x, lo y, hi x, hi y of the cube's colour zone
  double place_z;            // get_location_bounds' hard-coded 0.4
  int* which;                // [N] out: first cube outside its zone, -1: none
  double* pick;              // [N][7] out: cube position + grasp quaternion
  double* bounds;            // [N][6] out: place bounds of the selected cube (for k_pose_search)
};

// Camera + shading parameters of mre_render (csrc/mre_render.hip)
struct RenderArgs {
  int N, height, width;
  const float* geoms;        // [N][NG][16] from the step kernel's geometry export
  const int* nprops;         // [N]
  const uint8_t* prop_rgb;   // [N][NPROP][3] cube albedo
  float geom_rgb[NG][3];     // albedo of the static geoms (cube entries unused)
  float cam_pos[3], cam_mat[9];  // camera frame -> world, row-major (MuJoCo: looks along -z, y up)
  float fy;                  // focal length in pixels: 0.5 * height / tan(fovy / 2)
  float light_pos[3];        // positional scene light (arena.xml)
  float ambient, head_diffuse, light_diffuse;
  float checker[2][3], checker_size;  // ground plane (geom type 0) checker colours / square size [m]
  float zfar;                // depth written where nothing is hit
  uint8_t* rgb;              // [N][H][W][3] or null
  float* depth;              // [N][H][W] or null
  uint8_t* seg;              // [N][H][W] geom index, 255 = background, or null
  const uint8_t* env_mask;   // [N] or null
  // geoms [g0, g1) are cast; with a background (the image of the static geoms for this camera,
  // rendered once) every pixel starts from it and only the moving geoms are composited on top
  int g0, g1;
  const float* bg_depth;     // [H][W] or null
  const uint8_t* bg_rgb;     // [H][W][3]
  const uint8_t* bg_seg;     // [H][W]
};

}  // namespace mre
