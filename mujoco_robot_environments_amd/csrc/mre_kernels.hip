// mre_kernels.hip -- gfx950 (MI355X) kernels for the batched RearrangementEnv step.
//
// One environment per 64-lane wavefront (block = 64 threads), whole per-env
// working set in LDS, state rows read/written once per launch with coalesced
// accesses.  A launch runs `nsteps` physics steps of dt = 1 ms:
//     per step:  S1 (position + velocity stage)  ->  [control at tick boundary]
//                -> S2 (actuation, smooth acceleration, constraint solve, integrate)
// which is the reference's dm_control legacy step (mj_step2 then mj_step1,
// models/robot_arm.py:77-81) with the trailing mj_step1 of step k evaluated at
// the head of step k+1 (same state, same result).
//
// Lane mappings: lane = body for tree quantities, lane = dof for generalized
// vectors, lane = mass-matrix entry for CRB, lane = collision pair for the narrow
// phase, lane = constraint row for assembly, lanes = dofs grouped in islands for
// the PGS sweeps (mre_solver.h); the robot's L'DL factorisation and solves are
// unrolled at compile time over its dof tree (ROBOT_DOF_PARENT, mre_dev.h).
// Phases are noinline functions called from the kernel body only (no nested
// calls, no callee-saved registers, no scratch).  This file is compiled twice:
// plain (compact constraint capacities, entry points k_step / k_settle) and with
// -DMRE_LARGE_CAPS (k_step_large), see mre_dev.h.
#include <hip/hip_runtime.h>

#include "mre_dev.h"
#include "mre_math.h"
#include "mre_collide.h"

namespace mre {
using ModelP = MRE_MODEL_PTR(DevModel);
#if defined(MRE_PHASE_STAMPS) && MRE_PHASE_STAMPS >= 4
__shared__ unsigned long long dbg_acc[4];   // diagnostic builds only (MRE_DBG_STAMP)
#endif

// OSC scratch (mre_osc.h); lives in LDS region R1 (see Sm)
struct OscSm {
  float J[6][7], M[7][7], MiJt[7][6], Li[6][6], Lam[6][6], V[6][6], Jbar[7][6];
  float ep[3], eo[3], F[6], LF[6], tn[7], Jbt[6], xd[6], w[6];
};

// constraint block: a triple of scalar rows (type 0) or the three rows of a contact (type 2)
struct alignas(8) Blk {
  uint16_t row0;            // first efc row
  uint8_t type, nrows;
  uint8_t rslot;            // first robot-row slot or BLK_NONE
  uint8_t pa, pb;           // cubes touched (0xF = none)
  uint8_t primary : 4;      // island that accounts the block's cost change
  uint8_t bslot : 4;        // slot of the second cube's Jacobian part (cube-cube contacts)
};

// bytes the PGS solver's operand table needs on top of the body-frame region (mre_solver.h)
constexpr int TAB_BYTES = 8 * (MAXBLK * 5 + 1) + 4 * 48;
constexpr int FRAME_BYTES = (int)sizeof(OscSm) > 4 * (NB * 16) ? (int)sizeof(OscSm) : 4 * (NB * 16);
constexpr int R1_MIN = TAB_BYTES - FRAME_BYTES > 0 ? TAB_BYTES - FRAME_BYTES : 4;
constexpr int MD_LD = 17;  // row stride of the dense robot mass matrix (Newton): odd, conflict-free columns

struct Sm {
  // state.  The robot's 15 joints are carried in double-float form: qpos / qvel hold the value rounded to
  // float32 and qlo the remainder (angles [0:15], velocities [16:31]) -- see robot_q().  The warm start
  // needs no array of its own: between the integration of one step and the solve of the next, qacc IS
  // qacc_warmstart (mj_advance copies it), so the launch loads the warm-start row into qacc and stores qacc back.
  float qpos[NQP], qvel[NVP], qlo[QFINE], ctrl[NU];
  // generalized vectors
  // (qfrc_con is dead between integrate and the next solve: its head carries the fp64-evaluated
  //  residuals of the two connect rows from connect_residuals to assemble_constraints)
  float qfrc_smooth[NVP], qacc_smooth[NVP], qacc[NVP], qfrc_bias[NVP], qfrc_con[NVP];
  // LDS regions reused along the step (lifetimes: S1a kinematics..factor, S1b velocity stage,
  // S1c collision + assembly, tick-boundary controller, S2 solve + integrate)
  union {  // body frames (S1a..S1c) | OSC scratch (tick boundary: nothing reads the frames between the
           // assembly and the next position stage) | S2: head of the PGS operand table, or the Newton
           // solver's generalized vectors
    struct { float xpos[NB][3], xquat[NB][4], xmat[NB][9]; };
    OscSm osc;
#ifdef MRE_NEWTON
    struct { float nw_Ma[NVP], nw_grad[NVP], nw_search[NVP], nw_Mv[NVP]; };
#endif
  };
#ifndef MRE_NEWTON
  char tab_room[R1_MIN];  // R1: (S2) tail of the operand table
#endif
  float cdof[NRV][6];  // robot dofs only; cube cdofs are implicit (prop_cdof)
  union {  // R2: contact geometry (S1c) | jar + forces (+ J*search, Newton) (S2)
    struct { float con_pos[NCON_MAX][3], con_frame[NCON_MAX][9], con_dist[NCON_MAX]; };
#ifdef MRE_NEWTON
    struct { float jar[NEFC_MAX], frc[NEFC_MAX], jv[NEFC_MAX]; };
#else
    // pyr_f: pyramidal cones -- the four edge forces of every contact (frc holds their image on the contact's
    // three rows); rides in the room the contact geometry leaves behind jar and frc
    struct { float jar[NEFC_MAX], frc[NEFC_MAX], pyr_f[4 * NCON_MAX]; };
#endif
  };
  float com_robot[3];
  float site_xpos[NSITE][3], site_xmat[1][9];  // orientation of the controller site only
  // robot block of the sparse mass matrix and its factors
#ifdef MRE_NEWTON
  // (Newton builds keep no factor of M: its one user, qacc_smooth, factors in registers (smooth_forces); the implicit
  //  integrator's M - h dF/dv is staged in the constraint block, which is dead by then: mh_store().  The 448 bytes
  //  went into the robot-row pool, NRROW_MAX 62 -> 69: a closed grasp -- 57 rows -- stays on the compact kernel.)
  float qM[NMR];
#else
  float qM[NMR], qLD[NMR], qLDinv[NRV + 1];  // qLD doubles as the factor of M - h dF/dv in integrate
#endif
  // per-env cube constants
  float prop_mass[NPROP], prop_inertia[NPROP][3], prop_size[NPROP][3];
  union { float scratch[64]; int iscr[64]; };
  float osc_tgt[16];
  int nprops;
  // active contacts (pair order)
  int ncon, nefc, nl, nrrow, npp, overflow, solver_iters;
  int finger_contact;   // an active contact touches a finger body
  uint8_t con_pair[NCON_MAX], con_rslot[NCON_MAX], con_bslot[NCON_MAX], con_b1[NCON_MAX], con_b2[NCON_MAX];
  uint16_t lim_info[NRV + 1];
  // ---- contiguous block [JpA .. hdr]: written only after collision; hosts the per-lane
  // clip buffers of the narrow phase (mre_solver.h: collide)
  // Its head doubles as the home of what only S1a / S1b need (dead before the collision):
  union {
    float JpA[3 * NCON_MAX][6];          // prop part A of every contact row
    struct {  // spatial inertias (S1a/S1b); gP / gC: per gripper dof, the momentum map crb * cdof and the
              // cdof about the pinch site in the frame of the arm's last link (gripper_local)
      float cinert[NB][10], crb[NRB][10], gP[NRB - GRIP_BODY0][6], gC[NRB - GRIP_BODY0][6];
      double gpose[NRB - GRIP_BODY0][7];   // pose (p, q) of every finger body in the arm link's frame (kinematics)
    };
  };
  float JpB[3 * NPP_MAX][6];             // prop part B (cube-cube contacts only)
  union {
    float Jr[NRROW_MAX][NRV];
    struct {  // velocity-stage temporaries (S1b); gI / gS: every finger body's OWN spatial inertia and its cdof about
              // the pinch site in the arm link's frame, fp64 (gripper_local -> finger_bias)
      float cdof_dot[NV][6], cvel[NB][6], cfrc[NB][6];
      alignas(8) double gI[NRB - GRIP_BODY0][10];
      double gS[NRB - GRIP_BODY0][6];
    };
  };
#ifdef MRE_NEWTON
  // ---- Newton solver (mre_newton.h)
  float efc_R[NEFC_MAX], efc_aref[NEFC_MAX];  // regulariser and reference acceleration of every row
  float frc_r[NRROW_MAX];                      // forces of the rows with a robot part, in slot order
  float con_fric[NCON_MAX];                    // friction coefficient of every contact
  float hc[NCON_MAX][6];                       // cone Hessian of contacts in the middle zone (00,01,02,11,12,22)
  float Md[NRV][MD_LD];                        // dense robot block of the mass matrix
  alignas(8) float W[NV * (NV + 1) / 2];       // Cholesky factor, packed by columns (transposed solve); after the solve: fp64 scratch of nw_robot_polish
  uint8_t rstate[NEFC_MAX];                    // row state after the last constraint update
  uint8_t clist[NPROP][NCON_MAX];              // contacts touching cube p (bit 7: the cube is part B)
  uint8_t ccount[NPROP], cpl_robot, cpl_cubes; // coupling of the Hessian blocks (robot-cube p, cube p-q)
  // per row, for every cube c: byte offset (from the start of Sm) of the row's six Jacobian words on that cube's
  // dofs -- its JpA row, its JpB row, or `zrow` where the row does not touch the cube (nw_build_lists)
  alignas(8) uint16_t jdesc[NEFC_MAX][4];
  float zrow[24];                              // zeros (three consecutive "rows" of a part that does not exist)
#else
  float Br[NRROW_MAX][NRV];
  // one 64-byte record per constraint block (scalar-row triple g -> record g, contact c -> record
  // 8 + c): [0:3] regulariser R of its rows, [3:6] aref (S1) -> efc_b (S2), [6:9] 1/A_ii,
  // [9:15] symmetric 3x3 block of A (00,01,02,11,12,22), [15] friction coefficient
  alignas(16) float blkrec[MAXBLK][16];
  // constraint blocks (scalar row or 3-row contact) and their island schedule
  Blk blk[MAXBLK];
  uint8_t sched[MAXBLK][8];  // per (schedule step, island < 5): block index or SCHED_NONE
#endif
  uint16_t hdr[NEFC_MAX];  // per row: robot slot | propA << 8 | propB << 12

  int nblk, nsched;
};

// Residency is the budget the whole layout is built around: 160 KB of LDS per CU, allocated in
// 512-byte granules -- 8 workgroups per CU for the compact capacities, 6 for the large ones.
#if defined(MRE_LARGE_CAPS)
static_assert(sizeof(Sm) <= 27136, "large-capacity Sm must fit 6 workgroups per CU");
#else
static_assert(sizeof(Sm) <= 20480, "compact Sm must fit 8 workgroups per CU");
#endif

// where integrate_setup stages M - h dF/dv for factor_solve_robot
#ifdef MRE_NEWTON
MRE_DEV float* mh_store(Sm& s) { return &s.JpA[0][0]; }
static_assert(sizeof(((Sm*)0)->JpA) >= sizeof(float) * NMR, "M - h dF/dv fits the head of the constraint block");
#else
MRE_DEV float* mh_store(Sm& s) { return s.qLD; }
#endif

struct BodyRegs {
  float anchor[3], axis[3], xipos[3], ximat[9];
};

// Angle / velocity of robot dof d (< NRV) with its low-order word added (fp64).
// Why: a float32 joint angle is off by up to 3e-8 rad (fingers) .. 1.2e-7 rad (arm) after every step.  The soft
// rows that close the 2F-85 four-bars turn a position error into K = 4e4 1/s^2 times as much acceleration, and links
// of a few grams integrate that into 1e-4 .. 5e-3 rad within 600 .. 1000 steps; the arm's own rounding is a random
// walk that reaches 4e-6 rad and shakes the fingers it carries by another 6 .. 9e-5 rad
// (tests/diagnostics/finger_precision_study.py: the fp64 oracle with its whole state rounded to float32 after every
// step leaves the 1e-4 bar in 7 .. 11 of 64 envs; with the 15 robot joints kept in fp64 and EVERY intermediate array
// rounded to float32 it stays within 1.6e-5 in 64 of 64).  The quantities that see an angle through a stiff row read
// the sum: the finger frame (hinge_local_d), the joint-equality and limit residuals, the tendon length and the
// position actuators, and the integrator.  Everything else reads the float32 word.
MRE_DEV double robot_q(const Sm& s, int d) { return (double)s.qpos[d] + (double)s.qlo[d]; }
MRE_DEV double robot_v(const Sm& s, int d) { return (double)s.qvel[d] + (double)s.qlo[QFINE / 2 + d]; }

MRE_DEV bool prop_is_active(const Sm& s, int propid) { return propid < 0 || propid < s.nprops; }

// What the position stage reads of its lane's body, taken from the body's record (BodyRec, mre_dev.h) in one group of
// independent loads at the phase's entry.
struct BodyK {
  float quat[4], pos[3], mass, jnt_pos[3], qpos0, jnt_axis[3], ipos[3], iquat[4], inertia[3];
  int qposadr, propid, dofadr, parent;
};
MRE_DEV BodyK load_body(ModelP M, int b) {
  const auto* R = &M->body_rec[b];
  BodyK B;
#pragma unroll
  for (int k = 0; k < 4; k++) { B.quat[k] = R->quat[k]; B.iquat[k] = R->iquat[k]; }
#pragma unroll
  for (int k = 0; k < 3; k++) { B.pos[k] = R->pos[k]; B.jnt_pos[k] = R->jnt_pos[k]; B.jnt_axis[k] = R->jnt_axis[k];
                                B.ipos[k] = R->ipos[k]; B.inertia[k] = R->inertia[k]; }
  B.mass = R->mass; B.qpos0 = R->qpos0; B.qposadr = R->qposadr; B.propid = R->propid; B.dofadr = R->dofadr;
  B.parent = R->parent;
  return B;
}

MRE_DEV bool body_is_active(ModelP M, const Sm& s, int b) {
  int p = M->body_propid[b];
  return p < 0 || p < s.nprops;
}

// ---- fp64 helpers for the finger linkage (gripper_local here, connect_residuals in mre_solver.h)
// The finger links weigh a few grams and sit 0.5 m from the robot's centre of mass: in the c-frame
// (spatial quantities about that centre, fp32) their inertias are differences of 1e-3-sized terms
// that leave 1e-5 kg m^2 -- 2e-5 of relative error in the finger rows of M (measured against the
// oracle: 2e-3 rad/s^2 of systematic error on finger accelerations of 50..130 rad/s^2, i.e. a drift
// of 1e-4 .. 3e-3 rad over 1000 steps).  Everything below the arm's last link is a function of the
// eight finger joint angles alone, so it is evaluated in THAT link's frame, about the pinch site, in
// fp64 (sin / cos by Taylor polynomials, |half angle| < 1), and only the results are rounded.
MRE_DEV void sincos_poly_d(double x, double& sn, double& cs) {
  // Taylor polynomials to x^15 / x^16 in Horner form with the reciprocal factorials as constants (the nested
  // z / 6 * (1 - z / 20 * ...) form costs a full fp64 division per term)
  const double z = x * x;
  double ps = -1.0 / 1307674368000.0;
  ps = ps * z + 1.0 / 6227020800.0;
  ps = ps * z - 1.0 / 39916800.0;
  ps = ps * z + 1.0 / 362880.0;
  ps = ps * z - 1.0 / 5040.0;
  ps = ps * z + 1.0 / 120.0;
  ps = ps * z - 1.0 / 6.0;
  sn = x + x * (z * ps);
  double pc = 1.0 / 20922789888000.0;
  pc = pc * z - 1.0 / 87178291200.0;
  pc = pc * z + 1.0 / 479001600.0;
  pc = pc * z - 1.0 / 3628800.0;
  pc = pc * z + 1.0 / 40320.0;
  pc = pc * z - 1.0 / 720.0;
  pc = pc * z + 1.0 / 24.0;
  pc = pc * z - 0.5;
  cs = 1.0 + z * pc;
}
MRE_DEV void dq_mul(double* r, const double* a, const double* b) {
  const double w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  const double x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  const double y = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  const double z = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  r[0] = w; r[1] = x; r[2] = y; r[3] = z;
}
MRE_DEV void dq_rot(double* r, const double* q, const double* v) {
  // v + 2 w (u x v) + 2 u x (u x v)
  const double ux = q[1], uy = q[2], uz = q[3], w = q[0];
  const double cx = uy * v[2] - uz * v[1], cy = uz * v[0] - ux * v[2], cz = ux * v[1] - uy * v[0];
  const double dx = uy * cz - uz * cy, dy = uz * cx - ux * cz, dz = ux * cy - uy * cx;
  r[0] = v[0] + 2.0 * (w * cx + dx); r[1] = v[1] + 2.0 * (w * cy + dy); r[2] = v[2] + 2.0 * (w * cz + dz);
}
// pose of hinge body b in its parent's frame (mj_kinematics, one body): position p, rotation q
// (the body's constants come in its record, loaded once by the caller: BodyK)
MRE_DEV void hinge_local_d(const BodyK& B, const Sm& s, double* p, double* q) {
  double q0[4], ql[4], ax[3], jp[3], t0[3], t1[3];
  for (int k = 0; k < 4; k++) q0[k] = (double)B.quat[k];
  for (int k = 0; k < 3; k++) { ax[k] = (double)B.jnt_axis[k]; jp[k] = (double)B.jnt_pos[k]; }
  const int qa = B.qposadr;
  // (the half angle of an arm joint reaches 1.9 rad: the polynomials are evaluated at a quarter of the angle, where
  //  their truncation is below 1e-16, and doubled)
  double s4, c4;
  sincos_poly_d(0.25 * (robot_q(s, qa) - (double)B.qpos0), s4, c4);
  const double sn = 2.0 * s4 * c4, cs = 1.0 - 2.0 * s4 * s4;
  ql[0] = cs; ql[1] = ax[0] * sn; ql[2] = ax[1] * sn; ql[3] = ax[2] * sn;
  dq_mul(q, q0, ql);
  const double n = rsq64(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int k = 0; k < 4; k++) q[k] *= n;
  dq_rot(t0, q0, jp);
  dq_rot(t1, q, jp);
  for (int k = 0; k < 3; k++) p[k] = (double)B.pos[k] + t0[k] - t1[k];
}
template <int CTRL>
MRE_DEV double dpp_row_d(double v, double fill) {   // the row shift CTRL of a double (two dwords), `fill` where the row has no source lane
  const long long b = __builtin_bit_cast(long long, v), f = __builtin_bit_cast(long long, fill);
  const int lo = __builtin_amdgcn_update_dpp((int)(f & 0xFFFFFFFFll), (int)(b & 0xFFFFFFFFll), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(f >> 32), (int)(b >> 32), CTRL, 0xF, 0xF, false);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned)lo);
}
MRE_DEV double readlane_d(double v, int lane) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xFFFFFFFFll), lane), hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned)lo);
}
MRE_DEV void dq2mat(double* m, const double* q) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  m[0] = w * w + x * x - y * y - z * z; m[1] = 2 * (x * y - w * z); m[2] = 2 * (x * z + w * y);
  m[3] = 2 * (x * y + w * z); m[4] = w * w - x * x + y * y - z * z; m[5] = 2 * (y * z - w * x);
  m[6] = 2 * (x * z - w * y); m[7] = 2 * (y * z + w * x); m[8] = w * w - x * x - y * y + z * z;
}
MRE_DEV double dpp_shr1_d(double v) {   // the value of lane l - 1 (same DPP row)
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xFFFFFFFFll), 0x111, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x111, 0xF, 0xF, false);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned)lo);
}
MRE_DEV double dpp_shl1_d(double v) {   // the value of lane l + 1 (same DPP row; 0 past the row)
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xFFFFFFFFll), 0x101, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x101, 0xF, 0xF, false);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned)lo);
}

// ------------------------------------------------------------ mj_kinematics
// A body frame in registers.
struct Frame { float p[3], q[4], m[9]; };

// The arm is a chain (body k hangs off body k - 1, one hinge each: mre_create checks the dof tree against
// ROBOT_DOF_PARENT).  Lane k computes link k's pose in its PARENT's frame (one hinge), and the world poses are the
// inclusive prefix products of those rigid transforms, (q, p) o (q', p') = (q q', p + R(q) p'), taken over lanes
// 1..7 in three DPP steps -- instead of seven dependent hinges evaluated by every lane.  A finger body sits one or
// two hinges below link 7: its lane evaluates its pose in link 7's frame (what gripper_local / connect_rows_local
// read as `gpose`) and composes it with link 7's world frame, read from lane 7; a cube's frame is its free joint's qpos.
//
// ROUND 5: the robot's frames are evaluated in fp64 from the double-float joint angles (robot_q) and rounded to float32
// ONCE, where they are stored.  Until round 4 the chain ran in float32 on the float32 words of the angles: seven
// float32 transforms leave link 7 3e-7 m / 2e-7 rad off, differently at every step, and that shake of the base of the
// few-gram finger links was the largest single source of the device-vs-oracle gap -- the fp64 oracle with ONLY its
// arm frames rounded link by link (mro_set_round32 bit 2048) is 1.5e-6 (median) / 2.2e-5 (90 %) / 1.9e-3 (99 %) off on
// the finger joints after 1000 steps of the bench law, the device was 9e-7 / 1.5e-5 / 1.1e-4, every other float32
// array of the pipeline rounded by itself stays 10 x below that, and the frames rounded once from an exact chain
// (bit 32768) cost 1.2e-7 / 1.7e-6 / 1.7e-5 (tests/diagnostics/arm_frame_study.py, profiles/r05a_arm_frame_study.log).
// writeback: store the normalised free-joint quaternions in qpos (mj_kinematics does); the
// query-only pass at the end of a launch must leave the state bits alone
MRE_DEV float dpp_shr(float v, float fill, int sh) {
  // value of lane l - sh within the row of 16 (fill where there is none)
  int r;
  const int vi = __builtin_bit_cast(int, v), fi = __builtin_bit_cast(int, fill);
  if (sh == 1) r = __builtin_amdgcn_update_dpp(fi, vi, 0x111, 0xF, 0xF, false);
  else if (sh == 2) r = __builtin_amdgcn_update_dpp(fi, vi, 0x112, 0xF, 0xF, false);
  else r = __builtin_amdgcn_update_dpp(fi, vi, 0x114, 0xF, 0xF, false);
  return __builtin_bit_cast(float, r);
}
template <int CTRL>
MRE_DEV void chain_step_d(double (&q)[4], double (&p)[3]) {
  // (q, p) <- (q, p) of the lane CTRL shifts below, composed with this lane's (identity where there is none)
  double aq[4], ap[3], nq[4], t[3];
  aq[0] = dpp_row_d<CTRL>(q[0], 1.0);
#pragma unroll
  for (int c = 1; c < 4; c++) aq[c] = dpp_row_d<CTRL>(q[c], 0.0);
#pragma unroll
  for (int c = 0; c < 3; c++) ap[c] = dpp_row_d<CTRL>(p[c], 0.0);
  dq_mul(nq, aq, q);
  dq_rot(t, aq, p);
#pragma unroll
  for (int c = 0; c < 4; c++) q[c] = nq[c];
#pragma unroll
  for (int c = 0; c < 3; c++) p[c] = ap[c] + t[c];
}
template <bool WRITEBACK>
MRE_DEV void kinematics(ModelP M, Sm& s, int l, BodyRegs& br, const BodyK& B) {
  constexpr int LINK7 = GRIP_BODY0 - 1;
  const bool arm = l >= 1 && l <= LINK7, fin = l >= GRIP_BODY0 && l < NRB;
  // (the lane's site, for the last part: its record is fetched now, with the body's)
  const auto* SR = &M->site_rec[l < NSITE ? l : 0];
  const int site_b = SR->body, eef_site = M->opt_rec.eef_site;
  const float site_pos[3] = {SR->pos[0], SR->pos[1], SR->pos[2]};
  const float site_quat[4] = {SR->quat[0], SR->quat[1], SR->quat[2], SR->quat[3]};
  // ---- every robot body in its parent's frame (fp64; identity elsewhere)
  double q[4] = {1.0, 0.0, 0.0, 0.0}, p[3] = {0.0, 0.0, 0.0};
  if (arm || fin) hinge_local_d(B, s, p, q);
  // a finger body that hangs off another finger body (9, 11, 13, 15 off 8, 10, 12, 14: the dof tree mre_create
  // checks) takes its parent's pose from the lane below: its pose in link 7's frame
  {
    double pp[3], pq[4];
#pragma unroll
    for (int k = 0; k < 3; k++) pp[k] = dpp_shr1_d(p[k]);
#pragma unroll
    for (int k = 0; k < 4; k++) pq[k] = dpp_shr1_d(q[k]);
    if (fin) {
      if (B.parent >= GRIP_BODY0) {
        double t[3], q2[4];
        dq_rot(t, pq, p);
#pragma unroll
        for (int k = 0; k < 3; k++) p[k] = pp[k] + t[k];
        dq_mul(q2, pq, q);
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = q2[k];
      }
#pragma unroll
      for (int k = 0; k < 3; k++) s.gpose[l - GRIP_BODY0][k] = p[k];
#pragma unroll
      for (int k = 0; k < 4; k++) s.gpose[l - GRIP_BODY0][3 + k] = q[k];
    }
  }
  // ---- arm: inclusive prefix product over lanes 1..7 (shifts 1, 2, 4 inside the DPP row; lane 0 is the identity).
  // The finger lanes run the same instructions on a copy that is thrown away (their own (q, p) is kept aside).
  double wq[4], wp[3];
#pragma unroll
  for (int k = 0; k < 4; k++) wq[k] = arm ? q[k] : (k == 0 ? 1.0 : 0.0);
#pragma unroll
  for (int k = 0; k < 3; k++) wp[k] = arm ? p[k] : 0.0;
  chain_step_d<0x111>(wq, wp);
  chain_step_d<0x112>(wq, wp);
  chain_step_d<0x114>(wq, wp);
  {  // fingers: link 7's world frame (lane 7) composed with the pose in its frame
    double q7[4], p7[3];
#pragma unroll
    for (int k = 0; k < 4; k++) q7[k] = readlane_d(wq[k], LINK7);
#pragma unroll
    for (int k = 0; k < 3; k++) p7[k] = readlane_d(wp[k], LINK7);
    if (fin) {
      double t[3];
      dq_rot(t, q7, p);
      dq_mul(wq, q7, q);
#pragma unroll
      for (int k = 0; k < 3; k++) wp[k] = p7[k] + t[k];
    }
  }
  Frame mine;
  v3zero(br.anchor); v3zero(br.axis);
  v3zero(br.xipos);
  const int b = l < NB ? l : 0;
  if (arm || fin) {
    // world frame, joint anchor and axis, inertial frame: fp64, each rounded once
    const double n = rsq64(wq[0] * wq[0] + wq[1] * wq[1] + wq[2] * wq[2] + wq[3] * wq[3]);
#pragma unroll
    for (int k = 0; k < 4; k++) wq[k] *= n;
    double Rm[9], t[3], qi[4];
    dq2mat(Rm, wq);
#pragma unroll
    for (int k = 0; k < 4; k++) mine.q[k] = (float)wq[k];
#pragma unroll
    for (int k = 0; k < 3; k++) mine.p[k] = (float)wp[k];
#pragma unroll
    for (int k = 0; k < 9; k++) mine.m[k] = (float)Rm[k];
    const double jp[3] = {(double)B.jnt_pos[0], (double)B.jnt_pos[1], (double)B.jnt_pos[2]};
    const double ax[3] = {(double)B.jnt_axis[0], (double)B.jnt_axis[1], (double)B.jnt_axis[2]};
    const double ip[3] = {(double)B.ipos[0], (double)B.ipos[1], (double)B.ipos[2]};
    const double iq[4] = {(double)B.iquat[0], (double)B.iquat[1], (double)B.iquat[2], (double)B.iquat[3]};
#pragma unroll
    for (int r = 0; r < 3; r++) {
      // the joint anchor is fixed in the body: x + R jnt_pos; a rotation about the axis leaves the axis where it was
      br.anchor[r] = (float)(wp[r] + Rm[3 * r] * jp[0] + Rm[3 * r + 1] * jp[1] + Rm[3 * r + 2] * jp[2]);
      br.axis[r] = (float)(Rm[3 * r] * ax[0] + Rm[3 * r + 1] * ax[1] + Rm[3 * r + 2] * ax[2]);
      br.xipos[r] = (float)(wp[r] + Rm[3 * r] * ip[0] + Rm[3 * r + 1] * ip[1] + Rm[3 * r + 2] * ip[2]);
    }
    dq_mul(qi, wq, iq);
    dq2mat(Rm, qi);
#pragma unroll
    for (int k = 0; k < 9; k++) br.ximat[k] = (float)Rm[k];
    (void)t;
  }
  if (l >= NRB && l < NB) {   // cubes: free joints
    const int qa = B.qposadr;
    v3copy(mine.p, &s.qpos[qa]);
    for (int k = 0; k < 4; k++) mine.q[k] = s.qpos[qa + 3 + k];
    // mj_kinematics normalises the quaternion in qpos.  The state is a double-float pair that the integrator keeps at
    // unit length to 1e-16 (the float32 word alone is off by its rounding, 6e-8): only a quaternion that is really not
    // normalised -- handed in by the caller, whose low words are zero -- is written back.
    const float n2 = mine.q[0] * mine.q[0] + mine.q[1] * mine.q[1] + mine.q[2] * mine.q[2] + mine.q[3] * mine.q[3];
    qnormalize(mine.q);
    if (WRITEBACK && fabsf(n2 - 1.f) > 1e-5f) for (int k = 0; k < 4; k++) s.qpos[qa + 3 + k] = mine.q[k];
    q2mat(mine.m, mine.q);
    v3copy(br.anchor, mine.p);
    br.axis[0] = 0.f; br.axis[1] = 0.f; br.axis[2] = 1.f;
  }
  if (l == 0) {   // the world body
    v3zero(mine.p);
    mine.q[0] = 1.f; mine.q[1] = mine.q[2] = mine.q[3] = 0.f;
    q2mat(mine.m, mine.q);
    q2mat(br.ximat, mine.q);
  }
  if (l < NB) {
    v3copy(s.xpos[b], mine.p);
    for (int k = 0; k < 4; k++) s.xquat[b][k] = mine.q[k];
    for (int k = 0; k < 9; k++) s.xmat[b][k] = mine.m[k];
    if (l >= NRB) {   // cubes: the inertial frame from the float32 frame (robot bodies: above, fp64)
      float tmp[3], qi[4];
      m3mulv(tmp, mine.m, B.ipos);
      v3add(br.xipos, mine.p, tmp);
      qmul(qi, mine.q, B.iquat);
      q2mat(br.ximat, qi);
    }
  }
  MRE_SYNC();
  // sites (lane = site)
  if (l < NSITE) {
    const int b = site_b;
    float tmp[3], q[4];
    m3mulv(tmp, s.xmat[b], site_pos);
    v3add(s.site_xpos[l], s.xpos[b], tmp);
    qmul(q, s.xquat[b], site_quat);
    if (l == eef_site) q2mat(s.site_xmat[0], q);
  }
  keep_live(site_b); keep_live(eef_site);
#pragma unroll
  for (int k = 0; k < 3; k++) keep_live(site_pos[k]);
#pragma unroll
  for (int k = 0; k < 4; k++) keep_live(site_quat[k]);
}

// ---------------------------------------------------------------- mj_comPos
MRE_DEV void com_pos(ModelP M, Sm& s, int l, const BodyRegs& br, const BodyK& B, float robot_mass) {
  const bool robot = (l >= 1 && l < NRB);
  float mass = 0.f;
  if (l < NB) mass = (B.propid >= 0) ? s.prop_mass[B.propid] : B.mass;
  float c0 = robot ? mass * br.xipos[0] : 0.f;
  float c1 = robot ? mass * br.xipos[1] : 0.f;
  float c2 = robot ? mass * br.xipos[2] : 0.f;
  wave_sum3(c0, c1, c2);
  const float inv = 1.0f / robot_mass;
  float com[3] = {c0 * inv, c1 * inv, c2 * inv};
  if (l == 0) v3copy(s.com_robot, com);
  if (l >= 1 && l < NB) {
    const int b = l, pid = B.propid;
    if (pid >= 0) v3copy(com, br.xipos);  // each cube is its own tree: subtree COM = own COM
    float inertia[3];
    if (pid >= 0) v3copy(inertia, s.prop_inertia[pid]); else v3copy(inertia, B.inertia);
    float dif[3], tmp[9];
    v3sub(dif, br.xipos, com);
    const float* mat = br.ximat;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++)
        tmp[3 * r + c] = mat[3 * r] * inertia[0] * mat[3 * c] + mat[3 * r + 1] * inertia[1] * mat[3 * c + 1] +
                         mat[3 * r + 2] * inertia[2] * mat[3 * c + 2];
    float* ci = s.cinert[b];
    ci[0] = tmp[0] + mass * (dif[1] * dif[1] + dif[2] * dif[2]);
    ci[1] = tmp[4] + mass * (dif[0] * dif[0] + dif[2] * dif[2]);
    ci[2] = tmp[8] + mass * (dif[0] * dif[0] + dif[1] * dif[1]);
    ci[3] = tmp[1] - mass * dif[0] * dif[1];
    ci[4] = tmp[2] - mass * dif[0] * dif[2];
    ci[5] = tmp[5] - mass * dif[1] * dif[2];
    ci[6] = mass * dif[0]; ci[7] = mass * dif[1]; ci[8] = mass * dif[2]; ci[9] = mass;
    // cdof (mju_dofCom)
    const int da = B.dofadr;
    float off[3];
    v3sub(off, com, br.anchor);
    if (pid < 0) {
      v3copy(s.cdof[da], br.axis);
      v3cross(s.cdof[da] + 3, br.axis, off);
    }
    // cube cdofs are not stored: translation k = [0; e_k], rotation k = [xmat column k; 0]
    // (each cube is its own tree, c-frame origin = its COM) -- see prop_cdof()
  }
  if (l == 0) for (int k = 0; k < 10; k++) s.cinert[0][k] = 0.f;
}

// S1a: kinematics + comPos as one real function so that the per-lane body frame registers
// (anchor, axis, inertial frame) never leave the register file
MRE_PHASE_FN void position_stage(ModelP M, Sm& s, int l) {
  MRE_DBG_T0();
  BodyRegs br;
  const BodyK B = load_body(M, l < NB ? l : 0);
  const float robot_mass = M->opt_rec.robot_mass;
  kinematics<true>(M, s, l, br, B);
  MRE_DBG_STAMP(5, 0);
  com_pos(M, s, l, br, B, robot_mass);
  MRE_SYNC();
  MRE_DBG_STAMP(5, 1);
}
// kinematics only (site queries at the end of a launch)
MRE_PHASE_FN void kinematics_only(ModelP M, Sm& s, int l) {
  BodyRegs br;
  const BodyK B = load_body(M, l < NB ? l : 0);
  kinematics<false>(M, s, l, br, B);
  MRE_SYNC();
}

// cdof of cube body b, local dof j (mju_dofCom with zero offset)
MRE_DEV void prop_cdof(const Sm& s, int b, int j, float* c) {
  c[0] = c[1] = c[2] = c[3] = c[4] = c[5] = 0.f;
  if (j < 3) {
    c[3 + j] = 1.f;
  } else {
    const int k = j - 3;
    c[0] = s.xmat[b][k]; c[1] = s.xmat[b][3 + k]; c[2] = s.xmat[b][6 + k];
  }
}

// spatial inertia (10) of body c about point O, axes of the frame its pose (p, q) is given in
MRE_DEV void inert_about_d(const BodyK& B, const double* p, const double* q, const double* O, double* ci) {
  double ip[3] = {(double)B.ipos[0], (double)B.ipos[1], (double)B.ipos[2]}, t[3], qi[4];
  double iq[4] = {(double)B.iquat[0], (double)B.iquat[1], (double)B.iquat[2], (double)B.iquat[3]};
  dq_rot(t, q, ip);
  const double d[3] = {p[0] + t[0] - O[0], p[1] + t[1] - O[1], p[2] + t[2] - O[2]};
  dq_mul(qi, q, iq);
  // rotation matrix columns of qi
  double R[9];
  {
    const double w = qi[0], x = qi[1], y = qi[2], z = qi[3];
    R[0] = w * w + x * x - y * y - z * z; R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
    R[3] = 2 * (x * y + w * z); R[4] = w * w - x * x + y * y - z * z; R[5] = 2 * (y * z - w * x);
    R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = w * w - x * x - y * y + z * z;
  }
  const double m = (double)B.mass;
  const double in[3] = {(double)B.inertia[0], (double)B.inertia[1], (double)B.inertia[2]};
  double T[9];
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++)
      T[3 * r + k] = R[3 * r] * in[0] * R[3 * k] + R[3 * r + 1] * in[1] * R[3 * k + 1] + R[3 * r + 2] * in[2] * R[3 * k + 2];
  ci[0] += T[0] + m * (d[1] * d[1] + d[2] * d[2]);
  ci[1] += T[4] + m * (d[0] * d[0] + d[2] * d[2]);
  ci[2] += T[8] + m * (d[0] * d[0] + d[1] * d[1]);
  ci[3] += T[1] - m * d[0] * d[1];
  ci[4] += T[2] - m * d[0] * d[2];
  ci[5] += T[5] - m * d[1] * d[2];
  ci[6] += m * d[0]; ci[7] += m * d[1]; ci[8] += m * d[2]; ci[9] += m;
}

// lane = finger body: its subtree's spatial inertia and its cdof about the pinch site, in the frame
// of the arm's last link, and the momentum map P = crb * cdof that the finger rows of M are built
// from (crb_mass_matrix).  Chains below the arm are at most two bodies deep (checked in mre_create).
MRE_PHASE_FN void gripper_local(ModelP M, Sm& s, int l) {
  const bool fin = l >= GRIP_BODY0 && l < NRB;
  const int b = fin ? l : GRIP_BODY0;
  // the body's record and the pinch site: one group of loads, issued before the pose is read from LDS
  const BodyK B = load_body(M, b);
  const float tcp[3] = {M->opt_rec.tcp_pos[0], M->opt_rec.tcp_pos[1], M->opt_rec.tcp_pos[2]};
  const double* pose = s.gpose[b - GRIP_BODY0];
  const double p[3] = {pose[0], pose[1], pose[2]}, q[4] = {pose[3], pose[4], pose[5], pose[6]};
  const double O[3] = {(double)tcp[0], (double)tcp[1], (double)tcp[2]};
  // the body's own spatial inertia; a body off link 7 adds its child's, which the lane above has just computed
  // (bodies 9, 11, 13, 15 hang off 8, 10, 12, 14: the dof tree mre_create checks)
  double ci[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (fin) inert_about_d(B, p, q, O, ci);
  double up[10];
#pragma unroll
  for (int k = 0; k < 10; k++) up[k] = dpp_shl1_d(ci[k]);
  if (fin) {
#pragma unroll
    for (int k = 0; k < 10; k++) s.gI[b - GRIP_BODY0][k] = ci[k];
    if (B.parent < GRIP_BODY0 && (b & 1) == 0) {   // (the odd body above hangs off this one: mre_create checks the body tree)
#pragma unroll
      for (int k = 0; k < 10; k++) ci[k] += up[k];
    }
    double ax[3] = {(double)B.jnt_axis[0], (double)B.jnt_axis[1], (double)B.jnt_axis[2]};
    double jp[3] = {(double)B.jnt_pos[0], (double)B.jnt_pos[1], (double)B.jnt_pos[2]};
    double u[3], a[3];
    dq_rot(u, q, ax);
    dq_rot(a, q, jp);
    const double r[3] = {O[0] - p[0] - a[0], O[1] - p[1] - a[1], O[2] - p[2] - a[2]};
    const double cd[6] = {u[0], u[1], u[2], u[1] * r[2] - u[2] * r[1], u[2] * r[0] - u[0] * r[2], u[0] * r[1] - u[1] * r[0]};
    double P[6];
    P[0] = ci[0] * cd[0] + ci[3] * cd[1] + ci[4] * cd[2] - ci[8] * cd[4] + ci[7] * cd[5];
    P[1] = ci[3] * cd[0] + ci[1] * cd[1] + ci[5] * cd[2] + ci[8] * cd[3] - ci[6] * cd[5];
    P[2] = ci[4] * cd[0] + ci[5] * cd[1] + ci[2] * cd[2] - ci[7] * cd[3] + ci[6] * cd[4];
    P[3] = ci[8] * cd[1] - ci[7] * cd[2] + ci[9] * cd[3];
    P[4] = ci[6] * cd[2] - ci[8] * cd[0] + ci[9] * cd[4];
    P[5] = ci[7] * cd[0] - ci[6] * cd[1] + ci[9] * cd[5];
    for (int k = 0; k < 6; k++) { s.gC[b - GRIP_BODY0][k] = (float)cd[k]; s.gP[b - GRIP_BODY0][k] = (float)P[k]; s.gS[b - GRIP_BODY0][k] = cd[k]; }
  }
  MRE_SYNC();
}

// One side of a `connect` constraint in the frame of the arm's last link: the anchor point x of body
// b and, for the finger dofs on the way up (b, then its parent if that is a finger body), the lever
// vectors u_c x (x - a_c) (axis u_c, joint anchor a_c), times `sign`.
// (par: b's parent; H[0], H[1]: joint axis and anchor of b and of its parent, loaded by the caller)
struct HingeK { float ax[3], jp[3]; };
MRE_DEV HingeK load_hinge(ModelP M, int b) {
  const auto* R = &M->body_rec[b];
  HingeK H;
#pragma unroll
  for (int k = 0; k < 3; k++) { H.ax[k] = R->jnt_axis[k]; H.jp[k] = R->jnt_pos[k]; }
  return H;
}
MRE_DEV void connect_side_d(const Sm& s, int b, int par, const HingeK (&H)[2], const float* a, double sign, double* x,
                            double (*vec)[3]) {
  const double* pose = s.gpose[b - GRIP_BODY0];
  const double al[3] = {(double)a[0], (double)a[1], (double)a[2]};
  double t[3];
  dq_rot(t, pose + 3, al);
  for (int k = 0; k < 3; k++) x[k] = pose[k] + t[k];
#pragma unroll
  for (int m = 0; m < 2; m++) {
    vec[m][0] = vec[m][1] = vec[m][2] = 0.0;
    const int c = m == 0 ? b : par;
    if (c < GRIP_BODY0) break;
    const double* cp = s.gpose[c - GRIP_BODY0];
    const double ax[3] = {(double)H[m].ax[0], (double)H[m].ax[1], (double)H[m].ax[2]};
    const double jp[3] = {(double)H[m].jp[0], (double)H[m].jp[1], (double)H[m].jp[2]};
    double u[3], ja[3];
    dq_rot(u, cp + 3, ax);
    dq_rot(ja, cp + 3, jp);
    const double r[3] = {x[0] - cp[0] - ja[0], x[1] - cp[1] - ja[1], x[2] - cp[2] - ja[2]};
    vec[m][0] = sign * (u[1] * r[2] - u[2] * r[1]);
    vec[m][1] = sign * (u[2] * r[0] - u[0] * r[2]);
    vec[m][2] = sign * (u[0] * r[1] - u[1] * r[0]);
  }
}

// The two `connect` rows of the finger linkage, evaluated in the frame of the arm's last link in
// fp64 (lanes 0, 1 = the two constraints).  Their residual is a 1e-5 m difference of two anchor
// positions and their Jacobian entries are 0.03 m levers: taken from the fp32 world poses
// (|x| ~ 0.8 m) both carry 3..6e-8 m of rounding, which the stiff reference acceleration
// (K = 4e4 1/s^2) and the 25 N the rows transmit turn into torque noise on links of a few grams
// (measured: finger accelerations 3e-3 rad/s^2 off the fp64 oracle per step, finger joints
// 1e-4 .. 3e-2 rad off after 1000 steps; the same noise injected into the oracle reproduces it).
// Results go to the head of qfrc_con (dead between integrate and the next solve), 16 floats per
// constraint: [0:3] residual, [4 + 3 m : 7 + 3 m] lever vector of finger dof m (body1, its parent,
// body2, its parent; zero where the chain is shorter), all in the arm link's axes.
MRE_PHASE_FN void connect_rows_local(ModelP M, Sm& s, int l) {
  // the constraint's record, then the hinges of its two bodies and their parents: two trips to memory
  const auto* E = &M->eq_rec[l < 2 ? l : 0];
  const int type = E->type, b1 = E->b1, b2 = E->b2, pb1 = E->pb1, pb2 = E->pb2;
  float data[6];
#pragma unroll
  for (int k = 0; k < 6; k++) data[k] = E->data[k];
  // (a parent above the fingers takes no part: its slot repeats the body's own hinge, unused)
  const HingeK H1[2] = {load_hinge(M, b1), load_hinge(M, pb1 >= GRIP_BODY0 ? pb1 : b1)};
  const HingeK H2[2] = {load_hinge(M, b2), load_hinge(M, pb2 >= GRIP_BODY0 ? pb2 : b2)};
  if (l < 2 && type == 0) {
    double x1[3], x2[3], v1[2][3], v2[2][3];
    connect_side_d(s, b1, pb1, H1, data, 1.0, x1, v1);
    connect_side_d(s, b2, pb2, H2, data + 3, -1.0, x2, v2);
    float* o = &s.qfrc_con[16 * l];
    for (int k = 0; k < 3; k++) {
      o[k] = (float)(x1[k] - x2[k]);
      o[4 + k] = (float)v1[0][k]; o[7 + k] = (float)v1[1][k];
      o[10 + k] = (float)v2[0][k]; o[13 + k] = (float)v2[1][k];
    }
  }
  MRE_SYNC();
}

// Sums along the robot's body tree with lane = body (lanes 0..15 of the first DPP row; lane 0 = the world, which
// contributes nothing).  The tree is the one the kernels are unrolled for (ROBOT_DOF_PARENT, checked in mre_create):
// the arm is the chain 1..7, and below link 7 hang four two-body fingers (8 -> 9, 10 -> 11, 12 -> 13, 14 -> 15).
//   tree_prefix: x_b <- sum of x over b and its ancestors     (mj_comVel's accumulation down the tree)
//   tree_suffix: x_b <- sum of x over b and its descendants   (mj_rne's / mj_crb's accumulation up the tree)
// Row shifts instead of one loop per lane over its chain / its descendants; the order of the additions differs from
// the loops' (last-bit rounding).
constexpr bool robot_tree_is_chain_plus_two_body_fingers() {
  for (int d = 0; d < NRV; d++) {
    const int b = d + 1;   // body of dof d
    const int want = b < GRIP_BODY0 ? d - 1 : ((b & 1) ? d - 1 : GRIP_BODY0 - 2);
    if (ROBOT_DOF_PARENT[d] != want) return false;
  }
  return true;
}
static_assert(GRIP_BODY0 % 2 == 0 && NRB == 16 && robot_tree_is_chain_plus_two_body_fingers(),
              "tree_prefix / tree_suffix / the prefix kinematics are written for this body tree");
template <int CTRL>
MRE_DEV float dpp_row(float v) {  // lane's source by the row shift CTRL, 0 where the row has no such lane
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
template <int N>
MRE_DEV void tree_prefix(float (&x)[N], int l) {
  constexpr int LINK7 = GRIP_BODY0 - 1;
  float own[N], par[N];
#pragma unroll
  for (int c = 0; c < N; c++) { own[c] = x[c]; par[c] = dpp_row<0x111>(x[c]); }
#pragma unroll
  for (int c = 0; c < N; c++) x[c] += dpp_row<0x111>(x[c]);
#pragma unroll
  for (int c = 0; c < N; c++) x[c] += dpp_row<0x112>(x[c]);
#pragma unroll
  for (int c = 0; c < N; c++) x[c] += dpp_row<0x114>(x[c]);
  const bool finger = l >= GRIP_BODY0 && l < NRB, leaf = (l & 1) != 0;   // (bodies 9, 11, 13, 15 hang off 8, 10, 12, 14)
#pragma unroll
  for (int c = 0; c < N; c++) {
    const float p7 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x[c]), LINK7));
    x[c] = finger ? (p7 + (leaf ? par[c] : 0.f)) + own[c] : x[c];
  }
}
template <int N>
MRE_DEV void tree_suffix(float (&x)[N], int l) {
  float own[N], nxt[N];
#pragma unroll
  for (int c = 0; c < N; c++) { own[c] = x[c]; nxt[c] = dpp_row<0x101>(x[c]); }
#pragma unroll
  for (int c = 0; c < N; c++) x[c] += dpp_row<0x101>(x[c]);
#pragma unroll
  for (int c = 0; c < N; c++) x[c] += dpp_row<0x102>(x[c]);
#pragma unroll
  for (int c = 0; c < N; c++) x[c] += dpp_row<0x104>(x[c]);
#pragma unroll
  for (int c = 0; c < N; c++) x[c] += dpp_row<0x108>(x[c]);
  const bool finger = l >= GRIP_BODY0 && l < NRB, leaf = (l & 1) != 0;
#pragma unroll
  for (int c = 0; c < N; c++) x[c] = finger ? (leaf ? own[c] : own[c] + nxt[c]) : x[c];
}

// ------------------------------------------------------- mj_crb (robot block)
MRE_DEV void crb_mass_matrix(ModelP M, Sm& s, int l) {
  const int tcp_site = M->opt_rec.tcp_site;
  {  // composite inertia of every robot body = its own plus its descendants' (lane = body, tree_suffix)
    float acc[10];
#pragma unroll
    for (int k = 0; k < 10; k++) acc[k] = (l >= 1 && l < NRB) ? s.cinert[l][k] : 0.f;
    tree_suffix(acc, l);
    if (l >= 1 && l < NRB) {
#pragma unroll
      for (int k = 0; k < 10; k++) s.crb[l][k] = acc[k];
    }
  }
  MRE_SYNC();
  for (int e = l; e < NMR; e += 64) {
    const auto* R = &M->m_rec[e];   // (i, j, armature of dof i: one 16-byte load)
    const int i = R->i, j = R->j;
    const float armature = R->armature;
    float v;
    if (i >= GRIP_BODY0 - 1) {
      // rows of the finger dofs: momentum map of the finger subtree from gripper_local (fp64, frame
      // of the arm's last link, about the pinch site); an arm dof j is moved to the same point / axes
      const int root = GRIP_BODY0 - 1;   // body id of the arm's last link = dof id of the first finger dof
      float cj[6];
      if (j >= GRIP_BODY0 - 1) {
        for (int k = 0; k < 6; k++) cj[k] = s.gC[j - (GRIP_BODY0 - 1)][k];
      } else {
        float off[3], t[3], lin[3];
        v3sub(off, s.site_xpos[tcp_site], s.com_robot);
        v3cross(t, s.cdof[j], off);
        v3add(lin, s.cdof[j] + 3, t);
        m3tmulv(cj, s.xmat[root], s.cdof[j]);
        m3tmulv(cj + 3, s.xmat[root], lin);
      }
      v = dot6(cj, s.gP[i - (GRIP_BODY0 - 1)]);
    } else {
      float buf[6];
      mul_inert_vec(buf, s.crb[i + 1], s.cdof[i]);   // (robot dof i belongs to body i + 1: mre_create checks)
      v = dot6(s.cdof[j], buf);
    }
    if (i == j) v += armature;
    s.qM[e] = v;
  }
}

// x <- M^-1 x with x in registers: mj_solveLD unrolled over the compile-time dof tree
// (ROBOT_DOF_PARENT), every lane solving its own right-hand side; the factor entries are LDS
// reads at constant offsets.  Same operations in the same order as mj_solveLD.
typedef const __attribute__((address_space(3))) float* lds_cfloat_p;
template <int I, int K, class F>
MRE_DEV void solve_regs_back(float (&x)[NRV], const F& LD, float xi) {
  constexpr int j = robot_dof_anc(I, K);
  if constexpr (j >= 0) {
    constexpr int adr = robot_dof_madr(I) + 1 + K;
    x[j] -= LD[adr] * xi;
    solve_regs_back<I, K + 1, F>(x, LD, xi);
  }
}
template <int I, class F>
MRE_DEV void solve_regs_back_rows(float (&x)[NRV], const F& LD) {
  solve_regs_back<I, 0, F>(x, LD, x[I]);
  __builtin_amdgcn_sched_barrier(0);  // keep the factor reads of later rows out of the live set
  if constexpr (I > 0) solve_regs_back_rows<I - 1, F>(x, LD);
}
template <int I, int K, class F>
MRE_DEV void solve_regs_fwd(float (&x)[NRV], const F& LD, float& xi) {
  constexpr int j = robot_dof_anc(I, K);
  if constexpr (j >= 0) {
    constexpr int adr = robot_dof_madr(I) + 1 + K;
    xi -= LD[adr] * x[j];
    solve_regs_fwd<I, K + 1, F>(x, LD, xi);
  }
}
template <int I, class F>
MRE_DEV void solve_regs_fwd_rows(float (&x)[NRV], const F& LD) {
  float xi = x[I];
  solve_regs_fwd<I, 0, F>(x, LD, xi);
  x[I] = xi;
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (I + 1 < NRV) solve_regs_fwd_rows<I + 1, F>(x, LD);
}
MRE_DEV void solve_robot_regs(const float* LD_, const float* dinv_, float (&x)[NRV]) {
  // explicit LDS pointers, opaque to loop strength reduction: every factor entry is then one
  // ds_read at base + immediate offset (otherwise each address is hoisted into a register of its own)
  lds_cfloat_p LD = (lds_cfloat_p)LD_;
  lds_cfloat_p dinv = (lds_cfloat_p)dinv_;
  asm volatile("" : "+v"(LD), "+v"(dinv));
  solve_regs_back_rows<NRV - 1, lds_cfloat_p>(x, LD);
#pragma unroll
  for (int i = 0; i < NRV; i++) x[i] *= dinv[i];
  solve_regs_fwd_rows<0, lds_cfloat_p>(x, LD);
}

// mj_factorM on the robot block with the matrix in registers: every lane runs the whole
// elimination (312 multiply-adds, unrolled over the compile-time dof tree) on its own copy, which
// replaces 15 lock-step elimination rounds of table loads + LDS round trips; the wave then stores
// the factor (all lanes hold the same values).  Same operations as mj_factorM: for k = nv-1..0, for
// every ancestor i of k: tmp = L(k,i) / L(k,k), row i -= tmp * row k (ancestors of i), L(k,i) = tmp.
typedef __attribute__((address_space(3))) float* lds_float_p;
template <int K, int P, int Q>
MRE_DEV void factor_regs_upd(float (&A)[NMR], float tmp) {
  if constexpr (Q <= robot_dof_depth(K)) {
    constexpr int i = robot_dof_anc(K, P - 1);
    constexpr int dst = robot_dof_madr(i) + (Q - P), src = robot_dof_madr(K) + Q;
    A[dst] -= tmp * A[src];
    factor_regs_upd<K, P, Q + 1>(A, tmp);
  }
}
template <int K, int P>
MRE_DEV void factor_regs_anc(float (&A)[NMR], float inv) {
  if constexpr (P <= robot_dof_depth(K)) {
    constexpr int kp = robot_dof_madr(K) + P;
    const float tmp = A[kp] * inv;
    factor_regs_upd<K, P, P>(A, tmp);
    A[kp] = tmp;
    factor_regs_anc<K, P + 1>(A, inv);
  }
}
template <int K, class D>
MRE_DEV void factor_regs_rows(float (&A)[NMR], D& dinv) {
  constexpr int kk = robot_dof_madr(K);
  const float inv = 1.0f / A[kk];
  dinv[K] = inv;
  factor_regs_anc<K, 1>(A, inv);
  if constexpr (K > 0) factor_regs_rows<K - 1, D>(A, dinv);
}
// src: the matrix (qM, or M - h dF/dv already formed in LD); LD / dinv: factor and 1/D (all LDS)
MRE_DEV void factor_robot_regs(const float* src_, float* LD_, float* dinv_) {
  lds_cfloat_p src = (lds_cfloat_p)src_;
  lds_float_p LD = (lds_float_p)LD_, dinv = (lds_float_p)dinv_;
  asm volatile("" : "+v"(src), "+v"(LD), "+v"(dinv));
  float A[NMR];
#pragma unroll
  for (int e = 0; e < NMR; e++) A[e] = src[e];
  factor_regs_rows<NRV - 1, lds_float_p>(A, dinv);
#pragma unroll
  for (int e = 0; e < NMR; e++) LD[e] = A[e];
  MRE_SYNC();
}

// One right-hand side through the register-resident solve: every lane runs mj_solveLD on its own copy (the
// factor entries are broadcast LDS reads at constant offsets, issued ahead of the dependent chain) and lane i
// keeps component i.  Same operations in the same order as the serial routine; it replaced a level-parallel
// form (lane = dof, 9 tree levels up and 9 down, an LDS round trip per level) at a third of the instructions.
MRE_DEV void solve_robot_one(const float* LD, const float* dinv, float* xv, int l) {
  float x[NRV];
#pragma unroll
  for (int i = 0; i < NRV; i++) x[i] = xv[i];
  solve_robot_regs(LD, dinv, x);
  MRE_SYNC();
  float mine = 0.f;
#pragma unroll
  for (int i = 0; i < NRV; i++) mine = (l == i) ? x[i] : mine;
  if (l < NRV) xv[l] = mine;
  MRE_SYNC();
}

// Factor and one solve in one go, nothing stored: the implicit integrator's M - h dF/dv is factored for the single
// solve that follows it, so the factor never needs to leave the registers (saves the 111 LDS stores of the factor
// and the 111 loads of the solve).  src: the matrix, xv: right-hand side in, solution out (lane i keeps component i).
MRE_DEV void factor_solve_robot(const float* src_, float* xv, int l) {
  lds_cfloat_p src = (lds_cfloat_p)src_;
  asm volatile("" : "+v"(src));
  float A[NMR], dv[NRV], x[NRV];
#pragma unroll
  for (int e = 0; e < NMR; e++) A[e] = src[e];
#pragma unroll
  for (int i = 0; i < NRV; i++) x[i] = xv[i];
  factor_regs_rows<NRV - 1, float[NRV]>(A, dv);
  solve_regs_back_rows<NRV - 1, float[NMR]>(x, A);
#pragma unroll
  for (int i = 0; i < NRV; i++) x[i] *= dv[i];
  solve_regs_fwd_rows<0, float[NMR]>(x, A);
  MRE_SYNC();
  float mine = 0.f;
#pragma unroll
  for (int i = 0; i < NRV; i++) mine = (l == i) ? x[i] : mine;
  if (l < NRV) xv[l] = mine;
  MRE_SYNC();
}

}  // namespace mre
#include "mre_solver.h"
#ifdef MRE_NEWTON
#include "mre_newton.h"
#endif
#include "mre_osc.h"
namespace mre {

// ------------------------------------------------ mj_comVel + mj_rne + mj_passive
MRE_PHASE_FN void velocity_stage(ModelP M, Sm& s, int l) {
  constexpr int LINK7 = GRIP_BODY0 - 1;
  const bool rob = l >= 1 && l < NRB;   // lane = robot body l, whose hinge is dof l - 1
  // the model constants of the phase -- gravity, and for the last part (lane = dof) the dof's body, that body's first
  // dof and prop id -- in one group of loads
  const auto* DR = &M->dof_rec[l < NV ? l : 0];
  const int dof_b = DR->body, dof_pid = DR->propid, dof_da = DR->dofadr;
  const float grav[3] = {M->opt_rec.gravity[0], M->opt_rec.gravity[1], M->opt_rec.gravity[2]};
  // ---- robot: cvel, cdof_dot, cacc in registers (mj_comVel, mj_rne forward pass)
  float cd[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, qv = 0.f;
  if (rob) {
#pragma unroll
    for (int t = 0; t < 6; t++) cd[t] = s.cdof[l - 1][t];
    qv = s.qvel[l - 1];
  }
  float cv[6];
#pragma unroll
  for (int t = 0; t < 6; t++) cv[t] = cd[t] * qv;
  tree_prefix(cv, l);
  // the parent's velocity: the lane below, except for the bodies that hang off link 7
  float pv[6];
  {
    const bool off7 = l >= GRIP_BODY0 && l < NRB && (l & 1) == 0;
#pragma unroll
    for (int t = 0; t < 6; t++) {
      const float below = dpp_row<0x111>(cv[t]);
      const float v7 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cv[t]), LINK7));
      pv[t] = off7 ? v7 : below;
    }
  }
  float cdd[6], ca[6];
  cross_motion(cdd, pv, cd);
#pragma unroll
  for (int t = 0; t < 6; t++) ca[t] = cdd[t] * qv;
  tree_prefix(ca, l);
  // ---- cubes: free joints (lane = body)
  if (l >= NRB && l < NB) {
    const int b = l;
#pragma unroll
    for (int t = 0; t < 6; t++) { cv[t] = 0.f; ca[t] = 0.f; }
    const int da = NRV + 6 * (b - NRB);   // (a cube's first dof: the layout mre_create checks)
#pragma unroll
    for (int j = 0; j < 3; j++) cv[3 + j] += s.qvel[da + j];
    float cdot[3][6];
#pragma unroll
    for (int j = 3; j < 6; j++) {
      float c6[6];
      prop_cdof(s, b, j, c6);
      cross_motion(cdot[j - 3], cv, c6);
    }
#pragma unroll
    for (int j = 3; j < 6; j++) {
      float c6[6];
      prop_cdof(s, b, j, c6);
      const float q = s.qvel[da + j];
      for (int t = 0; t < 3; t++) cv[t] += c6[t] * q;
      for (int t = 0; t < 6; t++) ca[t] += cdot[j - 3][t] * q;
    }
  }
  // ---- cacc, cfrc_body (lane = body)
  float f[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (l >= 1 && l < NB) {
    const int b = l;
    ca[3] -= grav[0]; ca[4] -= grav[1]; ca[5] -= grav[2];
    if (l == LINK7) {   // spatial velocity and bias acceleration of the arm's last link, for finger_bias
#pragma unroll
      for (int t = 0; t < 6; t++) { s.scratch[t] = cv[t]; s.scratch[6 + t] = ca[t]; }
    }
    float t0[6], t1[6], g[6];
    mul_inert_vec(t0, s.cinert[b], cv);
    cross_force(t1, cv, t0);
    mul_inert_vec(g, s.cinert[b], ca);
#pragma unroll
    for (int t = 0; t < 6; t++) f[t] = g[t] + t1[t];
    if (b >= NRB) {
#pragma unroll
      for (int t = 0; t < 6; t++) s.cfrc[b][t] = f[t];
    }
  }
  // robot: force on the subtree of every body, then lane = dof (dof l belongs to body l + 1: one row shift)
  tree_suffix(f, l);
  float tot[6];
#pragma unroll
  for (int t = 0; t < 6; t++) tot[t] = dpp_row<0x101>(f[t]);
  MRE_SYNC();
  // qfrc_bias (lane = dof): cdof . sum of cfrc over the subtree of the dof's body
  if (l < NV) {
    const int b = dof_b;
    float c6[6];
    if (b < NRB) {
#pragma unroll
      for (int t = 0; t < 6; t++) c6[t] = s.cdof[l][t];
    } else {
#pragma unroll
      for (int t = 0; t < 6; t++) tot[t] = s.cfrc[b][t];
      prop_cdof(s, b, l - dof_da, c6);
    }
    const bool act = prop_is_active(s, dof_pid);
    s.qfrc_bias[l] = act ? dot6(c6, tot) : 0.f;
  }
}

// ---- mj_rne on the finger subtree in fp64 (lane = finger body)
// The bias forces of the finger dofs are 1e-3 N m sums of terms that are 25 times larger in the c-frame (spatial
// quantities about the robot's centre of mass, half a metre away): evaluated there in float32 they are off by a few
// 1e-9 N m, and 3e-9 N m of noise on links of 1e-5 kg m^2 already costs 6e-5 rad over 1000 steps
// (tests/diagnostics/finger_precision_study.py "e2e-7,1e-3,1,3e-9").  The same recursion is run here in the frame of
// the arm's last link about the pinch site, where the terms are of the size of the result, in fp64, from link 7's
// spatial velocity and bias acceleration (velocity_stage, float32: inputs of the recursion, a relative error there is
// harmless) and gripper_local's fp64 inertias and cdofs; the result is rounded once.  Same operations as mj_rne:
// cvel = cvel_parent + cdof qvel, cdof_dot = cvel_parent x cdof, cacc = cacc_parent + cdof_dot qvel,
// cfrc = I cacc + cvel x* (I cvel), qfrc_bias = cdof . (cfrc summed over the subtree).
MRE_DEV void dcross3(double* r, const double* a, const double* b) {
  const double x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  r[0] = x; r[1] = y; r[2] = z;
}
MRE_DEV void dcross_motion(double* r, const double* vel, const double* v) {
  double a[3], b[3];
  dcross3(r, vel, v);
  dcross3(a, vel, v + 3);
  dcross3(b, vel + 3, v);
  for (int k = 0; k < 3; k++) r[3 + k] = a[k] + b[k];
}
MRE_DEV void dcross_force(double* r, const double* vel, const double* f) {
  double a[3], b[3];
  dcross3(a, vel, f);
  dcross3(b, vel + 3, f + 3);
  for (int k = 0; k < 3; k++) r[k] = a[k] + b[k];
  dcross3(r + 3, vel, f + 3);
}
MRE_DEV void dmul_inert_vec(double* r, const double* i, const double* v) {
  r[0] = i[0] * v[0] + i[3] * v[1] + i[4] * v[2] - i[8] * v[4] + i[7] * v[5];
  r[1] = i[3] * v[0] + i[1] * v[1] + i[5] * v[2] + i[8] * v[3] - i[6] * v[5];
  r[2] = i[4] * v[0] + i[5] * v[1] + i[2] * v[2] - i[7] * v[3] + i[6] * v[4];
  r[3] = i[8] * v[1] - i[7] * v[2] + i[9] * v[3];
  r[4] = i[6] * v[2] - i[8] * v[0] + i[9] * v[4];
  r[5] = i[7] * v[0] - i[6] * v[1] + i[9] * v[5];
}
MRE_PHASE_FN void finger_bias(ModelP M, Sm& s, int l) {
  constexpr int LINK7 = GRIP_BODY0 - 1;
  const bool fin = l >= GRIP_BODY0 && l < NRB;
  const int i = fin ? l - GRIP_BODY0 : 0;
  const int tcp_site = M->opt_rec.tcp_site;
  // link 7's spatial velocity / bias acceleration: c-frame (about the robot's centre of mass, world axes) -> about
  // the pinch site, axes of link 7
  double V7[6], A7[6];
  {
    const float* R = s.xmat[LINK7];
    float r[3];
    v3sub(r, s.site_xpos[tcp_site], s.com_robot);
    const double rd[3] = {(double)r[0], (double)r[1], (double)r[2]};
    for (int h = 0; h < 2; h++) {
      const float* c = &s.scratch[6 * h];
      const double w[3] = {(double)c[0], (double)c[1], (double)c[2]};
      double t[3];
      dcross3(t, w, rd);
      const double lin[3] = {(double)c[3] + t[0], (double)c[4] + t[1], (double)c[5] + t[2]};
      double* o = h == 0 ? V7 : A7;
      for (int k = 0; k < 3; k++) {   // R' x (R row-major: column k of R dotted with x)
        o[k] = (double)R[k] * w[0] + (double)R[3 + k] * w[1] + (double)R[6 + k] * w[2];
        o[3 + k] = (double)R[k] * lin[0] + (double)R[3 + k] * lin[1] + (double)R[6 + k] * lin[2];
      }
    }
  }
  double S[6], I[10];
#pragma unroll
  for (int k = 0; k < 6; k++) S[k] = fin ? s.gS[i][k] : 0.0;
#pragma unroll
  for (int k = 0; k < 10; k++) I[k] = fin ? s.gI[i][k] : 0.0;
  const double qd = fin ? robot_v(s, l - 1) : 0.0;
  // bodies 8, 10, 12, 14 hang off link 7; 9, 11, 13, 15 off the lane below (the tree mre_create checks)
  const bool child = fin && (l & 1) != 0;   // (the body tree mre_create checks)
  double v[6], a0[6], sd[6];
  dcross_motion(sd, V7, S);
#pragma unroll
  for (int k = 0; k < 6; k++) { v[k] = V7[k] + S[k] * qd; a0[k] = A7[k] + sd[k] * qd; }
  double pv[6], pa[6];
#pragma unroll
  for (int k = 0; k < 6; k++) { pv[k] = dpp_shr1_d(v[k]); pa[k] = dpp_shr1_d(a0[k]); }
  if (child) {
    dcross_motion(sd, pv, S);
#pragma unroll
    for (int k = 0; k < 6; k++) { v[k] = pv[k] + S[k] * qd; a0[k] = pa[k] + sd[k] * qd; }
  }
  double f[6], t0[6], t1[6];
  dmul_inert_vec(t0, I, v);
  dcross_force(t1, v, t0);
  dmul_inert_vec(f, I, a0);
#pragma unroll
  for (int k = 0; k < 6; k++) f[k] += t1[k];
  // force on the subtree: a body off link 7 adds its child's (the lane above)
  double up[6];
#pragma unroll
  for (int k = 0; k < 6; k++) up[k] = dpp_shl1_d(f[k]);
  if (fin && !child) {
#pragma unroll
    for (int k = 0; k < 6; k++) f[k] += up[k];
  }
  if (fin) {
    double b = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) b += S[k] * f[k];
    s.qfrc_bias[l - 1] = (float)b;
  }
  MRE_SYNC();
}

// ------------------------- mj_fwdActuation + mj_passive + mj_fwdAcceleration
// arm actuators (lanes 0..6) as `general` actuators on their joint: force -> qfrc_smooth[lane] (read back by
// the same lane in smooth_forces); returns (wave-uniform) the mask of the actuators clamped by forcerange.
// A function of its own so that the model reads stay out of the step loop's register budget.
MRE_PHASE_FN unsigned arm_actuation(ModelP M, Sm& s, int l) {
  bool arm_clamped = false;
  // the actuator on this lane's dof: the tail of the dof's record (one group of loads)
  const auto* R = &M->dof_rec[l < 7 ? l : 0];
  const float gain = R->act_gain, bias0 = R->act_bias0, bias1 = R->act_bias1, bias2 = R->act_bias2;
  const float ctrl_lo = R->act_ctrl_lo, ctrl_hi = R->act_ctrl_hi, force_lo = R->act_force_lo, force_hi = R->act_force_hi;
  const int forcelimited = R->act_forcelimited;
  if (l < 7) {
    float fa = (float)((double)(gain * clampf(s.ctrl[l], ctrl_lo, ctrl_hi) + bias0) +
                       (double)bias1 * robot_q(s, l) + (double)bias2 * robot_v(s, l));
    if (forcelimited) {
      if (fa <= force_lo) { fa = force_lo; arm_clamped = true; }
      if (fa >= force_hi) { fa = force_hi; arm_clamped = true; }
    }
    s.qfrc_smooth[l] = fa;
  }
  return (unsigned)__ballot(arm_clamped) & 0x7Fu;
}

// returns (wave-uniform) the actuators whose force is clamped by forcerange: bit a = arm actuator a, bit
// NU - 1 = the finger actuator (mjd_actuator_vel skips those in the implicit integrator)
// (the force assembly is a phase function of its own: its fp64 terms would otherwise sit in the kernel body's register
//  budget next to the unrolled robot solve -- 16 B/lane of scratch when it was inlined)
MRE_PHASE_FN unsigned smooth_forces_assemble(ModelP M, Sm& s, int l, unsigned arm_mask) {
  // (the tendon length and velocity from the full finger state: the actuator's position gain of 100 N / rad acts on
  //  joints with 5e-3 kg m^2 of armature)
  // the tendon / gripper-actuator block and the lane's dof record: one group of loads
  const auto* O = &M->opt_rec;
  const float ten_coef[2] = {O->ten_coef[0], O->ten_coef[1]};
  const int ten_dof[2] = {O->ten_dof[0], O->ten_dof[1]};
  const float grip_gainprm = O->grip_gainprm, grip_biasprm[3] = {O->grip_biasprm[0], O->grip_biasprm[1], O->grip_biasprm[2]};
  const float grip_forcerange[2] = {O->grip_forcerange[0], O->grip_forcerange[1]};
  const float grip_ctrlrange[2] = {O->grip_ctrlrange[0], O->grip_ctrlrange[1]};
  const auto* DR = &M->dof_rec[l < NV ? l : 0];
  const int dof_b = DR->body, dof_pid = DR->propid;
  const float dof_damping = DR->damping, dof_stiffness = DR->jnt_stiffness, dof_springref = DR->jnt_springref;
  const double ten_len = (double)ten_coef[0] * robot_q(s, ten_dof[0]) + (double)ten_coef[1] * robot_q(s, ten_dof[1]);
  const double ten_vel = (double)ten_coef[0] * robot_v(s, ten_dof[0]) + (double)ten_coef[1] * robot_v(s, ten_dof[1]);
  const float cg = clampf(s.ctrl[NU - 1], grip_ctrlrange[0], grip_ctrlrange[1]);
  float fg = (float)((double)(grip_gainprm * cg + grip_biasprm[0]) + (double)grip_biasprm[1] * ten_len +
                     (double)grip_biasprm[2] * ten_vel);
  bool clamped = false;
  if (fg <= grip_forcerange[0]) { fg = grip_forcerange[0]; clamped = true; }
  if (fg >= grip_forcerange[1]) { fg = grip_forcerange[1]; clamped = true; }
  if (l < NV) {
    const int b = dof_b;
    float f = 0.f;
    if (b < NRB) {
      // passive: spring + damper of the hinge
      // passive (spring + damper of the hinge), actuation and bias summed in fp64 and rounded once: the finger rows
      // are 1e-3 N m results of 1e-1 N m terms
      double fd = -(double)dof_stiffness * (robot_q(s, l) - (double)dof_springref) - (double)dof_damping * robot_v(s, l);
      if (l < 7) fd += (double)s.qfrc_smooth[l];
      if (l == ten_dof[0]) fd += (double)ten_coef[0] * (double)fg;
      if (l == ten_dof[1]) fd += (double)ten_coef[1] * (double)fg;
      f = (float)(fd - (double)s.qfrc_bias[l]);
    }
    const bool act = prop_is_active(s, dof_pid);
    f = act ? (b < NRB ? f : f - s.qfrc_bias[l]) : 0.f;
    s.qfrc_smooth[l] = f;
    s.qacc_smooth[l] = f;
  }
  MRE_SYNC();
  return arm_mask | (clamped ? 1u << (NU - 1) : 0u);
}
MRE_DEV unsigned smooth_forces(ModelP M, Sm& s, int l) {
  const unsigned arm_mask = arm_actuation(M, s, l);
  const unsigned mask = smooth_forces_assemble(M, s, l, arm_mask);
#ifndef MRE_NEWTON
  solve_robot_one(s.qLD, s.qLDinv, s.qacc_smooth, l);
#else
  factor_solve_robot(s.qM, s.qacc_smooth, l);   // same operations in the same order as factor_robot_regs + solve_robot_one: same bits
#endif
  if (l >= NRV && l < NV) {
    const int p = (l - NRV) / 6, k = (l - NRV) % 6;
    const float md = (k < 3) ? s.prop_mass[p] : s.prop_inertia[p][k - 3];
    s.qacc_smooth[l] = s.qacc_smooth[l] / md;
  }
  MRE_SYNC();
  return mask;
}

// ------------------------------------------- mj_implicit (implicitfast) + advance
// part 1: MH and the right-hand side; the kernel body then factors MH (factor_robot_regs, inlined
// there: a kernel has no callee-saved registers to spill) and calls part 2
// Newton builds integrate the solver's ACCELERATION, not its forces: with f = M qacc (the gradient of the converged
// primal problem is zero), (M - h D) x = f reads x = qacc + (M - h D)^-1 (h D qacc), D the diagonal derivative kept in
// MH -- the second term is ~2 % of the first, so a float32 solve of it is good to 1e-8 of qacc, and the robot's
// accelerations enter as the doubles of nw_robot_polish.  (PGS builds keep the force form: their qacc is
// qacc_smooth + M^-1 J' f by construction.)
MRE_PHASE_FN void integrate_setup(ModelP M, Sm& s, int l, unsigned act_clamped) {
  const bool grip_clamped = (act_clamped >> (NU - 1)) & 1u;
  const float h = M->opt_rec.timestep, grip_bias2 = M->opt_rec.grip_biasprm[2];
  // (mj_advance: qacc_warmstart = qacc -- the same array here, see Sm)
  // MH = M - h*dF/dv restricted to M's pattern (diagonal terms only here)
  for (int e = l; e < NMR; e += 64) {
    // the entry's record (MEntryRec): its dofs and the derivative terms of dof i -- the operands, the products are
    // formed here as before
    const auto* R = &M->m_rec[e];
    const int i = R->i, j = R->j, ten = R->ten;
    const float damping = R->damping, act_bias2 = R->act_bias2, ten_coef = R->ten_coef;
    float v = s.qM[e];
    if (i == j) {
      v += h * damping;
      if (i < 7 && ((act_clamped >> i) & 1u) == 0u) v -= h * act_bias2;
      if (!grip_clamped) {
        if (ten >= 0) v -= h * grip_bias2 * ten_coef * ten_coef;   // (dof i is one of the tendon's two)
      }
    }
    mh_store(s)[e] = v;
#ifdef MRE_NEWTON
    if (i == j) s.scratch[i] = (s.qM[e] - v) * s.qacc[i];   // h D_ii qacc_i
#endif
  }
#ifndef MRE_NEWTON
  if (l < NRV) s.scratch[l] = s.qfrc_smooth[l] + s.qfrc_con[l];
#endif
  MRE_SYNC();
}

// Stores of the words that travel with an env from one wave to the next inside a queue launch (step_body<QUEUE>,
// queue_push): write-through at agent scope (`sc1`: the bytes leave the XCD's L2 for memory with the store, no L2
// write-back before the env is listed).  One word, and a row of n words (n % 4 == 0, 16-byte aligned, the same row for
// every lane) at 16 bytes per lane from LDS.
MRE_DEV void q_store(float* p, float v) {
  __hip_atomic_store(reinterpret_cast<int*>(p), __float_as_int(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
MRE_DEV void q_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <bool WT>
MRE_DEV void travel_store(float* p, float v) {
  if (WT) q_store(p, v); else *p = v;
}
typedef unsigned q_u32x4 __attribute__((ext_vector_type(4)));
// (zero_last: the row's last word is stored as zero -- the warm start's padding)
MRE_DEV void q_store_row(float* row, const float* src, int n, int l, bool zero_last = false) {
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(row, 0, n * 4, 0x00020000);
  if (4 * l < n) {
    q_u32x4 v;
    v.x = __float_as_uint(src[4 * l]); v.y = __float_as_uint(src[4 * l + 1]); v.z = __float_as_uint(src[4 * l + 2]);
    v.w = zero_last && 4 * l + 4 == n ? 0u : __float_as_uint(src[4 * l + 3]);
    __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, 16 * l, 0, 16 /* sc1 */);
  }
}

// part 2 (after the solve of MH x = f, also run from the kernel body): advance velocities and positions
// clo: the cubes' low-order state words of this env in HBM (row of StepArgs::qfine from QFINE_CUBE_Q on) or null.
// With them a cube's pose and velocity advance in fp64 on the double-float pair, like the robot's joints: a float32
// position is off by up to 3e-8 m after every step, a random walk that the envs whose reference trajectory amplifies a
// difference a hundredfold (cubes knocked flying by the arm) take past the 1e-4 bar -- the fp64 oracle with ONLY the
// cubes' state rounded to float32 leaves it in exactly the two cube exits of the 256-env sample, and with the cubes'
// state in double it does not (profiles/NOTES.md, round 4).
// WT (queue launches): the cubes' low words are stored write-through at agent scope -- they travel with the env to the
// wave that steps its next tick (queue_push: the list of travelling words).  Same arithmetic either way.
template <bool WT>
MRE_PHASE_FN void integrate(ModelP M, Sm& s, int l, unsigned flags, bool polished, float* clo) {
  // the time step, the lane's dof record (first part: lane = dof) and body record (second part: lane = body)
  const float h = M->opt_rec.timestep;
  const auto* DR = &M->dof_rec[l < NV ? l : 0];
  const int dof_b = DR->body, dof_pid = DR->propid;
  const auto* BR = &M->body_rec[l < NB ? l : 0];
  const int body_qa = BR->qposadr, body_da = BR->dofadr, body_pid = BR->propid;
  const bool freeze = (flags & F_FREEZE_ROBOT) != 0;
  // the cubes' low-order words (HBM): the velocity word of a cube dof's lane, the seven pose words of a cube body's
  // lane -- read here, together, instead of one by one between the stores that update them
  float vl_in = 0.f, ql_in[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (clo != nullptr) {
    if (l >= NRV && l < NV) vl_in = clo[(QFINE_CUBE_V - QFINE_CUBE_Q) + (l - NRV)];
    if (l >= NRB && l < NB) {
#pragma unroll
      for (int k = 0; k < 7; k++) ql_in[k] = clo[7 * (l - NRB) + k];
    }
  }
  keep_live(dof_pid); keep_live(body_pid); keep_live(body_qa); keep_live(body_da);
  if (l < NV) {
    const int b = dof_b;
    if (b < NRB) {
      if (!freeze) {   // robot joint: the velocity advances in fp64 (double-float pair, robot_q)
#ifdef MRE_NEWTON
        const double acc = polished ? reinterpret_cast<const double*>(&s.nw_Mv[0])[l] : (double)s.qacc[l];
        const double v = robot_v(s, l) + (double)h * (acc + (double)s.scratch[l]);
#else
        const double v = robot_v(s, l) + (double)h * (double)s.scratch[l];
#endif
        const float hi = (float)v;
        s.qvel[l] = hi; s.qlo[QFINE / 2 + l] = (float)(v - (double)hi);
      }
    } else if (prop_is_active(s, dof_pid)) {
      // free joints carry no damping: MH = M on cube blocks
      if (clo != nullptr) {
        float* const vl = clo + (QFINE_CUBE_V - QFINE_CUBE_Q) + (l - NRV);
        const double v = (double)s.qvel[l] + (double)vl_in + (double)h * (double)s.qacc[l];
        const float hi = (float)v, lo = (float)(v - (double)hi);
        s.qvel[l] = hi; travel_store<WT>(vl, lo);
        s.scratch[l] = lo;   // (scratch[NRV ..]: free here; the body lanes below read the new low words from it)
      } else {
        s.qvel[l] += h * s.qacc[l];
      }
    }
  }
  MRE_SYNC();
  if (l >= 1 && l < NB) {
    const int b = l, qa = body_qa, da = body_da;
    if (b < NRB) {
      if (!freeze) {
        const double q = robot_q(s, qa) + (double)h * robot_v(s, da);
        const float hi = (float)q;
        s.qpos[qa] = hi; s.qlo[qa] = (float)(q - (double)hi);
      }
    } else if (prop_is_active(s, body_pid) && clo != nullptr) {
      // mj_integratePos of a free joint on the double-float state: position, then q <- normalize(q (x) exp(h w / 2))
      float* const ql = clo + 7 * (b - NRB);
      double vv[6];
      for (int k = 0; k < 6; k++) vv[k] = (double)s.qvel[da + k] + (double)s.scratch[da + k];
      for (int k = 0; k < 3; k++) {
        const double x = (double)s.qpos[qa + k] + (double)ql_in[k] + (double)h * vv[k];
        const float hi = (float)x;
        s.qpos[qa + k] = hi; travel_store<WT>(ql + k, (float)(x - (double)hi));
      }
      double q0[4], qn[4];
      for (int k = 0; k < 4; k++) q0[k] = (double)s.qpos[qa + 3 + k] + (double)ql_in[3 + k];
      const double wn2 = vv[3] * vv[3] + vv[4] * vv[4] + vv[5] * vv[5];
      if (wn2 > 1e-60) {
        const double inv = rsq64(wn2), half = 0.5 * (double)h * wn2 * inv;
        double sn, cs;
        sincos_poly_d(half, sn, cs);
        const double ax = vv[3] * inv * sn, ay = vv[4] * inv * sn, az = vv[5] * inv * sn;
        qn[0] = q0[0] * cs - q0[1] * ax - q0[2] * ay - q0[3] * az;
        qn[1] = q0[0] * ax + q0[1] * cs + q0[2] * az - q0[3] * ay;
        qn[2] = q0[0] * ay - q0[1] * az + q0[2] * cs + q0[3] * ax;
        qn[3] = q0[0] * az + q0[1] * ay - q0[2] * ax + q0[3] * cs;
      } else {
        for (int k = 0; k < 4; k++) qn[k] = q0[k];
      }
      const double nn = qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3];
      const double sc = nn > 1e-30 ? rsq64(nn) : 1.0;
      for (int k = 0; k < 4; k++) {
        const double x = qn[k] * sc;
        const float hi = (float)x;
        s.qpos[qa + 3 + k] = hi; travel_store<WT>(ql + 3 + k, (float)(x - (double)hi));
      }
    } else if (prop_is_active(s, body_pid)) {
      for (int k = 0; k < 3; k++) s.qpos[qa + k] += h * s.qvel[da + k];
      float w[3] = {s.qvel[da + 3], s.qvel[da + 4], s.qvel[da + 5]};
      const float ang = v3normalize(w) * h;
      float qr[4], qn[4], q0[4];
      axisangle2q(qr, w, ang);
      for (int k = 0; k < 4; k++) q0[k] = s.qpos[qa + 3 + k];
      qmul(qn, q0, qr);
      qnormalize(qn);
      for (int k = 0; k < 4; k++) s.qpos[qa + 3 + k] = qn[k];
    }
  }
  MRE_SYNC();
}

// =========================================================================
// Diagnostic builds only (-DMRE_PHASE_STAMPS=set): per-phase s_memtime deltas of the launch are
// summed into four buckets and returned through the stats rows (tools/phase_stamps.py).
#ifdef MRE_PHASE_STAMPS
#define MRE_STAMP(k)                                                         \
  do {                                                                       \
    if ((k) < 12 || MRE_PHASE_STAMPS == 3) {                                 \
      const unsigned long long now_ = __builtin_amdgcn_s_memtime();          \
      if ((k) / 4 == MRE_PHASE_STAMPS) stamp_acc[(k) % 4] += now_ - stamp_t; \
      stamp_t = now_;                                                        \
    }                                                                        \
  } while (0)
#else
#define MRE_STAMP(k) do {} while (0)
#endif

// Body of one launch (nsteps physics steps of one env per workgroup); instantiated by the two
// entry points below so that profiler summaries separate control ticks from settling launches.
//
// QUEUE (k_step_queue, StepArgs::q_head): the workgroup is a persistent wave that steps ONE control tick of one env per
// pass of the loop below and takes its (env, tick) from the launch's ready lists; the rows it stores at the end of a pass
// are the rows another wave -- on any CU of any XCD -- loads when it takes the env for its next tick, so the rows are
// published before the env is listed (queue_push: write-through stores -> vmcnt(0) -> atomic list entry in the Newton
// kernels, plain stores -> release fence -> vmcnt(0) -> atomic list entry in the PGS ones) and loaded behind an
// agent-scope acquire after it was taken (queue_take; MI355X_MICROARCH.md, inter-workgroup visibility).  Per tick the
// arithmetic is that of a one-tick launch: results are bit-identical.
MRE_DEV int q_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The ready lists are kept per SHARD (StepArgs::q_shards): wave w belongs to shard w % q_shards, entry i of the launch's
// dispatch order to shard i % q_shards (the order is longest-first, so the shards get equal shares of the work), and an
// env stays in its shard.  One list for all 2048 waves was built first and ran 35x slower than the per-tick launches:
// every wave went for the same head word, a compare-and-swap succeeds for one of the waves that read the same value, and
// the retries of the others are atomics on that one word again.  Within a shard (128 waves, one entry taken every 3 us)
// two takers rarely meet.
//
// Capacity fallback inside the launch.  Shards q_shards .. q_shards + q_lshards - 1 are the LARGE kernel's (env e: shard
// q_shards + e % q_lshards): k_step_queue_large runs next to k_step_queue with a few waves, takes the envs the host
// flagged large (their bucket 0, written by the host) -- and every
// env a compact wave hands over: a tick that overflows the compact capacities is abandoned (rows not stored, the cubes'
// low words put back), the env is listed in the large shard for the SAME tick and stays there for the rest of the launch.
// No re-run, no host in the loop: a launch of 50 ticks would otherwise be repeated whole, alone, on one wave.  Large
// waves wait for work (a hand-over can come at any time) until every env of the launch is through (q_done == N).
#ifdef MRE_LARGE_CAPS
constexpr bool Q_LARGE = true;
#else
constexpr bool Q_LARGE = false;
#endif
MRE_DEV int* q_bucket(const StepArgs& a, int t, int sh) {
  const int S = a.q_shards;
  return a.q_buf + (size_t)t * a.q_stride + (sh < S ? (size_t)sh * a.q_cap : (size_t)S * a.q_cap + (size_t)(sh - S) * a.q_capl);
}

// One look at a shard: the ready env that is furthest behind (lowest tick; first come first served within a tick).
// 1: taken; 0: nothing ready; -1: internal error (q_err set).
MRE_DEV int queue_pop_shard(const StepArgs& a, int l, int sh, int& env, int& tick) {
  const int S = a.q_shards;
  const bool order0 = sh < S;               // a compact shard's bucket 0 is its share of the dispatch order
  const int n0 = (a.N - sh + S - 1) / S;
  int* const head = a.q_head + sh * QUEUE_TICKS_MAX;
  const int* const tail = a.q_tail + sh * QUEUE_TICKS_MAX;
  for (;;) {
    // one lane per bucket, 64 buckets at a time; the loads of all the launch's buckets are issued together
    int h[QUEUE_TICKS_MAX / 64], tl[QUEUE_TICKS_MAX / 64];
#pragma unroll
    for (int c = 0; c < QUEUE_TICKS_MAX / 64; c++) {
      const int b = c * 64 + l;
      h[c] = 0; tl[c] = 0;
      if (b < a.q_nticks) { h[c] = q_load(head + b); tl[c] = (b == 0 && order0) ? n0 : q_load(tail + b); }
    }
    int t = -1, ht = 0;
#pragma unroll
    for (int c = 0; c < QUEUE_TICKS_MAX / 64; c++) {
      if (t < 0 && c * 64 < a.q_nticks) {
        const unsigned long long ready = __ballot(h[c] < tl[c]);
        if (ready != 0ull) {
          const int k = __ffsll((long long)ready) - 1;
          t = c * 64 + k;
          ht = __builtin_amdgcn_readlane(h[c], k);
        }
      }
    }
    if (t < 0) return 0;
    int got = -1;
    if (l == 0) {
      if (t == 0 && order0) {
        // all of bucket 0 is there from the start: a ticket past its end is harmless (the launch's first pass is
        // every wave of the shard here at once)
        const int i = __hip_atomic_fetch_add(head, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (i < n0) got = a.env_order != nullptr ? a.env_order[sh + S * i] : sh + S * i;
      } else {
        int expect = ht;
        if (__hip_atomic_compare_exchange_strong(head + t, &expect, ht + 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT)) {
          // (the entry was counted in q_tail before it was written: the wave that lists it is two instructions away)
          const int* slot = q_bucket(a, t, sh) + ht;
          int v = q_load(slot);
          for (unsigned spin = 0; v == 0; ++spin) {
            if (spin > (1u << 20)) { *a.q_err = 1; v = -1; break; }   // cannot happen; never hang the GPU on a bug
            __builtin_amdgcn_s_sleep(4);
            v = q_load(slot);
          }
          got = v < 0 ? -2 : v - 1;
        }
      }
    }
    got = __builtin_amdgcn_readfirstlane(got);
    if (got == -2) return -1;
    if (got < 0) continue;   // another wave took that entry: look again
    env = got; tick = t;
    return 1;
  }
}
// Compact waves: own shard first, then the next shard that has something ready (a wave without work helps elsewhere
// before it leaves); false when no shard has.  A compact wave that finds nothing leaves: every env that is not listed is
// held by a wave that will list it and then look here itself, so work never waits for a wave that has left, and no
// compact wave ever waits for work.  Large waves: the large shard only, and they wait -- see above.
// (wait = false, the early take of step_body: one look at every shard, large waves included)
MRE_DEV bool queue_pop(const StepArgs& a, int l, int home, int& env, int& tick, int& shard, bool wait = true) {
  const int S = a.q_shards;
  if (Q_LARGE) {
    // the large kernel's own shards (q_lshards of them, numbered from S; an env handed over goes to S + env % q_lshards):
    // own shard first, then the others -- a closing grasp phase puts hundreds of waves here, and one list for all of them
    // is the compare-and-swap storm the compact side had
    const int SL = a.q_lshards;
    for (unsigned idle = 0;; ++idle) {
      int r = 0;
      for (int k = 0; k < SL && r == 0; ++k) {
        const int sh = S + (home + k < SL ? home + k : home + k - SL);
        r = queue_pop_shard(a, l, sh, env, tick);
        if (r != 0) shard = sh;
      }
      if (r != 0) return r > 0;
      // Waiting is a matter of speed only: the host enqueues a second launch of this kernel BEHIND the compact one
      // (q_wait == 0: it takes what is listed and leaves), so whatever this launch leaves undone is done there.  It
      // leaves when every env is through; when no compact wave has shown up after ~3 ms (the two kernels are not
      // running side by side: a profiler that serialises dispatches, two streams on one hardware queue); after ~2 s.
      if (!wait || a.q_wait == 0 || q_load(a.q_done) >= a.N) return false;
      if (idle > 512u && q_load(a.q_started) == 0) return false;
      if (idle > (1u << 18)) return false;
      __builtin_amdgcn_s_sleep(127);
    }
  }
  for (int k = 0; k < S; ++k) {
    const int sh = home + k < S ? home + k : home + k - S;
    const int r = queue_pop_shard(a, l, sh, env, tick);
    if (r != 0) { shard = sh; return r > 0; }
  }
  return false;
}
// List the env as ready for `tick` in `shard` (its rows are stored).
//
// No release fence: every word that another wave of the launch reads after taking the env is stored WRITE-THROUGH at
// agent scope by the one wave that holds the env (q_store / q_store_row, agent-scope atomics), this wave waits for all
// its stores (vmcnt(0)) and only then lists the env with agent-scope atomics; the taking wave's agent-scope acquire drops
// its compute unit's stale lines (MI355X_MICROARCH.md, inter-workgroup visibility: write-through payload, every storing
// wave drained, atomic flag).  The words that travel, and who stores them:
//   qpos, qvel, qacc_ws, qfine[0 .. QFINE), ctrl          rows, 16 bytes per lane, first thing after the tick's last step
//   qfine[QFINE_CUBE_Q ..): the cubes' low words          integrate<true>, every step; put back from cube_lo_keep when the
//                                                         tick is abandoned
//   converged                                             one byte, lane 0 (controller launches)
//   q_acc[env][0 .. 4)                                    lane 0: high-water marks, duration, `moved`
//   nstep, status                                         agent-scope atomic add / or
// A plain store to any of them under QUEUE would be a bug: it may still sit in this XCD's L2 when the env is taken on
// another.  What only the host reads, after the launch, is stored plainly only where ONE wave stores it in a launch:
// launch_info and sites by the env's last tick.  A trace row (diagnostic) is stored write-through: the rows of an
// abandoned tick are written a second time by the large kernel's wave.  Stats by the last tick only (stored every tick, the
// host read an earlier tick's words for envs that had changed XCDs: a dirty line left in one XCD's L2 is written back
// whenever, possibly after the last tick's store from another; profiles/NOTES.md, round 19).
//
// Q_WRITE_THROUGH says which instantiations publish this way: the Newton ones.  The PGS queue kernels sit at 256 VGPRs
// with scratch, and the 16-byte row stores added scratch to the large one (profiles/NOTES.md, round 19): they keep plain
// stores where they were and the agent-scope release fence here.  Both kernels of a launch are of one solver, so a launch
// never mixes the two forms.
#ifdef MRE_NEWTON
constexpr bool Q_WRITE_THROUGH = true;
#else
constexpr bool Q_WRITE_THROUGH = false;
#endif
MRE_DEV void queue_push(const StepArgs& a, int l, int env, int tick, int shard) {
  if (!Q_WRITE_THROUGH) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  // every store of this wave has left for memory (after the fence: the compiler may drop the fence's own wait)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (l == 0) {
    const int i = __hip_atomic_fetch_add(a.q_tail + shard * QUEUE_TICKS_MAX + tick, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(q_bucket(a, tick, shard) + i, env + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// An item as a queue wave takes it: the (env, tick) and the env's rows in registers, one word per lane and array.  The
// take needs nothing from the item the wave is working on, and that item's stores need nothing from the take -- so a wave
// takes its NEXT item while the current one finishes (step_body: after the solver of the tick's last step), and the
// atomics, the acquire and the first-touch loads of the rows run under the integrator and the epilogue instead of in
// front of an idle SIMD slot.  The rows go to LDS at the start of the next pass (the current item still uses Sm).
struct QueueItem {
  bool have = false;
  int env = 0, tick = 0, shard = 0, nprops = 0;
  float qpos = 0.f, qvel = 0.f, qacc = 0.f, qfine = 0.f, ctrl = 0.f, prop_size = 0.f;
};
// Which kernels take early: the Newton instantiations (profiles/r19a_kernel_resource_usage.txt: no scratch beyond the
// parent's 8 bytes, two waves per SIMD).  The PGS queue kernels sit at 256 VGPRs with scratch already and keep the
// serial take.
#ifdef MRE_NEWTON
constexpr bool Q_EARLY_TAKE = true;
#else
constexpr bool Q_EARLY_TAKE = false;
#endif
MRE_DEV void queue_take(const StepArgs& a, int l, int home, bool wait, QueueItem& it) {
  it.have = queue_pop(a, l, home, it.env, it.tick, it.shard, wait);
  if (!it.have) return;
  if (it.tick > 0 || Q_LARGE) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const size_t e = (size_t)it.env;
  it.qpos = l < NQP ? a.qpos[e * NQP + l] : 0.f;
  it.qvel = l < NVP ? a.qvel[e * NVP + l] : 0.f;
  it.qacc = l < NVP ? a.qacc_ws[e * NVP + l] : 0.f;
  it.qfine = l < QFINE && a.qfine != nullptr ? a.qfine[e * QFINE_ROW + l] : 0.f;
  it.ctrl = l < NU ? a.ctrl[e * NU + l] : 0.f;
  it.prop_size = l < NPROP * 3 ? a.prop_size[e * NPROP * 3 + l] : 0.f;
  it.nprops = a.nprops[e];
}

template <bool QUEUE>
MRE_DEV void step_body(const StepArgs& a, Sm& s) {
  OscSm& osc = s.osc;
  const int l = threadIdx.x;
  int env = 0, qtick = 0, qshard = 0;
  if (!QUEUE) {
    if ((int)blockIdx.x >= a.N) return;
    env = a.env_order != nullptr ? a.env_order[blockIdx.x] : (int)blockIdx.x;
  }
  if (QUEUE && !Q_LARGE && l == 0) __hip_atomic_fetch_add(a.q_started, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (QUEUE && Q_LARGE && a.q_wait != 0) {
    // The waiting large launch is enqueued BEFORE the launch's lists are reset, so that its workgroups are placed before
    // the compact kernel's fill the compute units' LDS (a large workgroup placed late starts when a compact wave
    // leaves: at the end).  It touches nothing until the reset is through: the host's stream then writes the launch's
    // number to q_gen.  (Bounded like every wait here: what this launch does not do, the one behind the compact kernel does.)
    for (unsigned idle = 0; q_load(a.q_gen) != a.q_gen_expect; ++idle) {
      if (idle > 1024u) return;
      __builtin_amdgcn_s_sleep(127);
    }
  }
  const int qhome = QUEUE ? (int)(blockIdx.x % (unsigned)(Q_LARGE ? a.q_lshards : a.q_shards)) : 0;
  QueueItem next;   // QUEUE: the item of the pass to come (taken early, or here)
 for (;;) {
  if (QUEUE) {
    // Nothing taken early -- the first pass, nothing was ready then, or a kernel that takes serially: the look of a wave
    // that has listed its own env ("a wave that finds nothing ready leaves"; large waves wait as they always did).  The
    // env this wave has just listed is in the lists by now, so it is found here if no other wave took it.
    if (!next.have) queue_take(a, l, qhome, true, next);
    if (!next.have) return;
    env = next.env; qtick = next.tick; qshard = next.shard;
    next.have = false;
  }
  const int step_lo = QUEUE ? qtick * a.control_steps : 0, step_hi = QUEUE ? step_lo + a.control_steps : a.nsteps;
  if (QUEUE && !Q_LARGE && qtick == 0 && a.large != nullptr && a.large[env] != 0) continue;   // (in the large shard's list)
  if (!QUEUE || (!Q_LARGE && qtick == 0)) {
  // (QUEUE: an env that is left out here still counts as through)
#define MRE_PASS_SKIP { if (QUEUE) { if (l == 0) __hip_atomic_fetch_add(a.q_done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); continue; } return; }
  // the launch is split between the compact and the large kernel by the env's flag (capacity fallback)
  if (!QUEUE && a.large != nullptr && (a.large[env] != 0) != (a.want_large != 0)) return;
  if (a.env_mask != nullptr && a.env_mask[env] == 0) {
    // "not part of this launch" for the host's read of the launch info
    if (a.launch_info != nullptr && l < 4) a.launch_info[(size_t)env * 4 + l] = -1;
    MRE_PASS_SKIP;
  }
  if (a.pending != nullptr && a.pending[env] != 0) {
    // overflowed the compact kernel in an earlier launch whose info the host has not read yet: wait for the re-run
    if (a.launch_info != nullptr && l < 4) a.launch_info[(size_t)env * 4 + l] = l == 0 ? -2 : -1;
    MRE_PASS_SKIP;
  }
#undef MRE_PASS_SKIP
  }
  ModelP M = (ModelP)a.M;

  // ---- load state (one coalesced row per array); with a save area, the rows as they were before this launch are
  // copied aside on the way (the host puts an env that overflows the compact capacities back to them and re-runs it)
  // (QUEUE: nothing is re-run, so no save area; the rows were loaded into registers when the item was taken: queue_take)
  const bool save = !QUEUE && a.sv_qpos != nullptr && step_lo == 0;
  if (l < NQP) {
    const float v = QUEUE ? next.qpos : a.qpos[(size_t)env * NQP + l];
    s.qpos[l] = v;
    if (save) a.sv_qpos[(size_t)env * NQP + l] = v;
  }
  if (l < NVP) {
    const float v = QUEUE ? next.qvel : a.qvel[(size_t)env * NVP + l], w = QUEUE ? next.qacc : a.qacc_ws[(size_t)env * NVP + l];
    s.qvel[l] = v;
    s.qacc[l] = w;      // warm start (see Sm)
    s.qfrc_con[l] = 0.f;
    if (save) { a.sv_qvel[(size_t)env * NVP + l] = v; a.sv_qacc_ws[(size_t)env * NVP + l] = w; }
  }
  if (l < QFINE) {
    const float v = QUEUE ? next.qfine : a.qfine != nullptr ? a.qfine[(size_t)env * QFINE_ROW + l] : 0.f;
    s.qlo[l] = v;
    if (save && a.qfine != nullptr) a.sv_qfine[(size_t)env * QFINE_ROW + l] = v;
  }
  if (save && a.qfine != nullptr && l < QFINE_ROW - QFINE)   // the cubes' words stay in HBM; the restore point takes a copy
    a.sv_qfine[(size_t)env * QFINE_ROW + QFINE + l] = a.qfine[(size_t)env * QFINE_ROW + QFINE + l];
  // (QUEUE, compact: the same words as they are before this tick, should the tick be abandoned -- hand-over below)
  float cube_lo_keep = 0.f;
  if (QUEUE && !Q_LARGE && a.qfine != nullptr && l < QFINE_ROW - QFINE) cube_lo_keep = a.qfine[(size_t)env * QFINE_ROW + QFINE + l];
  if (l < NU) {
    const float v = QUEUE ? next.ctrl : a.ctrl[(size_t)env * NU + l];
    s.ctrl[l] = v;
    if (save) a.sv_ctrl[(size_t)env * NU + l] = v;
  }
  if (save && l == 0) {
    if (a.nstep != nullptr) a.sv_nstep[env] = a.nstep[env];
    a.sv_status[env] = a.status[env];
    a.sv_converged[env] = a.converged != nullptr ? a.converged[env] : (uint8_t)0;
  }
  if (l == 0) { s.nprops = QUEUE ? next.nprops : a.nprops[env]; s.overflow = 0; s.ncon = 0; s.nefc = 0; s.solver_iters = 0; }
#ifdef MRE_NEWTON
  if (l < 24) s.zrow[l] = 0.f;
#endif
  if (l < NPROP * 3) {
    const float sz = QUEUE ? next.prop_size : a.prop_size[(size_t)env * NPROP * 3 + l];
    s.prop_size[l / 3][l % 3] = sz;
  }
  MRE_SYNC();
  if (l < NPROP) {
    const float m = M->body_mass[NRB + l];
    const float* z = s.prop_size[l];
    s.prop_mass[l] = m;
    s.prop_inertia[l][0] = m / 3.f * (z[1] * z[1] + z[2] * z[2]);
    s.prop_inertia[l][1] = m / 3.f * (z[0] * z[0] + z[2] * z[2]);
    s.prop_inertia[l][2] = m / 3.f * (z[0] * z[0] + z[1] * z[1]);
  }
  MRE_SYNC();

#if defined(MRE_PHASE_STAMPS) && MRE_PHASE_STAMPS >= 4
  if (l < 4) dbg_acc[l] = 0ull;
#endif
#ifdef MRE_PHASE_STAMPS
  unsigned long long stamp_acc[4] = {0, 0, 0, 0};
  unsigned long long stamp_t = __builtin_amdgcn_s_memtime();
#endif
  // (QUEUE: the flag travels with the env from tick to tick through a.converged, as it does from launch to launch)
  bool arm_converged = ((a.flags & F_CONV_CONTINUE) != 0 || (QUEUE && qtick > 0)) && a.converged != nullptr && a.converged[env] != 0;
  float grip_cmd = 0.f;
  const OscConfig* oscp = a.osc + (size_t)env * a.osc_stride;  // per-env gains when tuning a population
  int hw_ncon = 0, hw_nefc = 0, hw_nrrow = 0, hw_npp = 0;  // high-water marks of this launch
  // the env's own duration in this launch is the cost key of the heavy-first dispatch of the next one
  const unsigned long long launch_t0 = __builtin_amdgcn_s_memtime();
  if (a.mode == CTRL_OSC) {
    if (l < 16) s.osc_tgt[l] = a.osc_target[(size_t)env * 16 + l];
    // MinMax.compute_control_output: max_val 255 (closed) / min_val 0 (open), min_max.yaml:3-4
    grip_cmd = a.grip_closed[env] ? M->act_ctrlrange[NU - 1][1] : M->act_ctrlrange[NU - 1][0];
    MRE_SYNC();
  }
  int steps_done = 0;
  bool settled = false;
  for (int step = step_lo; step < step_hi; ++step) {
    // ------------------------------------------------ S1: position stage
    MRE_STAMP(7);
    position_stage(M, s, l);
    MRE_STAMP(12);
    MRE_STAMP(13);
    gripper_local(M, s, l);
    if ((a.flags & F_NO_CONSTRAINTS) == 0) connect_rows_local(M, s, l);
    MRE_STAMP(14);
    crb_mass_matrix(M, s, l);
    MRE_SYNC();
#ifndef MRE_NEWTON
    factor_robot_regs(s.qM, s.qLD, s.qLDinv);
#endif
    // (Newton builds: the only user of M's factor is qacc_smooth = M^-1 qfrc_smooth -- PGS also solves M^-1 J' with it
    //  -- so the factor is formed where that one solve runs and never leaves the registers: smooth_forces)
    MRE_STAMP(15);
    MRE_STAMP(0);
    // ------------------------------------------------ S1b: velocity stage (before collision:
    // its temporaries share LDS region R2 with the contact geometry)

    velocity_stage(M, s, l);
    MRE_SYNC();
    finger_bias(M, s, l);
    MRE_STAMP(1);
    // ------------------------------------------------ S1c: collision + constraint assembly
    const bool constrained = (a.flags & F_NO_CONSTRAINTS) == 0;
    if (constrained) {

      collide(M, s, l, false, (a.flags & F_CLIP_ALWAYS) != 0);
      MRE_STAMP(2);
      assemble_constraints(M, s, l);
#ifdef MRE_NEWTON
      nw_build_lists(s, l, a.flags);
#else
      solve_robot_rows(s, l);
      assemble_blocks(M, s, l);
#endif
      MRE_STAMP(3);
      hw_ncon = max(hw_ncon, s.ncon); hw_nefc = max(hw_nefc, s.nefc);
      hw_nrrow = max(hw_nrrow, s.nrrow); hw_npp = max(hw_npp, s.npp);
    }

    // ------------------------------------------------ control at tick boundary
    if (a.mode == CTRL_SEQ && (step % a.control_steps) == 0) {
      const int tick = step / a.control_steps;
      if (l < NU) s.ctrl[l] = a.ctrl_seq[((size_t)tick * a.seq_stride + env) * NU + l];
      MRE_SYNC();
    }
    if (a.mode == CTRL_OSC && (step % a.control_steps) == 0) {
      // RobotArm.run_controller tick (robot_arm.py:69-88): is_converged() of the previous
      // tick is evaluated on the same (step1-fresh) state the next torque is computed from
      if (step > 0 && osc_converged(M, s, oscp, s.osc_tgt)) arm_converged = true;
      osc_compute(M, s, osc, oscp, s.osc_tgt, l);
      if (l == 0) s.ctrl[NU - 1] = grip_cmd;
      MRE_SYNC();
    }
    // ------------------------------------------------ S2
    MRE_STAMP(4);
    const unsigned clamped = smooth_forces(M, s, l);
    MRE_STAMP(5);
    bool polished = false;
    if (constrained) {
#if defined(MRE_NEWTON) && defined(MRE_PHASE_STAMPS)
      newton_solve(M, s, l, stamp_acc, stamp_t);
      polished = nw_robot_polish(M, s, l);
#elif defined(MRE_NEWTON)
      newton_solve(M, s, l);
      polished = nw_robot_polish(M, s, l);
#else
      if (M->opt_rec.cone == 0) solve_constraints_pyramidal(M, s, l);
      else solve_constraints(M, s, l);
#endif
      MRE_STAMP(6);
    } else {
      if (l < NVP) { s.qacc[l] = s.qacc_smooth[l]; s.qfrc_con[l] = 0.f; }
      MRE_SYNC();
    }

    // QUEUE: the next item, while this one finishes (QueueItem).  One look, never a wait; nothing ready: the wave looks
    // again after it has listed this env, at the top of the loop.
    if (QUEUE && Q_EARLY_TAKE && step + 1 == step_hi) queue_take(a, l, qhome, false, next);
    // (QUEUE: the cubes' low words were stored write-through by the last step's integrator, which drops them from this
    //  XCD's L2 -- one load per lane brings their lines back while the set-up below runs, for the integrator's reads)
    float cube_lo_warm = 0.f;
    if (QUEUE && Q_WRITE_THROUGH && a.qfine != nullptr && l < QFINE_ROW - QFINE) cube_lo_warm = a.qfine[(size_t)env * QFINE_ROW + QFINE + l];
    integrate_setup(M, s, l, clamped);
    factor_solve_robot(mh_store(s), s.scratch, l);
    if (QUEUE && Q_WRITE_THROUGH) keep_live(cube_lo_warm);
    integrate<QUEUE && Q_WRITE_THROUGH>(M, s, l, a.flags, polished, a.qfine != nullptr ? a.qfine + (size_t)env * QFINE_ROW + QFINE_CUBE_Q : nullptr);
    steps_done = step + 1 - step_lo;
    if ((a.flags & F_SETTLE_EXIT) != 0) {
      // PropPlacer's settle test on this env's own cubes (prop_initializer.py:247-258)
      float mv = 0.f, ma = 0.f;
      if (l >= NRV && l < NRV + 6 * s.nprops) { mv = fabsf(s.qvel[l]); ma = fabsf(s.qacc[l]); }
      mv = wave_max(mv); ma = wave_max(ma);
      settled = mv < 1e-3f && ma < 1e-2f && step + 1 > a.min_settle_steps;
    }
    if (a.trace != nullptr && env < a.trace_nenv && (a.trace_base + step) < a.trace_max) {
      // column 43 of the row carries the step's constraint census (an integer < 2^24, exact
      // in fp32): active contacts + 64 * (bit b - 1 set: the joint of robot body b is at a limit)
      if (l < TRACE_QVEL) {
        float v = l < NQ ? s.qpos[l] : 0.f;
        if (l == NQ && constrained) {
          int mask = 0;
          for (int k = 0; k < s.nl; k++) mask |= 1 << ((s.lim_info[k] & 0xFF) - 1);
          v = (float)(s.ncon + 64 * mask);
        }
        if (l == NQ + 1 && constrained) {
          // which pairs the active contacts belong to (22 bits: sum of squared pair keys; a contact that opens
          // while another one closes leaves the count above unchanged)
          unsigned h = 0u;
          for (int c = 0; c < s.ncon; c++) {
            const int pr = s.con_pair[c];
            const unsigned key = (unsigned)(M->pair_g1[pr] * 32 + M->pair_g2[pr] + 1);
            h = (h + key * key) & 0x3FFFFFu;
          }
          v = (float)h;
        }
        if (l == NQ + 2 && constrained && M->opt_rec.cone != 0) {
          // what the step's solve left behind, per row (22-bit hash; the oracle: mro_state_hash): a limit row pushing or
          // not, a contact open / sticking / sliding (|f_t| on the cone's boundary).  A solution that sits on one of
          // those boundaries within rounding is as legitimate a fork of two arithmetics as a contact that closes a
          // step apart: the parity tests count a difference here as a census switch too (elliptic cones).
          unsigned h = 0u;
          const int ns = 7 + s.nl;
          for (int i = 7; i < ns; i++) h += (s.frc[i] > 0.f ? 1u : 2u) * (unsigned)((i + 1) * (i + 1));
          for (int c = 0; c < s.ncon; c++) {
            const int i = ns + 3 * c;
#ifdef MRE_NEWTON
            const float mu = s.con_fric[c];
#else
            const float mu = s.blkrec[8 + c][15];
#endif
            const float fn = s.frc[i], ft2 = s.frc[i + 1] * s.frc[i + 1] + s.frc[i + 2] * s.frc[i + 2], lim = mu * fn;
            const unsigned z = fn <= 0.f ? 1u : (ft2 >= lim * lim * (1.f - 1e-4f) ? 3u : 2u);
            h += z * (unsigned)((c + 3) * (c + 3));
          }
          v = (float)(h & 0x3FFFFFu);
        }
        // (QUEUE, write-through: an abandoned tick's rows are written again by the large kernel's wave -- this wave's
        //  stores must have left for memory before the env is listed there, like the words that travel: queue_push)
        travel_store<QUEUE && Q_WRITE_THROUGH>(&a.trace[((size_t)(a.trace_base + step) * a.trace_nenv + env) * TRACE_W + l], v);
      }
      // columns TRACE_QVEL .. TRACE_QVEL + 38: qvel after the step (north_star compares qpos AND qvel; the float32 words)
      if (l < NVP)
        travel_store<QUEUE && Q_WRITE_THROUGH>(&a.trace[((size_t)(a.trace_base + step) * a.trace_nenv + env) * TRACE_W + TRACE_QVEL + l],
                                               l < NV ? s.qvel[l] : 0.f);
    }
    if (settled) break;
  }
  MRE_STAMP(7);
  if (a.settle_steps != nullptr && l == 0) a.settle_steps[env] = settled ? steps_done : -steps_done;
  // QUEUE, compact kernel: a tick that overflowed is abandoned and the env handed over to the large shard (queue_pop)
  const bool hand_over = QUEUE && !Q_LARGE && s.overflow != 0;
  if (QUEUE && Q_WRITE_THROUGH) {
    // ---- store state, first: the rows travel with the env (queue_push), write-through; they drain while the rest of the
    // epilogue runs, and the env is listed after this wave's vmcnt(0).  (Nothing below changes a row: the final
    // kinematics reads them.)
    if (hand_over) {
      if (a.qfine != nullptr && l < QFINE_ROW - QFINE) q_store(a.qfine + (size_t)env * QFINE_ROW + QFINE + l, cube_lo_keep);
    } else {
      q_store_row(a.qpos + (size_t)env * NQP, s.qpos, NQP, l);
      q_store_row(a.qvel + (size_t)env * NVP, s.qvel, NVP, l);
      q_store_row(a.qacc_ws + (size_t)env * NVP, s.qacc, NVP, l, true);
      if (a.qfine != nullptr) q_store_row(a.qfine + (size_t)env * QFINE_ROW, s.qlo, QFINE, l);
      q_store_row(a.ctrl + (size_t)env * NU, s.ctrl, NU, l);
    }
  }
  if (a.nstep != nullptr && l == 0 && !hand_over) {   // physics.data.time advances by steps_done * timestep
    // (QUEUE: words one wave after another updates are updated where every XCD sees them)
    if (QUEUE) __hip_atomic_fetch_add(a.nstep + env, steps_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else a.nstep[env] += steps_done;
  }
  if (a.nsteps == 0 && (a.flags & F_OSC_EVAL) != 0 && a.mode == CTRL_OSC) {
    // OSC.compute_control_output() on the current state (models/robot_arm.py:71): the position and
    // velocity stages the trailing mj_step1 would have left behind, then the torque law
    position_stage(M, s, l);
    gripper_local(M, s, l);
    crb_mass_matrix(M, s, l);
    MRE_SYNC();
    velocity_stage(M, s, l);
    MRE_SYNC();
    osc_compute(M, s, osc, oscp, s.osc_tgt, l);
    if (l == 0) s.ctrl[NU - 1] = grip_cmd;
    MRE_SYNC();
  }
  if (a.nsteps == 0 && (a.flags & F_DETECT) != 0 && a.contacts != nullptr) {
    // physics.forward() + physics.data.contact: kinematics, then every detected contact
    position_stage(M, s, l);
    collide(M, s, l, (a.flags & F_DETECT_ACTIVE) == 0, (a.flags & F_CLIP_ALWAYS) != 0);
    float* o = a.contacts + (size_t)env * (1 + 3 * CONTACT_EXPORT);
    const int n = s.ncon < CONTACT_EXPORT ? s.ncon : CONTACT_EXPORT;
    if (l == 0) o[0] = s.overflow ? -(float)s.ncon : (float)s.ncon;   // negative: the list is cut
    if (l < n) {
      const int pr = s.con_pair[l];
      o[1 + 3 * l] = (float)M->pair_g1[pr]; o[2 + 3 * l] = (float)M->pair_g2[pr]; o[3 + 3 * l] = s.con_dist[l];
      if (a.contacts_full != nullptr) {   // the rest of the mjContact record (mre_get_contacts_full)
        float* f = a.contacts_full + ((size_t)env * CONTACT_EXPORT + l) * 12;
        for (int k = 0; k < 3; k++) f[k] = s.con_pos[l][k];
        for (int k = 0; k < 9; k++) f[3 + k] = s.con_frame[l][k];
      }
    }
    MRE_SYNC();
    if (l == 0) s.overflow = 0;   // a cut detection list is reported in the count, not as a status bit
  }
  // ---- final kinematics: for the controller's convergence test and for the site / geom exports (a stepping
  // launch of mre_step / mre_rollout asks for neither: mre_get_sites refreshes the frames itself)
  // (QUEUE: what a launch does at its end is done after the env's last tick of the launch)
  const bool q_last = !QUEUE || (qtick + 1 == a.q_nticks && !hand_over);
  if (q_last && (a.mode == CTRL_OSC || a.sites != nullptr || a.geoms != nullptr)) kinematics_only(M, s, l);
  if (a.mode == CTRL_OSC && a.nsteps > 0 && !hand_over) {
    if (q_last && osc_converged(M, s, oscp, s.osc_tgt)) arm_converged = true;
    if (l == 0) {
      if (a.converged != nullptr) {
        // (QUEUE: travels with the env -- queue_push)
        if (QUEUE && Q_WRITE_THROUGH) __hip_atomic_store(a.converged + env, (uint8_t)(arm_converged ? 1 : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else a.converged[env] = arm_converged ? 1 : 0;
      }
      if (q_last && !arm_converged && a.status != nullptr && (a.flags & F_CONV_OPEN) == 0) {
        if (QUEUE) __hip_atomic_fetch_or(a.status + env, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else a.status[env] |= 1u;
      }
    }
  }
  if (a.geoms != nullptr && l < NG) {
    float p[3], R[9], size[3], rb;
    geom_pose(M, s, l, p, R, size, &rb);
    float* o = a.geoms + ((size_t)env * NG + l) * 16;
    const int pid = M->geom_propid[l];
    const bool active = pid < 0 || pid < s.nprops;
    for (int k = 0; k < 3; k++) o[k] = p[k];
    for (int k = 0; k < 9; k++) o[3 + k] = R[k];
    for (int k = 0; k < 3; k++) o[12 + k] = size[k];
    o[15] = active ? (float)M->geom_type[l] : -1.f;  // -1: cube slot not in use
  }
  if (a.sites != nullptr && q_last) {
    float* o = a.sites + (size_t)env * 16;
    if (l < 3) o[l] = s.site_xpos[M->opt_rec.tcp_site][l];
    if (l >= 3 && l < 6) o[l] = s.site_xpos[M->opt_rec.eef_site][l - 3];
    if (l == 6) {
      float q[4];
      mat2q(q, s.site_xmat[0]);
      o[6] = q[0]; o[7] = q[1]; o[8] = q[2]; o[9] = q[3];
    }
  }
  // ---- store state (QUEUE, write-through: done above)
  if (QUEUE && Q_WRITE_THROUGH) {
  } else if (hand_over) {
    if (a.qfine != nullptr && l < QFINE_ROW - QFINE) a.qfine[(size_t)env * QFINE_ROW + QFINE + l] = cube_lo_keep;
  } else {
    if (l < NQP) a.qpos[(size_t)env * NQP + l] = s.qpos[l];
    if (l < NVP) {
      a.qvel[(size_t)env * NVP + l] = s.qvel[l];
      a.qacc_ws[(size_t)env * NVP + l] = l < NV ? s.qacc[l] : 0.f;
    }
    if (l < QFINE && a.qfine != nullptr) a.qfine[(size_t)env * QFINE_ROW + l] = s.qlo[l];
    if (l < NU) a.ctrl[(size_t)env * NU + l] = s.ctrl[l];
  }
  // QUEUE: the env goes on to its next tick unless this was the launch's last one
  const bool q_more = QUEUE && !hand_over && qtick + 1 < a.q_nticks;
  if (l == 0 && a.launch_info != nullptr) {
    int* li = a.launch_info + (size_t)env * 4;
    unsigned long long dt = (__builtin_amdgcn_s_memtime() - launch_t0) >> 10;
    int moved = 0;   // QUEUE: the env was handed over to the large kernel in this launch
    if (QUEUE) {
      // high-water marks and the summed duration travel with the env (q_acc); the host reads the duration as that of
      // one tick (the mean), in the same unit as a one-tick launch reports it
      int* qa = a.q_acc + (size_t)env * 4;
      if (qtick > 0 || Q_LARGE) {
        hw_ncon = max(hw_ncon, q_load(qa + 0) & 0xFFFF); hw_nefc = max(hw_nefc, q_load(qa + 1));
        hw_nrrow = max(hw_nrrow, q_load(qa + 2) & 0xFFFF); hw_npp = max(hw_npp, q_load(qa + 2) >> 16);
        dt += (unsigned long long)q_load(qa + 3);
        moved = q_load(qa + 0) >> 16;
      }
      if (hand_over) moved = 1;
      if ((q_more || hand_over) && Q_WRITE_THROUGH) {
        q_store(qa + 0, hw_ncon | (moved << 16)); q_store(qa + 1, hw_nefc); q_store(qa + 2, hw_nrrow | (hw_npp << 16)); q_store(qa + 3, (int)dt);
      } else if (q_more || hand_over) {
        qa[0] = hw_ncon | (moved << 16); qa[1] = hw_nefc; qa[2] = hw_nrrow | (hw_npp << 16); qa[3] = (int)dt;
      }
      else dt /= (unsigned long long)(qtick + 1);
    }
    if (!q_more && !hand_over) {
      // bit 2 (QUEUE): moved to the large kernel inside the launch -- the host flags the env large, nothing to re-run
#ifdef MRE_LARGE_CAPS
      li[0] = (s.overflow ? 2 : 0) | (moved ? 4 : 0);
#else
      li[0] = s.overflow ? 1 : 0;
#endif
      li[1] = hw_ncon | ((int)(dt < 0x7FFFull ? dt : 0x7FFFull) << 16); li[2] = hw_nefc; li[3] = hw_nrrow | (hw_npp << 16);
    }
  }
#ifndef MRE_LARGE_CAPS
  if (!QUEUE && l == 0 && a.pending != nullptr && s.overflow) a.pending[env] = 1;
#endif
  if (l == 0 && a.status != nullptr && !hand_over) {
    unsigned st = 0;
    for (int k = 0; k < NQ; k++) if (!isfinite(s.qpos[k])) st |= 2u;
    if (s.overflow) st |= 4u;
    if (QUEUE) { if (st) __hip_atomic_fetch_or(a.status + env, st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    else a.status[env] |= st;
    // (QUEUE, write-through: the host reads the last tick's; a plain store per tick, from a wave on another XCD each
    //  time and with no write-back in between, could reach memory after a later tick's)
    if (a.stats != nullptr && a.nsteps > 0 && !(QUEUE && Q_WRITE_THROUGH && q_more)) {
      a.stats[env * 4 + 0] = s.ncon; a.stats[env * 4 + 1] = s.nefc;
      a.stats[env * 4 + 2] = s.solver_iters; a.stats[env * 4 + 3] = s.nl;
#ifdef MRE_PHASE_STAMPS
      for (int k = 0; k < 4; k++) a.stats[env * 4 + k] = (int)(stamp_acc[k] >> 4);
#if MRE_PHASE_STAMPS >= 4
      for (int k = 0; k < 4; k++) a.stats[env * 4 + k] = (int)(dbg_acc[k] >> 4);
#endif
#endif
    }
  }
  if (!QUEUE) return;
  if (hand_over) queue_push(a, l, env, qtick, a.q_shards + env % a.q_lshards);   // the same tick again, with the large capacities
  else if (q_more) queue_push(a, l, env, qtick + 1, qshard);
  else if (l == 0) __hip_atomic_fetch_add(a.q_done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // through
 }
}

// Entry points.  This file is compiled four times (lib.py): {compact, large capacities} x {PGS,
// Newton}; the kernel and launcher names carry the variant so that profiler summaries tell them apart.
#ifdef MRE_NEWTON
#define MRE_VARIANT(name) name##_newton
#else
#define MRE_VARIANT(name) name
#endif

#ifdef MRE_LARGE_CAPS
// large-capacity instantiation (mre_dev.h)
__global__ __launch_bounds__(64, 2) void MRE_VARIANT(k_step_large)(StepArgs a) {
  __shared__ Sm s;
  step_body<false>(a, s);
}
}  // namespace mre

extern "C" void MRE_VARIANT(mre_launch_step_large)(const mre::StepArgs* args, hipStream_t stream) {
  hipLaunchKernelGGL(mre::MRE_VARIANT(k_step_large), dim3(args->N), dim3(64), 0, stream, *args);
}
// the large kernel's waves of a queue launch (step_body: capacity fallback inside the launch)
namespace mre {
__global__ __launch_bounds__(64, 2) void MRE_VARIANT(k_step_queue_large)(StepArgs a) {
  __shared__ Sm s;
  step_body<true>(a, s);
}
}  // namespace mre
extern "C" void MRE_VARIANT(mre_launch_step_queue_large)(const mre::StepArgs* args, int nwaves, hipStream_t stream) {
  hipLaunchKernelGGL(mre::MRE_VARIANT(k_step_queue_large), dim3(nwaves), dim3(64), 0, stream, *args);
}
#else
// control ticks: mre_step / mre_rollout / mre_run_controller
__global__ __launch_bounds__(64, 2) void MRE_VARIANT(k_step)(StepArgs a) {
  __shared__ Sm s;
  step_body<false>(a, s);
}

// frozen-robot settling after prop placement (mre_place_props): same body, own name in traces
__global__ __launch_bounds__(64, 2) void MRE_VARIANT(k_settle)(StepArgs a) {
  __shared__ Sm s;
  step_body<false>(a, s);
}

// a rollout of several control ticks over more envs than the GPU holds waves (mre_rollout_ticks): persistent waves, one
// (env, tick) per pass -- see step_body
__global__ __launch_bounds__(64, 2) void MRE_VARIANT(k_step_queue)(StepArgs a) {
  __shared__ Sm s;
  step_body<true>(a, s);
}

#ifdef MRE_NEWTON
}  // namespace mre
extern "C" void mre_launch_step_newton(const mre::StepArgs* args, hipStream_t stream) {
  hipLaunchKernelGGL(mre::k_step_newton, dim3(args->N), dim3(64), 0, stream, *args);
}
extern "C" void mre_launch_settle_newton(const mre::StepArgs* args, hipStream_t stream) {
  hipLaunchKernelGGL(mre::k_settle_newton, dim3(args->N), dim3(64), 0, stream, *args);
}
extern "C" void mre_launch_step_queue_newton(const mre::StepArgs* args, int nwaves, hipStream_t stream) {
  hipLaunchKernelGGL(mre::k_step_queue_newton, dim3(nwaves), dim3(64), 0, stream, *args);
}
// waves of the queue kernel one compute unit holds at a time (its LDS block decides)
extern "C" int mre_queue_waves_per_cu_newton(void) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, mre::k_step_queue_newton, 64, 0) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return nb;
}
#else

// Physics.reset() + arm home pose (tasks/rearrangement.py:302-306); cubes parked
__global__ __launch_bounds__(64) void k_reset(const DevModel* M, int N, float* qpos, float* qvel,
                                              float* qacc_ws, float* qfine, float* ctrl, uint32_t* status,
                                              int* nstep, const uint8_t* mask) {
  const int env = blockIdx.x, l = threadIdx.x;
  if (env >= N) return;
  if (mask != nullptr && mask[env] == 0) return;
  if (l < NQP) {
    float v = (l < NQ) ? M->qpos0[l] : 0.f;
    if (l < 7) v = M->home_qpos[l];
    if (l >= NRV && l < NQ) {
      const int p = (l - NRV) / 7, k = (l - NRV) % 7;
      v = (k < 3) ? M->park_pos[p][k] : (k == 3 ? 1.f : 0.f);
    }
    qpos[(size_t)env * NQP + l] = v;
  }
  if (l < NVP) { qvel[(size_t)env * NVP + l] = 0.f; qacc_ws[(size_t)env * NVP + l] = 0.f; }
  for (int k = l; k < QFINE_ROW; k += 64) qfine[(size_t)env * QFINE_ROW + k] = 0.f;
  if (l < NU) ctrl[(size_t)env * NU + l] = 0.f;
  if (l == 0) { status[env] = 0u; nstep[env] = 0; }   // Physics.reset(): data.time = 0
}

// ---- demonstration logic around the step and the PropPlacer's rejection loop
// counter RNG of rng.py / mre_api.cpp (splitmix64 finaliser keyed by seed, global env id, tick, channel)
MRE_DEV unsigned long long mix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
MRE_DEV double uniform01(unsigned long long seed, unsigned long long env, unsigned long long tick, unsigned long long ch) {
  unsigned long long k = mix64(seed + 0x9E3779B97F4A7C15ull * env);
  k = mix64(k ^ (tick * 0xBF58476D1CE4E5B9ull));
  k = mix64(k ^ (ch * 0x94D049BB133111EBull));
  return (double)(k >> 11) * (1.0 / 9007199254740992.0);
}

// Rejection sampling of one cube's pose per env (SearchArgs, mre_dev.h): the inner loops of
// PropPlacer.__call__ (environment/prop_initializer.py:198-232) and of prop_place
// (tasks/rearrangement.py:628-663).  The reference moves the prop in a copy of the physics and calls
// physics.forward(); here the candidate pose lives in the wave's LDS copy of the body frames and only the
// cube's own pairs (<= 19 of the static table, table pairs dropped: both callers ignore them) go through
// the narrow phase, one lane per pair.
__global__ __launch_bounds__(64) void k_pose_search(SearchArgs a) {
  __shared__ Sm s;
  const int env = blockIdx.x, l = threadIdx.x;
  if (env >= a.N) return;
  if (a.env_mask != nullptr && a.env_mask[env] == 0) return;
  ModelP M = (ModelP)a.M;
  const int np = a.nprops[env];
  const int p = a.prop != nullptr ? a.prop[env] : a.fixed_prop;
  if (p < 0 || p >= np || p >= NPROP) {
    if (l == 0 && a.attempts != nullptr) a.attempts[env] = 0;
    return;
  }
  if (l < NQP) s.qpos[l] = a.qpos[(size_t)env * NQP + l];
  if (l < QFINE) s.qlo[l] = 0.f;   // the robot's frames from the float32 words of its angles (the robot is at rest at home when props are placed)
  if (l == 0) s.nprops = np;
  if (l < NPROP * 3) s.prop_size[l / 3][l % 3] = a.prop_size[(size_t)env * NPROP * 3 + l];
  MRE_SYNC();
  kinematics_only(M, s, l);
  // the cube's pairs, in table order
  const int gp = PROP_GEOM0 + p, table = 1, body = NRB + p;
  int cnt = 0;
  for (int pass = 0; pass < NPAIR / 64; pass++) {
    const int pr = l + 64 * pass;
    const int g1 = M->pair_g1[pr], g2 = M->pair_g2[pr];
    bool mine = g1 >= 0 && (g1 == gp || g2 == gp) && g1 != table && g2 != table;
    if (mine) mine = body_is_active(M, s, M->geom_body[g1]) && body_is_active(M, s, M->geom_body[g2]);
    const unsigned long long b = __ballot(mine);
    if (mine) s.iscr[cnt + __popcll(b & ((1ull << l) - 1ull))] = pr;
    cnt += __popcll(b);
  }
  MRE_SYNC();
  const int pr = l < cnt ? s.iscr[l] : -1;
  MRE_SYNC();
  float* buf = &s.JpA[0][0] + l * COLL_BUF;   // this lane's clip buffer (as in collide)
  const unsigned long long gid = (unsigned long long)(a.env_ids != nullptr ? a.env_ids[env] : a.env_id_offset + env);
  const unsigned long long tick0 = (unsigned long long)(a.tick_base != nullptr ? (long long)a.tick_base[env] : a.tick0);
  const double* bd = a.bounds != nullptr ? a.bounds + (size_t)env * 6 : a.shared_bounds;
  double pose[7];
  int used = -a.max_attempts;
  for (int att = 0; att < a.max_attempts; att++) {
    for (int k = 0; k < 3; k++) pose[k] = bd[k] + (bd[3 + k] - bd[k]) * uniform01(a.seed, gid, tick0 + att, k);
    if (a.yaw_mode) {
      const double yaw = 3.14159265358979323846 * uniform01(a.seed, gid, tick0 + att, 3);
      pose[3] = cos(yaw / 2); pose[4] = 0.0; pose[5] = 0.0; pose[6] = sin(yaw / 2);
    } else {
      for (int k = 0; k < 4; k++) pose[3 + k] = a.fixed_quat[k];
    }
    if (l == 0) {   // physics.forward() of the moved cube: a free body's frame is its qpos
      float xq[4] = {(float)pose[3], (float)pose[4], (float)pose[5], (float)pose[6]};
      qnormalize(xq);
      for (int k = 0; k < 3; k++) s.xpos[body][k] = (float)pose[k];
      for (int k = 0; k < 4; k++) s.xquat[body][k] = xq[k];
      q2mat(s.xmat[body], xq);
    }
    MRE_SYNC();
    bool hit = false;
    if (pr >= 0) {
      const int g1 = M->pair_g1[pr], g2 = M->pair_g2[pr];
      float p1[3], R1[9], s1[3], rb1, p2[3], R2[9], s2[3], rb2, normal[3] = {0.f, 0.f, 1.f}, df[3];
      geom_pose(M, s, g1, p1, R1, s1, &rb1);
      geom_pose(M, s, g2, p2, R2, s2, &rb2);
      const float inc = M->pair_margin[pr];
      int n = 0;
      FaceCand rc;
      unsigned rm = 0u;
      v3sub(df, p2, p1);
      if (M->geom_type[g1] == 0) {
        float nn[3] = {R1[2], R1[5], R1[8]};
        if (v3dot(df, nn) - rb2 <= inc) n = plane_box(p1, R1, p2, R2, s2, inc, normal, buf);
      } else {
        const float r = rb1 + rb2 + inc;
        if (v3dot(df, df) <= r * r) n = box_box(p1, R1, s1, p2, R2, s2, inc, normal, buf, (a.flags & F_CLIP_ALWAYS) != 0, rc, rm);
      }
      if (rm & FACE_IN_REGS) {   // an unclipped face contact: its candidates are in registers (mre_collide.h)
#pragma unroll
        for (int v = 0; v < 4; v++)
          if (((rm >> v) & 1u) != 0u && rc.d[v] < inc && rc.d[v] <= a.max_dist) hit = true;
      } else {
        for (int c = 0; c < n; c++) {
          const float d = cand_dist(buf, c);
          if (d < inc && d <= a.max_dist) hit = true;   // a detected contact (dist < margin) close enough to reject
        }
      }
    }
    const bool any = __ballot(hit) != 0ull;
    MRE_SYNC();
    if (!any) { used = att + 1; break; }
  }
  if (l == 0) {
    if (a.attempts != nullptr) a.attempts[env] = used;
    if (used > 0) {
      if (a.pose != nullptr) for (int k = 0; k < 7; k++) a.pose[(size_t)env * 7 + k] = pose[k];
      if (a.commit) {
        float* q = a.qpos + (size_t)env * NQP + NRV + 7 * p;
        for (int k = 0; k < 7; k++) q[k] = (float)pose[k];
        if (a.qfine != nullptr) {   // the accepted pose is an fp64 draw: its low-order words go with it, the cube starts at rest
          float* ql = a.qfine + (size_t)env * QFINE_ROW;
          for (int k = 0; k < 7; k++) ql[QFINE_CUBE_Q + 7 * p + k] = (float)(pose[k] - (double)(float)pose[k]);
          for (int k = 0; k < 6; k++) ql[QFINE_CUBE_V + 6 * p + k] = 0.f;
        }
      }
    }
  }
}

// mj_jacSite / mj_fullM / qfrc_bias of the arm on the current state (DynArgs, mre_dev.h): the position and velocity
// stages exactly as the controller evaluation of a zero-step launch runs them (step_body: F_OSC_EVAL), then the terms
// formed as osc_compute forms o.J and o.M (lane = matrix entry) -- the float32 numbers the in-kernel law consumes.
// The row is staged in LDS and leaves in one 512-byte store per wave; the state rows are read, never written.
__global__ __launch_bounds__(64) void k_arm_dynamics(DynArgs a) {
  __shared__ Sm s;
  __shared__ alignas(8) float row[DYN_W];
  const int env = blockIdx.x, l = threadIdx.x;
  if (env >= a.N) return;
  ModelP M = (ModelP)a.M;
  // ---- load state as a step launch does (step_body); the warm start and ctrl are no input of these stages
  if (l < NQP) s.qpos[l] = a.qpos[(size_t)env * NQP + l];
  if (l < NVP) { s.qvel[l] = a.qvel[(size_t)env * NVP + l]; s.qacc[l] = 0.f; s.qfrc_con[l] = 0.f; }
  if (l < QFINE) s.qlo[l] = a.qfine != nullptr ? a.qfine[(size_t)env * QFINE_ROW + l] : 0.f;
  if (l < NU) s.ctrl[l] = 0.f;
  if (l == 0) { s.nprops = a.nprops[env]; s.overflow = 0; s.ncon = 0; s.nefc = 0; s.solver_iters = 0; }
  if (l < NPROP * 3) s.prop_size[l / 3][l % 3] = a.prop_size[(size_t)env * NPROP * 3 + l];
  MRE_SYNC();
  if (l < NPROP) {
    const float m = M->body_mass[NRB + l];
    const float* z = s.prop_size[l];
    s.prop_mass[l] = m;
    s.prop_inertia[l][0] = m / 3.f * (z[1] * z[1] + z[2] * z[2]);
    s.prop_inertia[l][1] = m / 3.f * (z[0] * z[0] + z[2] * z[2]);
    s.prop_inertia[l][2] = m / 3.f * (z[0] * z[0] + z[1] * z[1]);
  }
  MRE_SYNC();
  position_stage(M, s, l);
  gripper_local(M, s, l);
  crb_mass_matrix(M, s, l);
  MRE_SYNC();
  velocity_stage(M, s, l);
  MRE_SYNC();
  const int st = a.site != 0 ? M->opt_rec.tcp_site : M->opt_rec.eef_site;
  if (l < 42) {
    const int r = l / 7, c = l % 7;
    const float* cd = s.cdof[c];
    float off[3], t[3];
    v3sub(off, s.site_xpos[st], s.com_robot);
    v3cross(t, cd, off);
    row[DYN_JAC + l] = (r < 3) ? (cd[3 + r] + t[r]) : cd[r - 3];
  }
  if (l < 49) {
    const int i = l / 7, j = l % 7;
    const int hi = i > j ? i : j, lo = i > j ? j : i;
    row[DYN_MASS + l] = s.qM[M->dof_Madr[hi] + (hi - lo)];
  }
  if (l >= 49 && l < 56) {
    const int d = l - 49;
    row[DYN_BIAS + d] = s.qfrc_bias[d];
    row[DYN_QPOS + d] = s.qpos[d];
    row[DYN_QVEL + d] = s.qvel[d];
  }
  if (l >= 56 && l < 59) row[DYN_POS + (l - 56)] = s.site_xpos[st][l - 56];
  if (l == 59) {
    // the controller site's orientation is kept as a matrix (osc_errors reads it); the pinch site's is composed here
    float q[4], m[9];
    if (a.site != 0) {
      const auto* SR = &M->site_rec[st];
      const float sq[4] = {SR->quat[0], SR->quat[1], SR->quat[2], SR->quat[3]};
      qmul(q, s.xquat[SR->body], sq);
      q2mat(m, q);
    } else {
      for (int k = 0; k < 9; k++) m[k] = s.site_xmat[0][k];
    }
    mat2q(q, m);
    for (int k = 0; k < 4; k++) row[DYN_QUAT + k] = q[k];
  }
  if (l < DYN_W - DYN_PAD) row[DYN_PAD + l] = 0.f;
  MRE_SYNC();
  reinterpret_cast<float2*>(a.out + (size_t)env * DYN_W)[l] = make_float2(row[2 * l], row[2 * l + 1]);
}

// mju_mat2Quat on a row-major matrix, fp64, normalised (model/compile.py: m2q)
MRE_DEV void mat2quat_d(const double* m, double* q) {
  const double t = m[0] + m[4] + m[8];
  if (t > 0) {
    const double w = sqrt(t + 1.0) * 2;
    q[0] = 0.25 * w; q[1] = (m[7] - m[5]) / w; q[2] = (m[2] - m[6]) / w; q[3] = (m[3] - m[1]) / w;
  } else if (m[0] > m[4] && m[0] > m[8]) {
    const double w = sqrt(1.0 + m[0] - m[4] - m[8]) * 2;
    q[0] = (m[7] - m[5]) / w; q[1] = 0.25 * w; q[2] = (m[1] + m[3]) / w; q[3] = (m[2] + m[6]) / w;
  } else if (m[4] > m[8]) {
    const double w = sqrt(1.0 + m[4] - m[0] - m[8]) * 2;
    q[0] = (m[2] - m[6]) / w; q[1] = (m[1] + m[3]) / w; q[2] = 0.25 * w; q[3] = (m[5] + m[7]) / w;
  } else {
    const double w = sqrt(1.0 + m[8] - m[0] - m[4]) * 2;
    q[0] = (m[3] - m[1]) / w; q[1] = (m[2] + m[6]) / w; q[2] = (m[5] + m[7]) / w; q[3] = 0.25 * w;
  }
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int k = 0; k < 4; k++) q[k] /= n;
}

// sort_colours' scan for the first cube outside its colour zone (tasks/rearrangement.py:727-749) and
// prop_pick for it (:579-595): position = the cube's, yaw folded by min(|yaw|, |yaw| - 90),
// grasp = mju_mat2Quat(Rz(yaw) Ry(180 deg)).  One thread per env, fp64 like the reference's numpy.
__global__ __launch_bounds__(64) void k_sort_select(SortArgs a) {
  const int env = blockIdx.x * 64 + threadIdx.x;
  if (env >= a.N) return;
  const float* q = a.qpos + (size_t)env * NQP + NRV;
  const int np = a.nprops[env];
  int which = -1;
  for (int p = 0; p < NPROP && p < np; p++) {
    const double* z = a.zones + ((size_t)env * NPROP + p) * 4;
    const double x = q[7 * p], y = q[7 * p + 1];
    if (!(z[0] <= x && x <= z[2] && z[1] <= y && y <= z[3])) { which = p; break; }
  }
  a.which[env] = which;
  const int p = which < 0 ? 0 : which;
  const float* c = q + 7 * p;
  double w = c[3], x = c[4], y = c[5], z = c[6];
  const double n = sqrt(w * w + x * x + y * y + z * z);
  w /= n; x /= n; y /= n; z /= n;
  const double r10 = 2 * (x * y + w * z), r00 = w * w + x * x - y * y - z * z;
  const double yaw = fabs(atan2(r10, r00) * (180.0 / 3.14159265358979323846));
  const double rz = (yaw < yaw - 90.0 ? yaw : yaw - 90.0) * (3.14159265358979323846 / 180.0);
  const double cs = cos(rz), sn = sin(rz);
  // Rz(rz) * diag(-1, 1, -1)
  const double m[9] = {-cs, -sn, 0.0, -sn, cs, 0.0, 0.0, 0.0, -1.0};
  double* o = a.pick + (size_t)env * 7;
  for (int k = 0; k < 3; k++) o[k] = c[k];
  mat2quat_d(m, o + 3);
  const double* zb = a.zones + ((size_t)env * NPROP + p) * 4;
  double* b = a.bounds + (size_t)env * 6;
  b[0] = zb[0]; b[1] = zb[1]; b[2] = a.place_z; b[3] = zb[2]; b[4] = zb[3]; b[5] = a.place_z;
}

// ---- capacity fallback helper (mre_api.cpp: launch_step).  The state rows are copied aside by the step kernel
// itself as it loads them (step_body), and the launch is split between the two kernels by StepArgs::large.
// put the selected envs back to their saved pre-launch state (one workgroup per env)
__global__ __launch_bounds__(64) void k_restore_rows(const uint8_t* sel, int env0, int N, float* qpos, const float* sv_qpos,
                                                     float* qvel, const float* sv_qvel, float* qacc_ws,
                                                     const float* sv_qacc_ws, float* qfine, const float* sv_qfine,
                                                     float* ctrl, const float* sv_ctrl, int* nstep, const int* sv_nstep,
                                                     uint32_t* status, const uint32_t* sv_status, uint8_t* converged,
                                                     const uint8_t* sv_converged, uint8_t* pending) {
  const int env = env0 + blockIdx.x, l = threadIdx.x;
  if ((int)blockIdx.x >= N || sel[env] == 0) return;
  if (l == 0 && pending != nullptr) pending[env] = 0;
  if (l < NQP) qpos[(size_t)env * NQP + l] = sv_qpos[(size_t)env * NQP + l];
  if (l < NVP) {
    qvel[(size_t)env * NVP + l] = sv_qvel[(size_t)env * NVP + l];
    qacc_ws[(size_t)env * NVP + l] = sv_qacc_ws[(size_t)env * NVP + l];
  }
  for (int k = l; k < QFINE_ROW; k += 64) qfine[(size_t)env * QFINE_ROW + k] = sv_qfine[(size_t)env * QFINE_ROW + k];
  if (l < NU) ctrl[(size_t)env * NU + l] = sv_ctrl[(size_t)env * NU + l];
  if (l == 0) { status[env] = sv_status[env]; converged[env] = sv_converged[env]; nstep[env] = sv_nstep[env]; }
}

// end-of-rollout rows for the gather over ranks (distributed.py): out[env] = qpos[43], qvel[39], status --
// packed on the device so that the row block goes straight into all_gather_into_tensor
__global__ __launch_bounds__(128) void k_pack_final(int N, const float* qpos, const float* qvel, const uint32_t* status, float* out) {
  const int env = blockIdx.x, l = threadIdx.x;
  if (env >= N) return;
  float v = 0.f;
  if (l < NQ) v = qpos[(size_t)env * NQP + l];
  else if (l < NQ + NV) v = qvel[(size_t)env * NVP + (l - NQ)];
  else if (l == NQ + NV) v = (float)status[env];   // (a small integer: exact)
  if (l <= NQ + NV) out[(size_t)env * (NQ + NV + 1) + l] = v;
}

}  // namespace mre

extern "C" void mre_launch_pack_final(int N, const float* qpos, const float* qvel, const uint32_t* status, float* out,
                                      hipStream_t stream) {
  hipLaunchKernelGGL(mre::k_pack_final, dim3(N), dim3(128), 0, stream, N, qpos, qvel, status, out);
}

extern "C" void mre_launch_restore_rows(const uint8_t* sel, int env0, int N, float* qpos, const float* sv_qpos, float* qvel,
                                        const float* sv_qvel, float* qacc_ws, const float* sv_qacc_ws, float* qfine,
                                        const float* sv_qfine, float* ctrl, const float* sv_ctrl, int* nstep,
                                        const int* sv_nstep, uint32_t* status, const uint32_t* sv_status,
                                        uint8_t* converged, const uint8_t* sv_converged, uint8_t* pending,
                                        hipStream_t stream) {
  hipLaunchKernelGGL(mre::k_restore_rows, dim3(N), dim3(64), 0, stream, sel, env0, N, qpos, sv_qpos, qvel, sv_qvel,
                     qacc_ws, sv_qacc_ws, qfine, sv_qfine, ctrl, sv_ctrl, nstep, sv_nstep, status, sv_status, converged,
                     sv_converged, pending);
}

extern "C" void mre_launch_pose_search(const mre::SearchArgs* args, hipStream_t stream) {
  hipLaunchKernelGGL(mre::k_pose_search, dim3(args->N), dim3(64), 0, stream, *args);
}

extern "C" void mre_launch_arm_dynamics(const mre::DynArgs* args, hipStream_t stream) {
  hipLaunchKernelGGL(mre::k_arm_dynamics, dim3(args->N), dim3(64), 0, stream, *args);
}

extern "C" void mre_launch_sort_select(const mre::SortArgs* args, hipStream_t stream) {
  hipLaunchKernelGGL(mre::k_sort_select, dim3((args->N + 63) / 64), dim3(64), 0, stream, *args);
}

extern "C" void mre_launch_reset(const mre::DevModel* M, int N, float* qpos, float* qvel, float* qacc_ws, float* qfine,
                                 float* ctrl, uint32_t* status, int* nstep, const uint8_t* mask, hipStream_t stream) {
  hipLaunchKernelGGL(mre::k_reset, dim3(N), dim3(64), 0, stream, M, N, qpos, qvel, qacc_ws, qfine, ctrl, status, nstep,
                     mask);
}

extern "C" void mre_launch_step(const mre::StepArgs* args, hipStream_t stream) {
  hipLaunchKernelGGL(mre::k_step, dim3(args->N), dim3(64), 0, stream, *args);
}

extern "C" void mre_launch_settle(const mre::StepArgs* args, hipStream_t stream) {
  hipLaunchKernelGGL(mre::k_settle, dim3(args->N), dim3(64), 0, stream, *args);
}
extern "C" void mre_launch_step_queue(const mre::StepArgs* args, int nwaves, hipStream_t stream) {
  hipLaunchKernelGGL(mre::k_step_queue, dim3(nwaves), dim3(64), 0, stream, *args);
}
extern "C" int mre_queue_waves_per_cu(void) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, mre::k_step_queue, 64, 0) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return nb;
}
#endif  // MRE_NEWTON
#endif  // MRE_LARGE_CAPS
