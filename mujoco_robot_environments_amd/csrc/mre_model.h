// mre_model.h -- host side of the model: the tables parsed out of the model blob and the one function that turns a
// blob into the DevModel the kernels read.  No HIP: mre_model.cpp compiles and runs as a plain host program.
#pragma once
#include <cstddef>
#include <string>

#include "mre_dev.h"

namespace mre {

// Every table of the blob (fp32) and what is derived from it, as model building sees it.  It lives for the duration of
// build_model() only.  The device gets the per-lane records packed from it and a copy of the few tables that DevModel
// lists; build_model() compares every record field against this struct before it returns.
struct ModelTables {
  // ---- bodies (index = body id)
  int body_parent[NB], body_dofadr[NB], body_qposadr[NB], body_propid[NB];
  int chain_len[NB];             // dofs root->body (robot bodies; cubes: 0, handled apart)
  int chain_dof[NB][MAXCHAIN];
  float body_pos[NB][3], body_quat[NB][4], body_ipos[NB][3], body_iquat[NB][4];
  float body_mass[NB], body_inertia[NB][3], body_invweight0[NB][2];
  float jnt_pos[NB][3], jnt_axis[NB][3], jnt_range[NB][2], jnt_stiffness[NB], jnt_springref[NB];
  float jnt_solref[NB][2], jnt_solimp[NB][5];
  int jnt_limited[NB];
  // ---- dofs
  int dof_body[NV], dof_parent[NV], dof_Madr[NV + 1];
  float dof_armature[NV], dof_damping[NV], dof_invweight0[NV], qpos0[NQP];
  // ---- robot mass-matrix structure
  int M_i[NMR], M_j[NMR];        // entry e = M(i, j), j ancestor-or-self of i
  float robot_mass;              // sum of robot body masses (subtree mass of link1)
  float M0_diag_robot_sum;       // sum_i M0(i,i) over robot dofs (meaninertia)
  // ---- geoms / pairs / sites
  int geom_type[NG], geom_body[NG], geom_propid[NG];
  float geom_size[NG][3], geom_pos[NG][3], geom_quat[NG][4], geom_rbound[NG];
  int pair_g1[NPAIR], pair_g2[NPAIR], pair_single[NPAIR];
  float pair_friction[NPAIR][3], pair_solref[NPAIR][2], pair_solimp[NPAIR][5];
  float pair_margin[NPAIR], pair_gap[NPAIR];
  int site_body[NSITE];
  float site_pos[NSITE][3], site_quat[NSITE][4];
  int eef_site, tcp_site;
  // ---- equality / tendon / actuation
  int eq_type[NEQ], eq_obj[NEQ][2];
  float eq_data[NEQ][8], eq_solref[NEQ][2], eq_solimp[NEQ][5];
  int ten_dof[2];
  float ten_coef[2];
  float act_ctrlrange[NU][2], grip_gainprm, grip_biasprm[3], grip_forcerange[2];
  // arm actuators 0..6 as MuJoCo `general` actuators on their joint: force = gain ctrl + bias0 + bias1 q +
  // bias2 qvel, clamped to forcerange when limited.  motor.yaml: gain 1, bias 0, unlimited;
  // position.yaml (LasaDrawEnv deployment config): gain kp, bias (0, -kp, -kv), forcerange +-87 / +-12
  float act_gain[NU], act_bias[NU][3], act_forcerange[NU][2];
  int act_forcelimited[NU];
  // ---- options
  float timestep, gravity[3], impratio, tolerance;
  int iterations;
  int cone;                      // mjtCone: 0 = pyramidal, 1 = elliptic
  float home_qpos[7];
  float park_pos[NPROP][3];      // where inactive cube slots are parked
};

// Parses `blob`, checks it against the topology the kernels are compiled for, and fills `m` (tables, packed records) and
// `solver` (mjtSolver of the blob: 0 = PGS, 2 = Newton).  Returns the empty string, or why the model is refused
// (MRE_ERR_MODEL); `m` and `solver` are unspecified then.
std::string build_model(const void* blob, size_t nbytes, DevModel& m, int& solver);

}  // namespace mre
