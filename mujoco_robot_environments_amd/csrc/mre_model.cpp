// mre_model.cpp -- from the model blob (mujoco_robot_environments_amd/model/compile.py: to_blob) to the DevModel the
// kernels read: parse the tables, check them against the topology the kernels are compiled for, derive the chain and
// mass-matrix tables, pack the per-lane records and compare every record field with the table it came from.
// Plain host code: no HIP runtime call, so it also builds and runs as an ordinary program.
#include "mre_model.h"

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/mre.h"

namespace mre {

namespace {
struct Blob {
  const unsigned char* p;
  size_t n;
  bool find(const char* name, uint32_t* code, uint32_t* count, uint64_t* off) const {
    uint32_t ne;
    memcpy(&ne, p + 8, 4);
    const unsigned char* t = p + 16;
    for (uint32_t k = 0; k < ne; k++, t += 48)
      if (strncmp((const char*)t, name, 32) == 0) {
        memcpy(code, t + 32, 4); memcpy(count, t + 36, 4); memcpy(off, t + 40, 8);
        return *off + (size_t)(*count) * (*code ? 8 : 4) <= n;
      }
    return false;
  }
  bool ints(const char* name, int* dst, int expect) const {
    uint32_t c, cnt; uint64_t off;
    if (!find(name, &c, &cnt, &off) || c != 0 || (int)cnt != expect) return false;
    memcpy(dst, p + off, 4 * (size_t)cnt);
    return true;
  }
  bool flts(const char* name, float* dst, int expect) const {
    uint32_t c, cnt; uint64_t off;
    if (!find(name, &c, &cnt, &off) || c != 1 || (int)cnt != expect) return false;
    for (uint32_t k = 0; k < cnt; k++) {
      double v;
      memcpy(&v, p + off + 8 * (size_t)k, 8);
      dst[k] = (float)v;
    }
    return true;
  }
};
}  // namespace

#define RI(name, dst, n) if (!b.ints(name, (int*)(dst), n)) return std::string("model entry ") + name
#define RF(name, dst, n) if (!b.flts(name, (float*)(dst), n)) return std::string("model entry ") + name

// The per-lane records of mre_dev.h (BodyRec .. OptRec): filled from the host's tables, then every field of the device
// model is compared with the table entry it packs -- a record that disagrees with its table would change results silently.
static bool same_bits(const void* a, const void* b, size_t n) { return memcmp(a, b, n) == 0; }
static std::string pack_records(const ModelTables& t, DevModel& m) {
  if (t.ten_dof[0] == t.ten_dof[1] || t.ten_dof[0] < 0 || t.ten_dof[0] >= NRV || t.ten_dof[1] < 0 || t.ten_dof[1] >= NRV)
    return "the gripper tendon must couple two different robot dofs";
  for (int e = 0; e < NEQ; e++)
    for (int k = 0; k < 2; k++)
      if (t.eq_obj[e][k] < 1 || t.eq_obj[e][k] >= NRB) return "equality constraints must couple robot bodies";
  if (t.tcp_site < 0 || t.tcp_site >= NSITE || t.eef_site < 0 || t.eef_site >= NSITE) return "tcp_site / eef_site name no site";
  // (the phases take a finger body's place in the tree from its number: even bodies hang off the arm's last link, odd ones off the body below)
  for (int b = 1; b < NRB; b++)
    if (t.body_parent[b] != ROBOT_DOF_PARENT[b - 1] + 1) return "robot body tree differs from the one the kernels are unrolled for (mre_dev.h)";
  for (int d = 0; d < NV; d++)
    if (t.dof_body[d] != (d < NRV ? d + 1 : NRB + (d - NRV) / 6)) return "dof layout differs from the compiled kernels";
  auto ten_of = [&](int d) { return d == t.ten_dof[0] ? 0 : (d == t.ten_dof[1] ? 1 : -1); };
  for (int b = 0; b < NB; b++) {
    BodyRec& r = m.body_rec[b];
    memset(&r, 0, sizeof(r));
    for (int c = 0; c < 4; c++) { r.quat[c] = t.body_quat[b][c]; r.iquat[c] = t.body_iquat[b][c]; }
    for (int c = 0; c < 3; c++) { r.pos[c] = t.body_pos[b][c]; r.ipos[c] = t.body_ipos[b][c]; r.jnt_pos[c] = t.jnt_pos[b][c];
                                  r.jnt_axis[c] = t.jnt_axis[b][c]; r.inertia[c] = t.body_inertia[b][c]; }
    for (int c = 0; c < 2; c++) { r.jnt_range[c] = t.jnt_range[b][c]; r.invweight0[c] = t.body_invweight0[b][c]; }
    r.mass = t.body_mass[b]; r.qposadr = t.body_qposadr[b]; r.dofadr = t.body_dofadr[b]; r.propid = t.body_propid[b];
    r.qpos0 = (r.qposadr >= 0 && r.qposadr < NQ) ? t.qpos0[r.qposadr] : 0.f;
    r.jnt_stiffness = t.jnt_stiffness[b]; r.jnt_springref = t.jnt_springref[b];
    r.parent = t.body_parent[b]; r.jnt_limited = t.jnt_limited[b];
  }
  for (int d = 0; d < NV; d++) {
    DofRec& r = m.dof_rec[d];
    memset(&r, 0, sizeof(r));
    const int b = t.dof_body[d];
    if (b < 0 || b >= NB) return "dof_bodyid names a body that does not exist";
    r.body = b; r.propid = t.body_propid[b]; r.dofadr = t.body_dofadr[b]; r.ten = ten_of(d);
    r.armature = t.dof_armature[d]; r.damping = t.dof_damping[d]; r.invweight0 = t.dof_invweight0[d];
    r.ten_coef = r.ten >= 0 ? t.ten_coef[r.ten] : 0.f;
    r.jnt_stiffness = t.jnt_stiffness[b]; r.jnt_springref = t.jnt_springref[b];
    if (d < 7) {   // arm actuator d drives dof d (checked in build_model)
      r.act_gain = t.act_gain[d]; r.act_bias0 = t.act_bias[d][0]; r.act_bias1 = t.act_bias[d][1]; r.act_bias2 = t.act_bias[d][2];
      r.act_ctrl_lo = t.act_ctrlrange[d][0]; r.act_ctrl_hi = t.act_ctrlrange[d][1];
      r.act_force_lo = t.act_forcerange[d][0]; r.act_force_hi = t.act_forcerange[d][1];
      r.act_forcelimited = t.act_forcelimited[d];
    }
  }
  for (int e = 0; e < NMR; e++) {
    MEntryRec& r = m.m_rec[e];
    memset(&r, 0, sizeof(r));
    r.i = t.M_i[e]; r.j = t.M_j[e];
    r.armature = t.dof_armature[r.i]; r.damping = t.dof_damping[r.i];
    r.act_bias2 = r.i < 7 ? t.act_bias[r.i][2] : 0.f;
    r.ten = ten_of(r.i); r.ten_coef = r.ten >= 0 ? t.ten_coef[r.ten] : 0.f;
  }
  for (int k = 0; k < NROWREC; k++) memset(&m.row_rec[k], 0, sizeof(RowRec));
  for (int e = 0; e < NEQ; e++) {
    RowRec& r = m.row_rec[e];
    const int b1 = t.eq_obj[e][0], b2 = t.eq_obj[e][1];
    for (int c = 0; c < 2; c++) r.solref[c] = t.eq_solref[e][c];
    for (int c = 0; c < 5; c++) r.solimp[c] = t.eq_solimp[e][c];
    // (the kernels treat equalities 0 and 1 as the `connect` rows of the finger linkage, 2 as the joint coupling)
    r.invw1 = e < 2 ? t.body_invweight0[b1][0] : t.dof_invweight0[b1 - 1];
    r.invw2 = e < 2 ? t.body_invweight0[b2][0] : t.dof_invweight0[b2 - 1];
    EqRec& q = m.eq_rec[e];
    memset(&q, 0, sizeof(q));
    q.type = t.eq_type[e]; q.b1 = b1; q.b2 = b2; q.pb1 = t.body_parent[b1]; q.pb2 = t.body_parent[b2];
    q.root = b1;
    while (q.root >= GRIP_BODY0) q.root = t.body_parent[q.root];
    for (int c = 0; c < 8; c++) q.data[c] = t.eq_data[e][c];
    q.qpos0_1 = t.qpos0[b1 - 1]; q.qpos0_2 = t.qpos0[b2 - 1];
    q.root_chain_len = t.chain_len[q.root];
    for (int c = 0; c < MAXCHAIN; c++) q.root_chain[c] = t.chain_dof[q.root][c];
  }
  for (int b = 1; b < NRB; b++) {
    RowRec& r = m.row_rec[ROWREC_JNT + b];
    for (int c = 0; c < 2; c++) r.solref[c] = t.jnt_solref[b][c];
    for (int c = 0; c < 5; c++) r.solimp[c] = t.jnt_solimp[b][c];
    r.invw1 = t.dof_invweight0[b - 1];
  }
  for (int k = 0; k < NPAIR; k++) {
    if (t.pair_g1[k] < 0) continue;
    RowRec& r = m.row_rec[ROWREC_PAIR + k];
    const int b1 = t.geom_body[t.pair_g1[k]], b2 = t.geom_body[t.pair_g2[k]];
    for (int c = 0; c < 2; c++) r.solref[c] = t.pair_solref[k][c];
    for (int c = 0; c < 5; c++) r.solimp[c] = t.pair_solimp[k][c];
    r.margin = t.pair_margin[k]; r.gap = t.pair_gap[k]; r.friction = t.pair_friction[k][0];
    r.invw1 = (b1 > 0 && b1 < NRB) ? t.body_invweight0[b1][0] : 0.f;
    r.invw2 = (b2 > 0 && b2 < NRB) ? t.body_invweight0[b2][0] : 0.f;
  }
  for (int k = 0; k < NSITE; k++) {
    SiteRec& r = m.site_rec[k];
    memset(&r, 0, sizeof(r));
    if (t.site_body[k] < 0 || t.site_body[k] >= NB) return "site_bodyid names a body that does not exist";
    r.body = t.site_body[k];
    for (int c = 0; c < 3; c++) r.pos[c] = t.site_pos[k][c];
    for (int c = 0; c < 4; c++) r.quat[c] = t.site_quat[k][c];
  }
  {
    OptRec& o = m.opt_rec;
    memset(&o, 0, sizeof(o));
    o.timestep = t.timestep; o.impratio = t.impratio; o.tolerance = t.tolerance; o.iterations = t.iterations;
    for (int c = 0; c < 3; c++) { o.gravity[c] = t.gravity[c]; o.grip_biasprm[c] = t.grip_biasprm[c]; }
    o.cone = t.cone;
    for (int c = 0; c < 2; c++) { o.ten_coef[c] = t.ten_coef[c]; o.ten_dof[c] = t.ten_dof[c]; o.grip_forcerange[c] = t.grip_forcerange[c];
                                  o.grip_ctrlrange[c] = t.act_ctrlrange[NU - 1][c]; }
    o.grip_gainprm = t.grip_gainprm; o.robot_mass = t.robot_mass; o.M0_diag_robot_sum = t.M0_diag_robot_sum;
    o.tcp_site = t.tcp_site; o.eef_site = t.eef_site;
    for (int c = 0; c < 3; c++) o.tcp_pos[c] = t.site_pos[t.tcp_site][c];
  }

  // ---- verification: every field against the table entry it packs (bit patterns: a NaN compares equal to itself)
  bool ok = true;
#define SAME(a, b) ok = ok && sizeof(a) == sizeof(b) && same_bits(&(a), &(b), sizeof(a))
  for (int b = 0; b < NB && ok; b++) {
    const BodyRec& r = m.body_rec[b];
    SAME(r.quat, t.body_quat[b]); SAME(r.pos, t.body_pos[b]); SAME(r.mass, t.body_mass[b]); SAME(r.jnt_pos, t.jnt_pos[b]);
    SAME(r.jnt_axis, t.jnt_axis[b]); SAME(r.qposadr, t.body_qposadr[b]); SAME(r.ipos, t.body_ipos[b]);
    SAME(r.propid, t.body_propid[b]); SAME(r.iquat, t.body_iquat[b]); SAME(r.inertia, t.body_inertia[b]);
    SAME(r.dofadr, t.body_dofadr[b]); SAME(r.jnt_range, t.jnt_range[b]); SAME(r.invweight0, t.body_invweight0[b]);
    SAME(r.jnt_stiffness, t.jnt_stiffness[b]); SAME(r.jnt_springref, t.jnt_springref[b]); SAME(r.parent, t.body_parent[b]);
    SAME(r.jnt_limited, t.jnt_limited[b]);
    if (b >= 1) SAME(r.qpos0, t.qpos0[t.body_qposadr[b]]);
  }
  for (int d = 0; d < NV && ok; d++) {
    const DofRec& r = m.dof_rec[d];
    const int b = t.dof_body[d];
    SAME(r.body, t.dof_body[d]); SAME(r.propid, t.body_propid[b]); SAME(r.dofadr, t.body_dofadr[b]);
    ok = ok && r.ten == (d == t.ten_dof[0] ? 0 : (d == t.ten_dof[1] ? 1 : -1));
    SAME(r.armature, t.dof_armature[d]); SAME(r.damping, t.dof_damping[d]); SAME(r.invweight0, t.dof_invweight0[d]);
    if (r.ten >= 0) SAME(r.ten_coef, t.ten_coef[r.ten]);
    SAME(r.jnt_stiffness, t.jnt_stiffness[b]); SAME(r.jnt_springref, t.jnt_springref[b]);
    if (d < 7) {
      SAME(r.act_gain, t.act_gain[d]); SAME(r.act_bias0, t.act_bias[d][0]); SAME(r.act_bias1, t.act_bias[d][1]);
      SAME(r.act_bias2, t.act_bias[d][2]); SAME(r.act_ctrl_lo, t.act_ctrlrange[d][0]); SAME(r.act_ctrl_hi, t.act_ctrlrange[d][1]);
      SAME(r.act_force_lo, t.act_forcerange[d][0]); SAME(r.act_force_hi, t.act_forcerange[d][1]);
      SAME(r.act_forcelimited, t.act_forcelimited[d]);
    }
  }
  for (int e = 0; e < NMR && ok; e++) {
    const MEntryRec& r = m.m_rec[e];
    SAME(r.i, t.M_i[e]); SAME(r.j, t.M_j[e]);
    const int i = t.M_i[e];
    SAME(r.armature, t.dof_armature[i]); SAME(r.damping, t.dof_damping[i]);
    if (i < 7) SAME(r.act_bias2, t.act_bias[i][2]);
    ok = ok && r.ten == (i == t.ten_dof[0] ? 0 : (i == t.ten_dof[1] ? 1 : -1));
    if (r.ten >= 0) SAME(r.ten_coef, t.ten_coef[r.ten]);
  }
  for (int e = 0; e < NEQ && ok; e++) {
    const RowRec& r = m.row_rec[e];
    const EqRec& q = m.eq_rec[e];
    const int b1 = t.eq_obj[e][0], b2 = t.eq_obj[e][1];
    SAME(r.solref, t.eq_solref[e]); SAME(r.solimp, t.eq_solimp[e]);
    if (e < 2) { SAME(r.invw1, t.body_invweight0[b1][0]); SAME(r.invw2, t.body_invweight0[b2][0]); }
    else { SAME(r.invw1, t.dof_invweight0[b1 - 1]); SAME(r.invw2, t.dof_invweight0[b2 - 1]); }
    SAME(q.type, t.eq_type[e]); SAME(q.b1, t.eq_obj[e][0]); SAME(q.b2, t.eq_obj[e][1]);
    SAME(q.pb1, t.body_parent[b1]); SAME(q.pb2, t.body_parent[b2]); SAME(q.data, t.eq_data[e]);
    SAME(q.qpos0_1, t.qpos0[b1 - 1]); SAME(q.qpos0_2, t.qpos0[b2 - 1]);
    int root = b1;
    while (root >= GRIP_BODY0) root = t.body_parent[root];
    ok = ok && q.root == root;
    SAME(q.root_chain_len, t.chain_len[root]);
    for (int c = 0; c < MAXCHAIN; c++) SAME(q.root_chain[c], t.chain_dof[root][c]);
  }
  for (int b = 1; b < NRB && ok; b++) {
    const RowRec& r = m.row_rec[ROWREC_JNT + b];
    SAME(r.solref, t.jnt_solref[b]); SAME(r.solimp, t.jnt_solimp[b]); SAME(r.invw1, t.dof_invweight0[b - 1]);
  }
  for (int k = 0; k < NPAIR && ok; k++) {
    if (t.pair_g1[k] < 0) continue;
    const RowRec& r = m.row_rec[ROWREC_PAIR + k];
    const int b1 = t.geom_body[t.pair_g1[k]], b2 = t.geom_body[t.pair_g2[k]];
    SAME(r.solref, t.pair_solref[k]); SAME(r.solimp, t.pair_solimp[k]); SAME(r.margin, t.pair_margin[k]);
    SAME(r.gap, t.pair_gap[k]); SAME(r.friction, t.pair_friction[k][0]);
    if (b1 > 0 && b1 < NRB) SAME(r.invw1, t.body_invweight0[b1][0]);
    if (b2 > 0 && b2 < NRB) SAME(r.invw2, t.body_invweight0[b2][0]);
  }
  for (int k = 0; k < NSITE && ok; k++) {
    const SiteRec& r = m.site_rec[k];
    SAME(r.body, t.site_body[k]); SAME(r.pos, t.site_pos[k]); SAME(r.quat, t.site_quat[k]);
  }
  {
    const OptRec& o = m.opt_rec;
    SAME(o.timestep, t.timestep); SAME(o.impratio, t.impratio); SAME(o.tolerance, t.tolerance); SAME(o.iterations, t.iterations);
    SAME(o.gravity, t.gravity); SAME(o.cone, t.cone); SAME(o.ten_coef, t.ten_coef); SAME(o.ten_dof, t.ten_dof);
    SAME(o.grip_gainprm, t.grip_gainprm); SAME(o.grip_biasprm, t.grip_biasprm); SAME(o.grip_forcerange, t.grip_forcerange);
    SAME(o.grip_ctrlrange, t.act_ctrlrange[NU - 1]); SAME(o.robot_mass, t.robot_mass);
    SAME(o.M0_diag_robot_sum, t.M0_diag_robot_sum); SAME(o.tcp_site, t.tcp_site); SAME(o.eef_site, t.eef_site);
    SAME(o.tcp_pos, t.site_pos[t.tcp_site]);
  }
#undef SAME
  if (!ok) return "a packed model record differs from the table it was filled from";
  return std::string();
}

std::string build_model(const void* blob, size_t nbytes, DevModel& m, int& solver) {
  if (nbytes < 16) return "blob too small";
  Blob b{(const unsigned char*)blob, nbytes};
  uint32_t magic;
  memcpy(&magic, b.p, 4);
  if (magic != 0x4D524542u) return "bad blob magic";
  uint32_t nentry;
  memcpy(&nentry, b.p + 8, 4);
  if (16 + 48 * (size_t)nentry > nbytes) return "blob too small";   // the entry table that Blob::find walks
  ModelTables t;
  memset(&t, 0, sizeof(t));
  memset(&m, 0, sizeof(m));
  int nbody, nv, nq, nM, ngeom, nsite, npair, neq, nprop, nu;
  RI("nbody", &nbody, 1); RI("nv", &nv, 1); RI("nq", &nq, 1); RI("nM", &nM, 1); RI("ngeom", &ngeom, 1);
  RI("nsite", &nsite, 1); RI("npair", &npair, 1); RI("neq", &neq, 1); RI("nprop", &nprop, 1);
  RI("nu", &nu, 1);
  if (nbody != NB || nv != NV || nq != NQ || ngeom != NG || nsite != NSITE || npair > NPAIR ||
      neq != NEQ || nprop != NPROP || nu != NU)
    return "scene dimensions differ from the compiled kernels";
  int body_jnttype[NB], act_dof[NU];   // read for the topology checks below only
  RI("body_parentid", t.body_parent, NB); RI("body_jnttype", body_jnttype, NB);
  RI("body_dofadr", t.body_dofadr, NB); RI("body_qposadr", t.body_qposadr, NB);
  RI("body_propid", t.body_propid, NB);
  RF("body_pos", t.body_pos, NB * 3); RF("body_quat", t.body_quat, NB * 4);
  RF("body_ipos", t.body_ipos, NB * 3); RF("body_iquat", t.body_iquat, NB * 4);
  RF("body_mass", t.body_mass, NB); RF("body_inertia", t.body_inertia, NB * 3);
  RF("body_invweight0", t.body_invweight0, NB * 2);
  RF("jnt_pos", t.jnt_pos, NB * 3); RF("jnt_axis", t.jnt_axis, NB * 3); RF("jnt_range", t.jnt_range, NB * 2);
  RF("jnt_stiffness", t.jnt_stiffness, NB); RF("jnt_springref", t.jnt_springref, NB);
  RF("jnt_solref", t.jnt_solref, NB * 2); RF("jnt_solimp", t.jnt_solimp, NB * 5);
  RI("jnt_limited", t.jnt_limited, NB);
  RI("dof_bodyid", t.dof_body, NV); RI("dof_parentid", t.dof_parent, NV); RI("dof_Madr", t.dof_Madr, NV);
  t.dof_Madr[NV] = nM;
  RF("dof_armature", t.dof_armature, NV); RF("dof_damping", t.dof_damping, NV);
  RF("dof_invweight0", t.dof_invweight0, NV); RF("qpos0", t.qpos0, NQ);
  RI("geom_type", t.geom_type, NG); RI("geom_bodyid", t.geom_body, NG); RI("geom_propid", t.geom_propid, NG);
  RF("geom_size", t.geom_size, NG * 3); RF("geom_pos", t.geom_pos, NG * 3);
  RF("geom_quat", t.geom_quat, NG * 4); RF("geom_rbound", t.geom_rbound, NG);
  {
    std::vector<int> pg(2 * npair);
    RI("pair_geom", pg.data(), 2 * npair);
    for (int k = 0; k < NPAIR; k++) { t.pair_g1[k] = -1; t.pair_g2[k] = -1; }
    for (int k = 0; k < npair; k++) { t.pair_g1[k] = pg[2 * k]; t.pair_g2[k] = pg[2 * k + 1]; }
  }
  RI("pair_single", t.pair_single, npair);
  RF("pair_friction", t.pair_friction, npair * 3); RF("pair_solref", t.pair_solref, npair * 2);
  RF("pair_solimp", t.pair_solimp, npair * 5); RF("pair_margin", t.pair_margin, npair);
  RF("pair_gap", t.pair_gap, npair);
  for (int k = 0; k < NPAIR; k++) {
    PairRec& r = m.pair_rec[k];
    memset(&r, 0, sizeof(r));
    r.g1 = t.pair_g1[k]; r.g2 = t.pair_g2[k];
    if (r.g1 < 0) { r.g2 = -1; r.b1 = r.b2 = 0; r.pid1 = r.pid2 = -1; continue; }
    if (r.g1 >= NG || r.g2 < 0 || r.g2 >= NG) return "pair table names a geom that does not exist";
    r.b1 = t.geom_body[r.g1]; r.b2 = t.geom_body[r.g2];
    r.pid1 = t.geom_propid[r.g1]; r.pid2 = t.geom_propid[r.g2];
    r.type1 = t.geom_type[r.g1]; r.single = (t.pair_single[k] & 0xFF) | (t.geom_type[r.g2] << 8);
    if (t.geom_type[r.g1] == 2 || (t.geom_type[r.g2] == 2 && t.geom_type[r.g1] != 1))
      return "cylinder pairs: only box (geom 1) - cylinder (geom 2) is implemented";
    for (int c = 0; c < 3; c++) { r.pos1[c] = t.geom_pos[r.g1][c]; r.pos2[c] = t.geom_pos[r.g2][c];
                                  r.size1[c] = t.geom_size[r.g1][c]; r.size2[c] = t.geom_size[r.g2][c]; }
    for (int c = 0; c < 4; c++) { r.quat1[c] = t.geom_quat[r.g1][c]; r.quat2[c] = t.geom_quat[r.g2][c]; }
    r.rb1 = t.geom_rbound[r.g1]; r.rb2 = t.geom_rbound[r.g2];
    r.margin = t.pair_margin[k]; r.gap = t.pair_gap[k];
  }
  RI("site_bodyid", t.site_body, NSITE); RF("site_pos", t.site_pos, NSITE * 3);
  RF("site_quat", t.site_quat, NSITE * 4);
  RI("eef_site", &t.eef_site, 1); RI("tcp_site", &t.tcp_site, 1);
  RI("eq_type", t.eq_type, NEQ); RI("eq_obj", t.eq_obj, NEQ * 2); RF("eq_data", t.eq_data, NEQ * 8);
  RF("eq_solref", t.eq_solref, NEQ * 2); RF("eq_solimp", t.eq_solimp, NEQ * 5);
  RI("ten_dof", t.ten_dof, 2); RF("ten_coef", t.ten_coef, 2);
  RI("act_dof", act_dof, NU); RF("act_ctrlrange", t.act_ctrlrange, NU * 2);
  RF("grip_gainprm", &t.grip_gainprm, 1); RF("grip_biasprm", t.grip_biasprm, 3);
  RF("grip_forcerange", t.grip_forcerange, 2);
  // arm actuators: motors (gain 1, no bias, unlimited force) unless the blob says otherwise
  for (int a = 0; a < NU; a++) { t.act_gain[a] = 1.f; t.act_forcelimited[a] = 0; }
  { uint32_t c, cnt; uint64_t off;
    if (b.find("act_gainprm", &c, &cnt, &off)) {
      RF("act_gainprm", t.act_gain, NU); RF("act_biasprm", t.act_bias, NU * 3);
      RF("act_forcerange", t.act_forcerange, NU * 2); RI("act_forcelimited", t.act_forcelimited, NU);
    } }
  RF("opt_timestep", &t.timestep, 1); RF("opt_gravity", t.gravity, 3); RF("opt_impratio", &t.impratio, 1);
  RF("opt_tolerance", &t.tolerance, 1); RI("opt_iterations", &t.iterations, 1);
  solver = MRE_SOLVER_PGS;  // older blobs carry no opt_solver
  { uint32_t c, cnt; uint64_t off; if (b.find("opt_solver", &c, &cnt, &off)) RI("opt_solver", &solver, 1); }
  if (solver != MRE_SOLVER_PGS && solver != MRE_SOLVER_NEWTON) return "opt_solver must be 0 (PGS) or 2 (Newton)";
  { uint32_t c, cnt; uint64_t off; int cone = 1;  // mjtCone; older blobs carry no opt_cone (elliptic)
    if (b.find("opt_cone", &c, &cnt, &off)) RI("opt_cone", &cone, 1);
    if (cone != 0 && cone != 1) return "opt_cone must be 0 (pyramidal) or 1 (elliptic)";
    t.cone = cone; }
  RF("home_qpos", t.home_qpos, 7);
  float M0d[NV];
  RF("M0_diag", M0d, NV);

  // ---- verify the topology the kernels assume: robot = bodies 1..15 with one hinge
  // each (dof = body-1), cubes = bodies 16..19 with free joints (dofs 15+6p)
  for (int bb = 1; bb < NB; bb++) {
    bool ok = bb < NRB ? (body_jnttype[bb] == 1 && t.body_dofadr[bb] == bb - 1 && t.body_qposadr[bb] == bb - 1 &&
                          t.body_propid[bb] < 0 && t.body_parent[bb] < bb)
                       : (body_jnttype[bb] == 2 && t.body_dofadr[bb] == NRV + 6 * (bb - NRB) &&
                          t.body_qposadr[bb] == NRV + 7 * (bb - NRB) && t.body_propid[bb] == bb - NRB &&
                          t.body_parent[bb] == 0);
    if (!ok) return "body layout differs from the compiled kernels";
  }
  if (t.dof_Madr[NRV] != NMR) return "robot mass-matrix size differs";
  for (int a = 0; a < 7; a++)
    if (act_dof[a] != a) return "arm actuators must drive dofs 0..6";

  int body_level[NB] = {0};   // parents precede children (body layout, above)
  for (int bb = 1; bb < NB; bb++) body_level[bb] = body_level[t.body_parent[bb]] + 1;
  for (int bb = 0; bb < NB; bb++)
    if (body_level[bb] > MAXCHAIN) return "tree deeper than MAXCHAIN";

  // ---- derived tables
  t.robot_mass = 0;
  for (int bb = 1; bb < NRB; bb++) {
    t.robot_mass += t.body_mass[bb];
    int chain[MAXCHAIN], n = 0;
    for (int d = t.body_dofadr[bb]; d >= 0; d = t.dof_parent[d]) {
      if (n >= MAXCHAIN) return "dof chain too long";
      chain[n++] = d;
    }
    t.chain_len[bb] = n;
    for (int k = 0; k < n; k++) t.chain_dof[bb][k] = chain[n - 1 - k];
  }
  for (int i = 0; i < NRV; i++) {
    int adr = t.dof_Madr[i];
    for (int j = i; j >= 0; j = t.dof_parent[j], adr++) { t.M_i[adr] = i; t.M_j[adr] = j; }
    if (adr != t.dof_Madr[i + 1]) return "dof_Madr inconsistent";
  }
  for (int i = 0; i < NRV; i++)
    if (t.dof_parent[i] != ROBOT_DOF_PARENT[i] || t.dof_Madr[i] != robot_dof_madr(i))
      return "robot dof tree differs from the one the kernels are unrolled for (mre_dev.h)";
  t.M0_diag_robot_sum = 0;
  for (int i = 0; i < NRV; i++) t.M0_diag_robot_sum += M0d[i];
  for (int p = 0; p < NPROP; p++) {  // same parking grid as the oracle's reset
    t.park_pos[p][0] = 2.0f + 0.5f * p; t.park_pos[p][1] = 2.0f; t.park_pos[p][2] = -5.0f;
  }
  // ---- the tables the device still indexes directly
#define KEEP(x) static_assert(sizeof(m.x) == sizeof(t.x), #x); memcpy(&m.x, &t.x, sizeof(m.x))
  KEEP(body_propid); KEEP(chain_len); KEEP(chain_dof); KEEP(body_mass);
  KEEP(dof_Madr); KEEP(qpos0); KEEP(M_i); KEEP(M_j);
  KEEP(geom_type); KEEP(geom_body); KEEP(geom_propid); KEEP(geom_size); KEEP(geom_pos); KEEP(geom_quat); KEEP(geom_rbound);
  KEEP(pair_g1); KEEP(pair_g2); KEEP(pair_margin);
  KEEP(act_ctrlrange); KEEP(home_qpos); KEEP(park_pos);
#undef KEEP
  std::string err = pack_records(t, m);
  if (!err.empty()) return err;
  int prop_geom0 = -1;
  for (int g = 0; g < NG; g++) if (t.geom_propid[g] == 0) prop_geom0 = g;
  if (prop_geom0 != PROP_GEOM0 || t.geom_type[1] != 1 || t.geom_body[1] != 0)
    return "mre_create: expected geom 1 = the table (static box) and one geom per cube slot";
  return std::string();
}

}  // namespace mre
